"""pkg/ptracers away from the grids it was developed on (test_gpu_ptracers.py): the k-march forms
of launch_tracer_step with a passive tracer's TracerArgs, lists past MG_XMAX = 8 tracers whose
launch order is far from their list order, ragged tilings, a parameter change on a stepped model,
and cube twins that can tell the tracer's operands from salt's.

The reference for tracer X is the oracle's salt with salt := X (test_gpu_ptracers.py): a whole
run under a linear EOS with sBeta = 0 and saltForcing = 0, CG2D summed in the device's order, or
one THERMODYNAMICS call after DO_OCEANIC_PHYS ran with the true salt.  Every X is a _wet_random
field of its own, and every tracer's diffusivities differ from salt's and from the other
tracers': a kernel that read f.salt, diffKrS, salt's scratch or another tracer's slot changes
bits.  Each reference builder runs once per module and asserts that what it returns is not
degenerate (every result differs from its X, any two results of one case differ).  The device
runs are cached the same way, one per (case, switches), and shared by the tests that assert
on them.

Bars: np.array_equal throughout; nothing is measured.

  A  the march forms on the synthetic LLC (functional route: ptr_batch_ok is false with a march):
     (14, 31, 7, 4) with the environment untouched, (12, 4, 6, 2) under every
     MGCM_TRACER_MARCH / MGCM_TRACER_MARCH2 form, and a surface-relaxed tracer at Nr = 31 per call;
  B  eleven tracers per call on tutorial_global_oce_latlon, every launch class of ptr_tables_sync
     non-empty, two calls on one model (both parity tables);
  C  nine tracers, 4 + 1 steps, the gyre in tiles of 31 x 2 and of 1 x 62 points;
  D  global_ocean.90x40x15 (OL = 3, r*, linear EOS) in tiles of 18 x 8 and of 5 x 5 points;
  E  mgcm_ptracer_param on a stepped model;
  F  the cube: a random tracer against a second model whose salt is that tracer.
"""
import contextlib
import functools
import itertools
import os

import numpy as np
import pytest

from test_gpu_ptracers import (BOTH, GYRE_TRACERS, LATLON_STATE, OCEAN90_OVER, OCEAN90_TRACERS, _device_order, _exch3,
                               _gyre_cfg, _inner, _latlon_model, _sum_plan, _wet_random)

pytestmark = pytest.mark.gpu
SWITCHES = ("MGCM_PTR_BATCH", "MGCM_TRACER_MARCH", "MGCM_TRACER_MARCH2", "MGCM_OVERLAP")


@contextlib.contextmanager
def _env(**kw):
    """The library's switches for the models made inside (None: unset); the cached device runs set
    them here, so that what a run used is what its cache key says."""
    assert set(kw) <= set(SWITCHES), kw
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _assert_distinct(sel, xs, refs):
    """A vacuous comparison must not pass: every reference differs from the field it started
    from, and any two references differ from each other."""
    for no, (x, r) in enumerate(zip(xs, refs), 1):
        assert np.isfinite(r[sel]).all(), no
        assert not np.array_equal(r[sel], x[sel]), no
    for (i, a), (j, b) in itertools.combinations(enumerate(refs, 1), 2):
        assert not np.array_equal(a[sel], b[sel]), (i, j)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _eq(a, b, what):
    assert a.shape == b.shape, what
    assert np.array_equal(a, b), (what, float(np.abs(a - b).max()), int((a != b).sum()))


def _names(n):
    return ["pTracer%02d" % no for no in range(1, n + 1)]


# ---- A: the march forms on the synthetic LLC -------------------------------------------------
# launch_tracer_step (csrc/kernels_thermo.hip) with a passive tracer's TracerArgs: c' in the
# tracer's adv1, T* in its scr, the pair in the tracers' own arena.  Which shape selects which
# form: test_gpu_shapes_step.py, "the synthetic LLC".
LLC_DEEP = (14, 31, 7, 4)    # nx = 15 odd: the one-column k_tracer_march, by default (Nr >= 30), and k_tracer_impl<true>
LLC_EVEN = (12, 4, 6, 2)     # sNx, OLx, nx, n3 all even: the 16-byte pair forms
LLC_TRACERS = (dict(advScheme=2, diffKr=3e-5), dict(advScheme=2, diffKr=2e-5))   # (salt's diffKrS is 1e-5)
MARCH_OFF = (("MGCM_TRACER_MARCH", "0"), ("MGCM_TRACER_MARCH2", None))
DEFAULTS = (("MGCM_TRACER_MARCH", None), ("MGCM_TRACER_MARCH2", None))
# MGCM_TRACER_MARCH, MGCM_TRACER_MARCH2 -> the form reached on LLC_EVEN
EVEN_FORMS = {"chunked_pairs": ("1", None),     # k_tracer_march2<false, false> in level chunks + k_tracer_impl<false>
              "fwd_backsub": ("2", None),       # k_tracer_march2<true, false> + k_tracer_backsub
              "fwd_flat": ("3", None),          # k_tracer_march2<true, true>, pairs dealt over the workgroups
              "fwd_rows": ("3", "1"),           # k_tracer_march2<true, true>, whole tile rows per workgroup
              "one_column": ("3", "0")}         # k_tracer_march + k_tracer_impl<false>
LLC_FIELDS = ("theta", "uVel", "etaN", "salt")


@functools.lru_cache(maxsize=None)
def _llc_base(case):
    from mitgcm_amd import configs
    n, Nr, tile, OL = case
    return configs.llc_synthetic(n=n, Nr=Nr, tile=tile, OL=OL)


def _llc_cfg(case, salt=None, **over):
    """configs.llc_synthetic with salt passive (sBeta = 0, saltForcing = 0); salt: the initial
    salt instead of the configuration's."""
    def cfg():
        g, params, state = _llc_base(case)
        params, state = dict(params), dict(state)
        params.update(sBeta=0.0, saltForcing=0)
        params.update(over)
        if salt is not None:
            state["salt"] = salt
        return g, params, state
    return cfg


@functools.lru_cache(maxsize=None)
def _llc_reference(case):
    """Per tracer a 4-step oracle run with salt := X and diffKrS := the tracer's diffKr."""
    from oracle.harness import oracle_from_config
    g = _llc_base(case)[0]
    plan = _sum_plan(_llc_cfg(case))
    rng = np.random.default_rng(1000 * case[0] + case[1])
    xs = [_wet_random(g, rng) for _ in LLC_TRACERS]
    out = []
    for sp, x in zip(LLC_TRACERS, xs):
        o, _ = oracle_from_config(_llc_cfg(case, diffKrS=sp["diffKr"]))
        _device_order(o, plan)
        o.arr("salt")[:] = x
        for _ in range(4):
            o.forward_step()
        out.append(np.array(o.arr("salt")))
    _assert_distinct(_inner(g), xs, out)
    _frozen(*(xs + out))
    return g, xs, out


@functools.lru_cache(maxsize=None)
def _llc_plain(case, march):
    """Device models without passive tracers under the switches `march`, 4 steps in one call: the
    plain configuration, and per tracer the twin whose salt := X and diffKrS := the tracer's."""
    from mitgcm_amd import configs
    g, xs, _ = _llc_reference(case)
    with _env(**dict(march)):
        m = configs.make_model(_llc_cfg(case))
        m.forward_step(4)
        res = {n: m.get(n) for n in LLC_FIELDS}
        m.close()
        for no, (sp, x) in enumerate(zip(LLC_TRACERS, xs), 1):
            m = configs.make_model(_llc_cfg(case, salt=x, diffKrS=sp["diffKr"]))
            m.forward_step(4)
            res["twin%02d" % no] = m.get("salt")
            m.close()
    return res


@functools.lru_cache(maxsize=None)
def _llc_device(case, march, batch):
    from mitgcm_amd import configs
    g, xs, _ = _llc_reference(case)
    with _env(MGCM_PTR_BATCH=batch, **dict(march)):
        m = configs.make_model(_llc_cfg(case), ptracers=[dict(sp, init=x) for sp, x in zip(LLC_TRACERS, xs)])
        m.forward_step(4)
        res = {n: m.get(n) for n in LLC_FIELDS + tuple(_names(len(xs)))}
        m.close()
    return res


def _check_llc(case, march, batch):
    g, xs, ref = _llc_reference(case)
    dev, base = _llc_device(case, march, batch), _llc_plain(case, march)
    inner = _inner(g)
    for no, (name, salt) in enumerate(zip(_names(len(xs)), ref), 1):
        _eq(dev[name][inner], salt[inner], (name, "oracle"))
        _eq(dev[name], base["twin%02d" % no], (name, "a model whose salt is the tracer"))   # halos included
    for n in LLC_FIELDS:
        _eq(dev[n], base[n], (n, "a model without tracers"))
    return dev


@BOTH
def test_llc_deep_default_march_two_tracers(batch):
    """A1.  (14, 31, 7, 4), no switch set: Nr >= 30 turns the march on by itself, nx = 15 is odd,
    so each tracer runs k_tracer_march in level chunks (KC = 7: 7, 7, 7, 7, 3) and then
    k_tracer_impl<true>.  MGCM_PTR_BATCH is inert with a march on (ptr_batch_ok): both values
    meet the same references on the full arrays, hence each other."""
    dev, other = _check_llc(LLC_DEEP, DEFAULTS, batch), _llc_device(LLC_DEEP, DEFAULTS, 1 - batch)
    for name in _names(len(LLC_TRACERS)):
        _eq(dev[name], other[name], (name, "MGCM_PTR_BATCH=%d" % (1 - batch)))


@pytest.mark.parametrize("form", list(EVEN_FORMS))
def test_llc_even_march_forms_two_tracers(form):
    """A2.  (12, 4, 6, 2): the pair forms, each against the oracle, the salt twins and the plain
    model run under the same switches, and against the flat kernel's tracers
    (MGCM_TRACER_MARCH = 0): the forms are bit-identical restatements of it."""
    march = tuple(zip(("MGCM_TRACER_MARCH", "MGCM_TRACER_MARCH2"), EVEN_FORMS[form]))
    dev = _check_llc(LLC_EVEN, march, 0)
    flat = _check_llc(LLC_EVEN, MARCH_OFF, 0)
    for name in _names(len(LLC_TRACERS)):
        _eq(dev[name], flat[name], (name, "MGCM_TRACER_MARCH=0"))


LLC_STATE = tuple(n for n in LATLON_STATE if n not in ("uVelD", "vVelD", "uNM1", "vNM1"))   # (no CD scheme on the LLC)
LLC_RELAX = dict(advScheme=2, diffKr=4e-5, surfRelaxTau=864000.0, surfRelaxVal=2.0)


@functools.lru_cache(maxsize=None)
def _llc_forced_reference():
    """test_gpu_ptracers.py's _latlon_reference on (14, 31, 7, 4): two oracle steps,
    DO_OCEANIC_PHYS, then THERMODYNAMICS with salt := X twice, with the relaxation's
    surfaceForcingS and without it."""
    from oracle.harness import oracle_from_config
    o, g = oracle_from_config(_llc_cfg(LLC_DEEP))
    for _ in range(2):
        o.forward_step()
    state = {n: np.array(o.arr(n)) for n in LLC_STATE}
    myIter = o.get("myIter")
    o.L.oracle_oceanic_phys(o.h)
    keep = {n: np.array(o.arr(n)) for n in ("theta", "salt", "gtNm1", "gsNm1", "surfaceForcingS")}
    x = _wet_random(g, np.random.default_rng(1431))
    sp, out = LLC_RELAX, {}
    for forced in (True, False):
        for n, v in keep.items():
            o.arr(n)[:] = v
        o.arr("salt")[:] = x
        o.set(diffKrS=sp["diffKr"], saltForcing=0)
        if forced:
            sf = (((1.0 / sp["surfRelaxTau"]) * (sp["surfRelaxVal"] - x[:, 0])) * g.f["drF"][0]) * g.f["hFacC"][:, 0]
            o.arr("surfaceForcingS")[:] = sf
            o.set(saltForcing=1)
        o.L.oracle_thermodynamics(o.h)
        out[forced] = np.array(o.arr("salt"))
    theta = np.array(o.arr("theta"))
    inner = _inner(g)
    _assert_distinct(inner, [x, x], [out[True], out[False]])
    assert not np.array_equal(out[True][:, 0][inner], out[False][:, 0][inner])
    assert not np.array_equal(theta[inner], keep["theta"][inner])
    return g, state, myIter, keep["gsNm1"], x, out, theta


def test_llc_deep_forced_tracer_per_call():
    """A3.  A surface-relaxed tracer at Nr = 31 takes the generic k_tracer_rhs<false, true> and
    then k_tracer_impl<true>; its unforced twin in the same model (same X, same diffKr) takes
    k_tracer_march.  One THERMODYNAMICS call from the oracle's state, both against the oracle."""
    from mitgcm_amd import configs
    from mitgcm_amd._lib import lib
    g, state, myIter, gs0, x, ref, theta = _llc_forced_reference()
    free = {k: v for k, v in LLC_RELAX.items() if not k.startswith("surfRelax")}
    with _env(MGCM_PTR_BATCH=None, **dict(DEFAULTS)):
        m = configs.make_model(_llc_cfg(LLC_DEEP), ptracers=[dict(LLC_RELAX, init=x), dict(free, init=x)])
        for n, v in state.items():
            m.put(n, v)
        lib().mgcm_set_param(m.h, b"myIter", float(myIter))
        for no in (1, 2):
            m.put("gpTrNm1_%02d" % no, gs0)
        m.thermodynamics()
        forced, unforced, th = m.get("pTracer01"), m.get("pTracer02"), m.get("theta")
        assert m.ptracer_param(1, "surfRelaxTau") == 864000.0 and m.ptracer_param(2, "surfRelaxTau") == 0.0
        m.close()
    inner = _inner(g)
    _eq(th[inner], theta[inner], "theta: the call's own state")
    _eq(forced[inner], ref[True][inner], "the relaxed tracer")
    _eq(unforced[inner], ref[False][inner], "the unforced tracer")
    assert not np.array_equal(forced[:, 0][inner], unforced[:, 0][inner])   # the relaxation is seen at the surface


# ---- B: eleven tracers per call on tutorial_global_oce_latlon --------------------------------
# ptr_tables_sync's launch classes: (GM/Redi: 0, without: 3) + (U3 / C4: 0, C2: 1, multi-dimensional: 2).
# List order 1..11 -> launch order 9, 11, 5, 10, 3, 6, 4, 7, 2, 1, 8: tracer 1 in the last class,
# tracer 11 in the first, every class non-empty, useGMRedi on and off in each kind; tracers 9-11
# are the second launch_exchange_multi (MG_XMAX = 8 fields per launch).
def _b(no, advScheme, **kw):
    return dict(advScheme=advScheme, diffKh=100.0 + 50.0 * no, diffKr=(1 + no) * 1e-5, **kw)


LATLON11 = (_b(1, 33, useGMRedi=0), _b(2, 2, useGMRedi=0), _b(3, 30), _b(4, 4, useGMRedi=0), _b(5, 2),
            _b(6, 33, surfRelaxTau=864000.0, surfRelaxVal=2.0), _b(7, 3, useGMRedi=0), _b(8, 30, useGMRedi=0), _b(9, 4),
            _b(10, 2), _b(11, 3))
LATLON11_ORDER = (9, 11, 5, 10, 3, 6, 4, 7, 2, 1, 8)
AB_SCHEMES = (2, 3, 4)


def _launch_class(sp):
    s = sp["advScheme"]
    return (0 if sp.get("useGMRedi", 1) else 3) + (2 if s in (30, 33) else (1 if s == 2 else 0))


def test_latlon11_list_covers_every_launch_class():
    order = sorted(range(1, 12), key=lambda no: (_launch_class(LATLON11[no - 1]), no))
    assert tuple(order) == LATLON11_ORDER
    assert {_launch_class(sp) for sp in LATLON11} == set(range(6))
    assert {sp["advScheme"] for sp in LATLON11} == {2, 3, 4, 30, 33}
    assert len({sp["diffKh"] for sp in LATLON11}) == len({sp["diffKr"] for sp in LATLON11}) == 11
    assert sum(abs(a - b) for a, b in zip(order, range(1, 12))) >= 40   # far from the list's order


@functools.lru_cache(maxsize=None)
def _latlon11_reference():
    """_latlon_reference's pattern with the 11-entry list, two calls: per tracer THERMODYNAMICS
    with salt := X, then again from the exchanged result and its own gsNm1, the rest of the
    state as before the first call.  A tracer with useGMRedi = 0: GM/Redi off in the oracle for
    the THERMODYNAMICS call only (DO_OCEANIC_PHYS and the tensor ran with it on); that this
    changes the oracle's result is asserted here."""
    from oracle.harness import latlon_oracle
    o, g = latlon_oracle()
    for _ in range(3):
        o.forward_step()
    state = {n: np.array(o.arr(n)) for n in LATLON_STATE}
    myIter = o.get("myIter")
    o.L.oracle_fields_load(o.h)
    o.L.oracle_oceanic_phys(o.h)
    keep = {n: np.array(o.arr(n)) for n in ("theta", "salt", "gtNm1", "gsNm1", "surfaceForcingS")}
    assert o.get("useGMRedi") == 1.0
    rng = np.random.default_rng(20261111)
    xs = [_wet_random(g, rng) for _ in LATLON11]
    inner = _inner(g)

    def call(sp, x, gs, gm):
        for n, v in keep.items():
            o.arr(n)[:] = v
        o.arr("salt")[:] = x
        if gs is not None:
            o.arr("gsNm1")[:] = gs
        s = sp["advScheme"]
        o.set(saltAdvScheme=s, saltVertAdvScheme=s, diffKhS=sp["diffKh"], diffKrS=sp["diffKr"], saltForcing=0,
              multiDimAdvection=1, useGMRedi=gm)
        if "surfRelaxTau" in sp:
            sf = (((1.0 / sp["surfRelaxTau"]) * (sp["surfRelaxVal"] - x[:, 0])) * g.f["drF"][0]) * g.f["hFacC"][:, 0]
            o.arr("surfaceForcingS")[:] = sf
            o.set(saltForcing=1)
        o.L.oracle_thermodynamics(o.h)
        o.set(useGMRedi=1)
        return np.array(o.arr("salt")), np.array(o.arr("gsNm1"))
    first, second = [], []
    for sp, x in zip(LATLON11, xs):
        gm = int(sp.get("useGMRedi", 1))
        r1 = call(sp, x, None, gm)
        if not gm:
            assert not np.array_equal(call(sp, x, None, 1)[0][inner], r1[0][inner]), sp
        first.append(r1)
        second.append(call(sp, _exch3(g, r1[0]), r1[1], gm))
    _assert_distinct(inner, xs, [r[0] for r in first])
    _assert_distinct(inner, [r[0] for r in first], [r[0] for r in second])
    ab = [i for i, sp in enumerate(LATLON11) if sp["advScheme"] in AB_SCHEMES]
    _assert_distinct(inner, [keep["gsNm1"]] * len(ab), [first[i][1] for i in ab])
    _assert_distinct(inner, [first[i][1] for i in ab], [second[i][1] for i in ab])
    return g, state, myIter, keep["gsNm1"], xs, first, second


LATLON_STEPPED = ("theta", "salt", "gtNm1", "gsNm1")


@functools.lru_cache(maxsize=None)
def _latlon11_device(batch):
    """Two THERMODYNAMICS calls on one model (ptrFlip 0, then 1: both parity tables of the
    batched route, outside a graph).  Before the second call theta, salt and their histories are
    put back, so that DO_OCEANIC_PHYS repeats the first call's and only the passive tracers go
    on from their own results, as in the reference."""
    g, state, myIter, gs0, xs, _, _ = _latlon11_reference()
    with _env(MGCM_PTR_BATCH=batch):
        m = _latlon_model(state, myIter, [dict(sp, init=x) for sp, x in zip(LATLON11, xs)])
        plain = _latlon_model(state, myIter, None)
        for no, sp in enumerate(LATLON11, 1):
            if sp["advScheme"] in AB_SCHEMES:
                m.put("gpTrNm1_%02d" % no, gs0)
        calls = []
        for c in range(2):
            if c:
                for n in LATLON_STEPPED:
                    m.put(n, state[n])
                    plain.put(n, state[n])
            m.thermodynamics()
            plain.thermodynamics()
            res = {n: m.get(n) for n in _names(11)}
            res.update({"gpTrNm1_%02d" % no: m.get("gpTrNm1_%02d" % no) for no in range(1, 12)})
            res.update({n: m.get(n) for n in LATLON_STEPPED})
            res.update({"plain_" + n: plain.get(n) for n in LATLON_STEPPED})
            calls.append(res)
        m.close()
        plain.close()
    return calls


@BOTH
@pytest.mark.parametrize("call", [0, 1], ids=["first_call", "second_call"])
def test_latlon11_per_call_bitexact(call, batch):
    g, state, myIter, gs0, xs, first, second = _latlon11_reference()
    res, ref = _latlon11_device(batch)[call], (first, second)[call]
    inner = _inner(g)
    for no, (sp, (salt, gs)) in enumerate(zip(LATLON11, ref), 1):
        dev = res["pTracer%02d" % no]
        _eq(dev[inner], salt[inner], (no, sp["advScheme"], "oracle"))
        if sp["advScheme"] in AB_SCHEMES:
            _eq(res["gpTrNm1_%02d" % no][inner], gs[inner], (no, "gpTrNm1 against the oracle's gsNm1"))
        _eq(dev, _exch3(g, dev), (no, "halos: the exchange of the interior"))
    for n in LATLON_STEPPED:
        _eq(res[n], res["plain_" + n], (n, "a model without tracers"))
        assert not np.array_equal(res[n][inner], state[n][inner]), n


@pytest.mark.parametrize("call", [0, 1], ids=["first_call", "second_call"])
def test_latlon11_batch_equals_functional(call):
    a, b = _latlon11_device(0)[call], _latlon11_device(1)[call]
    for n in sorted(a):
        _eq(a[n], b[n], n)   # full arrays


# ---- C: nine tracers over 4 + 1 steps on ragged gyre tilings ----------------------------------
# (2, 31): tiles of 31 x 2 points; (62, 1): tiles of 1 x 62, narrower than the halo of 2.  Nine is
# the first count past MG_XMAX: tracer 9 is the second exchange launch of every step.
GYRE9 = tuple(dict(advScheme=(33, 2, 3)[i % 3], diffKh=150.0 + 100.0 * i, diffKr=(1.5 + i) * 1e-5) for i in range(9))
GYRE9_TILINGS = [(2, 31), (62, 1)]
GYRE_FIELDS = ("theta", "uVel", "etaN")


def _gyre_salt_cfg(nSx, nSy, sp):
    s = sp["advScheme"]
    return _gyre_cfg(nSx, nSy, saltStepping=1, saltAdvection=1, saltForcing=0, saltAdvScheme=s, saltVertAdvScheme=s,
                     diffKhS=sp.get("diffKh", 0.0), diffKrS=sp.get("diffKr", 0.0))


@functools.lru_cache(maxsize=None)
def _gyre9_reference(nSx, nSy):
    from oracle.harness import oracle_from_config
    g = _gyre_cfg(nSx, nSy)()[0]
    plan = _sum_plan(_gyre_cfg(nSx, nSy))
    rng = np.random.default_rng(900 + 100 * nSx + nSy)
    xs = [_wet_random(g, rng) for _ in GYRE9]
    out = []
    for sp, x in zip(GYRE9, xs):
        o, _ = oracle_from_config(_gyre_salt_cfg(nSx, nSy, sp))
        _device_order(o, plan)
        o.arr("salt")[:] = x
        for _ in range(5):
            o.forward_step()
        out.append(np.array(o.arr("salt")))
    _assert_distinct(_inner(g), xs, out)
    _frozen(*(xs + out))
    return g, xs, out


@functools.lru_cache(maxsize=None)
def _gyre9_plain(nSx, nSy):
    from mitgcm_amd import configs
    m = configs.make_model(_gyre_cfg(nSx, nSy))
    m.forward_step(4)
    m.forward_step(1)
    res = {n: m.get(n) for n in GYRE_FIELDS}
    m.close()
    return res


@BOTH
@pytest.mark.parametrize("tiles", GYRE9_TILINGS, ids=["%dx%d" % t for t in GYRE9_TILINGS])
def test_gyre_nine_tracers_ragged_tilings(tiles, batch):
    from mitgcm_amd import configs
    from mitgcm_amd._lib import lib
    g, xs, ref = _gyre9_reference(*tiles)
    cfg = _gyre_cfg(*tiles)
    specs = [dict(sp, init=x) for sp, x in zip(GYRE9, xs)]
    with _env(MGCM_PTR_BATCH=batch):
        m = configs.make_model(cfg, ptracers=specs)
        single = configs.make_model(cfg, ptracers=specs)
        m.forward_step(4)
        m.forward_step(1)
        for _ in range(5):
            single.forward_step(1)
        dev = {n: m.get(n) for n in GYRE_FIELDS + tuple(_names(9))}
        one = {n: single.get(n) for n in _names(9)}
        parity = lib().mgcm_tracer_parity(m.h, -1), lib().mgcm_tracer_parity(single.h, -1)
        m.close()
        single.close()
    for name, salt in zip(_names(9), ref):
        _eq(dev[name], salt, (name, "oracle"))   # exchanged halos included
        _eq(dev[name], one[name], (name, "single steps"))
    plain = _gyre9_plain(*tiles)
    for n in GYRE_FIELDS:
        _eq(dev[n], plain[n], (n, "a model without tracers"))
    assert parity[0] == parity[1] and parity[0] & 4, parity   # 5 steps: the tracers' pairs are flipped


# ---- D: OL = 3, r*, the fold, re-tiled --------------------------------------------------------
OCEAN90_TILINGS = [(5, 5), (18, 8)]   # tiles of 18 x 8 and of 5 x 5 points


def _ocean90_cfg(nSx, nSy):
    from mitgcm_amd import configs
    return lambda: configs.global_ocean_90x40x15(nSx=nSx, nSy=nSy, params_over=OCEAN90_OVER)


@functools.lru_cache(maxsize=None)
def _ocean90_retiled_reference(nSx, nSy):
    """test_gpu_ptracers.py's _ocean90_reference at another tiling: 7 oracle steps per tracer."""
    from oracle.harness import ocean90_oracle
    plan = _sum_plan(_ocean90_cfg(nSx, nSy))
    out, xs = [], None
    for no, sp in enumerate(OCEAN90_TRACERS):
        s = sp["advScheme"]
        o, g = ocean90_oracle(nSx=nSx, nSy=nSy,
                              params_over=dict(OCEAN90_OVER, saltAdvScheme=s, saltVertAdvScheme=s, diffKhS=0.0,
                                               diffKrS=sp["diffKr"], saltForcing=0, multiDimAdvection=1))
        if xs is None:
            rng = np.random.default_rng(9000 + 100 * nSx + nSy)
            xs = [_wet_random(g, rng) for _ in OCEAN90_TRACERS]
        _device_order(o, plan)
        o.arr("salt")[:] = xs[no]
        for _ in range(7):
            o.forward_step()
        out.append(np.array(o.arr("salt")))
    _assert_distinct(_inner(g), xs, out)
    _frozen(*(xs + out))
    return g, xs, out


@BOTH
@pytest.mark.parametrize("tiles", OCEAN90_TILINGS, ids=["%dx%d" % t for t in OCEAN90_TILINGS])
def test_ocean90_retiled_rstar_fold(tiles, batch):
    """test_ocean90_rstar_fold_and_pipelined_step's 6 + 1 steps (the default, pipelined step
    plan) on OL = 3 tiles of 18 x 8 and 5 x 5 points."""
    from mitgcm_amd import configs
    g, xs, ref = _ocean90_retiled_reference(*tiles)
    with _env(MGCM_PTR_BATCH=batch, MGCM_OVERLAP=1):   # (no timing-dependent choice of the layout)
        m = configs.make_model(_ocean90_cfg(*tiles), ptracers=[dict(sp, init=x) for sp, x in zip(OCEAN90_TRACERS, xs)])
        m.put("gpTrNm1_02", m.get("gsNm1"))   # the stand-in's AB2 history is the pickup's GsNm1
        m.forward_step(6)
        m.forward_step(1)
        dev = [m.get(n) for n in _names(2)]
        m.close()
    inner = _inner(g)
    for no, (d, salt) in enumerate(zip(dev, ref), 1):
        _eq(d[inner], salt[inner], (no, "oracle"))


# ---- E: mgcm_ptracer_param on a stepped model -------------------------------------------------
PARAM_CHANGES = {2: ("diffKr", "diffKrS", 5e-5), 3: ("diffKh", "diffKhS", 250.0)}   # tracer -> its name, salt's, the new value


@functools.lru_cache(maxsize=None)
def _gyre_param_reference():
    """Gyre (2, 2), GYRE_TRACERS, 6 oracle steps per tracer with salt := X: unchanged, and with
    the changed diffusivity set after step 3."""
    from oracle.harness import oracle_from_config
    g = _gyre_cfg(2, 2)()[0]
    plan = _sum_plan(_gyre_cfg(2, 2))
    rng = np.random.default_rng(606)
    xs = [_wet_random(g, rng) for _ in GYRE_TRACERS]
    changed, unchanged = [], []
    for no, (sp, x) in enumerate(zip(GYRE_TRACERS, xs), 1):
        for change in ((False, True) if no in PARAM_CHANGES else (False,)):
            o, _ = oracle_from_config(_gyre_salt_cfg(2, 2, sp))
            _device_order(o, plan)
            o.arr("salt")[:] = x
            for step in range(6):
                if step == 3 and change:
                    o.set(**{PARAM_CHANGES[no][1]: PARAM_CHANGES[no][2]})
                o.forward_step()
            (changed if change else unchanged).append(np.array(o.arr("salt")))
        if no not in PARAM_CHANGES:
            changed.append(unchanged[-1])
    inner = _inner(g)
    _assert_distinct(inner, xs, changed)
    _assert_distinct(inner, xs, unchanged)
    for no in PARAM_CHANGES:
        assert not np.array_equal(changed[no - 1][inner], unchanged[no - 1][inner]), no
    return g, xs, changed, unchanged


@BOTH
def test_ptracer_param_on_a_stepped_model(batch):
    """mgcm_ptracer_param between two graph-replayed calls: the table is marked stale, the graphs
    are dropped and both parity tables uploaded again before the next step."""
    from mitgcm_amd import configs
    from mitgcm_amd._lib import check, lib
    g, xs, changed, unchanged = _gyre_param_reference()
    specs = [dict(sp, init=x) for sp, x in zip(GYRE_TRACERS, xs)]
    with _env(MGCM_PTR_BATCH=batch):
        m, same = configs.make_model(_gyre_cfg(2, 2), ptracers=specs), configs.make_model(_gyre_cfg(2, 2), ptracers=specs)
        m.forward_step(3)
        for no, (name, _, value) in PARAM_CHANGES.items():
            check(lib().mgcm_ptracer_param(m.h, no, name.encode(), value), "mgcm_ptracer_param")
            assert m.ptracer_param(no, name) == value
        m.forward_step(3)
        same.forward_step(3)
        same.forward_step(3)
        dev, base = [m.get(n) for n in _names(3)], [same.get(n) for n in _names(3)]
        m.close()
        same.close()
    for no in (1, 2, 3):
        _eq(dev[no - 1], changed[no - 1], (no, "the oracle with the parameter changed after step 3"))
        _eq(base[no - 1], unchanged[no - 1], (no, "the oracle, unchanged"))
    for no in PARAM_CHANGES:
        assert not np.array_equal(dev[no - 1][_inner(g)], base[no - 1][_inner(g)]), no
    _eq(dev[0], base[0], "tracer 1: no parameter of its own changed")


# ---- F: cube twins that can see a wrong operand -------------------------------------------------
# test_cube_tracer_equals_salt / test_cube_multidim_tracer_equals_salt's configurations; the
# tracer is a random field with a diffKr that is not salt's, the reference a second model
# without tracers whose salt is that field and whose diffKrS is the tracer's.
CUBE_DST3 = dict(tempAdvScheme=33, tempVertAdvScheme=33, saltAdvScheme=33, saltVertAdvScheme=33, multiDimAdvection=1)
CUBES = {"c2_ol3": (9, 2, 3, {}), "dst3fl_ol4": (12, 2, 4, CUBE_DST3)}
CUBE_DIFFKR = 3e-5


def _cube_cfg(name, salt=None, **over):
    from mitgcm_amd import configs
    n, Nr, OL, scheme = CUBES[name]

    def cfg():
        g, params, state = configs.cube_synthetic(n, Nr, OL=OL, params_over=dict(scheme, sBeta=0.0, saltForcing=0, **over))
        if salt is not None:
            state = dict(state, salt=salt)
        return g, params, state
    return cfg


@functools.lru_cache(maxsize=None)
def _cube_twin(name):
    """The random X, and 2 steps of the model whose salt := X, diffKrS := the tracer's, and of the
    plain model (no passive tracer: MGCM_PTR_BATCH plays no part)."""
    from mitgcm_amd import configs
    g, params, state = _cube_cfg(name)()
    assert params["diffKrS"] != CUBE_DIFFKR
    x = _wet_random(g, np.random.default_rng(600 + CUBES[name][0]))
    assert not np.array_equal(x, state["salt"])
    res = {}
    for key, cfg in (("twin", _cube_cfg(name, salt=x, diffKrS=CUBE_DIFFKR)), ("plain", _cube_cfg(name))):
        m = configs.make_model(cfg)
        m.forward_step(2)
        res[key] = m.get("salt")
        m.close()
    return g, params, x, res


@BOTH
@pytest.mark.parametrize("name", list(CUBES))
def test_cube_random_tracer_equals_its_salt_twin(name, batch):
    from mitgcm_amd import configs
    g, params, x, ref = _cube_twin(name)
    with _env(MGCM_PTR_BATCH=batch):
        m = configs.make_model(_cube_cfg(name), ptracers=[dict(advScheme=params["saltAdvScheme"], diffKh=params["diffKhS"],
                                                               diffKr=CUBE_DIFFKR, init=x)])
        m.forward_step(2)
        tr, salt = m.get("pTracer01"), m.get("salt")
        m.close()
    _eq(tr, ref["twin"], "the tracer against the model whose salt it is")   # full arrays
    _eq(salt, ref["plain"], "salt against a model without tracers")
    inner = _inner(g)
    assert not np.array_equal(tr[inner], x[inner]) and not np.array_equal(tr[inner], salt[inner])
