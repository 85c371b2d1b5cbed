"""pkg/ptracers on the device (model.hip ptracers_on, kernels_ptracers.hip), both routes: one
launch_tracer_step per tracer (MGCM_PTR_BATCH=0, the default) and the batched kernels (=1).

The reference for a passive tracer X is the oracle's SALT with salt := X, saltForcing = 0 and
the tracer's scheme and diffusivities: under a linear EOS with sBeta = 0 salt is passive, so a
whole oracle run is the tracer's run bit for bit; with the non-linear EOS the stand-in holds
per call, for one THERMODYNAMICS after DO_OCEANIC_PHYS ran with the true salt.  Each reference
is computed once per module and shared by the two routes.

Bars: bit-identical wherever the oracle or another device run is the reference; the interior
source against deltaTtracer * source within 1e-12 (below); the 20-step age tracer of
tutorial_global_oce_latlon against the reference's monitor, >= 11 testreport digits on
trcstat max / min / mean / sd, >= 10 on del2."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import digits

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize("batch", [0, 1])
LATLON_STATE = ("uVel", "vVel", "wVel", "theta", "salt", "gtNm1", "gsNm1", "etaN", "etaH", "guNm1", "gvNm1", "etaNm1",
                "uVelD", "vVelD", "uNM1", "vNM1")


def _exch3(g, a):
    return np.stack([g.exch(a[:, k].copy()) for k in range(a.shape[1])], axis=1)


def _wet_random(g, rng):
    """A random field in [1, 6] on the wet cells, 0 on land, halos exchanged."""
    return _exch3(g, (1.0 + 5.0 * rng.random((g.nTiles, g.Nr, g.ny, g.nx))) * (g.f["maskC"] > 0.0))


def _inner(g):
    return (Ellipsis,) + g.sl(1, g.sNx, 1, g.sNy)


def _sum_plan(cfg):
    """The device CG2D's summation order for a configuration (it does not depend on the passive
    tracers): a multi-step oracle run is bit-identical to the device only when its dot products
    are summed in that order (tests/shapes.py assert_bitexact_steps)."""
    from mitgcm_amd import configs
    m = configs.make_model(cfg)
    plan = None if m.cg2d_kernel() == "block_ref" else m.cg2d_sum_plan() + (m.cg2d_fma(),)
    m.close()
    return plan


def _device_order(o, plan):
    if plan is not None:
        o.set_sum_plan(plan[0], plan[1], plan[2], plan[3], fma=plan[4])


# ---- 1, 2: one THERMODYNAMICS call on the lat-lon experiment (JMD95Z, GM/Redi, IVDC, implicit diffusion)
LATLON_TRACERS = (dict(advScheme=33, diffKr=3e-5), dict(advScheme=2, diffKh=300.0), dict(advScheme=3, diffKr=1e-5))
RELAX = dict(advScheme=33, diffKr=3e-5, surfRelaxTau=864000.0, surfRelaxVal=2.0)


@functools.lru_cache(maxsize=None)
def _latlon_reference():
    """Three oracle steps, DO_OCEANIC_PHYS with the true salt, then per tracer the stand-in
    THERMODYNAMICS; returns the uploaded state, the tracers' X and the oracle's results."""
    from oracle.harness import latlon_oracle
    o, g = latlon_oracle()
    for _ in range(3):
        o.forward_step()
    state = {n: np.array(o.arr(n)) for n in LATLON_STATE}
    myIter = o.get("myIter")
    o.L.oracle_fields_load(o.h)
    o.L.oracle_oceanic_phys(o.h)
    keep = {n: np.array(o.arr(n)) for n in ("theta", "salt", "gtNm1", "gsNm1", "surfaceForcingS")}
    rng = np.random.default_rng(20261020)
    xs = [_wet_random(g, rng) for _ in range(4)]
    out = []
    for sp, x in zip(LATLON_TRACERS + (RELAX,), xs):
        for n, v in keep.items():
            o.arr(n)[:] = v
        o.arr("salt")[:] = x
        s = sp["advScheme"]
        o.set(saltAdvScheme=s, saltVertAdvScheme=s, diffKhS=sp.get("diffKh", 0.0), diffKrS=sp.get("diffKr", 0.0),
              saltForcing=0, multiDimAdvection=1)
        if "surfRelaxTau" in sp:
            # surfaceForcingPTr = (((1/tau) * (val - pTracer(k=1))) * drF(1)) * hFacC(k=1), left to right
            sf = (((1.0 / sp["surfRelaxTau"]) * (sp["surfRelaxVal"] - x[:, 0])) * g.f["drF"][0]) * g.f["hFacC"][:, 0]
            o.arr("surfaceForcingS")[:] = sf
            o.set(saltForcing=1)
        o.L.oracle_thermodynamics(o.h)
        out.append((np.array(o.arr("salt")), np.array(o.arr("gsNm1"))))
    return g, state, myIter, keep["gsNm1"], xs, out


def _latlon_model(state, myIter, ptracers):
    from mitgcm_amd import configs
    from mitgcm_amd._lib import lib
    m = configs.make_model(configs.global_oce_latlon, ptracers=ptracers)
    for n, v in state.items():
        m.put(n, v)
    lib().mgcm_set_param(m.h, b"myIter", float(myIter))
    return m


@BOTH
def test_latlon_three_tracers_per_call_bitexact(batch, monkeypatch):
    monkeypatch.setenv("MGCM_PTR_BATCH", str(batch))
    g, state, myIter, gs0, xs, ref = _latlon_reference()
    specs = [dict(sp, init=x) for sp, x in zip(LATLON_TRACERS, xs)]
    m = _latlon_model(state, myIter, specs)
    plain = _latlon_model(state, myIter, None)
    for no in (1, 2, 3):
        m.put("gpTrNm1_%02d" % no, gs0)
    m.thermodynamics()
    plain.thermodynamics()
    inner = _inner(g)
    for no, (salt, gs) in enumerate(ref[:3], 1):
        dev = m.get("pTracer%02d" % no)
        assert np.array_equal(dev[inner], salt[inner]), (no, np.abs(dev[inner] - salt[inner]).max())
        assert not np.array_equal(dev[inner], xs[no - 1][inner])
        if LATLON_TRACERS[no - 1]["advScheme"] in (2, 3, 4):
            assert np.array_equal(m.get("gpTrNm1_%02d" % no)[inner], gs[inner]), no
    for n in ("theta", "salt", "gtNm1", "gsNm1"):
        assert np.array_equal(m.get(n), plain.get(n)), n
    m.close()
    plain.close()


@BOTH
def test_latlon_surface_relaxation_bitexact(batch, monkeypatch):
    monkeypatch.setenv("MGCM_PTR_BATCH", str(batch))
    g, state, myIter, gs0, xs, ref = _latlon_reference()
    m = _latlon_model(state, myIter, [dict(RELAX, init=xs[3])])
    m.thermodynamics()
    inner = _inner(g)
    dev, salt = m.get("pTracer01"), ref[3][0]
    assert np.array_equal(dev[inner], salt[inner]), np.abs(dev[inner] - salt[inner]).max()
    # (the relaxation is seen: the surface level differs from the unforced tracer's, ref[0], same scheme)
    assert m.ptracer_param(1, "surfRelaxTau") == 864000.0
    m.close()


# ---- 2b: PTRACERS_useGMRedi off for some tracers of a GM/Redi model (the mixed batch: two rhs launches)
MIXED = (dict(advScheme=33, diffKr=3e-5), dict(advScheme=2, diffKh=300.0, useGMRedi=0),
         dict(advScheme=33, diffKr=3e-5, useGMRedi=0), dict(advScheme=3, diffKr=1e-5))


def test_latlon_mixed_gmredi_batch_equals_functional(monkeypatch):
    """Four tracers, two of them without GM/Redi, one THERMODYNAMICS call: the batched route
    (k_ptr_rhs<true> on two, k_ptr_rhs<false> on two, one k_ptr_impl) against one
    launch_tracer_step per tracer, device against device, bit-identical.  Tracers 1 and 3 differ
    only in the switch and start from the same field: their results must differ (the switch is
    read), and tracer 1 must be the all-GM/Redi batch's tracer 1, the oracle-checked one."""
    g, state, myIter, gs0, xs, ref = _latlon_reference()
    specs = [dict(sp, init=xs[i]) for sp, i in zip(MIXED, (0, 1, 0, 2))]
    res = {}
    for batch in (0, 1):
        monkeypatch.setenv("MGCM_PTR_BATCH", str(batch))
        m = _latlon_model(state, myIter, specs)
        for no in (2, 4):
            m.put("gpTrNm1_%02d" % no, gs0)
        m.thermodynamics()
        res[batch] = [m.get("pTracer%02d" % no) for no in (1, 2, 3, 4)] + [m.get("gpTrNm1_02"), m.get("gpTrNm1_04")]
        assert m.ptracer_param(2, "useGMRedi") == 0.0 and m.ptracer_param(1, "useGMRedi") == -1.0
        m.close()
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b), np.abs(a - b).max()
    inner = _inner(g)
    assert np.array_equal(res[1][0][inner], ref[0][0][inner])
    assert not np.array_equal(res[1][0][inner], res[1][2][inner])
    assert np.array_equal(res[1][3][inner], ref[2][0][inner])   # scheme 3 with GM/Redi: the oracle's


# ---- 3: the interior source (explicit vertical diffusion, so one call shows the tendency itself)
def _gyre_cfg(nSx=2, nSy=2, **over):
    from mitgcm_amd import configs

    def cfg():
        g, params, state = configs.baroclinic_gyre(nSx=nSx, nSy=nSy, tempAdvScheme=33)
        params.update(multiDimAdvection=1)
        params.update(over)
        return g, params, state
    return cfg


@BOTH
def test_interior_source(batch, monkeypatch):
    """With and without interiorSource = 1e-3: no difference at k = 1 and on land, deltaTtracer *
    1e-3 = 1.2 elsewhere.  Values stay <= 10, so each of the two results is rounded by at most
    ~1e-15 and the increment itself by less; the bound is 300 times that."""
    from mitgcm_amd import configs
    monkeypatch.setenv("MGCM_PTR_BATCH", str(batch))
    cfg = _gyre_cfg(implicitDiffusion=0, ivdc_kappa=0.0)
    g = cfg()[0]
    x = _wet_random(g, np.random.default_rng(3))
    res = []
    for src in (0.0, 1e-3):
        m = configs.make_model(cfg, ptracers=[dict(advScheme=33, diffKr=1e-5, interiorSource=src, init=x)])
        m.thermodynamics()
        res.append(m.get("pTracer01")[_inner(g)])
        m.close()
    diff = res[1] - res[0]
    wet = g.f["maskC"][_inner(g)] > 0.0
    assert np.abs(res[1]).max() <= 10.0
    assert np.array_equal(diff[:, 0], np.zeros_like(diff[:, 0]))
    assert np.array_equal(diff[~wet], np.zeros_like(diff[~wet]))
    below = wet.copy()
    below[:, 0] = False
    assert below.sum() > 1000
    assert np.abs(diff[below] - 1200.0 * 1e-3).max() <= 1e-12, np.abs(diff[below] - 1.2).max()


# ---- 4: multi-step, graphs and parity on the gyre (linear EOS, sBeta = 0: salt is passive)
GYRE_TRACERS = (dict(advScheme=33, diffKr=1e-5), dict(advScheme=2, diffKh=1000.0, diffKr=1e-5),
                dict(advScheme=3, diffKh=500.0, diffKr=2e-5))


@functools.lru_cache(maxsize=None)
def _gyre_reference(nSx, nSy):
    """Per tracer an oracle run of 10 steps with salt := X (CG2D summed in the device's order);
    tracer 2 is replaced after step 4."""
    from oracle.harness import oracle_from_config
    g = _gyre_cfg(nSx, nSy)()[0]
    plan = _sum_plan(_gyre_cfg(nSx, nSy))
    rng = np.random.default_rng(100 * nSx + nSy)
    xs = [_wet_random(g, rng) for _ in range(3)]
    x2b = _wet_random(g, rng)
    out = []
    for no, (sp, x) in enumerate(zip(GYRE_TRACERS, xs), 1):
        s = sp["advScheme"]
        o, _ = oracle_from_config(_gyre_cfg(nSx, nSy, saltStepping=1, saltAdvection=1, saltForcing=0, saltAdvScheme=s,
                                            saltVertAdvScheme=s, diffKhS=sp.get("diffKh", 0.0), diffKrS=sp.get("diffKr", 0.0)))
        _device_order(o, plan)
        o.arr("salt")[:] = x
        for step in range(10):
            if step == 4 and no == 2:
                o.arr("salt")[:] = x2b
            o.forward_step()
        out.append(np.array(o.arr("salt")))
    return g, xs, x2b, out


@BOTH
@pytest.mark.parametrize("tiles", [(2, 2), (31, 2)])
def test_gyre_multi_step_graphs_and_parity(tiles, batch, monkeypatch):
    from mitgcm_amd import configs
    from mitgcm_amd._lib import lib
    monkeypatch.setenv("MGCM_PTR_BATCH", str(batch))
    g, xs, x2b, ref = _gyre_reference(*tiles)
    cfg = _gyre_cfg(*tiles)
    m = configs.make_model(cfg, ptracers=[dict(sp, init=x) for sp, x in zip(GYRE_TRACERS, xs)])
    plain = configs.make_model(cfg)
    single = configs.make_model(cfg, ptracers=[dict(sp, init=x) for sp, x in zip(GYRE_TRACERS, xs)])
    m.forward_step(4)
    m.put("pTracer02", x2b)
    m.forward_step(3)
    for _ in range(3):
        m.forward_step(1)
    plain.forward_step(4)
    plain.forward_step(3)
    for _ in range(3):
        plain.forward_step(1)
    for step in range(10):
        if step == 4:
            single.put("pTracer02", x2b)
        single.forward_step(1)
    for no, salt in enumerate(ref, 1):
        dev = m.get("pTracer%02d" % no)
        assert np.array_equal(dev, salt), (no, np.abs(dev - salt).max())   # exchanged halos included
    for n in ("theta", "uVel", "etaN"):
        assert np.array_equal(m.get(n), plain.get(n)), n
    # the parity bits are those a run of single steps leaves (10 steps: every pair back where it started)
    assert lib().mgcm_tracer_parity(m.h, -1) == lib().mgcm_tracer_parity(single.h, -1)
    m.prepare()
    assert lib().mgcm_tracer_parity(m.h, -1) == lib().mgcm_tracer_parity(single.h, -1)
    m.forward_step(3)
    for _ in range(3):
        single.forward_step(1)
    assert lib().mgcm_tracer_parity(m.h, -1) == lib().mgcm_tracer_parity(single.h, -1)
    assert lib().mgcm_tracer_parity(m.h, -1) & 4
    for no in (1, 2, 3):
        assert np.array_equal(m.get("pTracer%02d" % no), single.get("pTracer%02d" % no)), no
    for x in (m, plain, single):
        x.close()


# ---- 5: r*, the fold and the pipelined step on BASELINE config 2 with a linear EOS
OCEAN90_OVER = dict(eosType=0, tAlpha=2e-4, sBeta=0.0, rhoNil=1035.0)
OCEAN90_TRACERS = (dict(advScheme=33, diffKr=3e-5), dict(advScheme=2, diffKr=3e-5))


@functools.lru_cache(maxsize=None)
def _ocean90_reference():
    from mitgcm_amd import configs
    from oracle.harness import ocean90_oracle
    plan = _sum_plan(lambda: configs.global_ocean_90x40x15(params_over=OCEAN90_OVER))
    out, xs = [], None
    for no, sp in enumerate(OCEAN90_TRACERS):
        s = sp["advScheme"]
        o, g = ocean90_oracle(params_over=dict(OCEAN90_OVER, saltAdvScheme=s, saltVertAdvScheme=s, diffKhS=0.0,
                                               diffKrS=sp["diffKr"], saltForcing=0, multiDimAdvection=1))
        if xs is None:
            rng = np.random.default_rng(90)
            xs = [_wet_random(g, rng) for _ in OCEAN90_TRACERS]
        _device_order(o, plan)
        o.arr("salt")[:] = xs[no]
        for _ in range(7):
            o.forward_step()
        out.append(np.array(o.arr("salt")))
    return g, xs, out


STEP_FUSE_DEFAULT = 1 | 4 | 8 | 128 | 256 | 1024 | 2048 | 4096 | 8192 | 16384 | 32768


@BOTH
@pytest.mark.parametrize("pipe", [True, False])
def test_ocean90_rstar_fold_and_pipelined_step(pipe, batch, monkeypatch):
    from mitgcm_amd import configs
    monkeypatch.setenv("MGCM_PTR_BATCH", str(batch))
    monkeypatch.setenv("MGCM_OVERLAP", "1")   # (no timing-dependent choice of the layout, as test_gpu_step_pipeline.py)
    if not pipe:
        monkeypatch.setenv("MGCM_STEP_FUSE", str(STEP_FUSE_DEFAULT & ~16384))
    g, xs, ref = _ocean90_reference()
    m = configs.make_model(lambda: configs.global_ocean_90x40x15(params_over=OCEAN90_OVER),
                           ptracers=[dict(sp, init=x) for sp, x in zip(OCEAN90_TRACERS, xs)])
    m.put("gpTrNm1_02", m.get("gsNm1"))   # the stand-in's AB2 history is the pickup's GsNm1
    m.forward_step(6)
    lay = m.step_layout()
    assert lay["dyn_thermo_fused"] and lay["pipelined"] == pipe, lay
    m.forward_step(1)
    inner = _inner(g)
    for no, salt in enumerate(ref, 1):
        dev = m.get("pTracer%02d" % no)
        assert np.array_equal(dev[inner], salt[inner]), (no, np.abs(dev[inner] - salt[inner]).max())
    m.close()


# ---- 6: the age tracer of tutorial_global_oce_latlon against the reference's monitor
@BOTH
def test_latlon_age_tracer_20_steps_vs_reference_output(batch, monkeypatch, golden_dir):
    """Measured on MI355X: see DESIGN.md section 4 (the CPU restatement of the same formulas
    gave >= 13.40 digits, worst at trcstat_ptracer01_mean of step 14)."""
    from mitgcm_amd import configs
    from mitgcm_amd.model import dynstat
    monkeypatch.setenv("MGCM_PTR_BATCH", str(batch))
    gold = json.load(open(os.path.join(golden_dir, "tutorial_global_oce_latlon", "monitor.json")))
    m = configs.make_model(configs.global_oce_latlon, ptracers=configs.global_oce_latlon_ptracers())
    worst = {"trc": (99.0, None), "del2": (99.0, None), "check": (99.0, None), "other": (99.0, None)}
    for n in range(1, 21):
        m.forward_step(1)
        r = m.solve_stats()
        gs = gold[n]
        assert r["cg2d_iters"] == gs["cg2d_iters"], (n, r["cg2d_iters"], gs["cg2d_iters"])
        for k, v in m.trcstat().items():
            cls = "del2" if k.endswith("del2") else "trc"
            d = digits(v, gs[k])
            if d < worst[cls][0]:
                worst[cls] = (d, (n, k))
        # the dynstat bars of test_latlon_20_steps_vs_reference_output, in the same run
        r.update(dynstat(m))
        for k, v in r.items():
            if k not in gs or k in ("cg2d_iters", "cg2d_last_res") or k.endswith("_mean"):
                continue
            cls = "check" if (k == "cg2d_init_res" or (k.split("_")[1] in ("uvel", "vvel", "theta", "salt")
                                                       and not k.endswith("del2"))) else "other"
            d = digits(v, gs[k])
            if d < worst[cls][0]:
                worst[cls] = (d, (n, k))
    print("age tracer, 20 steps, MGCM_PTR_BATCH=%d: worst digits trcstat max/min/mean/sd %.2f at %s; del2 %.2f at %s; "
          "dynstat check list %.2f at %s; other %.2f at %s"
          % ((batch,) + worst["trc"] + worst["del2"] + worst["check"] + worst["other"]))
    assert all(w[1] is not None for w in worst.values()), worst   # every class compared something
    assert worst["trc"][0] >= 11.0 and worst["del2"][0] >= 10.0, worst
    assert worst["check"][0] >= 11.0 and worst["other"][0] >= 10.0, worst
    m.close()


# ---- 7: the overlap trial (test_overlap_trial_leaves_the_state_untouched's pattern)
@BOTH
def test_overlap_trial_leaves_the_ptracers_untouched(batch, monkeypatch):
    from mitgcm_amd import configs
    from mitgcm_amd._lib import lib
    monkeypatch.setenv("MGCM_PTR_BATCH", str(batch))
    cfg = _gyre_cfg()
    g = cfg()[0]
    rng = np.random.default_rng(8)
    specs = [dict(sp, init=_wet_random(g, rng)) for sp in GYRE_TRACERS[:2]]
    a, b = configs.make_model(cfg, ptracers=specs), configs.make_model(cfg, ptracers=specs)
    a.forward_step(10)
    for _ in range(10):
        b.forward_step(1)
    assert lib().mgcm_get_param(a.h, b"overlap") in (0.0, 1.0)
    assert lib().mgcm_get_param(b.h, b"overlap") == -1.0   # b never ran a graph batch
    for n in ("pTracer01", "pTracer02", "gpTrNm1_02", "theta", "uVel", "etaN"):
        assert np.array_equal(a.get(n), b.get(n)), n
    a.close()
    b.close()


# ---- 8: restart through pickup_ptracers
GYRE_CARRIED = ("uVel", "vVel", "wVel", "theta", "salt", "guNm1", "gvNm1", "gtNm1", "gsNm1", "etaN", "etaH", "dEtaHdt")


@BOTH
def test_restart_2_plus_2_through_pickup_ptracers(batch, monkeypatch, tmp_path):
    """2 steps, write_pickup (pickup + pickup_ptracers), a new model whose passive tracers and
    their AB2 histories come from pickup_ptracers.0000000002, 2 more steps: bit-identical to 4
    steps.  (The gyre is a cold-start configuration with no pickup reader of its own: the rest
    of its state goes from model to model as downloaded.)"""
    from mitgcm_amd import configs, pickup
    from mitgcm_amd._lib import lib
    monkeypatch.setenv("MGCM_PTR_BATCH", str(batch))
    cfg = _gyre_cfg()
    g = cfg()[0]
    rng = np.random.default_rng(12)
    specs = [dict(advScheme=2, diffKh=1000.0, diffKr=1e-5, init=_wet_random(g, rng)),
             dict(advScheme=33, diffKr=1e-5, init=_wet_random(g, rng))]
    a = configs.make_model(cfg, ptracers=specs)
    a.forward_step(4)
    b = configs.make_model(cfg, ptracers=specs)
    b.forward_step(2)
    assert pickup.write_pickup(b, str(tmp_path), simulation="gyre") == 2
    base = tmp_path / "pickup_ptracers.0000000002"
    meta = open(str(base) + ".meta").read()
    assert "'pTr01   ' 'pTr02   ' 'gPtr01m1'" in meta and "nrecords = [     3 ]" in meta
    carried = {n: b.get(n) for n in GYRE_CARRIED}
    b.close()

    def restart():
        gg, params, state = cfg()
        params.update(nIter0=2)
        state.update(carried)
        return gg, params, state
    c = configs.make_model(restart, ptracers=[{k: v for k, v in sp.items() if k != "init"} for sp in specs])
    lib().mgcm_set_param(c.h, b"myIter", 2.0)
    pickup.load_pickup_ptracers(c, str(tmp_path), 2)
    c.forward_step(2)
    inner = _inner(g)
    for n in ("pTracer01", "pTracer02", "gpTrNm1_01", "theta", "uVel", "etaN"):
        x, y = a.get(n)[inner], c.get(n)[inner]
        assert np.array_equal(x, y), (n, np.abs(x - y).max())
    assert a.my_iter() == c.my_iter() == 4
    a.close()
    c.close()


# ---- 9: what is refused, each with its reason
def _refusal(cfg, specs, match, **kw):
    from mitgcm_amd import configs
    from mitgcm_amd._lib import MgcmError
    with pytest.raises(MgcmError, match=match):
        configs.make_model(cfg, ptracers=specs, **kw).close()


def test_refusals():
    from mitgcm_amd import configs
    from mitgcm_amd._lib import MgcmError, check, lib
    gyre = _gyre_cfg()
    _refusal(gyre, [dict(advScheme=2, EvPrRn=0.0)], "pTracer01: PTRACERS_EvPrRn is not implemented")
    _refusal(gyre, [dict(advScheme=2), dict(advScheme=77)], "pTracer02: advScheme 77 not implemented")
    _refusal(lambda: configs.cube_synthetic(9, 2, OL=3), [dict(advScheme=3)],
             "pTracer01: advection schemes 3 / 4 need OLx, OLy >= 2 and a lat-lon topology")
    _refusal(lambda: configs.cube_synthetic(9, 2, OL=3), [dict(advScheme=4)],
             "pTracer01: advection schemes 3 / 4 need OLx, OLy >= 2 and a lat-lon topology")
    _refusal(configs.advect_xy_ab3_c4, [dict(advScheme=4)], "ADAMS_BASHFORTH3 .useAB3. are not implemented")
    # n > 99 (the C-ABI's own check; Model.add_ptracers refuses the list before it gets there)
    m = configs.make_model(gyre)
    with pytest.raises(MgcmError, match="100 tracers outside 1..99"):
        check(lib().mgcm_ptracers_alloc(m.h, 100), "mgcm_ptracers_alloc")
    with pytest.raises(MgcmError, match="call before mgcm_init"):
        check(lib().mgcm_ptracers_alloc(m.h, 2), "mgcm_ptracers_alloc")
    m.close()
    # a partial tile range, and the tile-sharded driver's phases
    m = configs.make_model(gyre, ptracers=[dict(advScheme=2)])
    with pytest.raises(MgcmError, match="passive tracers are not supported in tile-sharded runs .tile range .0, 2. of 4."):
        check(lib().mgcm_set_tile_range(m.h, 0, 2), "mgcm_set_tile_range")
    with pytest.raises(MgcmError, match="passive tracers are not supported by the tile-sharded driver"):
        check(lib().mgcm_step_phase(m.h, 16), "mgcm_step_phase")
    with pytest.raises(MgcmError, match="unknown parameter diffKz"):
        check(lib().mgcm_ptracer_param(m.h, 1, b"diffKz", 1.0), "mgcm_ptracer_param")
    with pytest.raises(MgcmError, match="unknown field pTracer02"):
        m.get("pTracer02")
    m.forward_step(1)   # ... and the model still steps
    m.close()


# ---- 10: the cube, functional route: the tracer is salt's twin
@BOTH
def test_cube_tracer_equals_salt(batch, monkeypatch):
    """cube_synthetic at the suite's smallest size, linear EOS with sBeta = 0 and saltForcing = 0:
    a tracer that starts as salt with salt's scheme and diffusivities stays bit-identical to it.
    The batched kernels do not apply on the cube: the switch changes nothing."""
    from mitgcm_amd import configs
    monkeypatch.setenv("MGCM_PTR_BATCH", str(batch))
    cfg = lambda: configs.cube_synthetic(9, 2, OL=3, params_over=dict(sBeta=0.0, saltForcing=0))
    g, params, state = cfg()
    m = configs.make_model(cfg, ptracers=[dict(advScheme=params["saltAdvScheme"], diffKh=params["diffKhS"],
                                               diffKr=params["diffKrS"], init=state["salt"])])
    m.forward_step(2)
    salt, tr = m.get("salt"), m.get("pTracer01")
    assert np.array_equal(salt, tr), np.abs(salt - tr).max()
    assert not np.array_equal(salt, state["salt"])
    assert np.array_equal(m.get("gsNm1")[_inner(g)], m.get("gpTrNm1_01")[_inner(g)])
    m.close()


@BOTH
def test_cube_multidim_tracer_equals_salt(batch, monkeypatch):
    """The cube's multi-dimensional passes (k_advg_*) with the tracer's own advScr1 / advScr2 /
    gAdv: cube_synthetic with OL = 4 (GAD_CHECK's overlap for DST3FL on the cube), theta and salt
    on scheme 33, and a scheme-33 tracer that starts as salt: bit-identical to salt after 2 steps."""
    from mitgcm_amd import configs
    monkeypatch.setenv("MGCM_PTR_BATCH", str(batch))
    over = dict(sBeta=0.0, saltForcing=0, tempAdvScheme=33, tempVertAdvScheme=33, saltAdvScheme=33, saltVertAdvScheme=33,
                multiDimAdvection=1)
    cfg = lambda: configs.cube_synthetic(12, 2, OL=4, params_over=over)
    g, params, state = cfg()
    m = configs.make_model(cfg, ptracers=[dict(advScheme=33, diffKh=params["diffKhS"], diffKr=params["diffKrS"],
                                               init=state["salt"])])
    m.forward_step(2)
    salt, tr = m.get("salt"), m.get("pTracer01")
    assert np.array_equal(salt[_inner(g)], tr[_inner(g)]), np.abs(salt - tr)[_inner(g)].max()
    assert np.array_equal(salt, tr)   # the exchanged halos too
    assert not np.array_equal(salt, state["salt"])
    m.close()
