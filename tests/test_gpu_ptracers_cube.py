"""The batched passive-tracer route (MGCM_PTR_BATCH=1) wherever there is no k-march: the cube
sphere and GAD_MULTIDIM_COMPRESSIBLE through k_ptr_advg_plane (kernels_ptracers.hip: every pass
of GAD_ADVECTION's general form for one (tracer, tile, level) in one workgroup, the frame in
LDS), EXCH2 topologies without cube corners through the lat-lon batched kernels.

Every comparison is np.array_equal.  The references are the functional route (one
launch_tracer_step per tracer, the explicit passes k_advg_*, which test_gpu_shapes_cube.py and
test_gpu_advect_cs.py pin to the oracle), a tracer-free model whose salt is the tracer, and the
oracle's theta on verification/advect_cs.  Which route ran is read back (Model.ptracers_route),
so that no comparison is one route against itself.

Shapes: the frame of cube_synthetic(12, ., OL=4) is 20 x 20 = 400 points, ragged over the
workgroup's whole waves (448 lanes by default; over 256, two trips with the second partly idle,
in test_cube_plane_kernel_at_other_workgroup_sizes); 6 x 4 tiles give 14 x 12 frames, smaller
than MG_PLANE_THREADS and not square; 4 x 4 tiles are as wide as the halo and come as
interior, one-edge and corner tiles; n = 9 is odd.  cube_synthetic(57, 2, OL=4) has frames of
65 x 65 x 16 B = 67 600 B, above the 64 KiB the plane kernel may take: the functional route."""
import functools

import numpy as np
import pytest

from test_gpu_ptracers import _gyre_cfg, _inner, _wet_random
from test_gpu_ptracers_sweep import CUBE_DIFFKR, CUBE_DST3, _env, _eq

pytestmark = pytest.mark.gpu

ROUTE = {0: "functional", 1: "batched"}
# scheme 33 with diffKr, scheme 30, scheme 2 with diffKh (Adams-Bashforth: gpTrNm1), scheme 33 with surface relaxation
CUBE_TRACERS = (dict(advScheme=33, diffKr=3e-5), dict(advScheme=30), dict(advScheme=2, diffKh=300.0),
                dict(advScheme=33, diffKr=2e-5, surfRelaxTau=864000.0, surfRelaxVal=2.0))
# GM/Redi in skew form (tutorial_global_oce_latlon's parameters), the list mixing PTRACERS_useGMRedi 1 and 0:
# k_ptr_rhs<true> on tracers 1 and 3, k_ptr_rhs<false> on 2 and 4
GM_SKEW = dict(useGMRedi=1, GM_background_K=1e3, GM_isopycK=1e3, GM_skewflx=1.0, GM_maxSlope=1e-2, GM_Kmin_horiz=50.0)
GM_MIX = (1, 0, 1, 0)
STATE = ("theta", "salt", "etaN")


def _names(specs):
    out = ["pTracer%02d" % no for no in range(1, len(specs) + 1)]
    return out + ["gpTrNm1_%02d" % no for no, sp in enumerate(specs, 1) if sp["advScheme"] in (2, 3, 4)]


def _run(cfg, specs, batch, advance, march=None):
    """A model of cfg with the tracers `specs` under MGCM_PTR_BATCH = batch, advanced by
    advance(m): its tracers (halos included), their Adams-Bashforth histories, STATE, the route."""
    from mitgcm_amd import configs
    with _env(MGCM_PTR_BATCH=batch, MGCM_TRACER_MARCH=march):
        m = configs.make_model(cfg, ptracers=list(specs))
        try:
            advance(m)
            m.sync()
            res = {n: m.get(n) for n in tuple(_names(specs)) + STATE}
            res["route"] = m.ptracers_route()
        finally:
            m.close()
    return res


def _three_single_steps(m):
    for _ in range(3):   # both parities of the step graph, then the first one's replay
        m.forward_step(1)


def _assert_routes_equal(g, specs, res, inits):
    """res[1] ran batched, res[0] functional, and they agree bit for bit; the tracers moved."""
    assert res[1]["route"]["route"] == "batched" and res[0]["route"]["route"] == "functional", (res[1]["route"], res[0]["route"])
    inner = _inner(g)
    for n in _names(specs):
        a, b = res[1][n], res[0][n]
        if n.startswith("gpTrNm1"):
            a, b = a[inner], b[inner]
        _eq(a, b, n)
    for n in STATE:
        _eq(res[1][n], res[0][n], n)
    for no, x in enumerate(inits, 1):
        assert not np.array_equal(res[1]["pTracer%02d" % no][inner], x[inner]), no
    for no in range(2, len(inits) + 1):   # distinct fields in, distinct fields out
        assert not np.array_equal(res[1]["pTracer01"][inner], res[1]["pTracer%02d" % no][inner]), no


# ---- route and launch count ----------------------------------------------------------------------
def _functional_launches(params, specs, cube):
    """What launch_tracer_step issues per tracer without a k-march (kernels_thermo.hip): the general
    GAD_ADVECTION as k_advg_init + passes x 2 directions x (fill, flux, fill, upd; no fills off
    the cube) + k_adv_r, then the right-hand side and, with implicitDiffusion, the solve."""
    n = 0
    for sp in specs:
        if sp["advScheme"] in (30, 33):
            n += 1 + (3 if cube else 2) * 2 * (4 if cube else 2) + 1
        n += 1 + (1 if params["implicitDiffusion"] else 0)
    return n


def test_route_and_launch_count_on_the_cube():
    from mitgcm_amd import configs
    cfg = lambda: configs.cube_synthetic(12, 2, OL=4, params_over=dict(multiDimAdvection=1))
    g, params, state = cfg()
    rng = np.random.default_rng(1202)
    specs = [dict(advScheme=s, diffKr=1e-5, init=_wet_random(g, rng)) for s in (33, 30, 2)]
    res = {b: _run(cfg, specs, b, lambda m: m.thermodynamics()) for b in (1, 0)}
    assert params["implicitDiffusion"] == 1
    expect = _functional_launches(params, specs, cube=True)
    assert expect == 2 * 28 + 2
    print("cube_synthetic(12, 2), tracers on 33 / 30 / 2: batched %r, functional %r" % (res[1]["route"], res[0]["route"]))
    assert res[1]["route"]["route"] == "batched" and res[1]["route"]["launches"] <= 5, res[1]["route"]
    assert res[0]["route"] == {"route": "functional", "launches": expect}, res[0]["route"]
    _assert_routes_equal(g, specs, res, [sp["init"] for sp in specs])


def test_route_none_without_tracers_and_batched_on_the_gyre():
    from mitgcm_amd import configs
    cfg = _gyre_cfg(2, 2)
    g = cfg()[0]
    with _env(MGCM_PTR_BATCH=1):
        plain = configs.make_model(cfg)
        plain.thermodynamics()
        assert plain.ptracers_route() == {"route": "none", "launches": 0}
        plain.close()
    res = _run(cfg, [dict(advScheme=33, diffKr=1e-5, init=_wet_random(g, np.random.default_rng(22)))], 1,
               lambda m: m.thermodynamics())
    # lat-lon: k_ptr_adv_x, _y, _r, k_ptr_rhs<false>, k_ptr_impl, as before
    assert res["route"] == {"route": "batched", "launches": 4 + cfg()[1]["implicitDiffusion"]}, res["route"]


def test_route_functional_with_a_march_on_the_llc():
    """MGCM_TRACER_MARCH=3 on a small llc_synthetic (test_gpu_ptracers_sweep.py's LLC_EVEN): the
    k-march forms keep the functional route whatever the switch says."""
    from mitgcm_amd import configs
    cfg = lambda: configs.llc_synthetic(n=12, Nr=4, tile=6, OL=2)
    g = cfg()[0]
    res = _run(cfg, [dict(advScheme=2, diffKr=3e-5, init=_wet_random(g, np.random.default_rng(124)))], 1,
               lambda m: m.thermodynamics(), march=3)
    assert res["route"]["route"] == "functional", res["route"]


def test_frame_above_the_lds_cap_keeps_the_functional_route():
    from mitgcm_amd import configs
    cfg = lambda: configs.cube_synthetic(57, 2, OL=4, params_over=dict(multiDimAdvection=1))
    g = cfg()[0]
    assert g.nx * g.ny * 16 == 67600 > 64 * 1024
    specs = [dict(advScheme=33, diffKr=3e-5, init=_wet_random(g, np.random.default_rng(57)))]
    res = {b: _run(cfg, specs, b, lambda m: m.thermodynamics()) for b in (1, 0)}
    assert res[1]["route"] == res[0]["route"] and res[1]["route"]["route"] == "functional", (res[1]["route"], res[0]["route"])
    for n in _names(specs):
        _eq(res[1][n], res[0][n], n)
    assert not np.array_equal(res[1]["pTracer01"][_inner(g)], specs[0]["init"][_inner(g)])


# ---- batched equals functional on the cube -------------------------------------------------------
CUBE_TILINGS = {"12x12_nr3": (12, 3, None, None), "6x4": (12, 2, 6, 4), "4x4": (12, 2, 4, 4), "9x9_odd": (9, 2, None, None)}


@pytest.mark.parametrize("tiling", list(CUBE_TILINGS))
def test_cube_batched_equals_functional(tiling):
    from mitgcm_amd import configs
    n, Nr, sNx, sNy = CUBE_TILINGS[tiling]
    cfg = lambda: configs.cube_synthetic(n, Nr, sNx, sNy, OL=4, params_over=dict(multiDimAdvection=1))
    g = cfg()[0]
    rng = np.random.default_rng(1000 * n + 10 * Nr + (sNx or 0))
    specs = [dict(sp, init=_wet_random(g, rng)) for sp in CUBE_TRACERS]
    res = {b: _run(cfg, specs, b, _three_single_steps) for b in (1, 0)}
    assert res[1]["route"]["launches"] == 4, res[1]["route"]   # the plane kernel, k_ptr_adv_r, k_ptr_rhs<false>, k_ptr_impl
    _assert_routes_equal(g, specs, res, [sp["init"] for sp in specs])


@pytest.mark.parametrize("threads", [256, 1024])
def test_cube_plane_kernel_at_other_workgroup_sizes(threads, monkeypatch):
    """MGCM_PTR_PLANE_THREADS, the A/B switch of k_ptr_advg_plane's threads per frame (default: the
    frame's points in whole waves, 512 at most -- 448 for the 400 points here): 256 takes two
    trips over the frame, 1024 leaves ten waves of sixteen idle at every barrier."""
    from mitgcm_amd import configs
    monkeypatch.setenv("MGCM_PTR_PLANE_THREADS", str(threads))
    cfg = lambda: configs.cube_synthetic(12, 3, OL=4, params_over=dict(multiDimAdvection=1))
    g = cfg()[0]
    rng = np.random.default_rng(threads)
    specs = [dict(sp, init=_wet_random(g, rng)) for sp in CUBE_TRACERS[:2]]
    res = {b: _run(cfg, specs, b, lambda m: m.forward_step(2)) for b in (1, 0)}
    _assert_routes_equal(g, specs, res, [sp["init"] for sp in specs])


def test_cube_gmredi_skew_mixed_list_batched_equals_functional():
    """GM/Redi in skew form on the 6 x 4 tiling, tracers 2 and 4 with PTRACERS_useGMRedi = 0: one
    more launch (both k_ptr_rhs), three steps in one call."""
    from mitgcm_amd import configs
    cfg = lambda: configs.cube_synthetic(12, 2, 6, 4, OL=4, params_over=dict(GM_SKEW, multiDimAdvection=1))
    g = cfg()[0]
    rng = np.random.default_rng(6400)
    x = _wet_random(g, rng)
    specs = [dict(sp, useGMRedi=gm, init=(x if no in (0, 3) else _wet_random(g, rng)))
             for no, (sp, gm) in enumerate(zip(CUBE_TRACERS, GM_MIX))]
    res = {b: _run(cfg, specs, b, lambda m: m.forward_step(3)) for b in (1, 0)}
    assert res[1]["route"]["launches"] == 5, res[1]["route"]
    # (tracers 1 and 4 start from one field, scheme 33 both: GM/Redi, diffKr and the relaxation tell them apart)
    _assert_routes_equal(g, specs, res, [sp["init"] for sp in specs])


# ---- a twin that can see a wrong operand ---------------------------------------------------------
def test_cube_batched_random_tracer_equals_its_salt_twin():
    """Sweep F of test_gpu_ptracers_sweep.py on 4 x 4 tiles with the switch on: a random scheme-33
    tracer against a tracer-free model whose salt is that field (sBeta = 0, saltForcing = 0, salt
    on scheme 33 with the tracer's diffKr): the explicit passes.  Two steps, whole arrays."""
    from mitgcm_amd import configs

    def cfg(salt=None, **over):
        def make():
            g, params, state = configs.cube_synthetic(12, 2, 4, 4, OL=4, params_over=dict(CUBE_DST3, sBeta=0.0, saltForcing=0, **over))
            return g, params, (state if salt is None else dict(state, salt=salt))
        return make
    g, params, state = cfg()()
    assert params["diffKrS"] != CUBE_DIFFKR
    x = _wet_random(g, np.random.default_rng(444))
    res = _run(cfg(), [dict(advScheme=33, diffKh=params["diffKhS"], diffKr=CUBE_DIFFKR, init=x)], 1, lambda m: m.forward_step(2))
    assert res["route"]["route"] == "batched", res["route"]
    twin = configs.make_model(cfg(salt=x, diffKrS=CUBE_DIFFKR))
    twin.forward_step(2)
    ref = twin.get("salt")
    twin.close()
    _eq(res["pTracer01"], ref, "the batched tracer against the model whose salt it is")
    inner = _inner(g)
    assert not np.array_equal(ref[inner], x[inner]) and not np.array_equal(res["pTracer01"][inner], res["salt"][inner])


# ---- advect_cs: cube and compressible on the real cs32 metrics -----------------------------------
@functools.lru_cache(maxsize=None)
def _advect_oracle_24():
    from mitgcm_amd import configs
    from oracle.harness import oracle_from_config
    o, g = oracle_from_config(configs.advect_cs)
    for _ in range(24):
        o.forward_step()
    th = np.array(o.arr("theta"))
    th.setflags(write=False)
    return th, g


@pytest.mark.parametrize("tile,steps", [((32, 32), 24), ((8, 8), 6), ((4, 32), 6)], ids=["32x32_24", "8x8_6", "4x32_6"])
def test_advect_cs_tracer_equals_the_oracles_theta(tile, steps):
    """verification/advect_cs steps theta alone (scheme 33, compressible, no diffusion, no
    forcing): a scheme-33 tracer without diffusion that starts as theta is theta's twin, so its
    interior is the oracle's theta bit for bit -- on the functional route (the precondition: the
    reference route alone meets the bar) and on the batched one."""
    from mitgcm_amd import configs
    from test_gpu_shapes_cube import _advect_oracle
    sNx, sNy = tile
    ref, g = _advect_oracle_24() if steps == 24 else _advect_oracle(sNx, sNy)
    out = configs.advect_cs(sNx=sNx, sNy=sNy)
    specs = [dict(advScheme=33, init=out[2]["theta"])]
    inner = _inner(g)
    for batch in (0, 1):
        res = _run(lambda: out, specs, batch, lambda m: m.forward_step(steps))
        assert res["route"]["route"] == ROUTE[batch], res["route"]
        if batch:   # the plane kernel, k_ptr_adv_r<true>, k_ptr_rhs<false>; no implicit diffusion
            assert res["route"]["launches"] == 3, res["route"]
        dev = res["pTracer01"]
        _eq(dev[inner], ref.reshape(dev.shape)[inner], ("the tracer against the oracle's theta", ROUTE[batch]))
        _eq(dev, res["theta"], ("the tracer against the device's theta, halos included", ROUTE[batch]))
        assert not np.array_equal(dev[inner], out[2]["theta"][inner])


# ---- lat-lon compressible ------------------------------------------------------------------------
def test_gyre_compressible_batched_equals_functional():
    """The baroclinic gyre on 2 x 2 tiles with multiDimCompressible = 1: two passes, no corner
    fills, vol carried through them (three LDS arrays)."""
    cfg = _gyre_cfg(2, 2, multiDimCompressible=1)
    g = cfg()[0]
    rng = np.random.default_rng(2233)
    specs = [dict(advScheme=33, diffKr=1e-5, init=_wet_random(g, rng)), dict(advScheme=30, diffKr=2e-5, init=_wet_random(g, rng))]
    res = {b: _run(cfg, specs, b, _three_single_steps) for b in (1, 0)}
    assert res[1]["route"]["launches"] == 3 + cfg()[1]["implicitDiffusion"], res[1]["route"]
    _assert_routes_equal(g, specs, res, [sp["init"] for sp in specs])


# ---- LLC without a march -------------------------------------------------------------------------
def test_llc_without_a_march_batched_equals_functional():
    """llc_synthetic with OL = 4 (GAD_CHECK's overlap for a multi-dimensional scheme on EXCH2) at
    n = 4 in 4 x 4 tiles, as wide as the halo (the smallest mgcm_init accepts), Nr = 3 < 30: no march.  mgcm_set_uv_map sets
    cubeCorners for every EXCH2 topology, so the functional route runs the general form here too
    (k_advg_*: the LLC's facets take the passes of their face numbers, the fills find no cube
    corner to fill where tileEdge has none) and the batched route restates it with the plane
    kernel: k_ptr_advg_plane, k_ptr_adv_r, k_ptr_rhs<false>, k_ptr_impl."""
    from mitgcm_amd import configs
    cfg = lambda: configs.llc_synthetic(n=4, Nr=3, tile=4, OL=4)
    g = cfg()[0]
    rng = np.random.default_rng(843)
    specs = [dict(advScheme=33, diffKr=3e-5, init=_wet_random(g, rng)), dict(advScheme=2, diffKr=2e-5, init=_wet_random(g, rng))]
    res = {b: _run(cfg, specs, b, _three_single_steps) for b in (1, 0)}
    assert res[1]["route"]["launches"] == 4, res[1]["route"]
    _assert_routes_equal(g, specs, res, [sp["init"] for sp in specs])
