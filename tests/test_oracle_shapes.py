"""The references of the shape sweeps (test_gpu_shapes_cg2d.py, test_gpu_shapes_step.py),
pinned on the CPU before the device is compared with them.

  * Every box shape: Oracle.cg2d agrees with a dense float64 solve of the same masked 5-point
    operator (shapes.dense_cg2d_solution shares only the coefficient arrays with it) within
    5e-10 of max|x| -- three times the worst agreement measured at cg2dTargetResidual = 1e-9
    when the sweep was designed (1.5e-10) -- and x is exactly 0.0 on land.
  * Every re-tiling of global_ocean.90x40x15 and tutorial_baroclinic_gyre: 4 oracle steps
    take the iteration counts of the one-tile run, and the un-tiled theta and etaN stay within
    1e-11 of the one-tile field's maximum (measured: 1.1e-12 or less) -- the tile loop of the
    oracle is right at odd, thin and many-tile layouts, only CG2D's summation order moves.
  * The cube sphere (test_gpu_shapes_cube.py): advect_cs on every device tiling is, un-tiled,
    np.array_equal to the one-tile-per-face oracle (no sum crosses a tile there);
    global_ocean.cs32x15 on every device tiling, with C2 and with DST3FL multi-dimensional
    tracers, takes the one-tile run's iteration counts and stays within 1e-9 (etaN), 1e-10
    (uVel) and 1e-12 (theta, salt) of the one-tile field's maximum -- about ten times the
    largest difference measured over tiles of 32x16, 16x16, 8x8, 32x8, 8x32, 16x8, 4x32 and
    32x4 when the sweep was designed (etaN 8.1e-11, uVel 2.0e-12, theta 3.6e-14, salt
    1.5e-14); the synthetic cube on its device cases within the 1e-11 of the other families.
"""
import functools

import numpy as np
import pytest

import shapes

OCEAN90_TILINGS = ((2, 1), (1, 8), (5, 5), (10, 1), (18, 8))
GYRE_TILINGS = ((31, 2), (2, 31), (1, 62), (62, 1))


# the multi-workgroup rows the device also solves with CG2D_SR (useSRCGSolver)
BOX_CASES = [(s, False) for s in shapes.BOX_SHAPES] + [((45, 41, 3, 1), True), ((33, 27, 11, 3), True)]


@pytest.mark.parametrize("shape,sr", BOX_CASES, ids=lambda v: "sr%d" % v if isinstance(v, bool) else "%dx%d_%dx%d" % v)
def test_box_oracle_cg2d_vs_dense_solve(shape, sr):
    ref = shapes.box_reference(shape, sr)
    g = ref["g"]
    print("box %s%s: oracle %d iterations, err_oracle %.2e" % (shape, " CG2D_SR" if sr else "", ref["iters_oracle"],
                                                              ref["err_oracle"]))
    assert 0 < ref["iters_oracle"] < 2000
    assert ref["err_oracle"] <= 5e-10, ref["err_oracle"]
    inner = (slice(None),) + g.sl(1, g.sNx, 1, g.sNy)
    land = g.f["maskInC"][inner] == 0.0
    assert land.any() and not land.all()
    assert np.all(ref["x_oracle"][inner][land] == 0.0)


def test_every_gpu_box_shape_is_pinned_here():
    """The device tests take their shapes from the list this file pins (shapes.BOX_SHAPES)."""
    import test_gpu_shapes_cg2d as dev
    assert set(dev.CASES) | set(dev.REF_CASES) == set(shapes.BOX_SHAPES)


def _four_steps(make):
    o, g = make()
    iters = []
    for _ in range(4):
        o.forward_step()
        iters.append(int(o.get("numIters")))
    return iters, shapes.untile(g, np.array(o.arr("theta"))), shapes.untile(g, np.array(o.arr("etaN")))


@functools.lru_cache(maxsize=None)
def _ocean90(nSx, nSy):
    from oracle.harness import ocean90_oracle
    return _four_steps(lambda: ocean90_oracle(nSx=nSx, nSy=nSy))


@functools.lru_cache(maxsize=None)
def _gyre(nSx, nSy):
    from mitgcm_amd import configs
    from oracle.harness import oracle_from_config
    return _four_steps(lambda: oracle_from_config(configs.baroclinic_gyre, nSx=nSx, nSy=nSy))


def _same_as_one_tile(run, tiling):
    it1, th1, eta1 = run(1, 1)
    it, th, eta = run(*tiling)
    assert it == it1, (tiling, it, it1)
    for name, a, a1 in (("theta", th, th1), ("etaN", eta, eta1)):
        d = float(np.abs(a - a1).max() / np.abs(a1).max())
        print("%s on %dx%d tiles: %s differs from the one-tile run by %.2e of its maximum" % (
            run.__name__, tiling[0], tiling[1], name, d))
        assert d <= 1e-11, (tiling, name, d)


@pytest.mark.parametrize("tiling", OCEAN90_TILINGS, ids=lambda t: "%dx%d" % t)
def test_ocean90_retiled_oracle_matches_one_tile(tiling):
    _same_as_one_tile(_ocean90, tiling)


@pytest.mark.parametrize("tiling", GYRE_TILINGS, ids=lambda t: "%dx%d" % t)
def test_baroclinic_gyre_retiled_oracle_matches_one_tile(tiling):
    _same_as_one_tile(_gyre, tiling)


# ---- the cube sphere ------------------------------------------------------------------------
CS32_TILES = ((16, 16), (8, 8), (32, 8), (8, 32), (16, 8), (4, 32))
CS32_TRACERS = ("c2", "dst3fl")
# (n, Nr, sNx, sNy, OL), tracers of every synthetic-cube run of the device file
SYNTH_CASES = (((12, 3, 4, 6, 4), "dst3fl"), ((12, 3, 6, 4, 4), "dst3fl"), ((12, 3, 4, 4, 4), "dst3fl"),
               ((9, 5, 3, 3, 3), "c2"), ((10, 1, 5, 2, 2), "c2"), ((9, 31, 9, 3, 3), "c2"), ((12, 3, 6, 4, 4), "c2"),
               ((12, 3, 6, 4, 4), "rstar"))
CS32_BARS = {"etaN": 1e-9, "uVel": 1e-10, "theta": 1e-12, "salt": 1e-12}


def test_every_gpu_cube_case_is_pinned_here():
    """The device file's tilings, tracer variants and synthetic cases are the ones this file
    pins; the exchange cases are synthetic cases too."""
    import test_gpu_shapes_cube as dev
    assert tuple(dev.CS32_TILES) == CS32_TILES
    assert tuple(dev.CS32_TRACERS) == CS32_TRACERS
    assert set(dev.CS32_RUNS) == {(t, tr) for t in CS32_TILES for tr in CS32_TRACERS}
    assert {(c, t) for c, t, _ in dev.SYNTH_RUNS} == set(SYNTH_CASES)
    assert set(dev.EXCH_CASES) <= {c for c, _ in SYNTH_CASES}
    for (sNx, sNy), tiles in dev.CS32_TILES.items():
        assert tiles == 6 * (32 // sNx) * (32 // sNy) <= shapes.MAX_MWG_PARTS and sNx * sNy <= 1024
    for (n, Nr, sNx, sNy, OL), _ in SYNTH_CASES:
        assert 6 * (n // sNx) * (n // sNy) <= 96 and sNx * sNy <= 1024


@functools.lru_cache(maxsize=None)
def _advect_cs(sNx, sNy):
    from mitgcm_amd import configs
    from oracle.harness import oracle_from_config
    o, g = oracle_from_config(configs.advect_cs, sNx=sNx, sNy=sNy)
    for _ in range(6):
        o.forward_step()
    return shapes.cube_untile(g, np.array(o.arr("theta")))


@pytest.mark.parametrize("tile", CS32_TILES, ids=lambda t: "%dx%d" % t)
def test_advect_cs_retiled_oracle_equals_one_tile(tile):
    one = _advect_cs(32, 32)
    assert one.max() > one.min()
    assert np.array_equal(_advect_cs(*tile), one)


def _cube_four_steps(make, fields):
    o, g = make()
    iters = []
    for _ in range(4):
        o.forward_step()
        iters.append(int(o.get("numIters")))
    return iters, {n: shapes.cube_untile(g, np.array(o.arr(n))) for n in fields}


@functools.lru_cache(maxsize=None)
def _cs32x15(sNx, sNy, tracers):
    import test_gpu_shapes_cube as dev
    from oracle.harness import cs32x15_oracle
    return _cube_four_steps(lambda: cs32x15_oracle(sNx=sNx, sNy=sNy, params_over=dev.CS32_TRACERS[tracers]),
                            tuple(CS32_BARS))


@functools.lru_cache(maxsize=None)
def _synth(case, tracers):
    import test_gpu_shapes_cube as dev
    return _cube_four_steps(lambda: dev.synth_oracle(case, dev.SYNTH_OVER[tracers]),
                            ("etaN", "uVel", "vVel", "wVel", "theta", "salt"))


def _cube_same_as_one_tile(what, got, one, bars):
    (it, f), (it1, f1) = got, one
    assert it == it1 and min(it1) > 0, (what, it, it1)
    for name in f1:
        d = float(np.abs(f[name] - f1[name]).max() / np.abs(f1[name]).max())
        print("%s: %s differs from the one-tile-per-face run by %.2e of its maximum" % (what, name, d))
        assert d <= bars[name], (what, name, d)


@pytest.mark.parametrize("tracers", CS32_TRACERS)
@pytest.mark.parametrize("tile", CS32_TILES, ids=lambda t: "%dx%d" % t)
def test_cs32x15_retiled_oracle_matches_one_tile(tile, tracers):
    _cube_same_as_one_tile("cs32x15 %s on tiles of %d x %d" % ((tracers,) + tile), _cs32x15(tile[0], tile[1], tracers),
                           _cs32x15(32, 32, tracers), CS32_BARS)


@pytest.mark.parametrize("case,tracers", SYNTH_CASES, ids=["n%d_Nr%d_%dx%d_OL%d-%s" % (c + (t,)) for c, t in SYNTH_CASES])
def test_cube_synthetic_retiled_oracle_matches_one_tile(case, tracers):
    n, Nr, sNx, sNy, OL = case
    _cube_same_as_one_tile("synthetic cube %s %s" % (case, tracers), _synth(case, tracers),
                           _synth((n, Nr, n, n, OL), tracers), dict.fromkeys(("etaN", "uVel", "vVel", "wVel", "theta", "salt"), 1e-11))
