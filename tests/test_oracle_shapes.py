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
