"""cg2dRefOrder in the multi-workgroup CG2D ('mwg_ref', k_cg2d_mwg<.., REF>): the sums in the
reference's own order -- every tile sequentially, j outer and i inner, from 0.0
(cg2d.F:211-243, 268-296, 305-337), the tile partials in tile order from 0.0
(global_sum_tile.F:161-191) -- on grids past the 4 096 points the single-workgroup
'block_ref' takes.  A tile cut into several parts is summed by a chain: each part adds its
points' terms to the carry of the part before it.

Every comparison here is against the PLAIN oracle (no set_sum_plan: oracle/solver.c sums per
tile sequentially, then in tile order) and is bit for bit; no tolerance appears anywhere.
"""
import functools
import os

import numpy as np
import pytest

import shapes
from conftest import digits

pytestmark = pytest.mark.gpu

# (Nx, Ny, nSx, nSy) -> (points of every part in part order, pinned)
BOXES = {
    # one tile of 96 x 48: strips of 9, 10, 9, 10, 10 rows -- a carry chain of 5, ragged strips
    (96, 48, 1, 1): ([864, 960, 864, 960, 960], 1),
    # 2 tiles of 45 x 46, strips of 15, 15, 16 rows each: chains and a tile sum together
    (90, 46, 2, 1): ([675, 675, 720] * 2, 1),
    # 6 tiles of 33 x 21, one part each: no carry, odd sizes, parts that end inside a wave
    (66, 63, 2, 3): ([693] * 6, 1),
    # 33 tiles of 6 x 22: more than 32 parts -- not pinned, the uncached block, hand-offs across XCDs
    (66, 66, 11, 3): ([132] * 33, 0),
}
IDS = ["%dx%d_%dx%d" % s for s in BOXES]
# 72 tiles of 6 x 11: more tile partials than wave 0 has lanes, so the tile sum takes a second
# sweep (64 partials, then 8); the solve only
MANY_TILES = {(72, 66, 12, 6): ([66] * 72, 0)}


def _assert_form(m, sizes, pinned):
    """The kernel, the parts' own-point counts (in part order) and the placement."""
    from mitgcm_amd._lib import lib
    assert m.cg2d_kernel() == "mwg_ref", m.cg2d_kernel()
    assert lib().mgcm_get_param(m.h, b"cg2dKernel") == 6.0
    assert m.cg2d_parts() == len(sizes) <= shapes.MAX_MWG_PARTS, (m.cg2d_parts(), len(sizes))
    plan, nt, ppt, ng = m.cg2d_sum_plan()
    got = [int(n) for n in (plan.reshape(ng, nt * ppt) >= 0).sum(axis=1)]
    assert got == list(sizes), got
    assert int(lib().mgcm_get_param(m.h, b"cg2dPinned")) == pinned


@functools.lru_cache(maxsize=None)
def _box_oracle_solve(shape, maxIters, nIterMin):
    """The plain oracle's solve of the seeded right-hand side from x = 0; computed once per
    case and shared (do not modify)."""
    from oracle.harness import oracle_from_config
    o, g = oracle_from_config(shapes.box_cfg(shape))
    b = shapes.box_rhs(g)
    b.setflags(write=False)
    return g, b, o.cg2d(b, np.zeros_like(b), maxIters, nIterMin)


def _solve_both(shape, maxIters, nIterMin):
    from mitgcm_amd import configs
    g, b, ref = _box_oracle_solve(shape, maxIters, nIterMin)
    m = configs.make_model(shapes.box_cfg(shape, cg2dRefOrder=1))
    try:
        _assert_form(m, *{**BOXES, **MANY_TILES}[shape])
        dev = m.cg2d(b, np.zeros_like(b), maxIters, nIterMin)
    finally:
        m.close()
    return g, dev, ref


@pytest.mark.parametrize("shape", list(BOXES) + list(MANY_TILES), ids=IDS + ["72x66_12x6"])
def test_box_mwg_ref_solve_bitexact(shape):
    """(a) the stand-alone solve to convergence: x, both residuals and the iteration count."""
    g, dev, ref = _solve_both(shape, 2000, -1)
    x, first, _, last, iters, _ = dev
    xo, first_o, _, last_o, iters_o, _ = ref
    print("box %s mwg_ref: iterations %d (oracle %d), first %.17e last %.17e" % (shape, iters, iters_o, first, last))
    assert 0 < iters_o < 2000, iters_o   # the oracle converged: the comparison is of a real solve
    assert iters == iters_o, (iters, iters_o)
    assert first == first_o, (first, first_o)
    assert last == last_o, (last, last_o)
    inner = (slice(None),) + g.sl(1, g.sNx, 1, g.sNy)
    assert np.array_equal(x[inner], xo[inner]), float(np.abs(x - xo)[inner].max())


def test_box_mwg_ref_minres_bitexact():
    """(c) cgUseMinResSol with fewer iterations than convergence needs: the lowest-residual
    solution, its residual and its iteration."""
    g, dev, ref = _solve_both((90, 46, 2, 1), 40, 0)
    x, first, minsq, last, iters, itmin = dev
    xo, first_o, minsq_o, last_o, iters_o, itmin_o = ref
    print("box (90, 46, 2, 1) mwg_ref minres: iterations %d nIterMin %d minResidualSq %.17e last %.17e"
          % (iters, itmin, minsq, last))
    assert iters_o == 40 and minsq_o >= 0.0, (iters_o, minsq_o)   # not converged, minres active
    assert (iters, itmin) == (iters_o, itmin_o), (iters, itmin, iters_o, itmin_o)
    assert minsq == minsq_o, (minsq, minsq_o)
    assert first == first_o and last == last_o, (first, first_o, last, last_o)
    inner = (slice(None),) + g.sl(1, g.sNx, 1, g.sNy)
    assert np.array_equal(x[inner], xo[inner]), float(np.abs(x - xo)[inner].max())


def _steps_bitexact(m, o, g, nsteps, fields):
    """nsteps FORWARD_STEPs of device model m and plain oracle o: after every step the solve's
    record and every dynstat value identical; at the end the interiors of `fields` equal.
    Returns the device's solve stats of every step."""
    from mitgcm_amd.model import dynstat
    hist = []
    for step in range(1, nsteps + 1):
        m.forward_step(1)
        o.forward_step()
        md = m.solve_stats()
        hist.append(dict(md))
        md.update(dynstat(m))
        od = o.dynstat()
        assert md["cg2d_iters"] > 0, (step, md["cg2d_iters"])   # -1: a hand-off timed out
        for k in ("cg2d_iters", "cg2d_init_res", "cg2d_last_res"):
            assert md[k] == od[k], (step, k, md[k], od[k])
        n = 0
        for k, v in md.items():
            if k in od:
                assert v == od[k], (step, k, v, od[k])
                n += 1
        assert n >= 24, n
    inner = (Ellipsis,) + g.sl(1, g.sNx, 1, g.sNy)
    bad = []
    for n in fields:
        dev = m.get(n)
        ref = np.array(o.arr(n)).reshape(dev.shape)
        if not np.array_equal(dev[inner], ref[inner]):
            bad.append((n, float(np.nanmax(np.abs(dev - ref)[inner]))))
    assert not bad, bad
    return hist


@pytest.mark.parametrize("shape", list(BOXES), ids=IDS)
def test_box_mwg_ref_4_steps_bitexact(shape):
    """(b) 4 graph-replayed steps: the solve inside FORWARD_STEP."""
    from mitgcm_amd import configs
    from oracle.harness import oracle_from_config
    m = configs.make_model(shapes.box_cfg(shape, cg2dRefOrder=1))
    try:
        _assert_form(m, *BOXES[shape])
        o, g = oracle_from_config(shapes.box_cfg(shape))
        hist = _steps_bitexact(m, o, g, 4, shapes.BOX_FIELDS)
    finally:
        m.close()
    print("box %s mwg_ref: iterations over 4 steps %s" % (shape, [h["cg2d_iters"] for h in hist]))


# the state list of test_gpu_refpin.py
STATE = ("uVel", "vVel", "wVel", "theta", "salt", "etaN", "etaH", "guNm1", "gvNm1", "gtNm1", "gsNm1", "totPhiHyd")


@pytest.mark.parametrize("sNx,sNy,tiles", [(32, 32, 6), (32, 16, 12), (16, 8, 48)], ids=["32-6", "16-12", "16x8-48"])
def test_cs32x15_mwg_ref_8_steps_bitexact(sNx, sNy, tiles):
    """Config 3 on 6 tiles, on the experiment's own 12 and on the 48 tiles of 16 x 8 of the
    reference's adjustment.cs-32x32x1 (more than 32 parts: not pinned to one XCD, a tile sum
    of 48 partials): 8 steps bit-identical to the plain oracle of the same tiling.  The default device path's cg2d_init_res is printed against this
    run: its distance from the reference-order value (tests/test_gpu_cs32x15.py holds it to
    10.5 digits) is summation order only, since this run differs from it in nothing else.
    storePhiHyd4Phys = 1 on both sides: the state list holds totPhiHyd, which the device keeps
    only under that switch (the oracle always, as DIAGS_PHI_HYD does); with JMD95Z nothing
    reads it, so no other value of the run depends on the switch."""
    from mitgcm_amd import configs
    from oracle.harness import cs32x15_oracle
    m = configs.make_model(lambda: configs.global_ocean_cs32x15(
        sNx=sNx, sNy=sNy, params_over={"cg2dRefOrder": 1, "storePhiHyd4Phys": 1}))
    m_def = configs.make_model(lambda: configs.global_ocean_cs32x15(sNx=sNx, sNy=sNy))
    try:
        _assert_form(m, [sNx * sNy] * tiles, 1 if tiles <= 32 else 0)
        assert m_def.cg2d_kernel() == "mwg"
        o, g = cs32x15_oracle(sNx=sNx, sNy=sNy, params_over={"storePhiHyd4Phys": 1})
        assert g.nTiles == tiles
        hist = _steps_bitexact(m, o, g, 8, STATE)
        worst = (99.0, None)
        for step in range(1, 9):
            m_def.forward_step(1)
            worst = min(worst, (digits(m_def.solve_stats()["cg2d_init_res"], hist[step - 1]["cg2d_init_res"]), step))
    finally:
        m.close()
        m_def.close()
    print("cs32x15 on %d tiles, 8 steps: mwg_ref == plain oracle bit for bit; the default device path (mwg, tree sums) "
          "against it: cg2d_init_res %.2f digits at step %s -- summation order only" % ((tiles,) + worst))


@pytest.mark.parametrize("tile,tiles,nsteps,pinned", [(None, 13, 4, 1), (15, 52, 2, 0)])
def test_llc30_mwg_ref_steps_bitexact(tile, tiles, nsteps, pinned):
    """LLC-30 as 13 tiles of 30 x 30 (13 parts) and as 52 tiles of 15 x 15 (52 parts, not
    pinned)."""
    from mitgcm_amd import configs
    from oracle.harness import oracle_from_config
    cfg = lambda: configs.llc_synthetic(n=30, Nr=10, tile=tile)

    def cfg_ref():
        g, params, state = cfg()
        params["cg2dRefOrder"] = 1
        return g, params, state
    m = configs.make_model(cfg_ref)
    try:
        pts = (tile or 30) ** 2
        _assert_form(m, [pts] * tiles, pinned)
        o, g = oracle_from_config(cfg)
        assert g.nTiles == tiles
        hist = _steps_bitexact(m, o, g, nsteps, ("uVel", "vVel", "wVel", "theta", "salt", "etaN"))
    finally:
        m.close()
    print("LLC-30 on %d tiles mwg_ref: iterations %s" % (tiles, [h["cg2d_iters"] for h in hist]))


def test_mwg_ref_refuses_cg2d_sr():
    from mitgcm_amd import configs
    with pytest.raises(Exception, match="cg2dRefOrder with useSRCGSolver"):
        configs.make_model(shapes.box_cfg((96, 48, 1, 1), cg2dRefOrder=1, useSRCGSolver=1)).close()


def test_mwg_ref_refuses_tile_range():
    """A tile range narrower than the domain: the chains and the tile sum need every tile."""
    from mitgcm_amd import configs
    from mitgcm_amd._lib import check, lib
    m = configs.make_model(shapes.box_cfg((90, 46, 2, 1), cg2dRefOrder=1))
    try:
        assert m.cg2d_kernel() == "mwg_ref"
        with pytest.raises(Exception, match="cg2dRefOrder in the multi-workgroup CG2D needs the whole domain"):
            check(lib().mgcm_set_tile_range(m.h, 0, 1), "mgcm_set_tile_range")
        with pytest.raises(Exception, match="cg2dRefOrder in the multi-workgroup CG2D runs the whole domain"):
            check(lib().mgcm_cg2d_tiles(m.h, 0, 1), "mgcm_cg2d_tiles")
        # the refusals left the model as it was: the whole-domain solve still runs
        g, b, ref = _box_oracle_solve((90, 46, 2, 1), 2000, -1)
        assert m.cg2d(b, np.zeros_like(b), 2000, -1)[4] == ref[4]
    finally:
        m.close()


def test_refhost_cs32_mwg_ref_bitexact(tmp_path):
    """The Fortran drop-ins under MGCM_CG2D_REFORDER=1 on the cs32 host layout (12 tiles of
    32 x 16), one device model, graph-replayed steps: bit-identical to the resident model with
    cg2dRefOrder = 1 on the same tiling (test_refhost_cs32_exch2_bitexact's flow)."""
    import subprocess
    from mitgcm_amd import configs
    from test_gpu_refhost import CHECK, REFBIN, _cs32_namelists, _read_out, _write_blob
    exe = os.path.join(REFBIN, "refhost_cs32")
    assert os.path.exists(exe), "refhost not built (oracle/build_refhost.py, __graft_entry__.build())"
    nsteps = 4
    m = configs.make_model(lambda: configs.global_ocean_cs32x15(sNy=16, params_over={"cg2dRefOrder": 1}))
    try:
        _assert_form(m, [512] * 12, 1)
        pdir = _cs32_namelists(str(tmp_path / "input"))
        w2 = m.g.topo.w2_arrays(ldNb=8, ldT=2 * m.g.nTiles)
        state = _write_blob(tmp_path / "refhost_in.bin", m, nsteps, monitor_days=2, w2=w2, undef=("ALLOW_CD_CODE",))
        env = dict(os.environ, MGCM_CG2D_REFORDER="1", MGCM_AMD_MODELS="1", MGCM_CG2D_MWG="0", MGCM_AMD_EAGER="0")
        r = subprocess.run([exe, str(tmp_path), pdir], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        out, st = _read_out(tmp_path / "refhost_out.bin", state, nsteps)
        m.forward_step(1)
        m.prepare()
        m.forward_step(nsteps - 1)
        m.sync()
        assert all(it > 0 for it in m.solve_history(nsteps - 1)[0])
        bad = [(n, float(np.abs(out[n] - m.get(n).reshape(-1)[:out[n].size]).max())) for n in CHECK
               if n in out and not np.array_equal(out[n], m.get(n).reshape(-1)[:out[n].size])]
    finally:
        m.close()
    assert not bad, bad
    assert len([n for n in CHECK if n in out]) >= 18
    assert st["downloads"] == 2 * len(state), (st, len(state))
