"""Land-block compaction of the single-workgroup CG2D (k_cg2d_bxy, model.hip choose_bxy, build_bxy): blocks
whose points are all dry columns with closed faces are left out of the solver's tables, which
lets a grid fit a geometry of fewer threads; the zero-on-land invariant that makes this exact
is checked where state enters from the host and by the solver itself.

The domains are channels built like shapes.box (barotropic-gyre parameters, one level) with
land placed so that whole blocks, blocks across a tile edge and across the periodic wrap, and
partially wet blocks all occur.
"""
import functools

import numpy as np
import pytest

from oracle.harness import oracle_from_config
from shapes import BOX_FIELDS, assert_bitexact_steps, box_rhs

pytestmark = pytest.mark.gpu

# k_cg2d_bxy's geometries, by name, and the default preference order (model.hip choose_bxy)
GEOM = {"2x4x512": (2, 4, 512), "2x2x1024": (2, 2, 1024), "3x4x256": (3, 4, 256), "3x2x512": (3, 2, 512)}
PREFERENCE = ("3x2x512", "2x4x512", "2x2x1024")


def channel(Nx, Ny, nSx, nSy, land, OL=2, seed=20261019):
    """shapes.box with the land given: land(bathy) zeroes cells of the global (Ny, Nx) bathymetry
    (depths seeded, uniform in 1500..5000 m)."""
    from mitgcm_amd.grid import Grid
    sNx, sNy = Nx // nSx, Ny // nSy
    rng = np.random.default_rng(seed)
    bathy = -(1500.0 + 3500.0 * rng.random((Ny, Nx)))
    land(bathy)
    wind = 0.1 * rng.standard_normal((Ny, Nx))
    g = Grid(sNx, sNy, OL, OL, 1, nSx, nSy)
    g.ini_vertical_grid([5000.0])
    g.ini_cartesian_grid(np.full(Nx, 20e3), np.full(Ny, 20e3), -20e3, -20e3)
    g.ini_cori(1e-4, 1e-11, selectCoriMap=1)
    g.ini_depths_masks(bathy, hFacMin=0.2, hFacMinDr=0.0, gBaro=9.81)
    g.ini_cg2d(1200.0, 1200.0, 1e-9)
    params = dict(deltaTMom=1200.0, deltaTFreeSurf=1200.0, deltaTClock=1200.0, abEps=0.01, rhoConst=1000.0,
                  gBaro=9.81, viscAhD=400.0, viscAhZ=400.0, viscA4D=0.0, viscA4Z=0.0, viscAr=0.0,
                  sideDragFactor=2.0, selectCoriScheme=0, momForcingOutAB=0, momDissip_In_AB=1,
                  cg2dMaxIters=1000, cg2dUseMinResSol=0, nIter0=0, no_slip_sides=1, no_slip_bottom=1)
    fu = g.z2()
    inner = g.sl(1, sNx, 1, sNy)
    for t in range(g.nTiles):
        bi, bj = t % nSx, t // nSx
        fu[t][inner] = wind[bj * sNy:(bj + 1) * sNy, bi * sNx:(bi + 1) * sNx]
    state = {"fu": g.exch(fu), "fv": g.z2(), "theta": np.full((g.nTiles, 1, g.ny, g.nx), 20.0),
             "salt": np.full((g.nTiles, 1, g.ny, g.nx), 30.0)}
    return g, params, state


def land_24x16(bathy):
    """1-based (I, J): the rectangle I = 7..15, J = 5..12 (whole 3x4 and 3x2 blocks, one across the
    tile edge 8|9), I = 22..24 and I = 1..3 at J = 1..4 (left-out blocks that are neighbours across
    the periodic wrap), single-cell islands (partially wet blocks), the northernmost row."""
    bathy[4:12, 6:15] = 0.0
    bathy[0:4, 21:24] = 0.0
    bathy[0:4, 0:3] = 0.0
    for I, J in ((5, 3), (18, 7), (20, 14), (11, 2), (3, 10), (17, 1), (24, 9)):
        bathy[J - 1, I - 1] = 0.0
    bathy[15, :] = 0.0


def land_96x36(bathy):
    """I = 25..72, J = 9..20: 16 x 3 = 48 whole 3x4 blocks; islands; the northernmost row."""
    bathy[8:20, 24:72] = 0.0
    for I, J in ((5, 3), (80, 7), (20, 30), (90, 22), (50, 2)):
        bathy[J - 1, I - 1] = 0.0
    bathy[35, :] = 0.0


def cfg_24x16(**over):
    def cfg():
        g, params, state = channel(24, 16, 3, 1, land_24x16)
        params.update(over)
        return g, params, state
    return cfg


def cfg_96x36():
    return channel(96, 36, 1, 1, land_96x36)


def dry_mask(g, nonlin=False):
    """Global (Ny, Nx) bool: the column is dry and its four faces are closed at every level
    (from hFacC / hFacW / hFacS, the rest-state h0Fac* under the non-linear free surface)."""
    c, w, s = (g.f[("h0Fac" if nonlin else "hFac") + n] for n in "CWS")
    own, e, n = g.sl(1, g.sNx, 1, g.sNy), g.sl(2, g.sNx + 1, 1, g.sNy), g.sl(1, g.sNx, 2, g.sNy + 1)
    out = np.zeros((g.sNy * g.nSy, g.sNx * g.nSx), dtype=bool)
    for t in range(g.nTiles):
        bi, bj = t % g.nSx, t // g.nSx
        sel = (t, slice(None))
        closed = ((c[sel + own] == 0) & (w[sel + own] == 0) & (w[sel + e] == 0) & (s[sel + own] == 0) &
                  (s[sel + n] == 0)).all(axis=0)
        out[bj * g.sNy:(bj + 1) * g.sNy, bi * g.sNx:(bi + 1) * g.sNx] = closed
    return out


def offsets(g):
    """Global (Ny, Nx) int: the 2-D flat offset (tile*ny*nx + local) of every interior point."""
    out = np.zeros((g.sNy * g.nSy, g.sNx * g.nSx), dtype=np.int64)
    jj, ii = np.meshgrid(np.arange(g.sNy), np.arange(g.sNx), indexing="ij")
    for t in range(g.nTiles):
        bi, bj = t % g.nSx, t // g.nSx
        out[bj * g.sNy:(bj + 1) * g.sNy, bi * g.sNx:(bi + 1) * g.sNx] = (
            t * g.ny * g.nx + (jj + g.OLy) * g.nx + ii + g.OLx)
    return out


def blocks(dry, BX, BY):
    """(number of blocks, bool per block: all of it dry), blocks in (J0, I0) order; None when the grid
    does not tile into BX x BY."""
    Ny, Nx = dry.shape
    if Nx % BX or Ny % BY:
        return None
    allDry = dry.reshape(Ny // BY, BY, Nx // BX, BX).all(axis=(1, 3))
    return allDry.size, allDry


def policy(dry, preference=PREFERENCE, force=None, compact=None):
    """(name, count of plan entries >= 0, compacted?) the selection of choose_bxy gives: the first
    geometry of the list whose full block count fits its threads (every block kept) or, failing
    that, whose count without the all-dry blocks does; compact=1 leaves them out wherever there are
    any, compact=0 never."""
    for name in ((force,) if force else preference):
        BX, BY, NT = GEOM[name]
        b = blocks(dry, BX, BY)
        if b is None:
            continue
        n, allDry = b
        nDry = 0 if compact == 0 else int(allDry.sum())
        if n <= NT and not (compact == 1 and nDry > 0):
            return name, n * BX * BY, False
        if nDry > 0 and 0 < n - nDry <= NT:
            return name, (n - nDry) * BX * BY, True
    return None


def check_plan(m, g, dry, name, compacted):
    """The model's summation plan is that of geometry `name`, holding exactly the points of the
    blocks kept."""
    BX, BY, NT = GEOM[name]
    plan, nt, ppt, ng = m.cg2d_sum_plan()
    assert (nt, ppt, ng) == (NT, BX * BY, 1), (nt, ppt, ng, name)
    n, allDry = blocks(dry, BX, BY)
    keep = ~np.repeat(np.repeat(allDry, BY, axis=0), BX, axis=1) if compacted else np.ones_like(dry)
    off = offsets(g)
    have = set(int(v) for v in plan[plan >= 0])
    assert int((plan >= 0).sum()) == int(keep.sum()) == len(have)
    assert have == set(int(v) for v in off[keep])
    if compacted:
        assert int(keep.sum()) == (n - int(allDry.sum())) * BX * BY
        assert not have & set(int(v) for v in off[~keep])
    return plan, nt, ppt, ng


@functools.lru_cache(maxsize=None)
def reference_24x16():
    """Computed once (do not modify): the grid, a masked seeded right-hand side and the
    reference-order oracle's solve of it."""
    o, g = oracle_from_config(cfg_24x16())
    b = box_rhs(g)
    xo, _, _, _, its, _ = o.cg2d(b, np.zeros_like(b), 2000, -1)
    b.setflags(write=False)
    xo.setflags(write=False)
    return g, b, xo, its


def forced(monkeypatch, name=None, compact=None):
    for k, v in (("MGCM_CG2D_BXY", name), ("MGCM_CG2D_COMPACT", compact)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


FORCED_CASES = [("3x4x256", {}), ("3x2x512", {}), ("2x4x512", {}), ("3x4x256", {"useSRCGSolver": 1}),
                ("3x4x256", {"cg2dUseMinResSol": 1})]


@pytest.mark.parametrize("name,over", FORCED_CASES, ids=lambda v: v if isinstance(v, str) else "+".join(v) or "std")
def test_forced_compaction_24x16(monkeypatch, name, over):
    """MGCM_CG2D_COMPACT=1 with each geometry forced: the plan holds the kept blocks only, 4 steps
    are bit-identical to the device-order oracle, a direct solve leaves x = 0.0 on land and takes
    the reference-order oracle's iterations +- 1."""
    from mitgcm_amd import configs
    forced(monkeypatch, name, 1)
    g, b, xo, its = reference_24x16()
    dry = dry_mask(g)
    BX, BY, NT = GEOM[name]
    n, allDry = blocks(dry, BX, BY)
    assert int(allDry.sum()) >= 8 and int(allDry.sum()) < n   # the land rectangles are whole blocks
    assert policy(dry, force=name, compact=1) == (name, (n - int(allDry.sum())) * BX * BY, True)
    cfg = cfg_24x16(**over)

    def after(m):
        check_plan(m, g, dry, name, True)

    kernel, _, _ = assert_bitexact_steps(cfg, 4, BOX_FIELDS, after=after)
    assert kernel == "bxy"
    if over:
        return
    m = configs.make_model(cfg)
    try:
        x, _, _, _, it, _ = m.cg2d(b, np.zeros_like(b), 2000, -1)
        check_plan(m, g, dry, name, True)   # the solve kept the compacted tables
    finally:
        m.close()
    inner = (slice(None),) + g.sl(1, g.sNx, 1, g.sNy)
    land = g.f["maskInC"][inner] == 0.0
    assert np.all(x[inner][land] == 0.0)
    assert abs(it - its) <= 1, (it, its)
    assert np.abs(x - xo)[inner].max() <= 1e-6 * np.abs(xo).max()


def test_natural_compaction_96x36(monkeypatch):
    """No switch set, a grid whose full 3x4 block count exceeds 256 but whose kept count fits: the
    form is the policy's and 4 steps are bit-identical."""
    forced(monkeypatch)
    g = cfg_96x36()[0]
    dry = dry_mask(g)
    n, allDry = blocks(dry, 3, 4)
    assert n == 288 and int(allDry.sum()) >= 40 and n - int(allDry.sum()) <= 256
    want = policy(dry)
    assert want is not None

    def after(m):
        check_plan(m, g, dry, want[0], want[2])

    kernel, _, _ = assert_bitexact_steps(cfg_96x36, 4, BOX_FIELDS, after=after)
    assert kernel == "bxy"


def test_eta_on_dropped_point_uncompacts(monkeypatch):
    """Model.set of a non-zero etaN on a left-out land point: the tables are rebuilt over the whole
    grid in the geometry used without compaction, and 2 steps are bit-identical to the oracle
    started from the same state."""
    from mitgcm_amd import configs
    from mitgcm_amd.model import dynstat
    forced(monkeypatch, "3x4x256", 1)
    g, _, _, _ = reference_24x16()
    dry = dry_mask(g)
    eta = g.z2()
    eta[(1,) + g.sl(2, 2, 6, 6)] = 0.25     # tile 1, local (2, 6) = global I = 10, J = 6: inside the rectangle
    assert dry[5, 9]
    base = cfg_24x16()

    def cfg():
        gg, params, state = base()
        state = dict(state, etaN=eta.copy())
        return gg, params, state

    m = configs.make_model(base)
    try:
        check_plan(m, g, dry, "3x4x256", True)
        m.set("etaN", eta)
        m.set("etaH", eta)
        plan, NT, PPT, NG = check_plan(m, g, dry, "2x4x512", False)
        assert int((plan >= 0).sum()) == dry.size
        od, _ = oracle_from_config(cfg)
        od.set_sum_plan(plan, NT, PPT, NG, fma=m.cg2d_fma())
        for step in (1, 2):
            m.forward_step(1)
            od.forward_step()
            md = m.solve_stats()
            md.update(dynstat(m))
            dd = od.dynstat()
            for k, v in md.items():
                if k in dd:
                    assert v == dd[k], (step, k, v, dd[k])
        inner = (Ellipsis,) + g.sl(1, g.sNx, 1, g.sNy)
        for n in BOX_FIELDS:
            dev = m.get(n)
            assert np.array_equal(dev[inner], np.array(od.arr(n)).reshape(dev.shape)[inner]), n
    finally:
        m.close()


def test_rhs_on_dropped_point_solves_uncompacted(monkeypatch):
    """A direct solve whose right-hand side is non-zero on a left-out point: the solver's guard
    sends it to the full tables of the 2x4x512 geometry; solution and iteration count are those of
    the model built with MGCM_CG2D_COMPACT=0 in that geometry."""
    from mitgcm_amd import configs
    g, b0, _, _ = reference_24x16()
    dry = dry_mask(g)
    b = b0.copy()
    b[(1,) + g.sl(2, 2, 6, 6)] = 0.5
    out = []
    for name, compact in (("3x4x256", 1), ("2x4x512", 0)):
        forced(monkeypatch, name, compact)
        m = configs.make_model(cfg_24x16())
        try:
            if compact:
                check_plan(m, g, dry, name, True)
            out.append(m.cg2d(b, np.zeros_like(b), 2000, -1))
            check_plan(m, g, dry, "2x4x512", False)
        finally:
            m.close()
    assert out[0][4] == out[1][4] > 0, (out[0][4], out[1][4])
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1:4] == out[1][1:4]


def test_config2_form(monkeypatch):
    """global_ocean.90x40x15 takes the form the policy gives for its own land."""
    from mitgcm_amd import configs
    forced(monkeypatch)
    m = configs.make_model(configs.global_ocean_90x40x15)
    try:
        g = m.g
        dry = dry_mask(g, nonlin=True)
        assert np.array_equal(dry, configs_land(g))
        name, count, compacted = policy(dry)
        plan, nt, ppt, ng = check_plan(m, g, dry, name, compacted)
        assert (nt, ppt, int((plan >= 0).sum())) == (GEOM[name][2], GEOM[name][0] * GEOM[name][1], count)
    finally:
        m.close()


def configs_land(g):
    """Global (Ny, Nx) bool: maskInC == 0."""
    out = np.zeros((g.sNy * g.nSy, g.sNx * g.nSx), dtype=bool)
    inner = g.sl(1, g.sNx, 1, g.sNy)
    for t in range(g.nTiles):
        bi, bj = t % g.nSx, t // g.nSx
        out[bj * g.sNy:(bj + 1) * g.sNy, bi * g.sNx:(bi + 1) * g.sNx] = g.f["maskInC"][t][inner] == 0.0
    return out
