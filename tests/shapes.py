"""Helpers of the shape-sweep tests (test_oracle_shapes.py, test_gpu_shapes_cg2d.py,
test_gpu_shapes_step.py, test_gpu_shapes_cube.py): a barotropic box of free size, the dense reference of the CG2D
solve, and the step loop that pins a device model bit for bit to the oracle.

A plain module, not a conftest: the test files import it by name.
"""
import functools

import numpy as np

from oracle.harness import oracle_from_config

# the largest part count of the multi-workgroup CG2D shown co-resident (LLC-90): the solver
# spin-waits on its peers, so no test may ask for more
MAX_MWG_PARTS = 117

# (Nx, Ny, nSx, nSy) of every box the CG2D and step sweeps run
BOX_SHAPES = ((64, 64, 1, 1), (2, 4, 1, 1), (64, 62, 1, 1), (62, 62, 31, 2), (90, 44, 2, 1), (92, 46, 1, 1),
              (45, 41, 3, 1), (7, 5, 1, 1), (33, 27, 11, 3), (126, 3, 1, 3), (45, 41, 1, 1), (64, 64, 2, 2))
# the fields a box step moves (theta and salt are carried along unchanged)
BOX_FIELDS = ("uVel", "vVel", "wVel", "theta", "salt", "etaN")


def box(Nx, Ny, nSx, nSy, OL=2, seed=20261019, periodic_land=True):
    """A flux-form barotropic box of Nx x Ny cells on nSx x nSy tiles: the parameters of
    configs.barotropic_gyre (20 km cells, one 5000 m level, viscAh = 400, beta plane,
    deltaT = 1200) with
      bathymetry  seeded (numpy default_rng(seed)): depths uniform in 1500..5000 m with
                  hFacMin = 0.2, so the elliptic operator's coefficients vary from cell to
                  cell, about 12 % of the cells islands, and (periodic_land) the northernmost
                  row land, which closes the doubly periodic domain to a zonal channel;
      wind        fu = 0.1 N(0,1) N/m2 at every cell, halo-exchanged;
      solver      ini_cg2d(1200, 1200, 1e-9).
    Returns (grid, params, state)."""
    from mitgcm_amd.grid import Grid
    assert Nx % nSx == 0 and Ny % nSy == 0, (Nx, Ny, nSx, nSy)
    sNx, sNy = Nx // nSx, Ny // nSy
    rng = np.random.default_rng(seed)
    bathy = -(1500.0 + 3500.0 * rng.random((Ny, Nx)))
    bathy[rng.random((Ny, Nx)) < 0.12] = 0.0
    if periodic_land:
        bathy[Ny - 1, :] = 0.0
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


def box_cfg(shape, **over):
    """A config callable (for configs.make_model / oracle_from_config) of box(*shape), with
    `over` added to its parameters."""
    def cfg():
        g, params, state = box(*shape)
        params.update(over)
        return g, params, state
    return cfg


def untile(g, a):
    """Tile layout (nTiles, [nz,] ny, nx) on the lat-lon tile grid of g -> global
    (nz, Ny, Nx), interiors only."""
    a = np.asarray(a)
    if a.ndim == 3:
        a = a[:, None]
    nz = a.shape[1]
    out = np.zeros((nz, g.sNy * g.nSy, g.sNx * g.nSx))
    inner = g.sl(1, g.sNx, 1, g.sNy)
    for t in range(g.nTiles):
        bi, bj = t % g.nSx, t // g.nSx
        out[:, bj * g.sNy:(bj + 1) * g.sNy, bi * g.sNx:(bi + 1) * g.sNx] = a[(t, slice(None)) + inner]
    return out


def cube_untile(g, a):
    """Tile layout (nTiles, [nz,] ny, nx) on a pkg/exch2 cube of n x n facets ->
    (6, nz, n, n), interiors only: tile t sits at rows tBy+1..tBy+sNy, columns
    tBx+1..tBx+sNx of facet topo.face[t]."""
    a = np.asarray(a)
    if a.ndim == 3:
        a = a[:, None]
    topo = g.topo
    (n, _), = set(topo.facet_dims)
    out = np.zeros((len(topo.facet_dims), a.shape[1], n, n))
    inner = g.sl(1, g.sNx, 1, g.sNy)
    for t in range(g.nTiles):
        tid = t + 1
        y0, x0 = topo.tBy[tid], topo.tBx[tid]
        out[topo.face[tid] - 1, :, y0:y0 + g.sNy, x0:x0 + g.sNx] = a[(t, slice(None)) + inner]
    return out


def dense_cg2d_solution(g, b):
    """The solution CG2D iterates towards, by a dense float64 solve: the 5-point operator
        (A x)(i,j) = aW(i,j) x(i-1,j) + aW(i+1,j) x(i+1,j) + aS(i,j) x(i,j-1) + aS(i,j+1) x(i,j+1)
                     + aC(i,j) x(i,j)
    assembled from g.f["aW2d" / "aS2d" / "aC2d"] on the wet points (maskInC > 0), the global
    index space periodic in both directions, with right-hand side untile(b) * g.cg2dNorm.
    Returns x on the global (Ny, Nx) grid, 0 on land."""
    aW, aS, aC = (untile(g, g.f[n])[0] for n in ("aW2d", "aS2d", "aC2d"))
    wet = untile(g, g.f["maskInC"])[0] > 0.0
    rhs = untile(g, b)[0] * g.cg2dNorm
    Ny, Nx = wet.shape
    idx = np.full((Ny, Nx), -1)
    idx[wet] = np.arange(int(wet.sum()))
    n = int(wet.sum())
    A = np.zeros((n, n))
    for j in range(Ny):
        for i in range(Nx):
            p = idx[j, i]
            if p < 0:
                continue
            A[p, p] += aC[j, i]
            iw, ie, js, jn = (i - 1) % Nx, (i + 1) % Nx, (j - 1) % Ny, (j + 1) % Ny
            for q, c in ((idx[j, iw], aW[j, i]), (idx[j, ie], aW[j, ie]), (idx[js, i], aS[j, i]),
                         (idx[jn, i], aS[jn, i])):
                if q >= 0:
                    A[p, q] += c
    x = np.zeros((Ny, Nx))
    x[wet] = np.linalg.solve(A, rhs[wet])
    return x


def box_rhs(g, seed=11):
    """Seeded random right-hand side on the wet interior points of g (tile layout, halos 0)."""
    rng = np.random.default_rng(seed)
    b = g.z2()
    inner = (slice(None),) + g.sl(1, g.sNx, 1, g.sNy)
    b[inner] = rng.standard_normal((g.nTiles, g.sNy, g.sNx))
    b[inner] *= g.f["maskInC"][inner]
    return b


def rel_err(g, x, dense):
    """max|x - dense| / max|dense| over the wet points; x in tile layout."""
    wet = untile(g, g.f["maskInC"])[0] > 0.0
    return float(np.abs(untile(g, x)[0] - dense)[wet].max() / np.abs(dense[wet]).max())


@functools.lru_cache(maxsize=None)
def box_reference(shape, sr=False):
    """Computed once per box shape and shared (do not modify): the grid, the seeded right-hand
    side, the dense solution, and the reference-order oracle's solve of it (x, iterations,
    relative error against the dense solution); sr: the oracle solves with CG2D_SR
    (useSRCGSolver)."""
    o, g = oracle_from_config(box_cfg(shape, **({"useSRCGSolver": 1} if sr else {})))
    b = box_rhs(g)
    dense = dense_cg2d_solution(g, b)
    xo, _, _, _, its, _ = o.cg2d(b, np.zeros_like(b), 2000, -1)
    for a in (b, dense, xo):
        a.setflags(write=False)
    return {"g": g, "b": b, "dense": dense, "x_oracle": xo, "iters_oracle": its,
            "err_oracle": rel_err(g, xo, dense)}


def assert_bitexact_steps(cfg, nsteps, fields, oracle_factory=oracle_from_config, after=None):
    """nsteps FORWARD_STEPs of the device model of cfg against two oracles made by
    oracle_factory(cfg) -> (oracle, grid): one summing CG2D in the device's order
    (cg2d_sum_plan, cg2d_fma; the plain oracle where the device itself sums in the reference's
    order, 'block_ref') and one in the reference's order.  Every step: cg2d_iters equal on all
    three; cg2d_init_res, cg2d_last_res and every dynstat value bit-identical to the
    device-order oracle.  At the end the interiors of `fields` np.array_equal.  after(model)
    runs on the stepped model before it is closed.
    Returns (cg2d_kernel(), cg2d_parts(), step_layout()) of the model."""
    from mitgcm_amd import configs
    from mitgcm_amd.model import dynstat
    m = configs.make_model(cfg)
    try:
        kernel, parts, layout = m.cg2d_kernel(), m.cg2d_parts(), m.step_layout()
        assert parts <= MAX_MWG_PARTS, parts
        od, g = oracle_factory(cfg)
        if kernel != "block_ref":
            plan, NT, PPT, NG = m.cg2d_sum_plan()
            od.set_sum_plan(plan, NT, PPT, NG, fma=m.cg2d_fma())
        o_ref, _ = oracle_factory(cfg)
        for step in range(1, nsteps + 1):
            m.forward_step(1)
            od.forward_step()
            o_ref.forward_step()
            md = m.solve_stats()
            md.update(dynstat(m))
            dd = od.dynstat()
            assert md["cg2d_iters"] == dd["cg2d_iters"] == int(o_ref.get("numIters")), (
                step, md["cg2d_iters"], dd["cg2d_iters"], o_ref.get("numIters"))
            for k, v in md.items():
                if k in dd:
                    assert v == dd[k], (step, k, v, dd[k])
        inner = (Ellipsis,) + g.sl(1, g.sNx, 1, g.sNy)
        bad = []
        for n in fields:
            dev = m.get(n)
            ref = np.array(od.arr(n)).reshape(dev.shape)
            if not np.array_equal(dev[inner], ref[inner]):
                diff = np.abs(dev - ref)[inner]
                bad.append((n, float(np.nanmax(diff)), np.unravel_index(int(np.nanargmax(diff)), diff.shape)))
        assert not bad, bad
        layout = m.step_layout()
        if after is not None:
            after(m)
    finally:
        m.close()
    return kernel, parts, layout
