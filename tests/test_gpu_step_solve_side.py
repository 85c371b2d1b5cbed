"""The pipelined step's grids on either side of the pressure solve compiled for
global_ocean.90x40x15's option set (MGCM_STEP_FUSE bit 131072, common.h OptsGO90 / MG_FUSE_SPEC2:
k_update_r_star_cg2d_a<true, 2, OptsGO90> with the next step's DO_OCEANIC_PHYS,
k_corr_cont<true, OptsGO90> with the next step's GMREDI_CALC_TENSOR).

Only which code is compiled changes, so everything is compared BITWISE.  The pinned kernels run
in the hoisting steps of a pipelined call (4 steps or more), so every run here is such a call:

  * config 2 re-tiled (5 x 5 tiles of 18 x 8 and 18 x 8 tiles of 5 x 5: ragged planes, column
    frames that cross tiles, halo points whose source lies in another tile): one 4-step call
    against the oracle, the state's interiors and every step's solve, 'solve_side_specialised' on;
  * those tilings and the one-tile layout with the default mask against the mask minus the bit:
    every field of the state with its halos and the solve history after one 6-step call and
    after 2 + 4 steps;
  * two of the newly listed options moved off the pinned set, one at a time: both keys read off
    and a 4-step call is the oracle's;
  * a pinned option moved by mgcm_set_param after 4 steps: the key flips off and the next 4 steps
    are those of a model that ran the generic kernels throughout.

Every one of these calls also runs k_rstar_exch_phi, which reads the halo topology from the
HaloRec table (common.h) with either mask.  The table's builder is a host function:

  * (no GPU) every entry of mgcm_halo_table on periodic lat-lon tilings of config 2's grid (1 x 1,
    5 x 5 and 18 x 8 tiles, OL = 3; periodic, and closed in y so that some halo points have no
    source) against the arithmetic it replaces.
"""
import numpy as np
import pytest

from test_gpu_refpin import STATE as OCEAN90_STATE
from test_gpu_step_pipeline import _differences

gpu = pytest.mark.gpu

SPEC2_BIT = 131072
# MGCM_STEP_FUSE as common.h's default composes it (mg_fuse_mask)
FUSE_DEFAULT = 1 | 4 | 8 | 128 | 256 | 1024 | 2048 | 4096 | 8192 | 16384 | 32768 | 65536 | SPEC2_BIT
KEY = "solve_side_specialised"
TILINGS = [(5, 5), (18, 8)]
LAYOUTS = [(1, 1)] + TILINGS


def _env(monkeypatch, mask):
    monkeypatch.setenv("MGCM_OVERLAP", "1")   # (no timing-dependent choice of the layout)
    monkeypatch.setenv("MGCM_STEP_FUSE", str(mask))


def _ocean90(nSx=1, nSy=1, **over):
    from mitgcm_amd import configs
    return lambda: configs.global_ocean_90x40x15(nSx=nSx, nSy=nSy, params_over=over or None)


def _snapshot(m, nhist):
    out = {n: m.get(n) for n in OCEAN90_STATE}
    it, fr, lr = m.solve_history(nhist)
    out["cg2d_iters"], out["cg2d_init_res"], out["cg2d_last_res"] = it.astype(np.float64), fr, lr
    out["myIter"] = np.array([float(m.my_iter())])
    return out


def _run(cfg, calls, mask, monkeypatch, before=None):
    """A model of cfg, before(m) on it, then forward_step(k) for k in calls.  Returns (snapshot
    after the last call with that call's solve history, step_layout())."""
    from mitgcm_amd import configs
    _env(monkeypatch, mask)
    m = configs.make_model(cfg)
    try:
        if before is not None:
            before(m)
        for k in calls:
            m.forward_step(k)
        return _snapshot(m, calls[-1]), m.step_layout()
    finally:
        m.close()


def _call_vs_oracle(cfg, oracle, nsteps, monkeypatch):
    """One forward_step(nsteps) call (default mask) against the oracle summing CG2D in the device's
    order: every step's iteration count and residuals and the state's interiors, bit for bit.
    Returns step_layout()."""
    from mitgcm_amd import configs
    monkeypatch.setenv("MGCM_OVERLAP", "1")
    monkeypatch.delenv("MGCM_STEP_FUSE", raising=False)
    m = configs.make_model(cfg)
    try:
        o, g = oracle()
        if m.cg2d_kernel() != "block_ref":
            plan, NT, PPT, NG = m.cg2d_sum_plan()
            o.set_sum_plan(plan, NT, PPT, NG, fma=m.cg2d_fma())
        m.forward_step(nsteps)
        layout = m.step_layout()
        it, fr, lr = m.solve_history(nsteps)
        for s in range(nsteps):
            o.forward_step()
            assert (int(o.get("numIters")), o.get("firstResidual"), o.get("lastResidual")) == (it[s], fr[s], lr[s]), s
        inner = (Ellipsis,) + g.sl(1, g.sNx, 1, g.sNy)
        bad = []
        for n in OCEAN90_STATE:
            dev = m.get(n)
            ref = np.array(o.arr(n)).reshape(dev.shape)
            if not np.array_equal(dev[inner], ref[inner]):
                bad.append((n, float(np.nanmax(np.abs(dev - ref)[inner]))))
        assert not bad, bad
        return layout
    finally:
        m.close()


def test_default_mask_has_the_bit():
    """(host only) FUSE_DEFAULT above is the earlier default mask with the new bit in it."""
    assert FUSE_DEFAULT & ~SPEC2_BIT == 1 | 4 | 8 | 128 | 256 | 1024 | 2048 | 4096 | 8192 | 16384 | 32768 | 65536


# ---- config 2 re-tiled, against the oracle --------------------------------------------------
@gpu
@pytest.mark.parametrize("tiling", TILINGS, ids=["%dx%d" % t for t in TILINGS])
def test_retiled_4_step_call_vs_oracle(tiling, monkeypatch):
    from oracle.harness import ocean90_oracle
    nSx, nSy = tiling
    layout = _call_vs_oracle(_ocean90(nSx, nSy), lambda: ocean90_oracle(nSx=nSx, nSy=nSy), 4, monkeypatch)
    assert layout[KEY] and layout["specialised"] and layout["pipelined"] and layout["phi_pipelined"], layout


# ---- against the generic instantiations -----------------------------------------------------
@gpu
@pytest.mark.parametrize("tiling", LAYOUTS, ids=["%dx%d" % t for t in LAYOUTS])
@pytest.mark.parametrize("calls", [(6,), (2, 4)], ids=["6", "2+4"])
def test_pinned_against_generic(tiling, calls, monkeypatch):
    """Default mask against the mask minus the bit: the state with its halos and the solve history."""
    cfg = _ocean90(*tiling)
    off, lay_off = _run(cfg, calls, FUSE_DEFAULT & ~SPEC2_BIT, monkeypatch)
    on, lay_on = _run(cfg, calls, FUSE_DEFAULT, monkeypatch)
    assert lay_on[KEY] and lay_on["pipelined"] and lay_on["phi_pipelined"], lay_on
    assert not lay_off[KEY] and lay_off["pipelined"] and lay_off["phi_pipelined"], lay_off
    assert lay_on["specialised"] and lay_off["specialised"], (lay_on, lay_off)
    assert np.isfinite(off["uVel"]).all() and np.abs(off["uVel"]).max() > 0.0
    bad = _differences(on, off)
    assert not bad, bad


# ---- options off the pinned set -------------------------------------------------------------
OFF_PIN = {"hydrostatic": dict(quasiHydrostatic=0), "no_freezing": dict(allowFreezing=0)}


@gpu
@pytest.mark.parametrize("case", list(OFF_PIN))
def test_off_pin_generic_4_step_call_vs_oracle(case, monkeypatch):
    """One newly listed option off the pinned set, default mask: generic kernels, the oracle's bits."""
    from oracle.harness import ocean90_oracle
    over = OFF_PIN[case]
    layout = _call_vs_oracle(_ocean90(**over), lambda: ocean90_oracle(params_over=over), 4, monkeypatch)
    assert layout["pipelined"] and not layout[KEY] and not layout["specialised"], layout


# ---- a pinned option moved after 4 steps ----------------------------------------------------
@gpu
def test_late_set_param_replans(monkeypatch):
    """4 pinned steps, then allowFreezing = 0 through mgcm_set_param: the plan drops the pinned
    instantiations, and the next 4 steps are those of a model that ran the same 8 steps and the
    same move with the generic kernels throughout."""
    from mitgcm_amd._lib import check, lib
    seen = {}

    def late(m):
        m.forward_step(4)
        seen["before"] = m.step_layout()[KEY]
        check(lib().mgcm_set_param(m.h, b"allowFreezing", 0.0), "mgcm_set_param")

    cfg = _ocean90()
    a, lay_a = _run(cfg, (4,), FUSE_DEFAULT, monkeypatch, before=late)
    assert seen["before"] and not lay_a[KEY] and not lay_a["specialised"] and lay_a["pipelined"], (seen, lay_a)
    b, lay_b = _run(cfg, (4,), FUSE_DEFAULT & ~SPEC2_BIT & ~65536, monkeypatch, before=late)
    assert not seen["before"] and not lay_b[KEY] and not lay_b["specialised"], (seen, lay_b)
    bad = _differences(a, b)
    assert not bad, bad


# ---- the halo-record table (host only) ------------------------------------------------------
def _latlon_src_of(sNx, sNy, nSx, nSy, OL, walls=False):
    """srcOf of the periodic lat-lon exchange (exch1_rx.template): per 2-D point of every tile,
    the flat offset of the interior point with the wrapped global index, -1 at interior points.
    walls: the domain is closed in y -- the halo rows beyond its southern and northern edge have
    no source (-1: the points that are neither interior nor mapped)."""
    nx, ny = sNx + 2 * OL, sNy + 2 * OL
    n2 = nx * ny
    t, jj, ii = np.meshgrid(np.arange(nSx * nSy), np.arange(ny), np.arange(nx), indexing="ij")
    i, j = ii - OL + 1, jj - OL + 1
    iG = ((t % nSx) * sNx + i - 1) % (sNx * nSx)
    jG = ((t // nSx) * sNy + j - 1) % (sNy * nSy)
    st = (jG // sNy) * nSx + iG // sNx
    src = st * n2 + (jG % sNy + OL) * nx + (iG % sNx + OL)
    interior = (i >= 1) & (i <= sNx) & (j >= 1) & (j <= sNy)
    jAll = (t // nSx) * sNy + j
    outside = walls & ((jAll < 1) | (jAll > sNy * nSy))
    return np.where(interior | outside, -1, src).astype(np.int64).ravel(), interior.ravel()


@pytest.mark.parametrize("walls", [False, True], ids=["periodic", "walls_in_y"])
@pytest.mark.parametrize("tiling", LAYOUTS, ids=["%dx%d" % t for t in LAYOUTS])
def test_halo_table_is_the_arithmetic_it_replaces(tiling, walls):
    """Every entry of mgcm_halo_table against the expressions the kernels evaluated per thread:
    where the value lives, (sq / n2) * n3 + sq % n2, mg_ij_of of the owner (what calc_r_star_fac's
    range tests are made on) and the interior / mapped flags.  Config 2's grid at OL = 3, periodic
    and with halo points that have no source (flags 0, the record names the point itself)."""
    import ctypes
    from mitgcm_amd._lib import lib
    nSx, nSy = tiling
    sNx, sNy, OL, Nr = 90 // nSx, 40 // nSy, 3, 15
    nx, ny = sNx + 2 * OL, sNy + 2 * OL
    n2, n3, nT = nx * ny, nx * ny * Nr, nSx * nSy
    src, interior = _latlon_src_of(sNx, sNy, nSx, nSy, OL, walls)
    unmapped = ~interior & (src < 0)
    assert unmapped.any() == walls and interior[src[src >= 0]].all()   # (every source is an interior point)
    out = np.full(4 * n2 * nT, -7, dtype=np.int32)
    rc = lib().mgcm_halo_table(sNx, sNy, OL, OL, Nr, nT, src.ctypes.data_as(ctypes.POINTER(ctypes.c_long)),
                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert rc == 0
    rec = out.reshape(-1, 4)
    q = np.arange(n2 * nT, dtype=np.int64)
    at = np.where(src >= 0, src, q)
    assert np.array_equal(rec[:, 0], at)
    assert np.array_equal(rec[:, 1], (at // n2) * n3 + at % n2)
    ti = (rec[:, 2] & 0xffff).astype(np.int16).astype(np.int64)
    tj = (rec[:, 2] >> 16).astype(np.int64)
    loc = at % n2
    ai, aj = loc % nx - OL + 1, loc // nx - OL + 1                          # mg_ij_of
    assert np.array_equal(ti, ai) and np.array_equal(tj, aj)
    assert np.array_equal(rec[:, 3] & 1, interior.astype(np.int32))
    assert np.array_equal((rec[:, 3] & 2) != 0, src >= 0) and not (rec[:, 3] & ~3).any()
    # a point that is neither interior nor mapped: flags 0, itself, its own (i, j) outside the interior
    assert (rec[unmapped, 3] == 0).all() and np.array_equal(rec[unmapped, 0], q[unmapped])
    assert not ((ti[unmapped] >= 1) & (ti[unmapped] <= sNx) & (tj[unmapped] >= 1) & (tj[unmapped] <= sNy)).any()
    # a grid whose 3-D offsets pass 2^31 is refused, the output untouched
    big = np.full(4, -7, dtype=np.int32)
    one = np.full(1, -1, dtype=np.int64)
    assert lib().mgcm_halo_table(40000, 40000, 3, 3, 2, 1, one.ctypes.data_as(ctypes.POINTER(ctypes.c_long)),
                                 big.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == -1
    assert (big == -7).all()
