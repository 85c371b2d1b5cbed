"""The pipelined step (MGCM_STEP_FUSE bit 16384, model.hip StepMode): the next step's
DO_OCEANIC_PHYS in this step's UPDATE_R_STAR grid and its GMREDI_CALC_TENSOR in this step's
correction-step grid, for calls of PIPE_MIN_STEPS steps or more.

Everything is compared BITWISE between the bit on and off (the bit-off model is the step as it
was): the prognostic state with its halos, every output of the hoisted pass, PmEpR, etaH,
dEtaHdt and the solve history (iterations and residuals); config 2 also against the oracle
summing CG2D in the device's order.

  * config 2 (global_ocean.90x40x15 from its pickups): one call of 3, 4, 5 and 7 steps (both
    sides of the threshold, odd and even), 3 + 4 against 7, a put of theta and of fu between two
    calls, the fields a get returns right after a call, the layout key;
  * one call of 20 steps across a change of the forcing record pair (iteration 36015);
  * three small r* grids cut from the same data (cold start, 4 levels), with closed north and
    south edges (halo rows that are neither interior nor mapped) and periodic x, freezing water
    in the first and last interior columns: a thin one-tile grid (sNy = 4), one with an odd
    number of points per level, and two tiles side by side;
  * where the pipelined step does not apply (the cube, a staggered step, the linear free
    surface) the key is off and the steps are those of the bit-off model.
"""
import functools
import os

import numpy as np
import pytest

from test_gpu_refpin import STATE as OCEAN90_STATE

pytestmark = pytest.mark.gpu

PIPE_BIT = 16384
FUSE_DEFAULT = 1 | 4 | 8 | 128 | 256 | 1024 | 2048 | 4096 | 8192 | PIPE_BIT   # common.h mg_fuse_on
PIPE_MIN_STEPS = 4                                                            # model.hip MG_PIPE_MIN_STEPS

# the outputs of DO_OCEANIC_PHYS + GMREDI_CALC_TENSOR
HEAD = ("rhoInSitu", "sigmaR", "IVDConvCount", "Kwx", "Kwy", "Kwz", "Kux", "Kvy", "SST", "SSS", "fu", "fv", "Qnet",
        "EmPmR", "surfaceForcingT", "surfaceForcingS")
FIELDS = tuple(dict.fromkeys(OCEAN90_STATE + HEAD + ("PmEpR", "etaH", "dEtaHdt", "gU", "gV")))


def _env(monkeypatch, on):
    monkeypatch.setenv("MGCM_OVERLAP", "1")   # (no timing-dependent choice of the layout)
    monkeypatch.setenv("MGCM_STEP_FUSE", str(FUSE_DEFAULT if on else FUSE_DEFAULT & ~PIPE_BIT))


def _snapshot(m, fields, nhist):
    out = {n: m.get(n) for n in fields}
    it, fr, lr = m.solve_history(nhist)
    out["cg2d_iters"], out["cg2d_init_res"], out["cg2d_last_res"] = it.astype(np.float64), fr, lr
    out["myIter"] = np.array([float(m.my_iter())])
    return out


def _differences(a, b):
    """Names whose arrays are not the same bits, with the largest difference."""
    bad = []
    for n in a:
        x, y = np.ascontiguousarray(a[n]), np.ascontiguousarray(b[n])
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append((n, float(np.nanmax(np.abs(x - y))) if x.shape == y.shape else "shape"))
    return bad


def _run(cfg, calls, fields, on, monkeypatch, between=None):
    """A model of cfg stepped by forward_step(k) for k in calls; between(m, i) runs after call i
    (not after the last).  Returns (snapshot after the last call, step_layout())."""
    from mitgcm_amd import configs
    _env(monkeypatch, on)
    m = configs.make_model(cfg)
    try:
        for i, k in enumerate(calls):
            m.forward_step(k)
            if between is not None and i + 1 < len(calls):
                between(m, i)
        return _snapshot(m, fields, min(calls[-1], 8)), m.step_layout()
    finally:
        m.close()


def _ocean90():
    from mitgcm_amd import configs
    return configs.global_ocean_90x40x15()


_OFF = {}


def _ocean90_off(nsteps, monkeypatch):
    """The bit-off model after one call of nsteps steps: computed once, shared, read-only."""
    if nsteps not in _OFF:
        snap, layout = _run(_ocean90, (nsteps,), FIELDS, False, monkeypatch)
        assert not layout["pipelined"] and layout["dyn_thermo_fused"], layout
        for a in snap.values():
            a.setflags(write=False)
        _OFF[nsteps] = snap
    return _OFF[nsteps]


# ---- config 2 from the pickup ---------------------------------------------------------------
@pytest.mark.parametrize("nsteps", [PIPE_MIN_STEPS - 1, PIPE_MIN_STEPS, PIPE_MIN_STEPS + 1, PIPE_MIN_STEPS + 3])
def test_ocean90_one_call(nsteps, monkeypatch):
    """One call on both sides of the threshold, odd and even; a get right after the call returns
    the call's last step's rhoInSitu, EmPmR, Kwx (and every other field) as the bit-off model's."""
    off = _ocean90_off(nsteps, monkeypatch)
    on, layout = _run(_ocean90, (nsteps,), FIELDS, True, monkeypatch)
    assert layout["pipelined"] == (nsteps >= PIPE_MIN_STEPS), (nsteps, layout)
    assert layout["dyn_thermo_fused"], layout
    bad = _differences(on, off)
    assert not bad, bad


def test_ocean90_split_calls(monkeypatch):
    """3 + 4 steps (a plain call, then a pipelined one starting on the other tracer buffers) and
    4 + 3 against 7 in one call."""
    off = _ocean90_off(7, monkeypatch)
    for calls in ((3, 4), (4, 3)):
        on, layout = _run(_ocean90, calls, FIELDS, True, monkeypatch)
        assert layout["pipelined"] == (calls[-1] >= PIPE_MIN_STEPS), (calls, layout)
        drop = ("cg2d_iters", "cg2d_init_res", "cg2d_last_res")   # (the history of the last call only)
        bad = _differences({k: v for k, v in on.items() if k not in drop},
                           {k: v for k, v in off.items() if k not in drop})
        assert not bad, (calls, bad)
        n = calls[-1]
        for k in drop:
            assert on[k][-n:].tobytes() == off[k][-n:].tobytes(), (calls, k)


def test_ocean90_put_between_calls(monkeypatch):
    """A call, a put of theta and of fu, another call: the stand-alone head of the second call
    reads what the host left, as the bit-off model does."""
    def between(m, i):
        th = m.get("theta")
        th[:, 0] += 0.25 * (th[:, 0] != 0.0)
        th[:, 0, 8:12, 10:14] = -2.5          # (below FREEZE_SURFACE's clamp)
        m.put("theta", th)
        m.put("fu", 1.5 * m.get("fu"))
    res = [_run(_ocean90, (5, 6), FIELDS, on, monkeypatch, between=between) for on in (False, True)]
    assert not res[0][1]["pipelined"] and res[1][1]["pipelined"]
    bad = _differences(res[1][0], res[0][0])
    assert not bad, bad


def test_ocean90_against_device_order_oracle(monkeypatch):
    """7 steps in one pipelined call against the oracle summing CG2D in the device's order: the
    state's interiors, the iteration counts and residuals of every step, bit for bit."""
    from mitgcm_amd import configs
    from oracle.harness import ocean90_oracle
    _env(monkeypatch, True)
    m = configs.make_model(configs.global_ocean_90x40x15)
    try:
        o, g = ocean90_oracle()
        plan, NT, PPT, NG = m.cg2d_sum_plan()
        o.set_sum_plan(plan, NT, PPT, NG, fma=m.cg2d_fma())
        m.forward_step(7)
        assert m.step_layout()["pipelined"]
        it, fr, lr = m.solve_history(7)
        for s in range(7):
            o.forward_step()
            assert (int(o.get("numIters")), o.get("firstResidual"), o.get("lastResidual")) == (it[s], fr[s], lr[s]), s
        inner = (Ellipsis,) + g.sl(1, g.sNx, 1, g.sNy)
        bad = []
        for n in OCEAN90_STATE:
            dev = m.get(n)
            ref = np.array(o.arr(n)).reshape(dev.shape)
            if not np.array_equal(dev[inner], ref[inner]):
                bad.append(n)
        assert not bad, bad
    finally:
        m.close()


def _trec1(it, p):
    """EXTERNAL_FIELDS_LOAD's first record at iteration it (phys.h, get_periodic_interval.F)."""
    cycle, period = p["externForcingCycle"], p["externForcingPeriod"]
    t = it * p["deltaTClock"]
    loc = t - period * 0.5 + cycle * (2 - round(t / cycle))
    return 1 + int(np.fmod(loc, cycle) / period)


def test_ocean90_across_forcing_record(monkeypatch):
    """One pipelined call in which the record pair of the monthly forcing changes, so the hoisted
    pass interpolates at myIter + 1 on both sides of the change."""
    nsteps = 20
    _, p, _, _ = _ocean90()
    recs = [_trec1(p["nIter0"] + s, p) for s in range(nsteps)]
    change = [s for s in range(1, nsteps) if recs[s] != recs[s - 1]]
    # the change falls on a step whose pass was hoisted (not the call's first), with hoisted
    # passes after it
    assert len(change) == 1 and 1 < change[0] < nsteps - 2, (recs, change)
    off, _ = _run(_ocean90, (nsteps,), FIELDS, False, monkeypatch)
    on, layout = _run(_ocean90, (nsteps,), FIELDS, True, monkeypatch)
    assert layout["pipelined"]
    bad = _differences(on, off)
    assert not bad, bad


# ---- small r* grids -------------------------------------------------------------------------
SMALL_NR = 4


def _closed_y_topology(sNx, sNy, OL, nSx):
    """EXCH1 periodic in x over nSx tiles, closed in y: the halo rows south of the first and
    north of the last interior row are their own source (neither interior nor mapped)."""
    from mitgcm_amd.topology import LatLonTopology

    class ClosedY(LatLonTopology):
        def src_of_point(self):
            if self._src is None:
                src = LatLonTopology.src_of_point(self).copy().reshape(self.nTiles, self.ny, self.nx)
                own = np.arange(src.size, dtype=np.int64).reshape(src.shape)
                src[:, :self.OLy] = own[:, :self.OLy]
                src[:, self.OLy + self.sNy:] = own[:, self.OLy + self.sNy:]
                self._src = src.ravel()
            return self._src

    return ClosedY(sNx, sNy, OL, OL, nSx, 1)


def small_rstar(Nx, Ny, nSx, x0=38, y0=6, OL=3, Nr=SMALL_NR):
    """An Nx x Ny x Nr window (origin x0, y0) of config 2's grid, bathymetry, forcing and
    Levitus start on nSx tiles side by side, with config 2's parameters (r*, real fresh-water
    flux, JMD95P, GM/Redi, CD scheme, biharmonic viscosity), started cold at iteration 0.
    Water colder than FREEZE_SURFACE's -1.9 fills the first and last interior columns."""
    from mitgcm_amd import configs
    from mitgcm_amd.grid import Grid
    d = os.path.join(configs.GOLDEN, "tutorial_global_oce_latlon")
    sNx = Nx // nSx
    assert sNx * nSx == Nx
    g = Grid(sNx, Ny, OL, OL, Nr, nSx, 1, topology=_closed_y_topology(sNx, Ny, OL, nSx))
    delR = configs.LATLON_DELR[:Nr]
    g.ini_vertical_grid(delR)
    g.ini_spherical_polar_grid(np.full(Nx, 4.0), np.full(Ny, 4.0), 4.0 * x0, -80.0 + 4.0 * y0)
    g.ini_cori(selectCoriMap=2)
    win = (Ellipsis, slice(y0, y0 + Ny), slice(x0, x0 + Nx))
    bathy = np.maximum(configs.read_bin(os.path.join(d, "bathymetry.bin"), (40, 90))[win], -float(sum(delR)))
    g.ini_depths_masks(bathy, hFacMin=0.05, hFacMinDr=50.0, gBaro=9.81)
    g.ini_cg2d(1800.0, 86400.0, 1e-13)
    _, params, _, _ = configs.global_ocean_90x40x15()
    params.update(nIter0=0, myIter=0, myTime=0.0, rSphere=g.rSphere)
    forcing = {}
    for name, fn in configs.LATLON_FORCING.items():
        rec = configs.read_bin(os.path.join(d, fn), (12, 40, 90))[win]
        forcing[name] = configs._to_tiles(g, rec * (params["rhoConstFresh"] if name == "EmPmR" else 1.0))
    mC = g.f["maskC"]

    def tracer(fn):
        a = configs._to_tiles(g, configs.read_bin(os.path.join(d, fn), (15, 40, 90))[:Nr][win])
        a = np.moveaxis(a, 0, 1).copy()
        a[mC == 0.0] = 0.0
        return a
    theta, salt = tracer("lev_t.bin"), tracer("lev_s.bin")
    for t, i in ((0, OL), (g.nTiles - 1, OL + sNx - 1)):       # first / last interior column: every level
        col = theta[t, :, OL:OL + Ny, i]
        # -8: the surface relaxation (1/60 per day towards at most 30 degrees) and Qnet warm it by a
        # few degrees over a test's steps, so the later, hoisted passes still find it below -1.9
        col[mC[t, :, OL:OL + Ny, i] != 0.0] = -8.0
    theta = g.exch(theta)
    rC, rF = g.f["rC"], g.f["rF"]
    phiRef = np.zeros(2 * Nr + 1)
    for k in range(Nr):
        phiRef[2 * k + 1] = (rC[k] - rF[0]) * 9.81 * -1.0
        phiRef[2 * k + 2] = (rF[k + 1] - rF[0]) * 9.81 * -1.0
    shape2 = (g.nTiles, g.ny, g.nx)
    state = {"theta": theta, "salt": salt, "tRef": np.full(Nr, 20.0), "sRef": np.full(Nr, 35.0),
             "pRef4EOS": np.array([1035.0 * (rC[k] - rF[0]) * 9.81 * -1.0 for k in range(Nr)]),
             "lambdaThetaClimRelax": np.full(shape2, 1.0 / 5184000.0),
             "lambdaSaltClimRelax": np.full(shape2, 1.0 / 15552000.0),
             "fu": forcing["taux"][0], "fv": forcing["tauy"][0], "Qnet": forcing["Qnet"][0],
             "EmPmR": forcing["EmPmR"][0], "SST": forcing["SST"][0], "SSS": forcing["SSS"][0], "phiRef": phiRef}
    for n in ("h0FacC", "h0FacW", "h0FacS", "recip_Rcol", "rLowW", "rLowS", "rSurfW", "rSurfS"):
        state[n] = g.f[n]
    return g, params, state, forcing


# (Nx, Ny, nSx): thin (sNy = 4); 21 x 11 = 231 points per level, odd; two tiles in x
SMALL = {"thin_24x4": (24, 4, 1), "odd_15x5": (15, 5, 1), "two_tiles_2x10x6": (20, 6, 2)}


@functools.lru_cache(maxsize=None)
def _small(case):
    return small_rstar(*SMALL[case])


def test_small_rstar_configs_freeze_and_close():
    """(host only) every small grid has freezing surface water in its first and last interior
    columns, whose images are mapped halo points, and halo rows that are neither interior nor
    mapped."""
    for case, (Nx, Ny, nSx) in SMALL.items():
        g, params, state, _ = _small(case)
        assert params["allowFreezing"] and params["nonlinFreeSurf"] > 0 and params["useRealFreshWaterFlux"]
        assert g.Nr >= 2
        src = g.topo.src_of_point().reshape(g.nTiles, g.ny, g.nx)
        own = np.arange(src.size).reshape(src.shape)
        assert (src[:, :g.OLy] == own[:, :g.OLy]).all() and (src[:, g.OLy + g.sNy:] == own[:, g.OLy + g.sNy:]).all()
        th1 = state["theta"][:, 0]
        inner = (slice(None),) + g.sl(1, g.sNx, 1, g.sNy)
        cold = th1 < -1.9
        n_inner = int(cold[inner].sum())
        n_halo = int(cold.sum()) - n_inner
        assert cold[0][g.sl(1, 1, 1, g.sNy)].any() and cold[-1][g.sl(g.sNx, g.sNx, 1, g.sNy)].any(), case
        assert n_inner > 0 and n_halo > 0, (case, n_inner, n_halo)
        mapped = (src != own)
        assert (cold & mapped).any(), case
        if case.startswith("odd"):
            assert (g.nx * g.ny) % 2 == 1
        if case.startswith("thin"):
            assert g.sNy <= 4


@pytest.mark.parametrize("case", list(SMALL))
def test_small_rstar_grids(case, monkeypatch):
    """6 steps in one call, the bit on against off: every field with its halos, theta included
    (the hoisted pass's clamp is stored exactly where the plain pass leaves it), and the hoisted
    passes did meet water below the clamp (theta(k=1) of the stepped model, as the host sees it)."""
    cfg = lambda: _small(case)
    res = [_run(cfg, (6,), FIELDS, on, monkeypatch) for on in (False, True)]
    (off, lay_off), (on, lay_on) = res
    assert lay_on["pipelined"] and lay_on["dyn_thermo_fused"] and not lay_off["pipelined"], (lay_on, lay_off)
    assert np.isfinite(off["theta"]).all() and np.isfinite(off["etaN"]).all()
    assert (off["theta"][:, 0] < -1.9).any()
    bad = _differences(on, off)
    assert not bad, bad


# ---- where the pipelined step does not apply ------------------------------------------------
def _cs32():
    from mitgcm_amd import configs
    return configs.global_ocean_cs32x15()


def _ocean90_stagger():
    from mitgcm_amd import configs
    return configs.global_ocean_90x40x15(params_over={"staggerTimeStep": 1})


def _latlon_linear():
    from mitgcm_amd import configs
    return configs.global_oce_latlon()


@pytest.mark.parametrize("cfg,fields", [(_cs32, ("uVel", "vVel", "theta", "salt", "etaN", "rhoInSitu", "Kwx", "EmPmR")),
                                        (_ocean90_stagger, FIELDS),
                                        (_latlon_linear, ("uVel", "vVel", "wVel", "theta", "salt", "etaN", "rhoInSitu",
                                                          "Kwx", "EmPmR", "surfaceForcingT"))],
                         ids=["cs32", "stagger", "linear_free_surface"])
def test_not_eligible(cfg, fields, monkeypatch):
    """The cube (EXCH2 vector maps), a staggered step and the linear free surface: the key is off
    with the bit on, and 5 steps are the bit-off model's."""
    res = [_run(cfg, (5,), fields, on, monkeypatch) for on in (False, True)]
    assert not res[0][1]["pipelined"] and not res[1][1]["pipelined"], (res[0][1], res[1][1])
    bad = _differences(res[1][0], res[0][0])
    assert not bad, bad
