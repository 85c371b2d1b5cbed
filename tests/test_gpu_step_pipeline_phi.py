"""The pipelined step's second rider (MGCM_STEP_FUSE bit 32768, with bit 16384; kernels_step.hip
k_rstar_exch_phi): the next step's CALC_PHI_HYD and del2uv in this step's last grid, beside
CALC_R_STAR + UPDATE_ETAH and the blocking exchanges, so that a step starts at the momentum grid.

Everything is compared BITWISE between bit 32768 on and off, the rest of the mask at the default
(the bit-off model is the pipelined step as it was): the prognostic state with its halos,
CALC_PHI_HYD's and del2uv's outputs, the nine r* factor fields, etaH, etaN, PmEpR, gU, gV and the
solve history.

  * three small r* grids (thin, odd plane size, two tiles; closed north and south rows, periodic
    x), 6 steps in one call; the on-model runs twice and must agree with itself bitwise (a read
    racing a write inside the merged grid would show there);
  * config 2 from its pickups: one call on both sides of the threshold, odd and even; split calls;
    a put of uVel whose halo is NOT the copy of its source between two calls (the stand-alone head
    of the next call reads the host's halo, as the plain step does); the layout key;
  * config 2, 7 steps against the oracle summing CG2D in the device's order;
  * where the pipelined step does not apply the key is off and the steps are the bit-off model's;
  * (host only) on every grid above a halo point's exchange source is never itself an image:
    the reads at the source rest on this.
"""
import numpy as np
import pytest

from test_gpu_refpin import STATE as OCEAN90_STATE
from test_gpu_step_pipeline import FUSE_DEFAULT as FUSE_WITHOUT_PHI
from test_gpu_step_pipeline import SMALL, _differences, small_rstar

gpu = pytest.mark.gpu

PHI_BIT = 32768
PHI_MIN_STEPS = 4        # model.hip MG_PIPE_MIN_STEPS: a call of fewer steps keeps the plain step
PIPE_MIN_STEPS = 4       # (the same threshold with bit 32768 off)

PHI_OUT = ("phiHydC", "totPhiHyd", "alphaRho", "dWtC", "dWtU", "dWtV", "del2u", "del2v")
RSTAR = ("rStarFacC", "rStarFacW", "rStarFacS", "rStarExpC", "rStarExpW", "rStarExpS", "rStarDhCDt", "rStarDhWDt",
         "rStarDhSDt")
FIELDS = tuple(dict.fromkeys(OCEAN90_STATE + PHI_OUT + RSTAR + ("etaH", "etaN", "PmEpR", "gU", "gV")))


def _env(monkeypatch, on):
    monkeypatch.setenv("MGCM_OVERLAP", "1")   # (no timing-dependent choice of the layout)
    monkeypatch.setenv("MGCM_STEP_FUSE", str(FUSE_WITHOUT_PHI | PHI_BIT if on else FUSE_WITHOUT_PHI))


def _snapshot(m, fields, nhist):
    out = {n: m.get(n) for n in fields}
    it, fr, lr = m.solve_history(nhist)
    out["cg2d_iters"], out["cg2d_init_res"], out["cg2d_last_res"] = it.astype(np.float64), fr, lr
    out["myIter"] = np.array([float(m.my_iter())])
    return out


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
        assert not layout["phi_pipelined"] and layout["pipelined"] == (nsteps >= PIPE_MIN_STEPS), layout
        for a in snap.values():
            a.setflags(write=False)
        _OFF[nsteps] = snap
    return _OFF[nsteps]


# ---- the small r* grids ---------------------------------------------------------------------
_SMALL_CFG = {}


def _small(case):
    if case not in _SMALL_CFG:
        _SMALL_CFG[case] = small_rstar(*SMALL[case])
    return _SMALL_CFG[case]


@gpu
@pytest.mark.parametrize("case", list(SMALL))
def test_small_rstar_grids(case, monkeypatch):
    """6 steps in one call: bit on against off, every field with its halos; and the on-model twice."""
    cfg = lambda: _small(case)
    off, lay_off = _run(cfg, (6,), FIELDS, False, monkeypatch)
    on, lay_on = _run(cfg, (6,), FIELDS, True, monkeypatch)
    again, _ = _run(cfg, (6,), FIELDS, True, monkeypatch)
    assert lay_on["phi_pipelined"] and lay_on["pipelined"] and lay_on["dyn_thermo_fused"], lay_on
    assert lay_off["pipelined"] and not lay_off["phi_pipelined"], lay_off
    assert np.isfinite(off["uVel"]).all() and np.isfinite(off["etaN"]).all()
    assert np.abs(off["rStarDhCDt"]).max() > 0.0 and np.abs(off["del2u"]).max() > 0.0   # (the riders' inputs are live)
    bad = _differences(on, off)
    assert not bad, bad
    bad = _differences(again, on)
    assert not bad, ("two runs of the on-model differ", bad)


# ---- config 2 from the pickup ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nsteps", [PHI_MIN_STEPS - 1, PHI_MIN_STEPS, PHI_MIN_STEPS + 1, PHI_MIN_STEPS + 3])
def test_ocean90_one_call(nsteps, monkeypatch):
    """One call on both sides of the threshold, odd and even, and the layout key."""
    off = _ocean90_off(nsteps, monkeypatch)
    on, layout = _run(_ocean90, (nsteps,), FIELDS, True, monkeypatch)
    assert layout["phi_pipelined"] == (nsteps >= PHI_MIN_STEPS), (nsteps, layout)
    assert layout["pipelined"] == (nsteps >= PHI_MIN_STEPS) and layout["dyn_thermo_fused"], (nsteps, layout)
    bad = _differences(on, off)
    assert not bad, bad


@gpu
def test_ocean90_split_calls(monkeypatch):
    """3 + 4 steps (a plain call, then a pipelined one starting on the other tracer buffers) and
    4 + 3 against 7 in one call."""
    off = _ocean90_off(7, monkeypatch)
    for calls in ((PHI_MIN_STEPS - 1, PHI_MIN_STEPS), (PHI_MIN_STEPS, PHI_MIN_STEPS - 1)):
        assert sum(calls) == 7
        on, layout = _run(_ocean90, calls, FIELDS, True, monkeypatch)
        assert layout["phi_pipelined"] == (calls[-1] >= PHI_MIN_STEPS), (calls, layout)
        drop = ("cg2d_iters", "cg2d_init_res", "cg2d_last_res")   # (the history of the last call only)
        bad = _differences({k: v for k, v in on.items() if k not in drop},
                           {k: v for k, v in off.items() if k not in drop})
        assert not bad, (calls, bad)
        n = calls[-1]
        for k in drop:
            assert on[k][-n:].tobytes() == off[k][-n:].tobytes(), (calls, k)


@gpu
def test_ocean90_put_uvel_halo_between_calls(monkeypatch):
    """A call, a put of uVel whose halo is deliberately not the copy of its source, another call:
    the next call's first CALC_PHI_HYD + del2uv (and momentum grid) read the host's halo."""
    g = _ocean90()[0]
    inner = (Ellipsis,) + g.sl(1, g.sNx, 1, g.sNy)
    seen = {}

    def between(m, i):
        u = m.get("uVel")
        halo = np.ones(u.shape, dtype=bool)
        halo[inner] = False
        wet = m.get("maskW") != 0.0
        u[halo & wet] += 0.03125
        src = g.topo.src_of_point()
        flat = u.reshape(g.nTiles, g.Nr, -1)
        img = np.stack([flat[src // (g.ny * g.nx), k, src % (g.ny * g.nx)].reshape(g.nTiles, g.ny, g.nx)
                        for k in range(g.Nr)], axis=1)
        seen["broken"] = int((img != u).sum())
        m.put("uVel", u)
    res = [_run(_ocean90, (5, 6), FIELDS, on, monkeypatch, between=between) for on in (False, True)]
    assert seen["broken"] > 0          # (the put halo differs from its source)
    assert res[1][1]["phi_pipelined"] and not res[0][1]["phi_pipelined"]
    bad = _differences(res[1][0], res[0][0])
    assert not bad, bad
    # and the put was seen: the state differs from the run without it
    plain, _ = _run(_ocean90, (5, 6), ("uVel",), True, monkeypatch)
    assert plain["uVel"].tobytes() != res[1][0]["uVel"].tobytes()


@gpu
def test_ocean90_against_device_order_oracle(monkeypatch):
    """7 steps in one call with the bit on against the oracle summing CG2D in the device's order:
    the state's interiors, the iteration counts and residuals of every step, bit for bit."""
    from mitgcm_amd import configs
    from oracle.harness import ocean90_oracle
    _env(monkeypatch, True)
    m = configs.make_model(configs.global_ocean_90x40x15)
    try:
        o, g = ocean90_oracle()
        plan, NT, PPT, NG = m.cg2d_sum_plan()
        o.set_sum_plan(plan, NT, PPT, NG, fma=m.cg2d_fma())
        m.forward_step(7)
        assert m.step_layout()["phi_pipelined"]
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


@gpu
@pytest.mark.parametrize("cfg,fields", [(_cs32, ("uVel", "vVel", "theta", "salt", "etaN", "phiHydC", "totPhiHyd")),
                                        (_ocean90_stagger, FIELDS),
                                        (_latlon_linear, ("uVel", "vVel", "wVel", "theta", "salt", "etaN", "phiHydC",
                                                          "gU", "gV"))],
                         ids=["cs32", "stagger", "linear_free_surface"])
def test_not_eligible(cfg, fields, monkeypatch):
    """The cube, a staggered step and the linear free surface: the key is off with the bit on, and
    5 steps are the bit-off model's."""
    res = [_run(cfg, (5,), fields, on, monkeypatch) for on in (False, True)]
    assert not res[0][1]["phi_pipelined"] and not res[1][1]["phi_pipelined"], (res[0][1], res[1][1])
    assert not res[1][1]["pipelined"], res[1][1]
    bad = _differences(res[1][0], res[0][0])
    assert not bad, bad


# ---- host only ------------------------------------------------------------------------------
def test_a_source_is_never_an_image():
    """srcOf[srcOf[q]] is the source itself (the device's -1) on every grid the tests above run the
    rider on: the three small grids and config 2."""
    grids = {case: _small(case)[0] for case in SMALL}
    grids["ocean90"] = _ocean90()[0]
    for name, g in grids.items():
        src = np.asarray(g.topo.src_of_point(), dtype=np.int64)
        own = np.arange(src.size, dtype=np.int64)
        assert src.shape == (g.nTiles * g.ny * g.nx,), name
        assert (src >= 0).all() and (src < src.size).all(), name
        mapped = src != own
        assert mapped.any(), name
        assert (src[src] == src).all(), name            # a source is its own source
        # and every source of a mapped point is interior
        s = src[mapped] % (g.ny * g.nx)
        i, j = s % g.nx - g.OLx, s // g.nx - g.OLy
        assert ((i >= 0) & (i < g.sNx) & (j >= 0) & (j < g.sNy)).all(), name
