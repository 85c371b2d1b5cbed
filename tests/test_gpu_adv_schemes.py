"""Multi-dimensional tracer advection with first-order upwind (1), DST2 (20) and OS7MP (7): the
device against tests/gad_reference.py (a numpy restatement that tests/test_gad_reference.py pins
to the oracle and to closed forms on the CPU), np.array_equal on tile interiors.

  1  advect_xy(OL=4), salt on 1 / 20 / 7, 80 single steps compared every 16th, tiles 20 x 10 and
     10 x 10 (the periodic wrap across tiles; a tile barely wider than two overlaps); scheme 7 at
     the default OL = 3 is refused;
  2  a thin doubly periodic box, 12 x 9 x 5 in 2 x 1 tiles, random partial cells with columns one
     and two levels deep, random u, v, w and tracers: every clipped index km4..kp3 of the vertical
     OS7MP stencil, both signs of w;
  3  the baroclinic gyre (OL = 4, 2 x 2 and 1 x 1 tiles) from its three-step state with the +12 K
     anomaly: theta after a pure-advection THERMODYNAMICS, two-pass route and
     multiDimCompressible, and gAdv of a full-physics call;
  4  passive tracers on [7, 20, 1, 33, 7] on both routes (MGCM_PTR_BATCH = 0 / 1), with the
     documented launch count of three scheme families, two-pass and k_ptr_advg_plane;
  5  GM_AdvForm's residual flow on global_ocean.90x40x15(OL=4) with scheme 7;
  6  EXCH2, schemes 1 and 20 only -- a weaker guarantee, no numpy driver for the cube's passes:
     the flux code is the one pinned above and the drivers are unchanged, so what is checked is
     that re-tiling the faces and the two passive-tracer routes give the same bits, and that
     scheme 1 on a uniform tracer gives the scheme-33 result (both fluxes are uTrans * T);
  7  forward_step(6), replayed from the step graph, against six single steps with scheme 7.

Before these schemes were built every make_model below ended in MgcmError at mgcm_init.
"""
import functools

import numpy as np
import pytest

import gad_reference as gr
from test_gpu_ptracers import _exch3, _inner, _wet_random
from test_gpu_ptracers_sweep import _env

pytestmark = pytest.mark.gpu

NEW = (1, 20, 7)


def _eq(dev, ref, what):
    assert dev.shape == ref.shape, what
    assert np.array_equal(dev, ref), (what, float(np.abs(dev - ref).max()), int((dev != ref).sum()))


def _set_iter(m, it):
    from mitgcm_amd._lib import lib
    lib().mgcm_set_param(m.h, b"myIter", float(it))


# ---- 1: advect_xy --------------------------------------------------------------------------------
def _advect_cfg(scheme, nSx, nSy, OL=4):
    from mitgcm_amd import configs

    def cfg():
        g, p, s = configs.advect_xy(nSx=nSx, nSy=nSy, OL=OL)
        p.update(saltAdvScheme=scheme, saltVertAdvScheme=scheme)
        return g, p, s
    return cfg


@pytest.mark.parametrize("tiling", [(1, 2), (2, 2)], ids=["20x10", "10x10"])
@pytest.mark.parametrize("scheme", NEW)
def test_advect_xy_80_steps(scheme, tiling):
    from mitgcm_amd import configs
    cfg = _advect_cfg(scheme, *tiling)
    g, p, s = cfg()
    assert (g.sNx, g.sNy, g.OLx) == (20 // tiling[0], 20 // tiling[1], 4)
    inner, dT = gr.interior(g), p["deltaTtracer"]
    S, ref = s["salt"].copy(), {}
    for n in range(1, 81):
        gAdv, _ = gr.gad_advection(g, S, s["uVel"], s["vVel"], np.zeros_like(S), scheme, dT)
        S = g.exch(S + dT * gAdv)
        if n % 16 == 0:
            ref[n] = S[inner].copy()
    m = configs.make_model(cfg)
    try:
        for n in range(1, 81):
            m.forward_step(1)
            if n % 16 == 0:
                _eq(m.get("salt")[inner], ref[n], "salt, scheme %d, step %d" % (scheme, n))
        assert np.abs(ref[80] - s["salt"][inner]).max() > 0.1
    finally:
        m.close()


def test_os7mp_refused_at_overlap_3():
    from mitgcm_amd import configs
    from mitgcm_amd._lib import MgcmError
    with pytest.raises(MgcmError) as e:
        configs.make_model(_advect_cfg(7, 1, 2, OL=3))
    assert "saltAdvScheme 7" in str(e.value) and "OLx, OLy >= 4" in str(e.value), str(e.value)


# ---- 2: the thin box -----------------------------------------------------------------------------
def _thin_box(schemeT, schemeS, seed=20261021):
    """12 x 9 x 5, doubly periodic cartesian, OL = 4, two tiles of 6 x 9; partial cells, about a
    sixth of the columns land, one level or two levels deep; momStepping off, both tracers advected
    only.  dx = dy = 10 km, deltaT = 1000 s: |u|, |v| <= 5 m/s and |w| <= 0.5 drC / deltaT keep
    every CFL number at or below 0.5."""
    from mitgcm_amd.grid import Grid
    Nx, Ny, delR = 12, 9, [40.0, 60.0, 80.0, 100.0, 120.0]
    g = Grid(6, 9, 4, 4, 5, 2, 1)
    g.ini_vertical_grid(delR)
    g.ini_cartesian_grid(np.full(Nx, 10.0e3), np.full(Ny, 10.0e3), 0.0, 0.0)
    g.ini_cori(0.0, 0.0, selectCoriMap=1)
    rng = np.random.default_rng(seed)
    depth = rng.uniform(150.0, 400.0, (Ny, Nx))
    kind = rng.random((Ny, Nx))
    depth[kind < 0.15] = 0.0
    depth[(kind >= 0.15) & (kind < 0.25)] = rng.uniform(15.0, 40.0, (Ny, Nx))[(kind >= 0.15) & (kind < 0.25)]
    depth[(kind >= 0.25) & (kind < 0.35)] = rng.uniform(50.0, 100.0, (Ny, Nx))[(kind >= 0.25) & (kind < 0.35)]
    g.ini_depths_masks(-depth, hFacMin=0.1, hFacMinDr=5.0, gBaro=9.81)
    dt = 1000.0
    g.ini_cg2d(dt, dt, 1e-13)
    params = dict(deltaTMom=dt, deltaTFreeSurf=dt, deltaTClock=dt, deltaTtracer=dt, abEps=0.1, rhoConst=999.8,
                  gravity=9.81, gBaro=9.81, momStepping=0, tempStepping=1, tempAdvection=1, tempForcing=0,
                  saltStepping=1, saltForcing=0, tempAdvScheme=schemeT, tempVertAdvScheme=schemeT,
                  saltAdvScheme=schemeS, saltVertAdvScheme=schemeS, multiDimAdvection=1, diffKhT=0.0, diffKrT=0.0,
                  diffKhS=0.0, diffKrS=0.0, implicitDiffusion=0, ivdc_kappa=0.0, exactConserv=0, cg2dMaxIters=100)
    shp = (g.nTiles, g.Nr, g.ny, g.nx)
    u = _exch3(g, rng.uniform(-5.0, 5.0, shp)) * g.f["maskW"]
    v = _exch3(g, rng.uniform(-5.0, 5.0, shp)) * g.f["maskS"]
    drC = np.asarray(g.f["drC"])[:g.Nr][None, :, None, None]
    w = _exch3(g, rng.uniform(-0.5, 0.5, shp) * drC / dt) * g.f["maskC"]
    w[:, 0] = 0.0
    state = {"uVel": u, "vVel": v, "wVel": w, "theta": _wet_random(g, rng), "salt": 30.0 + _wet_random(g, rng),
             "tRef": np.full(5, 3.0), "sRef": np.full(5, 33.0)}
    return g, params, state


@pytest.mark.parametrize("schemes", [(7, 1), (20, 7), (1, 20)], ids=["T7_S1", "T20_S7", "T1_S20"])
def test_thin_box_vertical_clips(schemes):
    from mitgcm_amd import configs
    cfg = lambda: _thin_box(*schemes)
    g, p, s = cfg()
    mC, w = g.f["maskC"], s["wVel"]
    inner = gr.interior(g)
    depth = mC[inner].sum(axis=1)
    assert (depth == 0).any() and (depth == 1).any() and (depth == 2).any() and (depth == 5).any()
    wetface = (mC[:, 1:] * mC[:, :-1] > 0.0)[inner]
    assert (w[:, 1:][inner][wetface] > 0.0).any() and (w[:, 1:][inner][wetface] < 0.0).any()
    dT = p["deltaTtracer"]
    drC = np.asarray(g.f["drC"])[:g.Nr][None, :, None, None]
    for vel, rd in ((s["uVel"], g.f["recip_dxC"][:, None]), (s["vVel"], g.f["recip_dyC"][:, None]), (w, 1.0 / drC)):
        assert np.abs(vel * dT * rd).max() <= 0.5
    m = configs.make_model(cfg)
    try:
        m.thermodynamics()
        for name, scheme in zip(("theta", "salt"), schemes):
            gAdv, _ = gr.gad_advection(g, s[name], s["uVel"], s["vVel"], w, scheme, dT)
            want = (s[name] + dT * gAdv)[inner]
            assert np.abs(want - s[name][inner]).max() > 1e-3
            _eq(m.get(name)[inner], want, "%s, scheme %d" % (name, scheme))
    finally:
        m.close()


# ---- 3: the baroclinic gyre ----------------------------------------------------------------------
GYRE_STATE = ("uVel", "vVel", "wVel", "theta", "gtNm1", "etaN")
PURE = dict(diffKhT=0.0, diffKrT=0.0, implicitDiffusion=0, ivdc_kappa=0.0, tempForcing=0)


def _gyre_cfg(nS, scheme, **over):
    from mitgcm_amd import configs

    def cfg():
        g, p, s = configs.baroclinic_gyre(nSx=nS, nSy=nS, tempAdvScheme=scheme, OL=4)
        p.update(multiDimAdvection=1)
        p.update(over)
        return g, p, s
    return cfg


@functools.lru_cache(maxsize=None)
def _gyre_three_step_state(nS):
    """The experiment itself (scheme 2) three steps on, theta with the +12 K anomaly of
    test_gpu_3d.py at the same global cells for both tilings; halos exchanged."""
    from mitgcm_amd import configs
    cfg = _gyre_cfg(nS, 2)
    g = cfg()[0]
    m = configs.make_model(cfg)
    try:
        m.forward_step(3)
        m.sync()
        st = {n: m.get(n) for n in GYRE_STATE}
        it = m.my_iter()
    finally:
        m.close()
    bump = np.zeros((g.Nr, 62, 62))
    bump[1, 37:43, 35:47] = 12.0
    th = st["theta"]
    for t in range(g.nTiles):
        bi, bj = t % nS, t // nS
        th[t][(slice(None),) + g.sl(1, g.sNx, 1, g.sNy)] += bump[:, bj * g.sNy:(bj + 1) * g.sNy, bi * g.sNx:(bi + 1) * g.sNx]
    st["theta"] = _exch3(g, th) * (g.f["maskC"] > 0.0)
    assert np.abs(st["wVel"]).max() > 0.0
    return g, st, it


def _gyre_model(nS, scheme, over):
    from mitgcm_amd import configs
    g, st, it = _gyre_three_step_state(nS)
    m = configs.make_model(_gyre_cfg(nS, scheme, **over))
    for n, v in st.items():
        m.put(n, v)
    _set_iter(m, it)
    return g, st, m


@pytest.mark.parametrize("comp", [0, 1], ids=["two_pass", "compressible"])
@pytest.mark.parametrize("nS", [2, 1], ids=["2x2", "1x1"])
@pytest.mark.parametrize("scheme", NEW)
def test_gyre_pure_advection_theta(scheme, nS, comp):
    g, st, m = _gyre_model(nS, scheme, dict(PURE, multiDimCompressible=comp))
    try:
        dT = m.params["deltaTtracer"]
        m.thermodynamics()
        gAdv, _ = gr.gad_advection(g, st["theta"], st["uVel"], st["vVel"], st["wVel"], scheme, dT, comp=bool(comp))
        inner = gr.interior(g)
        want = (st["theta"] + dT * gAdv)[inner]
        assert np.abs(want - st["theta"][inner]).max() > 1e-4
        _eq(m.get("theta")[inner], want, "theta")
    finally:
        m.close()


@pytest.mark.parametrize("comp", [0, 1], ids=["two_pass", "compressible"])
@pytest.mark.parametrize("nS", [2, 1], ids=["2x2", "1x1"])
@pytest.mark.parametrize("scheme", NEW)
def test_gyre_full_physics_gadv(scheme, nS, comp):
    """The configuration's own diffusion, IVDC, implicit solve and relaxation: GAD_ADVECTION's
    tendency is the scheme's part of that launch sequence (the rest is pinned by the existing tests)."""
    g, st, m = _gyre_model(nS, scheme, dict(multiDimCompressible=comp))
    try:
        assert m.params["implicitDiffusion"] == 1 and m.params["ivdc_kappa"] == 1.0 and m.params["diffKhT"] == 1000.0
        dT = m.params["deltaTtracer"]
        m.thermodynamics()
        gAdv, _ = gr.gad_advection(g, st["theta"], st["uVel"], st["vVel"], st["wVel"], scheme, dT, comp=bool(comp))
        inner = gr.interior(g)
        assert np.abs(gAdv[inner]).max() > 0.0
        _eq(m.get("gAdv")[inner], gAdv[inner], "gAdv")
        assert np.isfinite(m.get("theta")).all()
    finally:
        m.close()


# ---- 4: passive tracers --------------------------------------------------------------------------
PTR_SCHEMES = (7, 20, 1, 33, 7)
# launch_ptracers_batch: the passes of each scheme family present (here OS7MP, DST2U1 and DST3)
# are launches of their own -- k_ptr_adv_x, _y, _r on the two-pass route, k_ptr_advg_plane and
# k_ptr_adv_r in the general form -- then one right-hand side (no GM/Redi) and no implicit solve
PTR_BATCHED_LAUNCHES = {0: 3 * 3 + 1, 1: 3 * 2 + 1}


@pytest.mark.parametrize("comp", [0, 1], ids=["two_pass", "plane_kernel"])
@pytest.mark.parametrize("batch", [0, 1])
def test_gyre_ptracers_mixed_families(batch, comp):
    from mitgcm_amd import configs
    g, st, it = _gyre_three_step_state(2)
    rng = np.random.default_rng(520)
    specs = [dict(advScheme=s, diffKh=0.0, diffKr=0.0, init=_wet_random(g, rng)) for s in PTR_SCHEMES]
    over = dict(implicitDiffusion=0, ivdc_kappa=0.0, multiDimCompressible=comp)
    with _env(MGCM_PTR_BATCH=batch):
        m = configs.make_model(_gyre_cfg(2, 33, **over), ptracers=specs)
        try:
            for n, v in st.items():
                m.put(n, v)
            _set_iter(m, it)
            dT = m.params["deltaTtracer"]
            m.thermodynamics()
            route = m.ptracers_route()
            print("MGCM_PTR_BATCH=%d, multiDimCompressible=%d: %r" % (batch, comp, route))
            if batch:
                assert route == {"route": "batched", "launches": PTR_BATCHED_LAUNCHES[comp]}, route
            else:
                assert route["route"] == "functional", route
            inner = gr.interior(g)
            for no, sp in enumerate(specs, 1):
                gAdv, _ = gr.gad_advection(g, sp["init"], st["uVel"], st["vVel"], st["wVel"], sp["advScheme"], dT,
                                           comp=bool(comp))
                want = (sp["init"] + dT * gAdv)[inner]
                assert np.abs(want - sp["init"][inner]).max() > 1e-4
                _eq(m.get("pTracer%02d" % no)[inner], want, "pTracer%02d (scheme %d)" % (no, sp["advScheme"]))
        finally:
            m.close()


# ---- 5: the residual flow ------------------------------------------------------------------------
@pytest.mark.parametrize("tracer", ["salt", "theta"])
def test_ocean90_residual_flow_os7mp(tracer):
    """gAdv is the model's one scratch field, salt's after a call that steps both tracers on
    scheme 7; for theta's, salt goes back to scheme 2 (it then leaves gAdv alone; the residual
    flow is still formed for theta)."""
    from mitgcm_amd import configs
    over = dict(GM_AdvForm=1, GM_skewflx=0.0, multiDimAdvection=1, tempAdvScheme=7, tempVertAdvScheme=7)
    if tracer == "salt":
        over.update(saltAdvScheme=7, saltVertAdvScheme=7)
    m = configs.make_model(lambda: configs.global_ocean_90x40x15(OL=4, params_over=over))
    try:
        g = m.g
        assert g.OLx == 4
        T = m.get(tracer)
        if tracer == "theta":
            # nothing at the surface near freezing: FREEZE_SURFACE (DO_OCEANIC_PHYS, ahead of the
            # tracer steps of the same call) then leaves theta as the reference below reads it
            T[:, 0] = np.maximum(T[:, 0], -1.0)
            m.set("theta", T)
        m.thermodynamics()
        assert m.gm_res_flow()
        flow = [m.get(n) for n in ("uRes", "vRes", "wRes")]
        assert not np.array_equal(flow[0], m.get("uVel")) and np.abs(m.get("GM_PsiX")).max() > 0.0
        f = dict(g.f)
        for n in ("hFacC", "hFacW", "hFacS", "recip_hFacC"):   # r*: the device's current factors
            f[n] = m.get(n)
        gAdv, _ = gr.gad_advection(g, T, *flow, 7, m.params["deltaTtracer"], f=f)
        inner = gr.interior(g)
        assert np.abs(gAdv[inner]).max() > 0.0
        _eq(m.get("gAdv")[inner], gAdv[inner], "gAdv of " + tracer)
    finally:
        m.close()


# ---- 6: EXCH2, schemes 1 and 20 ------------------------------------------------------------------
def _adv(scheme, **over):
    return dict(dict(tempAdvScheme=scheme, tempVertAdvScheme=scheme, saltAdvScheme=scheme, saltVertAdvScheme=scheme,
                     multiDimAdvection=1), **over)


def _cube_cfg(over, tile=None):
    from mitgcm_amd import configs
    return lambda: configs.cube_synthetic(12, 3, tile, tile, OL=4, params_over=over)


def _llc_cfg(over, tile=None):
    from mitgcm_amd import configs

    def cfg():
        """llc_synthetic draws its tracers per tile and starts at rest: here theta, salt and a flow
        of 0.3 N(0,1) m/s are drawn on the facets' index space, one ocean at every tiling."""
        g, p, s = configs.llc_synthetic(n=8, Nr=3, tile=tile, OL=4)
        p.update(over)
        rng = np.random.default_rng(88)
        draw = lambda sc: configs._facets_to_tiles(g, [sc * rng.standard_normal((g.Nr, fNy, fNx)) for fNx, fNy in g.topo.facet_dims])
        wet = g.f["maskC"] > 0.0
        s["theta"] = g.exch(s["tRef"][None, :, None, None] + draw(0.5)) * wet
        s["salt"] = g.exch(35.0 + draw(0.05)) * wet
        u, v = g.topo.exchange_uv(draw(0.3), draw(0.3), True)
        s["uVel"], s["vVel"] = u * g.f["maskW"], v * g.f["maskS"]
        return g, p, s
    return cfg


EXCH2 = {"cube": (_cube_cfg, 6), "llc": (_llc_cfg, 4)}


def _to_faces(g, a):
    """Tile interiors of a (nTiles, Nr, ny, nx) field on the faces' index space: {face: (Nr, fNy, fNx)}."""
    topo, out = g.topo, {}
    for t in range(g.nTiles):
        tid = t + 1
        fa = out.setdefault(topo.face[tid], {})
        fa[(topo.tBy[tid], topo.tBx[tid])] = a[t][(slice(None),) + g.sl(1, g.sNx, 1, g.sNy)]
    faces = {}
    for f, parts in out.items():
        ny = max(by + p.shape[1] for (by, bx), p in parts.items())
        nx = max(bx + p.shape[2] for (by, bx), p in parts.items())
        full = np.full((a.shape[1], ny, nx), np.nan)
        for (by, bx), p in parts.items():
            full[:, by:by + p.shape[1], bx:bx + p.shape[2]] = p
        faces[f] = full
    return faces


@pytest.mark.parametrize("topo", list(EXCH2))
@pytest.mark.parametrize("scheme", [33, 1, 20])
def test_exch2_retiled_faces_same_bits(scheme, topo):
    """(a) theta and salt after 2 steps are the same on whole faces and on the faces cut into
    tiles.  momStepping is off: the flow is the configuration's initial one at every tiling, and
    no sum over tiles (the pressure solve's) stands between the tiling and the tracers -- with
    momentum stepped the CG2D sums run in tile order and no scheme is bit-identical across
    tilings.  Scheme 33 is the control: its kernels compute what they computed before the
    families, and it satisfies the same comparison."""
    from mitgcm_amd import configs
    mk, small = EXCH2[topo]
    over = _adv(scheme, momStepping=0)
    res = []
    for tile in (None, small):
        cfg = mk(over, tile)
        g = cfg()[0]
        m = configs.make_model(cfg)
        try:
            m.forward_step(1)
            m.forward_step(1)
            m.sync()
            res.append((g, {n: _to_faces(g, m.get(n)) for n in ("theta", "salt")}, cfg()[2]))
        finally:
            m.close()
    (g0, a, s0), (g1, b, _) = res
    assert g1.nTiles > g0.nTiles
    for n in ("theta", "salt"):
        assert sorted(a[n]) == sorted(b[n])
        for f in a[n]:
            _eq(a[n][f], b[n][f], "%s, face %d" % (n, f))
        before = _to_faces(g0, s0[n])
        assert any(not np.array_equal(a[n][f], before[f]) for f in a[n]), n


@pytest.mark.parametrize("topo", list(EXCH2))
def test_exch2_ptracers_batched_equals_functional(topo):
    """(b) tracers on 1, 20 and 33 (two families): MGCM_PTR_BATCH = 1 against 0, halos included."""
    from mitgcm_amd import configs
    mk, small = EXCH2[topo]
    cfg = mk(dict(multiDimAdvection=1), small)
    g = cfg()[0]
    rng = np.random.default_rng(61)
    specs = [dict(advScheme=s, diffKr=1e-5, init=_wet_random(g, rng)) for s in (1, 20, 33, 20)]
    res = {}
    for batch in (1, 0):
        with _env(MGCM_PTR_BATCH=batch, MGCM_TRACER_MARCH=0):
            m = configs.make_model(cfg, ptracers=specs)
            try:
                for _ in range(3):
                    m.forward_step(1)
                m.sync()
                res[batch] = ({no: m.get("pTracer%02d" % no) for no in range(1, 5)}, m.ptracers_route())
            finally:
                m.close()
    assert res[1][1]["route"] == "batched" and res[0][1]["route"] == "functional", (res[1][1], res[0][1])
    # two families in the general form (2 launches each), one right-hand side, the implicit solve
    assert res[1][1]["launches"] == 2 * 2 + 1 + cfg()[1]["implicitDiffusion"], res[1][1]
    for no in range(1, 5):
        _eq(res[1][0][no], res[0][0][no], "pTracer%02d" % no)
        assert not np.array_equal(res[1][0][no][_inner(g)], specs[no - 1]["init"][_inner(g)])


@pytest.mark.parametrize("topo", list(EXCH2))
def test_exch2_upwind_on_a_uniform_tracer_equals_the_oracles_dst3fl(topo):
    """(c) with a uniform tracer every flux of both schemes is exactly uTrans * T, so the device's
    scheme 1 gives the bits of the oracle's scheme 33 (one pure-advection THERMODYNAMICS)."""
    from mitgcm_amd import configs
    from oracle.harness import oracle_from_config
    mk, small = EXCH2[topo]
    pure = dict(PURE, diffKhS=0.0, diffKrS=0.0, saltForcing=0)
    o, g = oracle_from_config(mk(_adv(33, **pure), small))
    uni = {"theta": np.full((g.nTiles, g.Nr, g.ny, g.nx), 7.25), "salt": np.full((g.nTiles, g.Nr, g.ny, g.nx), 29.0)}
    for n, v in uni.items():
        o.arr(n).reshape(v.shape)[:] = v
    o.L.oracle_oceanic_phys(o.h)
    o.L.oracle_thermodynamics(o.h)
    m = configs.make_model(mk(_adv(1, **pure), small))
    try:
        for n, v in uni.items():
            m.put(n, v)
        m.thermodynamics()
        for n, v in uni.items():
            dev, ref = m.get(n)[_inner(g)], np.array(o.arr(n)).reshape(v.shape)[_inner(g)]
            _eq(dev, ref, n)
            assert np.isfinite(dev).all()
    finally:
        m.close()


def test_os7mp_refused_on_the_cube():
    from mitgcm_amd import configs
    from mitgcm_amd._lib import MgcmError
    with pytest.raises(MgcmError) as e:
        configs.make_model(_cube_cfg(_adv(7)))
    assert "tempAdvScheme 7" in str(e.value) and "EXCH2" in str(e.value) and "OLx, OLy >= 8" in str(e.value), str(e.value)
    with pytest.raises(MgcmError) as e:
        configs.make_model(_cube_cfg(dict(multiDimAdvection=1)), ptracers=[dict(advScheme=20), dict(advScheme=7)])
    assert "pTracer02: advScheme 7" in str(e.value) and "EXCH2" in str(e.value), str(e.value)


# ---- 7: the replayed step graph ------------------------------------------------------------------
def test_gyre_os7mp_graph_replay_equals_single_steps():
    from mitgcm_amd import configs
    cfg = _gyre_cfg(2, 7)
    a, b = configs.make_model(cfg), configs.make_model(cfg)
    try:
        a.forward_step(6)
        for _ in range(6):
            b.forward_step(1)
        a.sync()
        b.sync()
        for n in ("uVel", "vVel", "wVel", "theta", "etaN"):
            _eq(a.get(n), b.get(n), n)
        assert not np.array_equal(a.get("theta")[_inner(a.g)], cfg()[2]["theta"][_inner(a.g)])
    finally:
        a.close()
        b.close()

