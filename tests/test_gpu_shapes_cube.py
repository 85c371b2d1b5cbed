"""The cube sphere away from one or two full-width tiles per face: the family the shape sweeps
of test_gpu_shapes_step.py leave out.  With tiles of 32 x 32 or 32 x 16 every tile of the cube
has both its E and its W facet edge; here the faces are cut in x as well, so the per-tile
tileFace / tileEdge table (edge bits N=1 S=2 E=4 W=8) takes every value it can: interior tiles
(no edge), one-edge tiles, two-edge corner tiles, tiles as narrow as the halo.  That table
steers adv_cfg / mask_loc / k_advg_fill / k_advg_flux / k_advg_upd (kernels_thermo.hip),
vi_vort and the other corner fix-ups of MOM_VECINV (kernels_dyn.hip), the corner r* factors
(kernels_rstar.hip) and the EXCH2 vector maps.

  (a) advect_cs (DST3FL multi-dimensional, compressible) on 6 tilings: 6 steps, theta bit-exact
      to the oracle on the same tiling and, un-tiled, to the one-tile-per-face oracle (the one
      pinned to the reference's output.txt);
  (b) global_ocean.cs32x15 on the same tilings, 4 steps bit-exact (shapes.assert_bitexact_steps)
      with C2 tracers and with tempAdvScheme = saltAdvScheme = 33, multiDimAdvection -- the only
      place mask_loc meets land.  mgcm_init refuses GM_AdvForm with multi-dimensional
      advection whatever the DST3 scheme (30 as much as 33), so the scheme-33 runs take GM in
      the skew-flux form (GM_AdvForm = 0, GM_skewflx = 1), as test_gpu_options.py does for
      scheme 30; the C2 runs keep every option of the experiment, GM_AdvForm included;
  (e) the device EXCH2 scalar and vector exchanges against the host maps on tiles of 4 x 6
      and 3 x 3;
  (f) configs.cube_synthetic (anisotropic non-uniform metrics that differ across every rotated
      edge, random islands, u, v of full size from the first step) at odd sizes, non-square
      tiles, 1 and 31 levels, halos of 4, 3 and 2, the k-march forms, and once under r*.
The per-routine tests on (8, 8) and (16, 8) tiles are in test_gpu_cs32x15.py, the
reference-order CG2D on 48 tiles in test_gpu_cg2d_mwg_ref.py.  The oracle's side of every
re-tiling is pinned by test_oracle_shapes.py.  Every comparison with the oracle here is
np.array_equal / ==.
"""
import functools

import numpy as np
import pytest

import shapes
from test_gpu_cs32x15 import STATE
from test_gpu_monitor import _check as monitor_check

pytestmark = pytest.mark.gpu

# (sNx, sNy) of the 32 x 32 faces -> tiles = multi-workgroup CG2D parts (every tile is at most
# 1024 points, one part):
#   16 x 16  24 tiles, every one a two-edge corner tile
#   8 x 8    96 tiles: interior, one-edge and corner tiles
#   32 x 8   24 tiles, full width: E and W on all, N or S on the outer ones only
#   8 x 32   24 tiles, full height: the faces divided in x
#   16 x 8   48 tiles (the reference's adjustment.cs-32x32x1 tiling)
#   4 x 32   48 tiles as wide as the halo (OL = 4)
CS32_TILES = {(16, 16): 24, (8, 8): 96, (32, 8): 24, (8, 32): 24, (16, 8): 48, (4, 32): 48}
TILE_IDS = ["%dx%d" % t for t in CS32_TILES]

ADV33 = {"tempAdvScheme": 33, "tempVertAdvScheme": 33, "saltAdvScheme": 33, "saltVertAdvScheme": 33,
         "multiDimAdvection": 1}
# storePhiHyd4Phys = 1 on both sides: STATE holds totPhiHyd, which the device keeps only under
# that switch (the oracle always, as DIAGS_PHI_HYD does); with JMD95Z nothing reads it, so no
# other value of the run depends on it (test_gpu_cg2d_mwg_ref.py does the same)
CS32_TRACERS = {"c2": {"storePhiHyd4Phys": 1},
                "dst3fl": dict(ADV33, GM_AdvForm=0, GM_skewflx=1.0, storePhiHyd4Phys=1)}


def _monitor(m):
    bad, _ = monitor_check(m)
    assert not bad, bad


# ---- (a) advect_cs ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _advect_oracle(sNx, sNy):
    """theta of the oracle after 6 steps (tile layout) and its grid; computed once per tiling
    and shared (do not modify)."""
    from mitgcm_amd import configs
    from oracle.harness import oracle_from_config
    o, g = oracle_from_config(configs.advect_cs, sNx=sNx, sNy=sNy)
    for _ in range(6):
        o.forward_step()
    th = np.array(o.arr("theta"))
    th.setflags(write=False)
    return th, g


@pytest.mark.parametrize("tile", list(CS32_TILES), ids=TILE_IDS)
def test_advect_cs_retiled_6_steps_bitexact(tile):
    from mitgcm_amd import configs
    sNx, sNy = tile
    m = configs.make_model(configs.advect_cs, sNx=sNx, sNy=sNy)
    try:
        assert m.g.nTiles == CS32_TILES[tile]
        assert m.cg2d_parts() == CS32_TILES[tile] <= shapes.MAX_MWG_PARTS, m.cg2d_parts()
        m.forward_step(6)
        m.sync()
        dev = m.get("theta")
    finally:
        m.close()
    ref, g = _advect_oracle(sNx, sNy)
    inner = (Ellipsis,) + g.sl(1, g.sNx, 1, g.sNy)
    assert np.array_equal(dev[inner], ref.reshape(dev.shape)[inner]), float(np.abs(dev - ref.reshape(dev.shape))[inner].max())
    one, g1 = _advect_oracle(32, 32)
    assert np.array_equal(shapes.cube_untile(g, dev), shapes.cube_untile(g1, one))


# ---- (b) global_ocean.cs32x15 -----------------------------------------------------------------
CS32_RUNS = [(t, tr) for t in CS32_TILES for tr in CS32_TRACERS]


@pytest.mark.parametrize("tile,tracers", CS32_RUNS, ids=["%dx%d-%s" % (t[0], t[1], tr) for t, tr in CS32_RUNS])
def test_cs32x15_retiled_4_steps_bitexact(tile, tracers):
    from mitgcm_amd import configs
    from oracle.harness import cs32x15_oracle
    sNx, sNy = tile
    over = CS32_TRACERS[tracers]
    after = _monitor if tile == (8, 8) else None
    kernel, parts, layout = shapes.assert_bitexact_steps(
        lambda: configs.global_ocean_cs32x15(sNx=sNx, sNy=sNy, params_over=over), 4, STATE,
        oracle_factory=lambda cfg: cs32x15_oracle(sNx=sNx, sNy=sNy, params_over=over), after=after)
    print("cs32x15 on %d tiles of %d x %d, %s: CG2D %s, step layout %s" % (
        parts, sNx, sNy, tracers, kernel, sorted(k for k, v in layout.items() if v)))
    assert (kernel, parts) == ("mwg", CS32_TILES[tile])


# ---- (e) the EXCH2 exchanges on the device ----------------------------------------------------
EXCH_CASES = [(12, 3, 4, 6, 4), (9, 5, 3, 3, 3)]


@pytest.mark.parametrize("case", EXCH_CASES, ids=["n%d_Nr%d_%dx%d_OL%d" % c for c in EXCH_CASES])
def test_exchanges_device_vs_host_map(case):
    """DO_FIELDS_BLOCKING_EXCHANGES on random fields: uVel, vVel through the device vector map
    (with signs, corner fix-ups of the two-edge tiles only), theta and salt through the scalar
    map, each np.array_equal to the host gather of mitgcm_amd/exch2.py at every point, halos
    included.  Both cases have tiles as wide as the halo (sNx = OL = 4, sNx = sNy = OL = 3):
    the vector map then copies some corner-halo points from halo points, whose values from
    before the exchange it wants (exch2.py); applied as one in-place gather, as before this
    test, those entries raced with the fill of their sources and both cases failed."""
    from mitgcm_amd import configs
    from mitgcm_amd._lib import lib
    n, Nr, sNx, sNy, OL = case
    m = configs.make_model(lambda: configs.cube_synthetic(n, Nr, sNx, sNy, OL))
    try:
        g = m.g
        rng = np.random.default_rng(11)
        fld = {k: rng.standard_normal(m.get(k).shape) for k in ("uVel", "vVel", "theta", "salt")}
        for k, a in fld.items():
            m.put(k, a)
        assert lib().mgcm_blocking_exchanges(m.h) == 0
        m.sync()
        hu, hv = g.exch_uv(fld["uVel"].copy(), fld["vVel"].copy(), withSigns=True)
        want = {"uVel": hu, "vVel": hv, "theta": g.exch(fld["theta"].copy()), "salt": g.exch(fld["salt"].copy())}
        bad = {k: int((m.get(k) != a).sum()) for k, a in want.items() if not np.array_equal(m.get(k), a)}
        assert not bad, "points that differ from the host map: %s" % bad
    finally:
        m.close()


# ---- (f) the synthetic cube -------------------------------------------------------------------
FIELDS_3D = ("uVel", "vVel", "wVel", "theta", "salt", "etaN")
RSTAR = dict(ADV33, nonlinFreeSurf=4, select_rStar=2, exactConserv=1, hFacInf=0.2, hFacSup=2.0)
RSTAR_STATE = FIELDS_3D + ("etaH", "hFacC", "hFacW", "hFacS", "rStarFacC", "rStarFacW", "rStarFacS", "rStarExpC",
                           "aW2d", "aS2d", "aC2d")
# environment switches of the kernel forms (test_gpu_shapes_step.py explains them): the tracers'
# k-march takes its column-pair form only where sNx, OLx, nx and n3 are all even -- of the cases
# below (12, 3, 6, 4, 4) alone (sNx = 6, OLx = 4, nx = 14, n3 = 14 * 12 * 3)
FORMS = {"default": {}, "vi_kc3": {"MGCM_VI_KERNEL": "march", "MGCM_VI_KC": "3"},
         "tracer1": {"MGCM_TRACER_MARCH": "1"}, "tracer3": {"MGCM_TRACER_MARCH": "3"}}
# (n, Nr, sNx, sNy, OL), tracers ("c2" / "dst3fl" / "rstar": dst3fl under r*), form
SYNTH_RUNS = [
    ((12, 3, 4, 6, 4), "dst3fl", "default"),    # non-square tiles, 36 of them, no interior tile
    ((12, 3, 6, 4, 4), "dst3fl", "default"),    # the other way round
    ((12, 3, 4, 4, 4), "dst3fl", "default"),    # 54 tiles, an interior tile per face, tile width = OL
    ((9, 5, 3, 3, 3), "c2", "default"),         # odd size, interior tile, OL = 3
    ((10, 1, 5, 2, 2), "c2", "default"),        # one level, nx = 9 odd, sNy = OL = 2
    ((9, 31, 9, 3, 3), "c2", "default"),        # the deep grid whose defaults select the march forms
    ((9, 31, 9, 3, 3), "c2", "vi_kc3"),
    ((12, 3, 6, 4, 4), "c2", "tracer1"),        # the pair form of the tracers' k-march
    ((12, 3, 6, 4, 4), "c2", "tracer3"),
    ((12, 3, 6, 4, 4), "rstar", "default"),     # r* (corner r* factors) and DST3FL on a divided face
]
SYNTH_OVER = {"c2": {}, "dst3fl": ADV33, "rstar": RSTAR}


def synth_oracle(case, over):
    """The oracle of cube_synthetic(*case, params_over=over); under r* with INITIALISE_VARIA's
    r* sequence, as cs32x15_oracle runs it."""
    from mitgcm_amd import configs
    from oracle.harness import oracle_from_config
    n, Nr, sNx, sNy, OL = case
    o, g = oracle_from_config(lambda: configs.cube_synthetic(n, Nr, sNx, sNy, OL, params_over=over))
    if over.get("nonlinFreeSurf", 0) > 0:
        o.L.oracle_ini_nlfs_pickup(o.h)
    return o, g


@pytest.mark.parametrize("case,tracers,form", SYNTH_RUNS,
                         ids=["n%d_Nr%d_%dx%d_OL%d-%s-%s" % (c + (t, f)) for c, t, f in SYNTH_RUNS])
def test_cube_synthetic_4_steps_bitexact(case, tracers, form, monkeypatch):
    from mitgcm_amd import configs
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    n, Nr, sNx, sNy, OL = case
    over = SYNTH_OVER[tracers]
    after = _monitor if (case, tracers) == ((9, 5, 3, 3, 3), "c2") else None
    kernel, parts, layout = shapes.assert_bitexact_steps(
        lambda: configs.cube_synthetic(n, Nr, sNx, sNy, OL, params_over=over), 4,
        RSTAR_STATE if tracers == "rstar" else FIELDS_3D, oracle_factory=lambda cfg: synth_oracle(case, over),
        after=after)
    print("synthetic cube %s %s %s: CG2D %s, %d part(s), step layout %s" % (
        case, tracers, form, kernel, parts, sorted(k for k, v in layout.items() if v)))
    assert (kernel, parts) == ("mwg", 6 * (n // sNx) * (n // sNy))
