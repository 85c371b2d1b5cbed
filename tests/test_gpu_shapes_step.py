"""The whole step away from the shapes the kernels were tuned on: 4 FORWARD_STEPs of each case
bit-identical to the oracle (shapes.assert_bitexact_steps: iterations equal to the
reference-order oracle's, residuals, every dynstat value and the final fields identical to the
oracle summing CG2D in the device's order).

  * the free-size barotropic box (flux-form momentum, the fused small-grid launches) at every
    shape of test_gpu_shapes_cg2d.py;
  * global_ocean.90x40x15 (r*, CD scheme, GM, JMD95P, biharmonic viscosity, OL = 3) re-tiled
    into 45x40, 90x5, 18x8, 9x40 and 5x5 tiles, with the blocked and the multi-workgroup CG2D;
  * tutorial_baroclinic_gyre (OL = 2) re-tiled into 62x62, 2x31, 31x2, 62x1 and 1x62 tiles;
  * the synthetic LLC at 9, 15, 6, 5 and 7 points per tile edge, 3, 5, 4, 1 and 31 levels and
    halos of 4, 3 and 2, in the flat and the k-march forms of the tracer and momentum kernels.
The cube sphere (advect_cs, global_ocean.cs32x15 and a synthetic cube with their faces cut in
x and y) has a file of its own, test_gpu_shapes_cube.py.
One model of each family also runs the device MONITOR against the host restatement.
The oracle's side of the re-tilings is pinned by test_oracle_shapes.py.
"""
import pytest

import shapes
from test_gpu_monitor import _check as monitor_check
from test_gpu_refpin import STATE as OCEAN90_STATE
from test_gpu_shapes_cg2d import CASES as BOX_CASES

pytestmark = pytest.mark.gpu

FIELDS_3D = ("uVel", "vVel", "wVel", "theta", "salt", "etaN")


def _monitor(m):
    bad, _ = monitor_check(m)
    assert not bad, bad


def _record(what, kernel, parts, layout):
    print("%s: CG2D %s, %d part(s), step layout %s" % (what, kernel, parts, sorted(k for k, v in layout.items() if v)))


# ---- the barotropic box ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(BOX_CASES), ids=["%dx%d_%dx%d" % s for s in BOX_CASES])
def test_box_4_steps_bitexact(shape):
    """The kernel and part count expected of every shape: CASES of test_gpu_shapes_cg2d.py."""
    after = _monitor if shape == (45, 41, 3, 1) else None
    kernel, parts, layout = shapes.assert_bitexact_steps(shapes.box_cfg(shape), 4, shapes.BOX_FIELDS, after=after)
    _record("box %s" % (shape,), kernel, parts, layout)
    assert (kernel, parts) == (BOX_CASES[shape][0], len(BOX_CASES[shape][3]))


# ---- global_ocean.90x40x15 re-tiled ---------------------------------------------------------
# Default CG2D: the global 90 x 40 is 45 x 10 = 450 blocks of 2x4 whatever the tiling
# (k_cg2d_bxy forms its blocks on the global index space; they straddle the edges of the
# 45-, 9- and 5-wide tiles and of the 5-high ones).
# MGCM_CG2D_NOBLOCKED: the multi-workgroup solver; parts per tile = ceil(sNy / rows), rows =
# min(sNy, 1024 / sNx) (see test_gpu_shapes_cg2d.py):
#   (2, 1): tiles of 45 x 40, rows 22 -> 2 strips of 20 rows each, 4 parts;
#   (5, 5): tiles of 18 x 8, one part each, 25 parts of 144 points;
#   (1, 8): tiles of 90 x 5, one part each, 8 parts (ring of 180: the rows north and south).
# (18, 8) would be 144 parts, more than have been shown co-resident: default CG2D only.
OCEAN90 = [((2, 1), False, 1), ((1, 8), False, 1), ((5, 5), False, 1), ((10, 1), False, 1), ((18, 8), False, 1),
           ((2, 1), True, 4), ((5, 5), True, 25), ((1, 8), True, 8)]


@pytest.mark.parametrize("tiling,mwg,parts", OCEAN90,
                         ids=["%dx%d%s" % (t[0], t[1], "_mwg" if w else "") for t, w, _ in OCEAN90])
def test_ocean90_retiled_4_steps_bitexact(tiling, mwg, parts, monkeypatch):
    from mitgcm_amd import configs
    from oracle.harness import ocean90_oracle
    if mwg:
        monkeypatch.setenv("MGCM_CG2D_NOBLOCKED", "1")
    nSx, nSy = tiling
    after = _monitor if (tiling, mwg) == ((5, 5), False) else None
    kernel, got, layout = shapes.assert_bitexact_steps(
        lambda: configs.global_ocean_90x40x15(nSx=nSx, nSy=nSy), 4, OCEAN90_STATE,
        oracle_factory=lambda cfg: ocean90_oracle(nSx=nSx, nSy=nSy), after=after)
    _record("ocean90 on %d x %d tiles" % tiling, kernel, got, layout)
    assert (kernel, got) == ("mwg" if mwg else "bxy", parts)


# ---- tutorial_baroclinic_gyre re-tiled ------------------------------------------------------
# 62 % 4 != 0: k_cg2d_bxy 2x2 with 31 x 31 = 961 blocks at every tiling; tiles of 31 (odd) and
# of 2 columns or rows; (62, 1) is tiles of 1 x 62, narrower than the halo of 2: every halo
# column is then a copy from two tiles away
GYRE = [((1, 1), 2), ((31, 2), 2), ((2, 31), 2), ((2, 31), 33), ((1, 62), 2), ((62, 1), 2)]


@pytest.mark.parametrize("tiling,scheme", GYRE, ids=["%dx%d_adv%d" % (t[0], t[1], s) for t, s in GYRE])
def test_baroclinic_gyre_retiled_4_steps_bitexact(tiling, scheme):
    from mitgcm_amd import configs
    nSx, nSy = tiling
    kernel, parts, layout = shapes.assert_bitexact_steps(
        lambda: configs.baroclinic_gyre(nSx=nSx, nSy=nSy, tempAdvScheme=scheme), 4, FIELDS_3D)
    _record("baroclinic gyre on %d x %d tiles, tempAdvScheme %d" % (nSx, nSy, scheme), kernel, parts, layout)
    assert (kernel, parts) == ("bxy", 1)


# ---- the synthetic LLC ----------------------------------------------------------------------
# (n, Nr, tile, OL) -> tiles = multi-workgroup parts (every tile is one strip: tile^2 <= 1024)
LLC = {(9, 3, None, 4): 13, (15, 5, None, 3): 13, (12, 4, 6, 2): 52, (10, 1, 5, 4): 52, (14, 31, 7, 4): 52}
# The tracers' k-march (MGCM_TRACER_MARCH; the default from Nr >= 30, so on (14, 31, 7, 4) only)
# takes its 16-byte column-pair form only where sNx, OLx, nx and n3 are all even
# (launch_tracer_step, csrc/kernels_thermo.hip: `(d.sNx & 1) == 0 && (d.OLx & 1) == 0 && ...`):
#   (9, 3, None, 4)   sNx = 9 odd                      -> one-column k_tracer_march
#   (15, 5, None, 3)  sNx = 15, OLx = 3, nx = 21 odd   -> one-column k_tracer_march
#   (10, 1, 5, 4)     sNx = 5, nx = 13 odd             -> one-column k_tracer_march
#   (14, 31, 7, 4)    sNx = 7, nx = 15 odd             -> one-column k_tracer_march
#   (12, 4, 6, 2)     sNx = 6, OLx = 2, nx = 10, n3 = 400 even -> the column-pair k_tracer_march2
# so MGCM_TRACER_MARCH = 1 and 3 run the one-column march (ragged 32 x 8 thread tiles over tiles
# of 5 to 15 points) on four cases, which no other test runs, and the pair form at hx = 3 on
# the fifth.  Level chunks KC = (Nr + 4) / 5: Nr = 3, 4, 5 -> 1 (no remainder), Nr = 31 -> 7
# (chunks 7, 7, 7, 7, 3).  The in-march implicit solve (MGCM_TRACER_MARCH = 3) needs Nr > 1
# and the pair form.  MGCM_TRACER_MARCH2 = 1 (whole tile rows per workgroup) is a switch of the
# pair form: on (14, 31, 7, 4) it is inert (sNx odd, the run repeats tracer3 there: the case
# is kept as the deep grid whose defaults select the march forms), on (12, 4, 6, 2) it reaches
# the whole-rows k_tracer_march2 launch at hx = 3, TY = 85 > sNy.  MGCM_VI_KERNEL = march: the
# generic k-march of MOM_VECINV (no k_mom_vi_m2 instantiation at these block shapes),
# MGCM_VI_KC = 3 its ragged level chunks.
FORMS = {"default": {}, "tracer1": {"MGCM_TRACER_MARCH": "1"}, "tracer3": {"MGCM_TRACER_MARCH": "3"},
         "vi": {"MGCM_VI_KERNEL": "march"}, "vi_kc3": {"MGCM_VI_KERNEL": "march", "MGCM_VI_KC": "3"},
         "tracer3_rows": {"MGCM_TRACER_MARCH": "3", "MGCM_TRACER_MARCH2": "1"}}
LLC_RUNS = [(c, f) for c in LLC for f in FORMS
            if (f != "vi_kc3" or c[1] > 3) and (f != "tracer3_rows" or c in ((14, 31, 7, 4), (12, 4, 6, 2)))]


@pytest.mark.parametrize("case,form", LLC_RUNS,
                         ids=["n%d_Nr%d_t%s_OL%d-%s" % (c[0], c[1], c[2] or c[0], c[3], f) for c, f in LLC_RUNS])
def test_llc_reshaped_4_steps_bitexact(case, form, monkeypatch):
    from mitgcm_amd import configs
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    n, Nr, tile, OL = case
    after = _monitor if (case, form) == ((15, 5, None, 3), "default") else None
    kernel, parts, layout = shapes.assert_bitexact_steps(
        lambda: configs.llc_synthetic(n=n, Nr=Nr, tile=tile, OL=OL), 4, FIELDS_3D, after=after)
    _record("LLC %s %s" % (case, form), kernel, parts, layout)
    assert (kernel, parts) == ("mwg", LLC[case])
