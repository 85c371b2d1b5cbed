"""The CG2D kernels alone, away from the shapes they were tuned on: full, single-block and
tile-straddling k_cg2d_bxy grids, the fall-through to 2x2 blocks and to the multi-workgroup
solver, parts smaller than a wave, strips that do not divide the tile, sNy = 1, and the
reference-order k_cg2d_block at 1, 2 and 4 points per thread.

The domain is shapes.box (a barotropic channel of free size with islands and varying
depths).  Every case first asserts the kernel form it is there for -- worked out from
choose_bxy / build_mwg (csrc/model.hip) and written beside the case -- and then solves a
seeded right-hand side, compared with a dense float64 solve of the same operator
(shapes.dense_cg2d_solution; pinned against the oracle by test_oracle_shapes.py):
  * iterations within 1 of the reference-order oracle's;
  * x exactly 0.0 on land;
  * err_dev <= 2 * err_oracle, both max|x - dense| / max|dense| on the wet points, err_oracle
    from the CPU oracle: the two solves stop at the same tolerance, so their truncation errors
    have the same size, the order of the sums moves them at roundoff only, and the factor of
    2 leaves room for one iteration more or less.
"""
import numpy as np
import pytest

import shapes

pytestmark = pytest.mark.gpu

# How choose_bxy / build_mwg decide (Nx, Ny the global size, nPts = Nx*Ny):
#   k_cg2d_bxy 3x2 on 512 threads  where Nx % 3 == 0, Ny even and Nx/3 * Ny/2 <= 512, or as few
#     once the all-land blocks are left out (test_gpu_cg2d_compact.py; no case here);
#   k_cg2d_bxy 2x4 on 512 threads  where Nx % 2 == 0, Ny % 4 == 0 and Nx/2 * Ny/4 <= 512;
#   k_cg2d_bxy 2x2 on 1024 threads where Nx, Ny even and Nx/2 * Ny/2 <= 1024;
#   otherwise the multi-workgroup solver: 1024 threads x 1 point per part (cg2d_mwg_geometry);
#   every tile cut into strips of rows = min(sNy, 1024 / sNx, shrunk until 2 (sNx + rows) <=
#   1024 ring slots) rows, that is n = ceil(sNy / rows) parts per tile, part k holding rows
#   1 + k sNy / n .. (k + 1) sNy / n; the parts are pinned to one XCD while there are <= 32.
# Each case: (Nx, Ny, nSx, nSy) -> kernel, threads, points per thread, points per workgroup
# (blocks x points per block, or rows x sNx of every part), pinned
CASES = {
    # 32 x 16 = 512 blocks of 2x4: every thread of the 512 owns a block, 4096 points
    (64, 64, 1, 1): ("bxy", 512, 8, [4096], 0),
    # one block of 2x4: 511 idle threads
    (2, 4, 1, 1): ("bxy", 512, 8, [8], 0),
    # 62 % 4 != 0: falls through to 2x2, 32 x 31 = 992 blocks of 1024
    (64, 62, 1, 1): ("bxy", 1024, 4, [3968], 0),
    # 62 % 4 != 0: 31 x 31 = 961 blocks of 2x2, one block column per tile of 2 x 31 (the block
    # rows straddle the tile edge at j = 31 | 32)
    (62, 62, 31, 2): ("bxy", 1024, 4, [3844], 0),
    # 45 x 11 = 495 blocks of 2x4 on tiles of 45 x 44: block column 23 straddles the tile edge
    (90, 44, 2, 1): ("bxy", 512, 8, [3960], 0),
    # even, but 46 % 4 != 0 and 46 x 23 = 1058 blocks of 2x2 > 1024: multi-workgroup; rows =
    # 1024 / 92 = 11, 5 strips of 9, 9, 9, 9, 10 rows
    (92, 46, 1, 1): ("mwg", 1024, 1, [828, 828, 828, 828, 920], 1),
    # odd: multi-workgroup; tiles of 15 x 41 = 615 points, one part each
    (45, 41, 3, 1): ("mwg", 1024, 1, [615, 615, 615], 1),
    # one part of 35 points (less than one wave); every periodic neighbour is the part's own:
    # no ring, nothing exported (the import table once polled an export granule nobody wrote)
    (7, 5, 1, 1): ("mwg", 1024, 1, [35], 1),
    # 33 parts of 3 x 9 = 27 points: less than one wave each, and one part more than are pinned
    (33, 27, 11, 3): ("mwg", 1024, 1, [27] * 33, 0),
    # sNy = 1 (narrower than the halo): 3 parts of one row of 126; a part's ring is the rows
    # north and south of it (its west and east neighbours are its own), its second ring empty
    (126, 3, 1, 3): ("mwg", 1024, 1, [126, 126, 126], 1),
    # rows = 1024 / 45 = 22: 2 strips of 20 and 21 rows, which do not divide 41
    (45, 41, 1, 1): ("mwg", 1024, 1, [900, 945], 1),
}
IDS = ["%dx%d_%dx%d" % s for s in CASES]
# cg2dRefOrder cases: shape -> points per thread of k_cg2d_block
REF_CASES = {(7, 5, 1, 1): 1,      # 35 points, 989 idle threads
             (45, 41, 3, 1): 2,    # 1845 points on 3 tiles: 821 threads own 2
             (64, 64, 2, 2): 4}    # 4096 points on 4 tiles: the most it takes
# shapes.BOX_SHAPES is the one list of shapes: test_oracle_shapes.py pins the reference of each
assert set(CASES) | set(REF_CASES) == set(shapes.BOX_SHAPES)


def _assert_form(m, shape):
    from mitgcm_amd._lib import lib
    kernel, NT, PPT, sizes, pinned = CASES[shape]
    assert m.cg2d_kernel() == kernel, (shape, m.cg2d_kernel())
    assert lib().mgcm_get_param(m.h, b"cg2dKernel") in (3.0, 4.0, 5.0, 6.0)   # 1 and 2 are retired
    plan, nt, ppt, ng = m.cg2d_sum_plan()
    got = [int(n) for n in (plan.reshape(ng, nt * ppt) >= 0).sum(axis=1)]
    assert (nt, ppt, got) == (NT, PPT, sizes), (shape, nt, ppt, got)
    assert m.cg2d_parts() == len(sizes) <= shapes.MAX_MWG_PARTS
    assert int(lib().mgcm_get_param(m.h, b"cg2dPinned")) == pinned


def _solve_and_compare(shape, sr):
    from mitgcm_amd import configs
    ref = shapes.box_reference(shape, sr)
    g, b = ref["g"], ref["b"]
    m = configs.make_model(shapes.box_cfg(shape, **({"useSRCGSolver": 1} if sr else {})))
    try:
        _assert_form(m, shape)
        x, first, _, last, iters, _ = m.cg2d(b, np.zeros_like(b), 2000, -1)
    finally:
        m.close()
    err_dev = shapes.rel_err(g, x, ref["dense"])
    print("box %s%s: %s, iterations %d (oracle %d), err_dev %.3e err_oracle %.3e" % (
        shape, " CG2D_SR" if sr else "", CASES[shape][0], iters, ref["iters_oracle"], err_dev, ref["err_oracle"]))
    assert abs(iters - ref["iters_oracle"]) <= 1, (iters, ref["iters_oracle"])
    inner = (slice(None),) + g.sl(1, g.sNx, 1, g.sNy)
    assert np.all(x[inner][g.f["maskInC"][inner] == 0.0] == 0.0)
    assert np.isfinite(x[inner]).all()
    assert err_dev <= 2.0 * ref["err_oracle"], (err_dev, ref["err_oracle"])


@pytest.mark.parametrize("shape", list(CASES), ids=IDS)
def test_box_cg2d_vs_dense_solve(shape):
    _solve_and_compare(shape, False)


@pytest.mark.parametrize("shape", [(45, 41, 3, 1), (33, 27, 11, 3)], ids=lambda s: "%dx%d_%dx%d" % s)
def test_box_cg2d_sr_mwg_vs_dense_solve(shape):
    """useSRCGSolver (CG2D_SR) in the multi-workgroup solver, pinned and not; the oracle it is
    compared with runs CG2D_SR too."""
    _solve_and_compare(shape, True)


# cg2dRefOrder: k_cg2d_block<PPT> on one workgroup of 1024 threads, PPT the smallest of 1, 2, 4
# with nPts <= 1024 PPT (cg2d_block_ppt, csrc/kernels_solve.hip)
@pytest.mark.parametrize("shape,ppt", list(REF_CASES.items()), ids=["ppt1", "ppt2", "ppt4"])
def test_box_block_ref_4_steps_bitexact(shape, ppt):
    """4 steps with CG2D summed in the reference's order, bit-identical to the plain oracle."""
    from mitgcm_amd._lib import lib
    from oracle.harness import oracle_from_config
    Nx, Ny = shape[:2]
    assert 1024 * (ppt // 2) < Nx * Ny <= 1024 * ppt

    def after(m):   # no k_cg2d_bxy tables are built beside k_cg2d_block's: nothing is left out
        assert lib().mgcm_get_param(m.h, b"cg2dDroppedBlocks") == 0

    kernel, parts, _ = shapes.assert_bitexact_steps(
        shapes.box_cfg(shape, cg2dRefOrder=1), 4, shapes.BOX_FIELDS,
        oracle_factory=lambda cfg: oracle_from_config(shapes.box_cfg(shape)), after=after)
    assert (kernel, parts) == ("block_ref", 1)
