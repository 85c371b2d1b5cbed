// cg2d.h -- the host interface of the CG2D solvers: the launchers and geometry queries that
// kernels_solve.hip and kernels_cg2d_mwg.hip define and model.hip calls, declared once so that
// the compiler checks every definition and every call against the same signature.
#pragma once
#include "common.h"

namespace mgcm {

// ---- k_cg2d_bxy: BX x BY points per thread, NT threads, one workgroup (kernels_solve.hip)
int cg2d_bxy_variants();
// geometry of variant v; -1 when v names none
int cg2d_bxy_geometry(int v, int *bx, int *by, int *nt);
// nbx / blkx / nBlk: the block tables of variant v (model.hip build_bxy).
// dropG / nDrop / guardHit: the points of the all-land blocks the tables leave out, scanned for
// a non-zero by the prologue, and the word it sets on one (nullptr, 0, nullptr: none left out).
hipError_t launch_cg2d_bxy(int v, const Dims &d, const Params &p, const Fields &f, const unsigned *nbx, const int *blkx,
                           int nBlk, int maxIters, int nIterMin, SolveRecord *rec, int *stepCounter, const int *dropG,
                           int nDrop, int *guardHit, hipStream_t s);

// ---- k_cg2d_block: one point-per-thread workgroup of 1024 summing in the reference's order
// (cg2dRefOrder), up to cg2d_ref_max_points() points (kernels_solve.hip)
int cg2d_ref_max_points();
// points per thread (1, 2 or 4) for nPts points; 0 past cg2d_ref_max_points()
int cg2d_block_ppt(int nPts);
// nbr / gofs: the neighbour and offset tables of the padded points (model.hip build_block)
hipError_t launch_cg2d_block(const Dims &d, const Params &p, const Fields &f, const unsigned *nbr, const int *gofs,
                             int nPts, int maxIters, int nIterMin, SolveRecord *rec, int *stepCounter, hipStream_t s);

// ---- k_cg2d_mwg: persistent, one workgroup per part (kernels_cg2d_mwg.hip)
// threads per part, own points per thread, ring points per thread
int cg2d_mwg_geometry(int *nt, int *opt, int *rpt);
// parts [g0, g0 + gN) of T; gN < 0: every part
hipError_t launch_cg2d_mwg(const Dims &d, const Params &p, const Fields &f, const MwgTables &T, int maxIters,
                           int nIterMin, SolveRecord *rec, int *stepCounter, hipStream_t s, int g0 = 0, int gN = -1);

}  // namespace mgcm
