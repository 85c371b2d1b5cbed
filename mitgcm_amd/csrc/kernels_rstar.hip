// kernels_rstar.hip -- the r* coordinate of the non-linear free surface on the MI355X
// (nonlinFreeSurf = 4, select_rStar = 2; BASELINE config 2, global_ocean.90x40x15).
//
// Reference: model/src/calc_r_star.F:55-298   (rStarFac from etaH, EXCH, rStarExp/DhDt)
//            model/src/update_r_star.F:48-131 (hFac = h0Fac*rStarFac and reciprocals)
//            model/src/update_cg2d.F:49-199   (CG2D operator + preconditioner from hFac)
//
// Every kernel is elementwise or a short per-column sum over a 2-D field of a few
// thousand points: latency/launch bound.  Halo points are filled from their interior
// source (srcOf, the EXCH map of the tile topology) inside the same pass, because
// EXCH copies values that are computed by the same expression as the source's.
#include "common.h"
#include "launch.h"
#include "phys.h"
#include "rstar.h"
#include "ucg2d.h"

namespace mgcm {

// CALC_R_STAR's per-point pass: rstar.h calc_r_star_body
template <bool FUSE>
__global__ void __launch_bounds__(256) k_calc_r_star(Dims d, Params p, Fields f, const long *__restrict__ srcOf, int fromX) {
  calc_r_star_body<FUSE>(d, p, f, srcOf, (int)blockIdx.x, fromX);
}
// The end of FORWARD_STEP in one grid: CALC_R_STAR (with EXCH(eta) + UPDATE_ETAH, FUSE) on
// the first nbR blocks and DO_FIELDS_BLOCKING_EXCHANGES (k_exchange_multi's nbX x nz x nF
// grid, flattened) on the rest -- independent: CALC_R_STAR reads eta and writes the 2-D r*
// factors, the exchanges copy the 3-D state's halos.
template <bool FUSE>
__global__ void __launch_bounds__(256) k_rstar_exch(Dims d, Params p, Fields f, const long *__restrict__ srcOf, int nbR,
                                                    XFields x, const long *__restrict__ map, int nHalo, int *ctr, int nbX,
                                                    int nzMax, int fromX, int empNext) {
  const int b = (int)blockIdx.x;
  if (b < nbR) { calc_r_star_body<FUSE>(d, p, f, srcOf, b, fromX, empNext); return; }
  const int r = b - nbR;
  exchange_multi_body(d, x, map, nHalo, ctr, r % nbX, (r / nbX) % nzMax, r / (nbX * nzMax));
}

// CALC_R_STAR (with EXCH(eta) + UPDATE_ETAH, FUSE) on the first nbR blocks and
// DO_STAGGER_FIELDS_EXCHANGES (k_exchange_mixed's nbH x nz x (1 + x.n) grid, flattened: the
// vector pair u, v and the scalar fields) on the rest, in one grid -- independent: CALC_R_STAR
// reads eta and writes the 2-D r* factors, the exchanges copy u, v, w's halos
template <bool FUSE>
__global__ void __launch_bounds__(256) k_rstar_exmix(Dims d, Params p, Fields f, const long *__restrict__ srcOf, int nbR,
                                                     int fromX, double *u, double *v, int nzUV,
                                                     const long *__restrict__ uvMap, int nU, int nV, XFields x,
                                                     const long *__restrict__ map, int nHalo, int nbH, int nzMax) {
  const int b = (int)blockIdx.x;
  if (b < nbR) { calc_r_star_body<FUSE>(d, p, f, srcOf, b, fromX); return; }
  const int r = b - nbR;
  exchange_mixed_body(d, u, v, nzUV, uvMap, nU, nV, x, map, nHalo, nullptr, r % nbH, (r / nbH) % nzMax, r / (nbH * nzMax));
}

// UPDATE_R_STAR(.TRUE.) (update_r_star.F:60-92) and UPDATE_CG2D part 1
// (update_cg2d.F:82-143) in one pass over the columns of every 2-D point (column frame,
// common.h MG_COLF): each thread rewrites hFac = h0Fac*rStarFac and recip_hFac = 1/hFac
// (where wet; USE_MASK_AND_NO_IF undefined) at its levels, k-parallel and coalesced over i,
// and stages the operator terms faceArea*recip_dx/yC of its levels in LDS; thread (c, 0)
// then sums aW2d, aS2d in k order on 1..sNx+1 x 1..sNy+1 and scales them by
// cg2dNorm*implicSurfPress*implicDiv2DFlow (0 elsewhere).
// SFP: SOLVE_FOR_PRESSURE's right-hand side (k_sfp_rhs, kernels_solve.hip) in the same
// column pass (FORWARD_STEP: UPDATE_R_STAR + UPDATE_CG2D, then CALC_DIV_GHAT): the flux terms
// read hFacW(i+1) / hFacS(j+1) of the neighbouring columns, which this pass is rewriting, so
// they are formed from h0Fac*rStarFac there (the expression that column stores: same bits).
// opIn = 0: the operator was built at the start of the step (ucg2d.h, MG_FUSE_OPE) -- hFac only.
// nbPc > 0: the operator was built in an earlier launch of the step (opIn = 0) and UPDATE_CG2D's
// preconditioner rides here, on the first nbPc logical blocks (ucg2d_p_point; the column
// frame on the rest)
// PH (MG_FUSE_PIPE): the next step's DO_OCEANIC_PHYS on the first nbPh logical blocks
// (phys.h phys_hoist_body: it reads the new theta and salt, totPhiHyd, h0FacC*rStarFacC and
// EmPmR, none of which this pass writes, and writes nothing this pass reads)
// PH = 2 (MG_FUSE_PHIP): also keeps the factors it read in rStarFac{C,W,S}Prev, each column its
// own point -- the old factors of this step's CALC_R_STAR, for the next step's CALC_PHI_HYD riding
// in CALC_R_STAR's grid (rstar.h r_star_next_point)
// O (common.h): the option set the riders and the column frame are compiled for.  The pinned
// instantiation is the pipelined step's launch: the operator and the preconditioner were built
// beside DYNAMICS (opIn = 0, nbPc = 0; launch_update_r_star_cg2d refuses it anything else), so
// neither the operator's sums nor ucg2d_p_point are compiled into it
template <bool SFP, int PH, class O = OptsRun>
__global__ void __launch_bounds__(256) k_update_r_star_cg2d_a(Dims d, Params p, Fields f, int nc, int opIn,
                                                              const long *__restrict__ srcOf, int nbPc,
                                                              const int *iterPtr, int nbPh) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  int lb = mg_xcd_block();
  if constexpr (PH != 0) {
    if (lb < nbPh) { phys_hoist_body<O>(d, p, f, iterPtr, srcOf, lb); return; }
    lb -= nbPh;
  }
  if constexpr (!O::pinned) {
    if (lb < nbPc) { ucg2d_p_point(d, p, f, srcOf, lb); return; }
    lb -= nbPc;
  }
  MG_COLF_LB(1 - d.OLx, d.nx, 1 - d.OLy, d.ny, nc, lb)
  const int NS = d.Nr * NC_;
  double *sW = lds, *sS = lds + NS;
  double *fE = lds + 2 * NS, *fW = lds + 3 * NS, *fN = lds + 4 * NS, *fS = lds + 5 * NS;   // SFP only
  const long q = MG_I2(d, i, j, t);
  const bool opAny = !O::pinned && opIn && O::opEveryStep(p);
  const bool op = opAny && i >= 1 && i <= d.sNx + 1 && j >= 1 && j <= d.sNy + 1;
  const bool inner = i >= 1 && i <= d.sNx && j >= 1 && j <= d.sNy;
  if (valid) {
    const double fc = f.rStarFacC[q], fw = f.rStarFacW[q], fs = f.rStarFacS[q];
    if constexpr (PH == 2) {
      if (kk == 0) { f.rStarFacCPrev[q] = fc; f.rStarFacWPrev[q] = fw; f.rStarFacSPrev[q] = fs; }
    }
    double fwE = 0.0, fsN = 0.0;
    if (SFP && inner) { fwE = f.rStarFacW[MG_I2(d, i + 1, j, t)]; fsN = f.rStarFacS[MG_I2(d, i, j + 1, t)]; }
    MG_COLF_K(k) {
      const long q3 = MG_I3(d, i, j, k, t);
      const double hC = f.h0FacC[q3] * fc, hW = f.h0FacW[q3] * fw, hS = f.h0FacS[q3] * fs;
      f.hFacC[q3] = hC;
      f.hFacW[q3] = hW;
      f.hFacS[q3] = hS;
      if (f.maskC[q3] != 0.0) f.recip_hFacC[q3] = 1.0 / hC;
      if (f.maskW[q3] != 0.0) f.recip_hFacW[q3] = 1.0 / hW;
      if (f.maskS[q3] != 0.0) f.recip_hFacS[q3] = 1.0 / hS;
      const int me = (k - 1) * NC_ + cc;
      if (op) {
        double faceArea = f.dyG[q] * f.drF[k - 1] * hW;
        sW[me] = faceArea * f.recip_dxC[q];
        faceArea = f.dxG[q] * f.drF[k - 1] * hS;
        sS[me] = faceArea * f.recip_dyC[q];
      }
      if (SFP) {
        if (O::cdScheme(p)) {
          f.uNM1[q3] = f.uVel[q3];
          f.vNM1[q3] = f.vVel[q3];
        }
        if (inner) {   // k_sfp_rhs's CALC_DIV_GHAT flux terms of level k
          const double drF = f.drF[k - 1];
          const long qE = MG_I3(d, i + 1, j, k, t), qN = MG_I3(d, i, j + 1, k, t);
          fE[me] = f.dyG[MG_I2(d, i + 1, j, t)] * drF * (f.h0FacW[qE] * fwE) * f.gU[qE] / p.deltaTMom;
          fW[me] = f.dyG[q] * drF * hW * f.gU[q3] / p.deltaTMom;
          fN[me] = f.dxG[MG_I2(d, i, j + 1, t)] * drF * (f.h0FacS[qN] * fsN) * f.gV[qN] / p.deltaTMom;
          fS[me] = f.dxG[q] * drF * hS * f.gV[q3] / p.deltaTMom;
        }
      }
    }
  }
  __syncthreads();
  if (!valid || kk != 0) return;
  if (opAny) {
    double aW = 0.0, aS = 0.0;
    if (op) {
      for (int k = 1; k <= d.Nr; k++) {
        const int me = (k - 1) * NC_ + cc;
        aW = aW + sW[me];
        aS = aS + sS[me];
      }
      aW = aW * p.cg2dNorm * p.implicSurfPress * p.implicDiv2DFlow;
      aS = aS * p.cg2dNorm * p.implicSurfPress * p.implicDiv2DFlow;
    }
    f.aW2d[q] = aW;
    f.aS2d[q] = aS;
  }
  if (SFP) sfp_rhs_column<O>(d, p, f, q, inner, fE, fW, fN, fS, NC_, cc);
}

// UPDATE_CG2D part 2 (ucg2d.h ucg2d_p_point)
__global__ void __launch_bounds__(256) k_update_cg2d_p(Dims d, Params p, Fields f, const long *__restrict__ srcOf) {
  ucg2d_p_point(d, p, f, srcOf, (int)blockIdx.x);
}

hipError_t launch_calc_r_star(const Dims &d, const Params &p, const Fields &f, const long *srcOf, hipStream_t s,
                              bool fuseEtaH, int fromX) {
  const long n = d.n2 * d.nTiles;
  hipLaunchKernelGGL(fuseEtaH ? k_calc_r_star<true> : k_calc_r_star<false>, dim3((unsigned)((n + 255) / 256)), dim3(256),
                     0, s, d, p, f, srcOf, fromX);
  return hipGetLastError();
}

hipError_t launch_rstar_exch(const Dims &d, const Params &p, const Fields &f, const long *srcOf, bool fuseEtaH,
                             const XFields &x, const long *map, int nHalo, int *ctr, hipStream_t s, int fromX, int empNext) {
  const long n = d.n2 * d.nTiles;
  const int nbR = (int)((n + 255) / 256);
  int nzMax = 1;
  for (int q = 0; q < x.n; q++) nzMax = x.nz[q] > nzMax ? x.nz[q] : nzMax;
  const int nbX = ((nHalo > 0 ? nHalo : 1) + 255) / 256;
  const unsigned nb = (unsigned)(nbR + nbX * nzMax * (x.n > 0 ? x.n : 1));
  hipLaunchKernelGGL(fuseEtaH ? k_rstar_exch<true> : k_rstar_exch<false>, dim3(nb), dim3(256), 0, s, d, p, f, srcOf, nbR, x,
                     map, nHalo, ctr, nbX, nzMax, fromX, fuseEtaH ? empNext : 0);
  return hipGetLastError();
}

hipError_t launch_rstar_exmix(const Dims &d, const Params &p, const Fields &f, const long *srcOf, bool fuseEtaH, int fromX,
                              double *u, double *v, int nzUV, const long *uvMap, int nU, int nV, const XFields &x,
                              const long *map, int nHalo, hipStream_t s) {
  const long n = d.n2 * d.nTiles;
  const int nbR = (int)((n + 255) / 256);
  int nzMax = nzUV;
  for (int q = 0; q < x.n; q++) nzMax = x.nz[q] > nzMax ? x.nz[q] : nzMax;
  const int nh = (nU + nV) > nHalo ? nU + nV : nHalo;
  const int nbH = ((nh > 0 ? nh : 1) + 255) / 256;
  const unsigned nb = (unsigned)(nbR + nbH * nzMax * (1 + x.n));
  hipLaunchKernelGGL(fuseEtaH ? k_rstar_exmix<true> : k_rstar_exmix<false>, dim3(nb), dim3(256), 0, s, d, p, f, srcOf, nbR,
                     fromX, u, v, nzUV, uvMap, nU, nV, x, map, nHalo, nbH, nzMax);
  return hipGetLastError();
}

// opEarly: the operator and preconditioner were built beside DYNAMICS (launch_dyn_thermo);
// pcHere (with opEarly): only the operator was, the preconditioner rides in this launch
// iterPtr non-null: the next step's DO_OCEANIC_PHYS rides at the head of the grid; keepFac with it:
// the factors are also kept in rStarFac*Prev
// spec (StepPlan::spec2): the instantiation compiled for the pinned option set (common.h OptsGO90),
// which exists for the pipelined step's launch only: sfp, opEarly without pcHere, iterPtr, keepFac
hipError_t launch_update_r_star_cg2d(const Dims &d, const Params &p, const Fields &f, const long *srcOf, hipStream_t s,
                                     bool sfp, bool opEarly, bool pcHere, const int *iterPtr, bool keepFac, bool spec) {
  const long n = d.n2 * d.nTiles;
  const unsigned nb = (unsigned)((n + 255) / 256);
  const long ncol = (long)d.nx * d.ny * d.nT;
  const int nArr = sfp ? 6 : 2;
  const int nc = mg_colf_nc(ncol, d.Nr, nArr);
  auto kPlain = k_update_r_star_cg2d_a<false, 0>, kSfp = k_update_r_star_cg2d_a<true, 0>,
       kSfpPhys = k_update_r_star_cg2d_a<true, 1>, kSfpPhysKeep = k_update_r_star_cg2d_a<true, 2>;
  MG_ALLOW_LDS(kPlain);
  MG_ALLOW_LDS(kSfp);
  const int nbPc = (opEarly && pcHere && p.nonlinFreeSurf > 2) ? (int)nb : 0;
  if (spec && !(sfp && opEarly && !pcHere && iterPtr && keepFac && opts_match(p))) return hipErrorInvalidValue;
  if (iterPtr) {
    if (!sfp) return hipErrorInvalidValue;   // (one_step pipelines only the fused right-hand side's layout)
    MG_ALLOW_LDS(kSfpPhys);
    MG_ALLOW_LDS(kSfpPhysKeep);
    const int nbPh = phys_hoist_blocks(d);
    auto kPinned = k_update_r_star_cg2d_a<true, 2, OptsGO90>;
    MG_ALLOW_LDS(kPinned);
    hipLaunchKernelGGL(spec ? kPinned : keepFac ? kSfpPhysKeep : kSfpPhys, dim3(mg_colf_blocks(ncol, nc) + (unsigned)(nbPc + nbPh)), dim3(256),
                       mg_colf_lds(d.Nr, nc, nArr), s, d, p, f, nc, opEarly ? 0 : 1, srcOf, nbPc, iterPtr, nbPh);
  } else if (keepFac) {
    return hipErrorInvalidValue;
  } else
    hipLaunchKernelGGL(sfp ? kSfp : kPlain, dim3(mg_colf_blocks(ncol, nc) + (unsigned)nbPc), dim3(256),
                       mg_colf_lds(d.Nr, nc, nArr), s, d, p, f, nc, opEarly ? 0 : 1, srcOf, nbPc, (const int *)nullptr, 0);
  if (p.nonlinFreeSurf > 2 && !opEarly) hipLaunchKernelGGL(k_update_cg2d_p, dim3(nb), dim3(256), 0, s, d, p, f, srcOf);
  return hipGetLastError();
}

}  // namespace mgcm
