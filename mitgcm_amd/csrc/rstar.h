// rstar.h -- CALC_R_STAR's per-point work, shared by k_calc_r_star / k_rstar_exch / k_rstar_exmix
// (kernels_rstar.hip) and the end-of-step grid that also carries the next step's CALC_PHI_HYD and
// del2uv (kernels_step.hip k_rstar_exch_phi, MG_FUSE_PHIP).
#pragma once
#include "common.h"

namespace mgcm {

// CALC_R_STAR (calc_r_star.F:95-298) in one pass per 2-D point q: the new factors on
// the reference's ranges (:111-150, rStarAreaWeight = .TRUE.), EXCH_XY_RL(rStarFacC) +
// EXCH_UV_XY_RL(rStarFacW,S) by evaluating a halo point's factor at its interior source
// (lat-lon / single facet: scalar copies), then rStarDh*Dt = (Fac - Fac_old)/dtFS and
// rStarExp = Fac/Fac_old (:283-298).  Each thread reads and writes only its own point's
// factors, so the old values need no second buffer.
// The new etaH of k_exch_etaH at point q: EXCH_XY_RL of the eta k_corr_cont left in cg2d_b
// (the interior source of a halo point; the point itself inside; etaN where neither --
// fromX: the etaN SOLVE_FOR_PRESSURE's EXCH(cg2d_x) + etaN = recip_Bo*cg2d_x leaves there,
// recip_Bo*cg2d_x of the point itself, when that launch was skipped, see one_step).
__device__ __forceinline__ double eta_exch(const Dims &d, const Fields &f, const long *srcOf, long q, int fromX) {
  const long sq = srcOf[q];
  if (sq >= 0) return f.cg2d_b[sq];
  const long l = q % d.n2;
  const int i = (int)(l % d.nx) - d.OLx + 1, j = (int)(l / d.nx) - d.OLy + 1;
  if (i >= 1 && i <= d.sNx && j >= 1 && j <= d.sNy) return f.cg2d_b[q];
  return fromX ? f.recip_Bo[q] * f.cg2d_x[q] : f.etaN[q];
}

// The new factors fc, fw, fs of point q from the old ones oc, ow, os (kept where the point's
// source lies outside the reference's ranges).  WS = false: the centre factor only.
// SHORT (k_rstar_exch_phi's grid: its own CALC_R_STAR blocks and the rider, r_star_next_point;
// EXCH1 topologies, FUSE): the same values through shorter address chains -- where the value is
// computed and its (i, j) come from the point's HaloRec (one load, no division), and an interior
// point is nobody's image, so its eta is cg2d_b there without a look-up.  The expressions that
// form the factors are the ones below for both.
template <bool FUSE, bool WS = true, bool SHORT = false>
__device__ __forceinline__ void calc_r_star_fac(const Dims &d, const Params &p, const Fields &f,
                                                const long *__restrict__ srcOf, const HaloRec *__restrict__ rec, long q,
                                                int fromX, double oc, double ow, double os, double &fc, double &fw,
                                                double &fs) {
  auto inner = [&](int ii, int jj) { return ii >= 1 && ii <= d.sNx && jj >= 1 && jj <= d.sNy; };
  int i, j;
  long r;   // where the new value is computed
  if constexpr (SHORT) {
    const HaloRec h = rec[q];
    r = h.at2;
    i = h.i;
    j = h.j;
  } else {
    const long sq = srcOf[q];
    r = sq >= 0 ? sq : q;
    mg_ij_of(d, r, i, j);
  }
  // eta at qq = (ii, jj)
  auto eta = [&](long qq, int ii, int jj) {
    if constexpr (SHORT) {   // eta_exch's cases with (ii, jj) known: no index arithmetic
      if (inner(ii, jj)) return f.cg2d_b[qq];
      const long sqq = rec[qq].at2;   // (a mapped point's source is another point)
      if (sqq != qq) return f.cg2d_b[sqq];
      return fromX ? f.recip_Bo[qq] * f.cg2d_x[qq] : f.etaN[qq];
    } else {
      return FUSE ? eta_exch(d, f, srcOf, qq, fromX) : f.etaH[qq];
    }
  };
  fc = oc;
  fw = ow;
  fs = os;
  if (i >= 0 && i <= d.sNx + 1 && j >= 0 && j <= d.sNy + 1)   // kSurfC <= Nr <=> maskInC = 1
    fc = (f.maskInC[r] != 0.0) ? (eta(r, i, j) + f.Ro_surf[r] - f.R_low[r]) * f.recip_Rcol[r] : 1.0;
  if constexpr (WS) {
    // W/S factors: at the EXCH1 source as above, or (EXCH2 topology) in place on the
    // reference's ranges, their halos then refilled through the vector map (calc_r_star())
    const long rv = (!SHORT && p.cubeCorners) ? q : r;
    int iv = i, jv = j;
    if constexpr (!SHORT) mg_ij_of(d, rv, iv, jv);
    if (iv >= 1 && iv <= d.sNx + 1 && jv >= 1 && jv <= d.sNy) {
      if (f.maskInW[rv] != 0.0) {
        const double tmp = f.rSurfW[rv] - f.rLowW[rv];
        fw = (0.5 * (eta(rv - 1, iv - 1, jv) * f.rA[rv - 1] + eta(rv, iv, jv) * f.rA[rv]) * f.recip_rAw[rv] + tmp) / tmp;
      } else {
        fw = 1.0;
      }
    }
    if (iv >= 1 && iv <= d.sNx && jv >= 1 && jv <= d.sNy + 1) {
      if (f.maskInS[rv] != 0.0) {
        const double tmp = f.rSurfS[rv] - f.rLowS[rv];
        fs = (0.5 * (eta(rv - d.nx, iv, jv - 1) * f.rA[rv - d.nx] + eta(rv, iv, jv) * f.rA[rv]) * f.recip_rAs[rv] + tmp) / tmp;
      } else {
        fs = 1.0;
      }
    }
  }
}

// fuseEtaH: k_exch_etaH in the same pass (the FORWARD_STEP order exch_etaH -> CALC_R_STAR):
// each thread stores its own point's etaN, etaH, etaHnm1 (and PmEpR) and takes the etaH of
// the neighbours it reads from eta_exch, the same values k_exch_etaH stores.  The only
// cross-thread location both read and written is etaN at points neither interior nor
// mapped, which is rewritten with the value it holds.
// empNext (MG_FUSE_PIPE, with FUSE): the next step's DO_OCEANIC_PHYS ran earlier in this step
// and left its EmPmR in EmPmRnext (phys.h); this pass, the step's last reader of EmPmR, moves
// it over once it has formed PmEpR -- each thread its own point.
// TAB (k_rstar_exch_phi's grid: FUSE, EXCH1, every tile): the same pass reading the topology from
// the HaloRec table -- eta_exch's three cases from the record's flags, the factors by
// calc_r_star_fac's SHORT form -- instead of dividing 64-bit offsets
template <bool FUSE, bool TAB = false>
__device__ __forceinline__ void calc_r_star_body(const Dims &d, const Params &p, const Fields &f,
                                                 const long *__restrict__ srcOf, int lb, int fromX, int empNext = 0,
                                                 const HaloRec *__restrict__ rec = nullptr) {
  static_assert(FUSE || !TAB, "the table form is the fused pass's");
  const long q = (long)lb * blockDim.x + threadIdx.x;
  if (q >= d.n2 * d.nTiles) return;
  const int t = (int)(q / d.n2);
  if (t < d.t0 || t >= d.t0 + d.nT) return;
  if constexpr (FUSE) {   // k_exch_etaH (kernels_solve.hip), atInit = 0
    if (p.nonlinFreeSurf > 0 && p.useRealFreshWaterFlux) f.PmEpR[q] = -f.EmPmR[q];
    if (empNext) f.EmPmR[q] = f.EmPmRnext[q];
    double x;
    if constexpr (TAB) {
      const HaloRec h = rec[q];
      x = (h.flags & (MG_HR_INTERIOR | MG_HR_MAPPED)) ? f.cg2d_b[h.at2] : fromX ? f.recip_Bo[q] * f.cg2d_x[q] : f.etaN[q];
    } else {
      x = eta_exch(d, f, srcOf, q, fromX);
    }
    f.etaHnm1[q] = f.etaH[q];
    f.etaN[q] = x;
    f.etaH[q] = x;
  }
  const double oc = f.rStarFacC[q], ow = f.rStarFacW[q], os = f.rStarFacS[q];
  double fc, fw, fs;
  calc_r_star_fac<FUSE, true, TAB>(d, p, f, srcOf, rec, q, fromX, oc, ow, os, fc, fw, fs);
  f.rStarFacC[q] = fc;
  f.rStarFacW[q] = fw;
  f.rStarFacS[q] = fs;
  f.rStarDhCDt[q] = (fc - oc) / p.deltaTFreeSurf;
  f.rStarDhWDt[q] = (fw - ow) / p.deltaTFreeSurf;
  f.rStarDhSDt[q] = (fs - os) / p.deltaTFreeSurf;
  f.rStarExpC[q] = fc / oc;
  f.rStarExpW[q] = fw / ow;
  f.rStarExpS[q] = fs / os;
}

// What calc_r_star_body<true> is storing at point q in the same grid, for a reader that cannot
// wait for it (the next step's CALC_PHI_HYD, MG_FUSE_PHIP): rStarFacC and rStarDh{C,W,S}Dt formed
// by calc_r_star_fac from the factors UPDATE_R_STAR's pass kept aside (rStarFac*Prev, which no
// block of this grid writes) -- the same expressions on the same operands, so the same bits.
template <bool WS>
__device__ __forceinline__ void r_star_next_point(const Dims &d, const Params &p, const Fields &f,
                                                  const HaloRec *__restrict__ rec, long q, int fromX, double &facC,
                                                  double &dhC, double &dhW, double &dhS) {
  const double oc = f.rStarFacCPrev[q], ow = WS ? f.rStarFacWPrev[q] : 0.0, os = WS ? f.rStarFacSPrev[q] : 0.0;
  double fc, fw, fs;
  calc_r_star_fac<true, WS, true>(d, p, f, nullptr, rec, q, fromX, oc, ow, os, fc, fw, fs);
  facC = fc;
  dhC = (fc - oc) / p.deltaTFreeSurf;
  if constexpr (WS) {
    dhW = (fw - ow) / p.deltaTFreeSurf;
    dhS = (fs - os) / p.deltaTFreeSurf;
  }
}

// The 3-D offset at which a field that the end-of-step exchange is filling is read inside that
// grid: at the exchange source of (i,j,t) where it has one (the value the exchange copies into
// the point), else at the point itself (interior: stable; neither interior nor mapped: written by
// nobody).  A source is never itself an image, so nothing in the grid writes where this reads.
// The level-1 offset comes from the point's HaloRec (base3); level k lies (k-1)*n2 further.
__device__ __forceinline__ long mg_at_source3(const Dims &d, const HaloRec *__restrict__ rec, int i, int j, int t) {
  if (i >= 1 && i <= d.sNx && j >= 1 && j <= d.sNy) return MG_I3(d, i, j, 1, t);
  return rec[MG_I2(d, i, j, t)].base3;
}

}  // namespace mgcm
