// gm_tensor.h -- GMREDI_CALC_TENSOR's per-point body, shared by k_gm_tensor and the fused grids
// of kernels_step.hip (kernels_thermo.hip) and by the correction step's grid that carries the
// next step's tensor (kernels_solve.hip, MG_FUSE_PIPE).
#pragma once
#include "common.h"

namespace mgcm {

// GMREDI_CALC_TENSOR (pkg/gmredi/gmredi_calc_tensor.F:231-790; skew flux, GM_ExtraDiag
// = F, all isoFac/bolFac = 1) with GMREDI_SLOPE_LIMIT's gkw91 taper
// (gmredi_slope_limit.F:280-370), one thread per (i,j,k) on i,j = 2-OL..sN+OL-1.
// sigmaX/Y (GRAD_SIGMA, grad_sigma.F:80-101) are recomputed from rhoInSitu.
__device__ __forceinline__ void gm_slope_gkw91(const Params &p, double dSx, double dSy, double dSr, double &SlopeX,
                                               double &SlopeY, double &SlopeSqr, double &taper) {
  const double GM_bigSlope = 1.0e+02, maxSlopeSqr = p.GM_maxSlope * p.GM_maxSlope;
  if (dSr != 0.0 && dSr <= p.GM_Small_Number) dSr = p.GM_Small_Number;
  if (dSr == 0.0) {
    SlopeX = dSx != 0.0 ? copysign(GM_bigSlope, dSx) : 0.0;
    SlopeY = dSy != 0.0 ? copysign(GM_bigSlope, dSy) : 0.0;
  } else {
    const double dRdSigmaLtd = 1.0 / dSr;
    SlopeX = dSx * dRdSigmaLtd;
    SlopeY = dSy * dRdSigmaLtd;
  }
  SlopeSqr = SlopeX * SlopeX + SlopeY * SlopeY;
  taper = 1.0;
  if (SlopeSqr >= p.GM_slopeSqCutoff) { SlopeSqr = p.GM_slopeSqCutoff; taper = 0.0; }
  if (SlopeSqr == 0.0) taper = 1.0;
  else if (SlopeSqr > maxSlopeSqr && SlopeSqr < p.GM_slopeSqCutoff) taper = maxSlopeSqr / SlopeSqr;
}

// O: the option set the body is compiled for (common.h)
template <class O = OptsRun>
__device__ __forceinline__ void gm_tensor_body(const Dims &d, const Params &p, const Fields &f, int lb) {
  MG_PLANE_LB(2 - d.OLx, d.nx - 2, 2 - d.OLy, d.ny - 2, z, lb)
  const int t = d.t0 + z / d.Nr, k = z % d.Nr + 1;
  const int Nr = d.Nr;
  auto rho = [&](int ii, int jj, int kk) { return f.rhoInSitu[MG_I3(d, ii, jj, kk, t)]; };
  auto sX = [&](int ii, int jj, int kk) {
    return f.maskW[MG_I3(d, ii, jj, kk, t)] * f.recip_dxC[MG_I2(d, ii, jj, t)] * (rho(ii, jj, kk) - rho(ii - 1, jj, kk));
  };
  auto sY = [&](int ii, int jj, int kk) {
    return f.maskS[MG_I3(d, ii, jj, kk, t)] * f.recip_dyC[MG_I2(d, ii, jj, t)] * (rho(ii, jj, kk) - rho(ii, jj - 1, kk));
  };
  auto sR = [&](int ii, int jj, int kk) { return f.sigmaR[MG_I3(d, ii, jj, kk, t)]; };
  const double op25 = 0.25, op5 = 0.5, gs = p.gravitySign;
  const long q3 = MG_I3(d, i, j, k, t);
  const double isopycK = p.GM_isopycK * (1.0 + 1.0) * op5, bolus_K = p.GM_background_K * (1.0 + 1.0) * op5;
  double SlopeX, SlopeY, SlopeSqr, taper;
  // Kwx, Kwy, Kwz (W points, k >= 2; k = 1 stays 0)
  double kwx = 0.0, kwy = 0.0, kwz = 0.0;
  if (k >= 2) {
    const double maskFk = f.maskC[MG_I3(d, i, j, k - 1, t)] * f.maskC[q3];
    const double dSx = op25 * (sX(i + 1, j, k - 1) + sX(i, j, k - 1) + sX(i + 1, j, k) + sX(i, j, k)) * maskFk;
    const double dSy = op25 * (sY(i, j + 1, k - 1) + sY(i, j, k - 1) + sY(i, j + 1, k) + sY(i, j, k)) * maskFk;
    gm_slope_gkw91(p, dSx, dSy, gs * sR(i, j, k), SlopeX, SlopeY, SlopeSqr, taper);
    kwx = -gs * SlopeX * taper;
    kwy = -gs * SlopeY * taper;
    kwz = SlopeSqr * taper;
  }
  const double Kgm_tmp = isopycK * 1.0 + p.GM_skewflx * bolus_K * 1.0;
  f.Kwx[q3] = Kgm_tmp * kwx;
  f.Kwy[q3] = Kgm_tmp * kwy;
  f.Kwz[q3] = (isopycK * 1.0) * kwz;
  const int kp1 = k + 1 < Nr ? k + 1 : Nr;
  const double maskp1 = k >= Nr ? 0.0 : 1.0;
  {  // Kux (U points)
    const double mW = f.maskW[q3];
    const double dSx = sX(i, j, k) * mW;
    const double dSy = op25 * (sY(i - 1, j + 1, k) + sY(i, j + 1, k) + sY(i - 1, j, k) + sY(i, j, k)) * mW;
    const double dSr = op25 * (sR(i - 1, j, k) + sR(i, j, k) + (sR(i - 1, j, kp1) + sR(i, j, kp1)) * maskp1) * mW * gs;
    gm_slope_gkw91(p, dSx, dSy, dSr, SlopeX, SlopeY, SlopeSqr, taper);
    f.Kux[q3] = fmax((p.GM_isopycK * 1.0 * op5 * (1.0 + 1.0)) * taper, p.GM_Kmin_horiz);
    if (O::gmExtraDiag(p))   // GM_EXTRA_DIAGONAL Kuz (gmredi_calc_tensor.F:808-850)
      f.Kuz[q3] = -gs * (p.GM_isopycK * 1.0 * op5 * (1.0 + 1.0) - p.GM_skewflx * p.GM_background_K * 1.0 * op5 * (1.0 + 1.0)) *
                  SlopeX * taper;
  }
  {  // Kvy (V points)
    const double mS = f.maskS[q3];
    const double dSx = op25 * (sX(i, j, k) + sX(i + 1, j, k) + sX(i, j - 1, k) + sX(i + 1, j - 1, k)) * mS;
    const double dSy = sY(i, j, k) * mS;
    const double dSr = op25 * (sR(i, j - 1, k) + sR(i, j, k) + (sR(i, j - 1, kp1) + sR(i, j, kp1)) * maskp1) * mS * gs;
    gm_slope_gkw91(p, dSx, dSy, dSr, SlopeX, SlopeY, SlopeSqr, taper);
    f.Kvy[q3] = fmax((p.GM_isopycK * 1.0 * op5 * (1.0 + 1.0)) * taper, p.GM_Kmin_horiz);
    if (O::gmExtraDiag(p))   // Kvz (gmredi_calc_tensor.F:1053-1090)
      f.Kvz[q3] = -gs * (p.GM_isopycK * 1.0 * op5 * (1.0 + 1.0) - p.GM_skewflx * p.GM_background_K * 1.0 * op5 * (1.0 + 1.0)) *
                  SlopeY * taper;
  }
  if (O::gmAdvForm(p)) {
    // GMREDI_CALC_PSI_B (gmredi_calc_psi_b.F:86-212) + GMREDI_SLOPE_PSI gkw91
    // (gmredi_slope_psi.F:196-290): bolus stream-function at the top face of level k >= 2
    double psx = 0.0, psy = 0.0;
    if (k >= 2) {
      const double halfRL = 0.5, halfSign = halfRL * gs, half_K = p.GM_background_K * (1.0 + 1.0) * op25;
      const double slopeCutoff = sqrt(p.GM_slopeSqCutoff), loc_maxSlope = p.GM_maxSlope * 1.0;
      const double maxSlopeSqr = loc_maxSlope * loc_maxSlope;
      auto psi = [&](double Slope, double dSdr) {
        if (dSdr <= p.GM_Small_Number) dSdr = p.GM_Small_Number;
        Slope = Slope / dSdr;
        double tp = 1.0;
        if (fabs(Slope) >= slopeCutoff) { Slope = copysign(slopeCutoff, Slope); tp = 0.0; }
        const double Smod = fabs(Slope);
        if (Smod > loc_maxSlope && Smod < slopeCutoff) tp = maxSlopeSqr / (Slope * Slope + p.GM_Small_Number);
        return Slope * tp * (half_K * (1.0 + 1.0));
      };
      const double mkW = f.maskW[MG_I3(d, i, j, k - 1, t)] * f.maskW[q3];
      psx = psi((sX(i, j, k - 1) + sX(i, j, k)) * halfRL * mkW, (sR(i - 1, j, k) + sR(i, j, k)) * halfSign * mkW);
      const double mkS = f.maskS[MG_I3(d, i, j, k - 1, t)] * f.maskS[q3];
      psy = psi((sY(i, j, k - 1) + sY(i, j, k)) * halfRL * mkS, (sR(i, j - 1, k) + sR(i, j, k)) * halfSign * mkS);
    }
    f.GM_PsiX[q3] = psx;
    f.GM_PsiY[q3] = psy;
  }
}

}  // namespace mgcm
