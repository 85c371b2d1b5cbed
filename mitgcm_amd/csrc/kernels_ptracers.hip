// kernels_ptracers.hip -- pkg/ptracers on the device: every passive tracer of a batch per launch.
//
// PTRACERS_INTEGRATE (pkg/ptracers/ptracers_integrate.F:150-420) takes each tracer in use
// through SALT_INTEGRATE's sequence with the tracer's own parameters: CALC_3D_DIFFUSIVITY,
// GAD_ADVECTION (multi-dimensional schemes) or the advection inside GAD_CALC_RHS, the forcing
// (PTRACERS_APPLY_FORCING, ptracers_apply_forcing.F:76-92, from PTRACERS_FORCING_SURF's
// surfaceForcingPTr, ptracers_forcing_surf.F:60-75), ADAMS_BASHFORTH2 on the tendency,
// FREESURF_RESCALE_G, TIMESTEP_TRACER, GAD_IMPLICIT_R and CYCLE_TRACER.  One tracer at a time
// that is launch_tracer_step with the tracer's TracerArgs (the functional route, every
// topology).  On the small lat-lon grids a launch is a few microseconds of latency and a tracer
// takes up to five, so here the tracer index is a dimension of the grid: the kernels read the
// tracers' TracerArgs from a device table and run the bodies the one-tracer kernels run
// (adv_x/y/r_body, tracer_rhs_body, tracer_impl_body: kernels_thermo.hip) -- the same bits, at
// most five launches whatever the number of tracers (six when some take GM/Redi and some do
// not).  Opt-in, MGCM_PTR_BATCH=1: where the tracers hide beside the pressure solve a handful
// of them cost nothing either way, and the batched route wins from about 8 tracers on
// (model.hip ptr_batched).
//
// The tracers of a batch run concurrently, so each has its own gAdv / advScr1 / advScr2 / T* /
// c' scratch (model.hip's third arena); the bodies reach the multi-dimensional scratch through
// Fields pointers only (no arena-index addressing of those three), so a Fields copy with the
// three pointers moved is enough.
//
// Included by kernels_step.hip (one translation unit with kernels_thermo.hip's bodies).
#pragma once

namespace mgcm {

// the tracer of this block and its logical block inside the tracer's own grid: tracers in
// list order (the host sorts the longest bodies first), blocks XCD-remapped as elsewhere
struct PtrBlock { int it, lb; };
__device__ __forceinline__ PtrBlock ptr_block(int nbPer) {
  const int lbAll = mg_xcd_block();
  return PtrBlock{lbAll / nbPer, lbAll % nbPer};
}

// GAD_ADVECTION's X, Y and vertical passes of the multi-dimensional tracers in `list`
__global__ void __launch_bounds__(256) k_ptr_adv_x(Dims d, Fields f, const TracerArgs *__restrict__ tab,
                                                   const int *__restrict__ list, int nList, int nbPer) {
  const PtrBlock b = ptr_block(nbPer);
  if (b.it >= nList) return;
  const TracerArgs a = tab[list[b.it]];
  adv_x_body(d, ptr_fields(f, a), a, b.lb);
}
__global__ void __launch_bounds__(256) k_ptr_adv_y(Dims d, Fields f, const TracerArgs *__restrict__ tab,
                                                   const int *__restrict__ list, int nList, int nbPer) {
  const PtrBlock b = ptr_block(nbPer);
  if (b.it >= nList) return;
  const TracerArgs a = tab[list[b.it]];
  adv_y_body(d, ptr_fields(f, a), a, b.lb);
}
__global__ void __launch_bounds__(256) k_ptr_adv_r(Dims d, Params p, Fields f, const TracerArgs *__restrict__ tab,
                                                   const int *__restrict__ list, int nList, int nbPer) {
  const PtrBlock b = ptr_block(nbPer);
  if (b.it >= nList) return;
  const TracerArgs a = tab[list[b.it]];
  adv_r_body<false>(d, p, ptr_fields(f, a), a, a.adv2, a.adv2, b.lb);
}

// GAD_CALC_RHS + forcing + AB2 + TIMESTEP_TRACER of every tracer in `list`.  GM: the tracers
// of the list take GM/Redi (PTRACERS_useGMRedi); a batch that mixes both kinds is two
// launches (both bodies in one kernel spilled scalar registers to scratch).
template <bool GM>
__global__ void __launch_bounds__(256) k_ptr_rhs(Dims d, Params p, Fields f, const TracerArgs *__restrict__ tab,
                                                 const int *__restrict__ list, int nList, int nbPer,
                                                 const int *iterPtr) {
  const PtrBlock b = ptr_block(nbPer);
  if (b.it >= nList) return;
  const TracerArgs a = tab[list[b.it]];
  const Fields g = ptr_fields(f, a);
  p.useGMRedi = GM ? 1 : 0;
  tracer_rhs_body<GM, true>(d, p, g, a, iterPtr, b.lb);
}

// GAD_IMPLICIT_R + SOLVE_TRIDIAGONAL + CYCLE_TRACER of every tracer in `list`
__global__ void __launch_bounds__(256) k_ptr_impl(Dims d, Params p, Fields f, const TracerArgs *__restrict__ tab,
                                                  const int *__restrict__ list, int nList, int nbPer, int nc) {
  const PtrBlock b = ptr_block(nbPer);
  if (b.it >= nList) return;   // (uniform over the workgroup: no barrier is skipped by part of it)
  const TracerArgs a = tab[list[b.it]];
  p.useGMRedi = a.gm;
  tracer_impl_body<false>(d, p, f, a, nc, b.lb);
}

// where the batched kernels restate the one-tracer route: lat-lon passes (no cube corner
// fills, no compressible form), the flat right-hand side (no k-march), AB2
bool ptr_batch_ok(const Dims &d, const Params &p) {
  return !p.cubeCorners && !p.multiDimCompressible && !p.useAB3 && !tracer_march_on(d);
}

// tab: the TracerArgs of every tracer (device); lists: [md | all], the multi-dimensional
// tracers and every tracer in launch order (device), nMd and nAll entries, the second list
// starting at lists + stride, its first nGM tracers the ones that take GM/Redi
hipError_t launch_ptracers_batch(const Dims &d, const Params &p, const Fields &f, const TracerArgs *tab, const int *lists,
                                 int stride, int nMd, int nAll, int nGM, const int *iterPtr, hipStream_t s) {
  if (nAll <= 0) return hipSuccess;
  const dim3 blk(MG_PLANE_THREADS);
  const int nbI = (int)mg_plane_blocks(d.sNx, d.sNy, d.nT * d.Nr), nbF = (int)mg_plane_blocks(d.nx, d.ny, d.nT * d.Nr);
  if (nMd > 0) {
    hipLaunchKernelGGL(k_ptr_adv_x, dim3((unsigned)(nbF * nMd)), blk, 0, s, d, f, tab, lists, nMd, nbF);
    hipLaunchKernelGGL(k_ptr_adv_y, dim3((unsigned)(nbI * nMd)), blk, 0, s, d, f, tab, lists, nMd, nbI);
    hipLaunchKernelGGL(k_ptr_adv_r, dim3((unsigned)(nbI * nMd)), blk, 0, s, d, p, f, tab, lists, nMd, nbI);
  }
  const int *all = lists + stride;
  if (nGM > 0)
    hipLaunchKernelGGL(k_ptr_rhs<true>, dim3((unsigned)(nbI * nGM)), blk, 0, s, d, p, f, tab, all, nGM, nbI, iterPtr);
  if (nAll > nGM)
    hipLaunchKernelGGL(k_ptr_rhs<false>, dim3((unsigned)(nbI * (nAll - nGM))), blk, 0, s, d, p, f, tab, all + nGM,
                       nAll - nGM, nbI, iterPtr);
  if (p.implicitDiffusion) {
    const long ncol = (long)d.sNx * d.sNy * d.nT;
    const int nc = mg_colf_nc(ncol, d.Nr, 3);
    const int nbC = (int)mg_colf_blocks(ncol, nc);
    MG_ALLOW_LDS(k_ptr_impl);
    hipLaunchKernelGGL(k_ptr_impl, dim3((unsigned)(nbC * nAll)), blk, mg_colf_lds(d.Nr, nc, 3), s, d, p, f, tab, all, nAll,
                       nbC, nc);
  }
  return hipGetLastError();
}

}  // namespace mgcm
