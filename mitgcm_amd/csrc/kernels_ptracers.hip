// kernels_ptracers.hip -- pkg/ptracers on the device: every passive tracer of a batch per launch.
//
// PTRACERS_INTEGRATE (pkg/ptracers/ptracers_integrate.F:150-420) takes each tracer in use
// through SALT_INTEGRATE's sequence with the tracer's own parameters: CALC_3D_DIFFUSIVITY,
// GAD_ADVECTION (multi-dimensional schemes) or the advection inside GAD_CALC_RHS, the forcing
// (PTRACERS_APPLY_FORCING, ptracers_apply_forcing.F:76-92, from PTRACERS_FORCING_SURF's
// surfaceForcingPTr, ptracers_forcing_surf.F:60-75), ADAMS_BASHFORTH2 on the tendency,
// FREESURF_RESCALE_G, TIMESTEP_TRACER, GAD_IMPLICIT_R and CYCLE_TRACER.  One tracer at a time
// that is launch_tracer_step with the tracer's TracerArgs (the functional route, every
// topology and form).  A launch is a few microseconds of latency and a tracer takes up to five
// on a lat-lon grid, 28 on the cube (the general GAD_ADVECTION as explicit passes), so here the
// tracer index is a dimension of the grid: the kernels read the tracers' TracerArgs from a
// device table and run the bodies the one-tracer kernels run (adv_x/y/r_body, the advg_*_point
// functions, tracer_rhs_body, tracer_impl_body: kernels_thermo.hip) -- the same bits, at most
// five launches whatever the number of tracers (six on a lat-lon grid when some take GM/Redi
// and some do not) while the multi-dimensional tracers are of one scheme family; each further
// family present (common.h MG_ADV_*: {30, 33}, {1, 20}, {7}) adds its own pass launches, 3 on
// the lat-lon two-pass route and 2 in the general form (launch_ptracers_batch).  The general form -- EXCH2 topologies (cubeCorners) and
// GAD_MULTIDIM_COMPRESSIBLE -- runs every pass of a (tracer, tile, level) in one workgroup
// with the level's frame in LDS (k_ptr_advg_plane).  Opt-in, MGCM_PTR_BATCH=1; where it wins
// and where the tracers hide beside the pressure solve either way: model.hip ptr_batched,
// DESIGN.md section 3.  The k-march forms and frames above 64 KiB stay functional (ptr_batch_ok).
//
// The tracers of a batch run concurrently, so each has its own gAdv / advScr1 / advScr2 / T* /
// c' scratch (model.hip's third arena).  A table entry is all a kernel knows of its tracer: the
// bodies take the scratch, the GM/Redi switch and the flow the passes advect by from the
// TracerArgs, and Params and Fields reach them as the model's.
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

// GAD_ADVECTION's X, Y and vertical passes of the multi-dimensional tracers in `list`, all of
// the scheme family FAM (common.h MG_ADV_*: the flux function is compiled in)
template <int FAM>
__global__ void __launch_bounds__(256) k_ptr_adv_x(Dims d, Fields f, const TracerArgs *__restrict__ tab,
                                                   const int *__restrict__ list, int nList, int nbPer) {
  const PtrBlock b = ptr_block(nbPer);
  if (b.it >= nList) return;
  const TracerArgs a = tab[list[b.it]];
  adv_x_body<FAM>(d, f, a, b.lb);
}
template <int FAM>
__global__ void __launch_bounds__(256) k_ptr_adv_y(Dims d, Fields f, const TracerArgs *__restrict__ tab,
                                                   const int *__restrict__ list, int nList, int nbPer) {
  const PtrBlock b = ptr_block(nbPer);
  if (b.it >= nList) return;
  const TracerArgs a = tab[list[b.it]];
  adv_y_body<FAM>(d, f, a, b.lb);
}
// COMP: GAD_MULTIDIM_COMPRESSIBLE (the local volume in adv2); gen: the general form's loc is
// adv1 (k_ptr_advg_plane), the lat-lon passes' is adv2 (k_ptr_adv_y) -- launch_tracer_step's
// three k_adv_r launches
template <bool COMP, int FAM>
__global__ void __launch_bounds__(256) k_ptr_adv_r(Dims d, Params p, Fields f, const TracerArgs *__restrict__ tab,
                                                   const int *__restrict__ list, int nList, int nbPer, int gen) {
  const PtrBlock b = ptr_block(nbPer);
  if (b.it >= nList) return;
  const TracerArgs a = tab[list[b.it]];
  const double *L = gen ? a.adv1 : a.adv2;
  adv_r_body<COMP, FAM>(d, p, f, a, L, COMP ? a.adv2 : L, b.lb);
}

// GAD_ADVECTION's general form (cube tiles and / or GAD_MULTIDIM_COMPRESSIBLE: the explicit
// passes k_advg_init / _fill / _flux / _upd of kernels_thermo.hip) of the multi-dimensional
// tracers in `list`, one workgroup per (tracer, tile, level).  The passes of a level are
// tile-local -- they read the level's own halo-inclusive frame, exchanged before the step --
// so the frame lives in LDS through the whole sequence, a barrier standing where the
// functional route has a launch boundary: loc, the face fluxes of the current stage and,
// compressible, vol, nx * ny doubles each (ptr_plane_lds; at most 64 KiB, ptr_batch_ok).
// The points of a frame are a strided loop with the same trip count for every thread: lanes
// past the frame skip the work, never a barrier.  Nothing here touches gTscr, which the
// tracers of a batch would share; the interior of loc (vol) goes to the tracer's own adv1
// (adv2), all that adv_r_body reads.
template <int FAM>
__global__ void __launch_bounds__(1024) k_ptr_advg_plane(Dims d, Fields f, const TracerArgs *__restrict__ tab,
                                                        const int *__restrict__ list, int nList, int cube, int comp) {
  extern __shared__ double ptrFrame[];
  const int nz = d.nT * d.Nr, lb = mg_xcd_block();
  const int it = lb / nz, z = lb % nz;
  if (it >= nList) return;   // (uniform over the workgroup)
  const TracerArgs a = tab[list[it]];
  const int t = d.t0 + z / d.Nr, k = z % d.Nr + 1;
  const int nx = d.nx, np = d.nx * d.ny, nth = (int)blockDim.x, tid = (int)threadIdx.x;
  const int trips = (np + nth - 1) / nth, per = 4 * d.OLx * d.OLy, ctrips = (per + nth - 1) / nth;
  double *L = ptrFrame, *G = ptrFrame + np, *V = ptrFrame + 2 * np;   // (V: only touched when comp)
  const int face = cube ? f.tileFace[t] : 0, edges = cube ? f.tileEdge[t] : 0;
  for (int r = 0; r < trips; r++) {
    const int q = r * nth + tid;
    if (q < np) advg_init_point(d, f, a, comp != 0, 1 - d.OLx + q % nx, 1 - d.OLy + q / nx, k, t, L, V);
  }
  __syncthreads();
  for (int ipass = 1; ipass <= (cube ? 3 : 2); ipass++)
    for (int ydir = 0; ydir < 2; ydir++) {
      if (cube) {
        for (int r = 0; r < ctrips; r++) {
          const int c = r * nth + tid;
          if (c < per) advg_fill_point(d, face, edges, ipass, 2 * ydir, c, L);
        }
        __syncthreads();
      }
      for (int r = 0; r < trips; r++) {
        const int q = r * nth + tid;
        if (q < np)
          advg_flux_point<FAM>(d, f, a, ipass, ydir, cube != 0, face, edges, 1 - d.OLx + q % nx, 1 - d.OLy + q / nx, k, t, L, G);
      }
      __syncthreads();
      if (cube) {
        for (int r = 0; r < ctrips; r++) {
          const int c = r * nth + tid;
          if (c < per) advg_fill_point(d, face, edges, ipass, 2 * ydir + 1, c, L);
        }
        __syncthreads();
      }
      for (int r = 0; r < trips; r++) {
        const int q = r * nth + tid;
        if (q < np)
          advg_upd_point(d, f, a, ipass, ydir, cube != 0, comp != 0, face, edges, 1 - d.OLx + q % nx, 1 - d.OLy + q / nx, k,
                         t, L, V, G);
      }
      __syncthreads();
    }
  const int ni = d.sNx * d.sNy, itrips = (ni + nth - 1) / nth;
  for (int r = 0; r < itrips; r++) {
    const int q = r * nth + tid;
    if (q < ni) {
      const int i = 1 + q % d.sNx, j = 1 + q / d.sNx;
      const long q3 = MG_I3(d, i, j, k, t);
      a.adv1[q3] = L[MG_FR(d, i, j)];
      if (comp) a.adv2[q3] = V[MG_FR(d, i, j)];
    }
  }
}
inline size_t ptr_plane_lds(const Dims &d, const Params &p) {
  return (size_t)(p.multiDimCompressible ? 3 : 2) * d.nx * d.ny * sizeof(double);
}
// Threads per frame: 512, or the frame's points rounded up to whole waves where they are fewer.
// Measured on global_ocean.cs32x15 (40 x 40 frames, 4 tracers, profiles/r11/ptracers_cube/): the
// kernel takes 82 us at MG_PLANE_THREADS = 256 (seven trips per stage, each waiting for its own
// loads), 57 us at 512, 66 us at 1024 (16 waves per barrier); the step 0.511 / 0.496 / 0.504
// ms at 4 tracers and 0.544 / 0.534 / 0.560 at 8.  MGCM_PTR_PLANE_THREADS = 256 | 512 | 1024
// overrides it for A/B runs (read per launch).
inline unsigned ptr_plane_threads(const Dims &d) {
  const char *e = getenv("MGCM_PTR_PLANE_THREADS");
  const int v = e ? atoi(e) : 0;
  if (v == 256 || v == 512 || v == 1024) return (unsigned)v;
  const int waves = (d.nx * d.ny + 63) / 64;
  return (unsigned)(64 * std::min(8, std::max(1, waves)));
}

// GAD_CALC_RHS + forcing + AB2 + TIMESTEP_TRACER of every tracer in `list`.  GM: the tracers
// of the list take GM/Redi (TracerArgs::gm; the host sorts them); a batch that mixes both kinds is two
// launches (both bodies in one kernel spilled scalar registers to scratch).
template <bool GM>
__global__ void __launch_bounds__(256) k_ptr_rhs(Dims d, Params p, Fields f, const TracerArgs *__restrict__ tab,
                                                 const int *__restrict__ list, int nList, int nbPer,
                                                 const int *iterPtr) {
  const PtrBlock b = ptr_block(nbPer);
  if (b.it >= nList) return;
  const TracerArgs a = tab[list[b.it]];
  tracer_rhs_body<GM, true>(d, p, f, a, iterPtr, b.lb);
}

// GAD_IMPLICIT_R + SOLVE_TRIDIAGONAL + CYCLE_TRACER of every tracer in `list`
__global__ void __launch_bounds__(256) k_ptr_impl(Dims d, Params p, Fields f, const TracerArgs *__restrict__ tab,
                                                  const int *__restrict__ list, int nList, int nbPer, int nc) {
  const PtrBlock b = ptr_block(nbPer);
  if (b.it >= nList) return;   // (uniform over the workgroup: no barrier is skipped by part of it)
  const TracerArgs a = tab[list[b.it]];
  tracer_impl_body<false>(d, p, f, a, nc, b.lb);
}

// where the batched kernels restate the one-tracer route: the flat right-hand side (no k-march),
// AB2, and, where the model's multi-dimensional tracers (md) take the general form of
// GAD_ADVECTION, a frame k_ptr_advg_plane can hold in HIP's default dynamic LDS, 64 KiB -- no
// function attribute, and two workgroups or more to a CU's 160 KiB.  Larger tiles, the k-march
// forms and ADAMS_BASHFORTH3 keep the functional route.
#define MG_PTR_PLANE_LDS_MAX (64u * 1024u)
bool ptr_batch_ok(const Dims &d, const Params &p, bool md) {
  if (p.useAB3 || tracer_march_on(d)) return false;
  if (md && (p.cubeCorners || p.multiDimCompressible) && ptr_plane_lds(d, p) > MG_PTR_PLANE_LDS_MAX) return false;
  return true;
}

// tab: the TracerArgs of every tracer (device); lists: [md | all], the multi-dimensional
// tracers and every tracer in launch order (device), the second list starting at lists + stride,
// its first nGM tracers the ones that take GM/Redi.  The multi-dimensional list is sorted by
// scheme family, nMdFam[MG_ADV_NFAM] tracers each: the passes of a family are launches of their
// own (the flux function is a template parameter), as the right-hand side's GM / non-GM kinds are.
// nLaunch (or null): the kernel launches issued are added to it -- per family present 3 on the
// lat-lon two-pass route and 2 in the general form, then 1 or 2 right-hand sides and the
// implicit solve.  (The lists are all the kernels know of who they step: theta and salt could
// join one with TracerArgs of their own.)
hipError_t launch_ptracers_batch(const Dims &d, const Params &p, const Fields &f, const TracerArgs *tab, const int *lists,
                                 int stride, const int *nMdFam, int nAll, int nGM, const int *iterPtr, hipStream_t s,
                                 int *nLaunch) {
  if (nAll <= 0) return hipSuccess;
  int nl = 0;
  const dim3 blk(MG_PLANE_THREADS);
  const int nbI = (int)mg_plane_blocks(d.sNx, d.sNy, d.nT * d.Nr), nbF = (int)mg_plane_blocks(d.nx, d.ny, d.nT * d.Nr);
  const int *md = lists;
  for (int fam = 0; fam < MG_ADV_NFAM; md += nMdFam[fam], fam++) {
    const int nMd = nMdFam[fam];
    if (nMd <= 0) continue;
    const bool cube = p.cubeCorners != 0, comp = p.multiDimCompressible != 0;
    if (!cube && !comp) {   // lat-lon, 2 passes: the per-point X and Y passes
      MG_ADV_FAMILY(fam, hipLaunchKernelGGL(k_ptr_adv_x<FAM>, dim3((unsigned)(nbF * nMd)), blk, 0, s, d, f, tab, md, nMd, nbF));
      MG_ADV_FAMILY(fam, hipLaunchKernelGGL(k_ptr_adv_y<FAM>, dim3((unsigned)(nbI * nMd)), blk, 0, s, d, f, tab, md, nMd, nbI));
      MG_ADV_FAMILY(fam, hipLaunchKernelGGL((k_ptr_adv_r<false, FAM>), dim3((unsigned)(nbI * nMd)), blk, 0, s, d, p, f, tab, md,
                                            nMd, nbI, 0));
      nl += 3;
    } else {                // the general form: every pass of a level in one workgroup
      if (ptr_plane_lds(d, p) > MG_PTR_PLANE_LDS_MAX) return hipErrorInvalidValue;   // (ptr_batch_ok was not asked)
      MG_ADV_FAMILY(fam, hipLaunchKernelGGL(k_ptr_advg_plane<FAM>, dim3((unsigned)(d.nT * d.Nr * nMd)), dim3(ptr_plane_threads(d)),
                                            ptr_plane_lds(d, p), s, d, f, tab, md, nMd, (int)cube, (int)comp));
      if (comp)
        MG_ADV_FAMILY(fam, hipLaunchKernelGGL((k_ptr_adv_r<true, FAM>), dim3((unsigned)(nbI * nMd)), blk, 0, s, d, p, f, tab, md,
                                              nMd, nbI, 1));
      else
        MG_ADV_FAMILY(fam, hipLaunchKernelGGL((k_ptr_adv_r<false, FAM>), dim3((unsigned)(nbI * nMd)), blk, 0, s, d, p, f, tab, md,
                                              nMd, nbI, 1));
      nl += 2;
    }
  }
  const int *all = lists + stride;
  if (nGM > 0) {
    hipLaunchKernelGGL(k_ptr_rhs<true>, dim3((unsigned)(nbI * nGM)), blk, 0, s, d, p, f, tab, all, nGM, nbI, iterPtr);
    nl++;
  }
  if (nAll > nGM) {
    hipLaunchKernelGGL(k_ptr_rhs<false>, dim3((unsigned)(nbI * (nAll - nGM))), blk, 0, s, d, p, f, tab, all + nGM,
                       nAll - nGM, nbI, iterPtr);
    nl++;
  }
  if (p.implicitDiffusion) {
    const long ncol = (long)d.sNx * d.sNy * d.nT;
    const int nc = mg_colf_nc(ncol, d.Nr, 3);
    const int nbC = (int)mg_colf_blocks(ncol, nc);
    MG_ALLOW_LDS(k_ptr_impl);
    hipLaunchKernelGGL(k_ptr_impl, dim3((unsigned)(nbC * nAll)), blk, mg_colf_lds(d.Nr, nc, 3), s, d, p, f, tab, all, nAll,
                       nbC, nc);
    nl++;
  }
  if (nLaunch) *nLaunch += nl;
  return hipGetLastError();
}

}  // namespace mgcm
