// launch.h -- the host interface of the step's kernels: the launchers and predicates that the
// kernels_*.hip files define and model.hip calls, declared once so that the compiler checks
// every definition and every call against the same signature (cg2d.h does the same for the
// solvers).  Included by model.hip and by every file that defines one of them; default
// arguments live here only.
#pragma once
#include "common.h"

namespace mgcm {

// ---- kernels_dyn.hip (through kernels_step.hip)
hipError_t launch_mom_step(const Dims &, const Params &, const Fields &, const int *, hipStream_t, bool ring = true);
bool mom_ring_separable(const Dims &, const Params &);
hipError_t launch_mom_ring(const Dims &, const Params &, const Fields &, const int *, hipStream_t);
hipError_t launch_phys_ring(const Dims &, const Params &, const Fields &, const int *, hipStream_t);
hipError_t launch_phi_hyd(const Dims &, const Params &, const Fields &, hipStream_t);

// ---- kernels_solve.hip
hipError_t launch_sfp_rhs(const Dims &, const Params &, const Fields &, hipStream_t);
hipError_t launch_exchange(const Dims &, double *, const long *, int, int, hipStream_t);
hipError_t launch_correction(const Dims &, const Params &, const Fields &, hipStream_t);
hipError_t launch_bump_counter(int *, int, hipStream_t);
hipError_t launch_exchange_multi(const Dims &, const XFields &, const long *, int, int *, hipStream_t);
hipError_t launch_exchange_uv(const Dims &, double *, double *, const long *, int, int, int, hipStream_t);
hipError_t launch_exchange_mixed(const Dims &, double *, double *, int, const long *, int, int, const XFields &,
                                 const long *, int, int *, hipStream_t);
hipError_t launch_exchange_uv_pairs(const Dims &, double *const *, double *const *, int, const long *, int, int,
                                   hipStream_t);
hipError_t launch_exch_eta(const Dims &, const Params &, const Fields &, const long *, bool, int, hipStream_t,
                           int fromX = 0);
hipError_t launch_corr_cont(const Dims &, const Params &, const Fields &, int, hipStream_t, const long *etaSrc = nullptr,
                            bool gmNext = false, bool spec = false);
hipError_t launch_halo_pack(const Dims &, const XFields &, const long *, long, double *, int, hipStream_t);

// ---- kernels_cg2d_dist.hip
hipError_t launch_cgd(const Dims &, const Params &, const Fields &, int, double, double *, hipStream_t);
hipError_t launch_cgd_record(SolveRecord *, const int *, double, double, double, double, int, double, int, hipStream_t);
hipError_t launch_field_pack(double *, const long *, long, double *, int, hipStream_t);

// ---- kernels_rstar.hip
hipError_t launch_calc_r_star(const Dims &, const Params &, const Fields &, const long *, hipStream_t, bool fuseEtaH = false,
                              int fromX = 0);
hipError_t launch_rstar_exmix(const Dims &, const Params &, const Fields &, const long *, bool, int, double *, double *, int,
                              const long *, int, int, const XFields &, const long *, int, hipStream_t);
hipError_t launch_rstar_exch(const Dims &, const Params &, const Fields &, const long *, bool, const XFields &, const long *,
                             int, int *, hipStream_t, int fromX = 0, int empNext = 0);
hipError_t launch_update_r_star_cg2d(const Dims &, const Params &, const Fields &, const long *, hipStream_t, bool sfp = false,
                                     bool opEarly = false, bool pcHere = false, const int *iterPtr = nullptr,
                                     bool keepFac = false, bool spec = false);

// ---- kernels_thermo.hip (through kernels_step.hip)
bool phys_ring_ok(const Dims &, const Params &, const Fields &);
hipError_t launch_oceanic_phys(const Dims &, const Params &, const Fields &, const int *, hipStream_t, bool gm = true,
                               bool ring = false);
hipError_t launch_tracer_step(const Dims &, const Params &, const Fields &, const TracerArgs &, const int *, hipStream_t,
                              bool impl = true, int *nLaunch = nullptr);
hipError_t launch_gm_tensor(const Dims &, const Params &, const Fields &, hipStream_t);
hipError_t launch_gm_residual_flow(const Dims &, const Params &, const Fields &, hipStream_t);

// ---- kernels_step.hip
bool dyn_thermo_fusable(const Dims &, const Params &, const TracerArgs &, const TracerArgs &);
hipError_t launch_dyn_thermo(const Dims &, const Params &, const Fields &, const TracerArgs &, const TracerArgs &, const int *,
                             hipStream_t, const long *srcOf = nullptr, bool gmHere = true, bool l1Here = true, bool spec = false);
bool dyn_thermo_spec_ok(const Params &);
bool phi_pipe_ok(const Dims &, const Params &);
hipError_t launch_phi_del2(const Dims &, const Params &, const Fields &, hipStream_t);
hipError_t launch_rstar_exch_phi(const Dims &, const Params &, const Fields &, const HaloRec *, const XFields &, const long *, int,
                                 int *, hipStream_t, int fromX, int empNext);
bool dyn_thermo_takes_gm(const Params &);
bool gm_phi_fusable(const Dims &, const Params &);
hipError_t launch_gm_phi(const Dims &, const Params &, const Fields &, hipStream_t, bool op = false);
bool tracer_hpair_ok(const Dims &, const Params &, const TracerArgs &, const TracerArgs &);
hipError_t launch_tracer_hpair(const Dims &, const Params &, const Fields &, const TracerArgs &, const TracerArgs &,
                               const int *, hipStream_t);

// ---- kernels_monitor.hip
hipError_t launch_mon_stats(const Dims &, const MonSpecs &, int, double *, int, hipStream_t);

// ---- kernels_ptracers.hip (through kernels_step.hip)
bool ptr_batch_ok(const Dims &, const Params &, bool md);
hipError_t launch_ptracers_batch(const Dims &, const Params &, const Fields &, const TracerArgs *, const int *, int,
                                 const int *nMdFam, int, int, const int *, hipStream_t, int *nLaunch = nullptr);

}  // namespace mgcm
