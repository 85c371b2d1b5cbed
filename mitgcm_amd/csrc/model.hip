// model.hip -- host runtime of the MI355X hot path and its C-ABI (include/mitgcm_amd.h).
//
// Owns the device mirror of the reference's per-tile COMMON blocks (DYNVARS.h,
// GRID.h, SURFACE.h, FFIELDS.h, CG2D.h) for the tiles on one GPU, the halo
// topology (EXCH1 lat-lon by default, any EXCH2 map via mgcm_set_halo_map), and
// the launch sequence of FORWARD_STEP's device-resident subset.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <utility>
#include <string>
#include <vector>

#include "../../include/mitgcm_amd.h"
#include "cg2d.h"
#include "launch.h"

namespace mgcm {
// Host ranges the Fortran mirror registered for DMA (fortran_abi.hip register_host: the
// page-rounded extents of its bound COMMON arrays).  An unbound host array that shares an
// edge page is then partly registered, and the runtime refuses a copy that spans the edge of
// a registered range ("invalid argument"): mg_host_copy splits a host<->device copy at every
// registered-range edge, so each piece lies wholly inside or wholly outside one.
static std::vector<std::pair<uintptr_t, uintptr_t>> g_hostReg;
void mg_host_ranges_set(const uintptr_t *lo, const uintptr_t *hi, size_t n) {
  g_hostReg.clear();
  for (size_t i = 0; i < n; i++) g_hostReg.push_back({lo[i], hi[i]});
  std::sort(g_hostReg.begin(), g_hostReg.end());
}
hipError_t mg_host_copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
  if (g_hostReg.empty() || bytes == 0) return hipMemcpyAsync(dst, src, bytes, kind, s);
  const uintptr_t h = (uintptr_t)(kind == hipMemcpyHostToDevice ? src : dst), end = h + bytes;
  size_t off = 0;
  while (h + off < end) {
    const uintptr_t cur = h + off;
    uintptr_t cut = end;
    for (const auto &r : g_hostReg) {
      if (r.first > cur && r.first < cut) cut = r.first;
      if (r.second > cur && r.second < cut) cut = r.second;
    }
    const hipError_t e = hipMemcpyAsync((char *)dst + off, (const char *)src + off, cut - cur, kind, s);
    if (e != hipSuccess) return e;
    off += cut - cur;
  }
  return hipSuccess;
}
}  // namespace mgcm

using namespace mgcm;

static thread_local std::string g_err;
static int set_err(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}
#define HIPCHK(x)                                                                              \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) return set_err("%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
  } while (0)

enum FieldKind { F1D, F2D, F3D, FREC };   // FREC: 6 forcing fields x MG_MAXREC records of 2-D
#define MG_MAXREC 12
struct FieldDesc {
  const char *name;
  FieldKind kind;
  size_t off;  // offset of the pointer inside Fields
};

#define FD(n, k) {#n, k, offsetof(Fields, n)}
static const FieldDesc FIELDS[] = {
    FD(drF, F1D), FD(drC, F1D), FD(recip_drF, F1D), FD(recip_drC, F1D), FD(rF, F1D), FD(rC, F1D), FD(tRef, F1D), FD(sRef, F1D), FD(pRef4EOS, F1D), FD(phiRefC, F1D),
#define FD2(n) FD(n, F2D),
#define FD3(n) FD(n, F3D),
    MG_F2D_LIST(FD2)
    MG_F3D_LIST(FD3)
#undef FD2
#undef FD3
    FD(forcRec, FREC),
};
#undef FD

struct PDesc {
  const char *name;
  size_t off;
  bool isint;
};
#define PD(n) {#n, offsetof(Params, n), false}
#define PI_(n) {#n, offsetof(Params, n), true}
static const PDesc PARAMS[] = {
    PD(deltaTMom), PD(deltaTFreeSurf), PD(deltaTClock), PD(abEps), PD(alph_AB), PD(beta_AB), PI_(useAB3), PD(rhoConst), PD(gBaro), PD(viscAhD), PD(viscAhZ),
    PD(viscA4D), PD(viscA4Z), PD(viscAr), PD(sideDragFactor), PD(freeSurfFac), PD(implicSurfPress),
    PD(implicDiv2DFlow), PD(rkSign), PD(afFacMom), PD(vfFacMom), PD(pfFacMom), PD(cfFacMom), PD(foFacMom),
    PD(mtFacMom), PD(cg2dNorm), PD(cg2dTolerance_sq),
    PI_(momAdvection), PI_(momViscosity), PI_(momForcing), PI_(useCoriolis), PI_(no_slip_sides),
    PI_(no_slip_bottom), PI_(selectCoriScheme), PI_(momForcingOutAB), PI_(momDissip_In_AB),
    PI_(implicitViscosity), PI_(cg2dMaxIters), PI_(cg2dUseMinResSol), PI_(cg2dNormaliseRHS), PI_(nIter0), PI_(cg2dUseFMA), PI_(useSRCGSolver), PI_(cg2dRefOrder),
    PD(gravity), PD(gravitySign), PD(rhoNil), PD(tAlpha), PD(sBeta), PD(ivdc_kappa), PD(diffKhT), PD(diffKrT),
    PD(deltaTtracer), PI_(exactConserv), PI_(tempStepping), PI_(tempAdvection), PI_(tempForcing),
    PI_(implicitDiffusion), PI_(tempAdvScheme), PI_(saltStepping), PI_(saltAdvection), PI_(saltForcing),
    PI_(saltAdvScheme), PD(diffKhS), PD(diffKrS), PI_(multiDimAdvection), PI_(multiDimCompressible), PI_(momStepping),
    PI_(eosType), PI_(allowFreezing), PI_(useRealFreshWaterFlux), PI_(useCDscheme), PI_(useGMRedi),
    PI_(periodicExternalForcing), PI_(nForcRec), PD(HeatCapacity_Cp), PD(convertFW2Salt), PD(temp_EvPrRn),
    PD(salt_EvPrRn), PD(rCD), PD(epsAB_CD), PD(externForcingPeriod), PD(externForcingCycle), PD(GM_background_K),
    PD(GM_isopycK), PD(GM_skewflx), PD(GM_maxSlope), PD(GM_Kmin_horiz), PD(GM_Small_Number), PD(GM_slopeSqCutoff),
    PI_(GM_AdvForm), PI_(GM_ExtraDiag),
    PI_(nonlinFreeSurf), PI_(select_rStar), PI_(quasiHydrostatic), PI_(useNHMTerms), PI_(select3dCoriScheme),
    PI_(selectP_inEOS_Zc), PI_(storePhiHyd4Phys), PD(hFacInf),
    PI_(vectorInvariantMomentum), PI_(selectVortScheme), PI_(selectKEscheme), PI_(upwindShear),
    PI_(staggerTimeStep), PI_(tracForcingOutAB),
};
#undef PD
#undef PI_

// kernel families timed with hipEvents when timing is enabled
enum Kern { K_MOM, K_RHS, K_CG2D, K_EXCH, K_ETA, K_CORR, K_CONT, K_PHYS, K_TEMP, K_RSTAR, K_PHI, K_N };
static const char *KNAMES[K_N] = {"mom_step",   "sfp_rhs",    "cg2d",         "exchange",  "eta_update",
                                  "correction", "continuity", "oceanic_phys", "temp_step", "r_star", "phi_hyd"};

// the step sequences that are captured into graphs (model.hip STEP_SEQS)
enum StepSeq { SEQ_PLAIN2 = 0, SEQ_HOIST2, SEQ_HOIST_LAST, SEQ_PLAIN1, SEQ_LAST1, SEQ_N };

struct mgcm_model {
  Dims d{};
  Params p{};
  Fields f{};
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t ownStream = nullptr;   // created by mgcm_create; `stream` may be a caller's
  // THERMODYNAMICS runs on a second stream concurrently with DYNAMICS (fork after
  // DO_OCEANIC_PHYS, join before UPDATE_R_STAR / SOLVE_FOR_PRESSURE; MGCM_NO_OVERLAP=1 off)
  hipStream_t stream2 = nullptr;
  hipEvent_t evFork = nullptr, evJoin = nullptr;
  hipEvent_t evHand = nullptr;   // mgcm_stream_handoff
  bool overlap = true;
  std::vector<void *> allocs;
  // extra parameters kept on host only
  std::map<std::string, double> extra;
  // halo map (2*nHalo longs) and CG2D neighbour table
  long *d_halo = nullptr;
  long *d_srcOf = nullptr;    // per 2-D point: interior source of a halo point, -1 otherwise
  mgcm::HaloRec *d_haloRec = nullptr;   // per 2-D point: srcOf's topology as a record (common.h), or null (no 32-bit fit)
  int nHalo = 0;
  long *d_haloAll = nullptr;  // the map of EVERY tile's halo when this model steps a tile subset
  int nHaloAll = 0;           // (EXCH_*_RL on host arrays, mgcm_exchange_host, covers the domain)
  std::vector<long> h_halo;
  // The CG2D solver, selected once by mgcm_init and never changed after it; every table set
  // below exists only for the solver that reads it.  The values are those of
  // mgcm_get_param("cg2dKernel"): 3 k_cg2d_bxy, 4 k_cg2d_mwg, 5 k_cg2d_block (reference order,
  // cg2dRefOrder on up to one workgroup's points), 6 k_cg2d_mwg in the reference order
  // (cg2dRefOrder past that).  1 (a generic point-per-thread kernel summing in the tree order)
  // and 2 (a 2x2-blocked kernel) are retired: no grid could select either any more.
  enum class Cg2dSolver { Bxy = 3, Mwg = 4, BlockRef = 5, MwgRef = 6 };
  Cg2dSolver solver = Cg2dSolver::Bxy;
  bool useMwg() const { return solver == Cg2dSolver::Mwg || solver == Cg2dSolver::MwgRef; }
  int nPts = 0;               // interior points of the whole domain
  // BlockRef tables (build_block)
  unsigned *d_nbr = nullptr;  // packed (W|E<<16),(S|N<<16) compact neighbour indices, padded
  int *d_gofs = nullptr;      // 2-D flat offset of each (padded) interior point
  // Bxy tables (build_bxy)
  unsigned *d_nbx = nullptr;
  int *d_blkx = nullptr;
  int nBlkX = 0;
  int bxyVar = -1;              // k_cg2d_bxy geometry (kernels_solve.hip CGX[])
  // land-block compaction of the k_cg2d_bxy tables (choose_bxy): the 2-D offsets of the points
  // of the all-land blocks left out, which the solver's prologue scans for a non-zero; empty
  // under every other solver, so the land guards do nothing there
  std::vector<int> h_dropG;
  int *d_dropG = nullptr;
  int nDropBlk = 0;             // blocks left out (0: the tables cover the whole grid)
  bool noCompact = false;       // set once the zero-on-land invariant was seen broken: full tables from then on
  int *h_guard = nullptr;       // pinned host word the solver sets when its scan finds a non-zero
  int *d_guard = nullptr;       // its device address
  bool latlonTopology = true;   // false once a custom halo map (e.g. EXCH2 cube) is installed
  // Mwg, MwgRef tables (build_mwg, kernels_cg2d_mwg.hip): tables of every part, device buffers
  MwgTables mwg{};
  std::vector<void *> mwgAllocs;
  void *mwgShared = nullptr;   // another process's hand-off block, opened by IPC (mgcm_cg2d_shared_import)
  void *mwgBlock = nullptr;    // this model's own hand-off block (hipMalloc, or uncached once shared)
  std::vector<int> mwgPlan;   // summation plan for mgcm_cg2d_sum_plan: [(g*OPT + p)*NT + tid]
  // EXCH2 C-grid vector maps (mgcm_set_uv_map): [withSigns] -> (dst, code) pairs of this
  // process's tiles, u entries first; code = +-(src+1), src indexing [u | v]
  bool uvMap = false;
  std::vector<long> h_uv[2];
  long *d_uv[2] = {nullptr, nullptr};
  int nUvU[2] = {0, 0}, nUvV[2] = {0, 0};
  // the same maps over every tile (tile-sharded runs recompute the 2-D r* state of the whole
  // domain redundantly: CALC_R_STAR's EXCH_UV of the W/S factors covers remote tiles too)
  long *d_uvAll[2] = {nullptr, nullptr};
  int nUvUAll[2] = {0, 0}, nUvVAll[2] = {0, 0};
  // Entries of those maps whose source is a halo point that the same exchange fills (tiles
  // exactly as wide as the halo: the reference's second EXCH2_RX2_CUBE pass then copies a
  // corner-halo value its first pass left alone, exch2.py).  The reference reads every source
  // before it writes any halo, so such an entry takes the value from BEFORE the exchange: the
  // entries are kept out of the maps above and run as a launch of their own ahead of them
  // (uv_pre), [all tiles][withSigns]; they follow the main entries in the same buffer.
  struct UvPre { const long *map = nullptr; int nU = 0, nV = 0; } uvPre[2][2];
  int *d_tileInfo = nullptr;
  // device scratch of mgcm_exchange_host (EXCH_*_RL on caller arrays)
  double *exchBuf[2] = {nullptr, nullptr};
  long exchCap = 0;
  // hipGraphs of FORWARD_STEP sequences (step_graph)
  bool useGraph = true;
  struct StepGraph {
    hipGraphExec_t exec = nullptr;
    double *tr[4] = {};   // the tracer pointers after the sequence: theta, thetaNext, salt, saltNext
    int flip = 0;         // ... the passive tracers' parity after it
    int layout = 0;       // ... and the launch layout it runs (stepLayout)
  };
  // [THERMODYNAMICS overlap off/on][tracer buffer parity: bit 0 theta, 1 salt, 2 the passive tracers][StepSeq]
  StepGraph graphs[2][8][SEQ_N];
  // overlap auto-selection (ovl_trial): both graphs timed on a copy of the state
  bool ovlAuto = false, ovlDecided = false;
  float ovlMs[2] = {0.f, 0.f};
  hipEvent_t ovlEv[2] = {nullptr, nullptr};
  double *thetaA = nullptr, *saltA = nullptr;
  int stepLayout = 0;   // one_step's launch layout (mgcm_get_param "stepLayout")
  // the last ptracers_on (mgcm_get_param "ptrRoute", "ptrLaunches"): 0 no tracers, 1 functional, 2 batched;
  // the kernel launches it issued for PTRACERS_INTEGRATE, the exchanges not counted
  int ptrRoute = 0, ptrLaunches = 0;
  // whether the last THERMODYNAMICS launched k_gm_residual_flow (mgcm_get_param "gmResFlow"; StepPlan::resFlow)
  int gmResFlow = 0;
  // pkg/ptracers (mgcm_ptracers_alloc): a third arena, sized at run time, of PTR_NF 3-D fields
  // per tracer -- the ping-pong pair, gpTrNm1 and the tracer's own T*, advScr1 (also the
  // marches' c'), advScr2 and gAdv scratch: the batched kernels run the tracers concurrently
  struct PTracer {
    int advScheme = 2, useGMRedi = -1;   // (-1: the model's useGMRedi)
    double diffKh = 0.0, diffKr = 0.0, surfRelaxTau = 0.0, surfRelaxVal = 0.0, interiorSource = 0.0, EvPrRn = NAN;
    double *buf[2] = {nullptr, nullptr}, *gNm1 = nullptr, *scr = nullptr, *adv1 = nullptr, *adv2 = nullptr, *gAdv = nullptr;
  };
  std::vector<PTracer> ptr;
  double *a4 = nullptr;            // the arena
  int ptrFlip = 0;                 // which buffer of every pair is current (all swap together once per step)
  TracerArgs *d_ptrTab = nullptr;  // [2 parities][n] the batched kernels' table
  int *d_ptrList = nullptr;        // [2][n]: the multi-dimensional tracers, then every tracer in launch order
  int ptrNMd = 0, ptrNGM = 0;       // multi-dimensional tracers; tracers that take GM/Redi (first in launch order)
  int ptrNMdFam[MG_ADV_NFAM] = {0, 0, 0};   // the multi-dimensional tracers per scheme family (their list is sorted by it)
  bool ptrTabDirty = true;
  // THERMODYNAMICS of a sharded step on the second stream (mgcm_step_phase 16): 1 forked after
  // DO_OCEANIC_PHYS (joined before UPDATE_R_STAR), 2 to fork after CALC_DIV_GHAT, 3 forked
  // after it (joined before the correction step), 0 none pending
  int shardFork = 0;
  // mgcm_put_batch_async: two pinned host slots (each with the event of its last copy) and
  // one device buffer; a batch travels as [header | values] in one copy, then one scatter
  char *stHost[2] = {nullptr, nullptr};
  hipEvent_t stEv[2] = {nullptr, nullptr};    // slot q's scatter done (its pinned and device buffers free)
  hipEvent_t stCopied[2] = {nullptr, nullptr};   // slot q's copy done (the scatter may read it)
  size_t stCap = 0;
  int stNext = 0;
  char *stDev[2] = {nullptr, nullptr};
  hipStream_t stCopy = nullptr;   // the uploads' copy stream: a step's copy overlaps the step before
  // step counters: [0] = myIter, [1] = record slot
  int *d_ctr = nullptr;
  SolveRecord *d_rec = nullptr;
  int maxRec = 4096;
  int lastBatch = 0;
  double *monBuf = nullptr;   // MONITOR plane partials (mgcm_monitor)
  size_t monCap = 0;
  bool ready = false;
  // timing
  bool timing = false;
  std::vector<hipEvent_t> evPool;            // created once, reused
  size_t evUsed = 0;
  std::vector<std::pair<int, int>> evPairs;  // (kernel, start event index)
  double kms[K_N] = {0};
  int kcnt[K_N] = {0};
};
using Cg2dSolver = mgcm_model::Cg2dSolver;

static void drop_graphs(mgcm_model *m);
static int ptr_tables_sync(mgcm_model *m);
static int land_eta_check(mgcm_model *m, const char *name, const double *host, long n);

static long field_count(const mgcm_model *m, FieldKind k) {
  if (k == F1D) return m->d.Nr + 1;
  if (k == F2D) return m->d.n2 * m->d.nTiles;
  if (k == FREC) return 6L * MG_MAXREC * m->d.n2 * m->d.nTiles;
  return m->d.n3 * m->d.nTiles;
}
static const FieldDesc *find_field(const char *name) {
  for (auto &fd : FIELDS)
    if (!strcmp(fd.name, name)) return &fd;
  return nullptr;
}
static double *&field_ptr(mgcm_model *m, const FieldDesc *fd) {
  return *reinterpret_cast<double **>(reinterpret_cast<char *>(&m->f) + fd->off);
}
// A named field's device pointer and size: the Fields members, and the passive tracers'
// "pTracerNN" (the current buffer) / "gpTrNm1_NN", NN = 01..99 (PTRACERS_SIZE.h's two digits)
static bool lookup_field(mgcm_model *m, const char *name, double **ptr, long *n) {
  if (const FieldDesc *fd = find_field(name)) {
    *ptr = field_ptr(m, fd);
    *n = field_count(m, fd->kind);
    return true;
  }
  const bool tr = !strncmp(name, "pTracer", 7), g = !strncmp(name, "gpTrNm1_", 8);
  const char *dg = name + (tr ? 7 : 8);
  if ((!tr && !g) || dg[0] < '0' || dg[0] > '9' || dg[1] < '0' || dg[1] > '9' || dg[2]) return false;
  const int i = (dg[0] - '0') * 10 + (dg[1] - '0');
  if (i < 1 || i > (int)m->ptr.size()) return false;
  *ptr = tr ? m->ptr[i - 1].buf[m->ptrFlip] : m->ptr[i - 1].gNm1;
  *n = m->d.n3 * m->d.nTiles;
  return true;
}

// ------------------------------------------------------------------ timing
static int ev_next(mgcm_model *m) {
  if (m->evUsed == m->evPool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return -1;
    m->evPool.push_back(e);
  }
  return (int)m->evUsed++;
}
static int ev_begin(mgcm_model *m, int k) {
  (void)k;
  if (!m->timing) return -1;
  const int i = ev_next(m);
  if (i < 0) return -1;
  hipEventRecord(m->evPool[i], m->stream);
  return i;
}
static void ev_end(mgcm_model *m, int k, int startIdx) {
  if (!m->timing || startIdx < 0) return;
  const int i = ev_next(m);
  if (i < 0) return;
  hipEventRecord(m->evPool[i], m->stream);
  m->evPairs.push_back({k, startIdx});
}
// call with the stream drained
static void ev_collect(mgcm_model *m) {
  for (auto &pr : m->evPairs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, m->evPool[pr.second], m->evPool[pr.second + 1]) == hipSuccess) {
      m->kms[pr.first] += ms;
      m->kcnt[pr.first] += 1;
    }
  }
  m->evPairs.clear();
  m->evUsed = 0;
}
static void ev_free(mgcm_model *m) {
  for (auto e : m->evPool) hipEventDestroy(e);
  m->evPool.clear();
  m->evUsed = 0;
}

// ------------------------------------------------------------------ topology
// EXCH1 lat-lon periodic halo map (eesupp/src/exch1_rx.template:170-198): every
// halo point copies the interior point with the wrapped global index.
static void build_latlon_halo(mgcm_model *m) {
  const Dims &d = m->d;
  const int Nx = d.sNx * d.nSx, Ny = d.sNy * d.nSy;
  m->h_halo.clear();
  for (int t = 0; t < d.nTiles; t++) {
    const int bi = t % d.nSx, bj = t / d.nSx;
    for (int j = 1 - d.OLy; j <= d.sNy + d.OLy; j++)
      for (int i = 1 - d.OLx; i <= d.sNx + d.OLx; i++) {
        if (i >= 1 && i <= d.sNx && j >= 1 && j <= d.sNy) continue;
        int iG = ((bi * d.sNx + i - 1) % Nx + Nx) % Nx, jG = ((bj * d.sNy + j - 1) % Ny + Ny) % Ny;
        int st = (jG / d.sNy) * d.nSx + iG / d.sNx;
        m->h_halo.push_back(MG_I2(d, i, j, t));
        m->h_halo.push_back(MG_I2(d, iG % d.sNx + 1, jG % d.sNy + 1, st));
      }
  }
}

// The HaloRec table of an exchange map (common.h): for every 2-D point q of the nTiles tiles, where
// its value lives (srcOf[q], else q), that offset as the base of a 3-D column, the (i, j) of that
// owner, and whether q is interior / mapped.  Plain host code (mgcm_halo_table reaches it without
// a device).  Returns -1, out untouched, where an offset does not fit its 32-bit field.
namespace mgcm {
int mg_build_halo_table(const Dims &d, const long *srcOf, HaloRec *out) {
  if (d.n3 * d.nTiles >= (1L << 31) || d.nx + d.OLx >= (1 << 15) || d.ny + d.OLy >= (1 << 15)) return -1;
  const long N2 = d.n2 * d.nTiles;
  for (long q = 0; q < N2; q++) {
    const long sq = srcOf[q], at = sq >= 0 ? sq : q;
    int i, j, iq, jq;
    mg_ij_of(d, at, i, j);
    mg_ij_of(d, q, iq, jq);
    HaloRec h;
    h.at2 = (int)at;
    h.base3 = (int)((at / d.n2) * d.n3 + at % d.n2);
    h.i = (short)i;
    h.j = (short)j;
    h.flags = ((iq >= 1 && iq <= d.sNx && jq >= 1 && jq <= d.sNy) ? MG_HR_INTERIOR : 0) | (sq >= 0 ? MG_HR_MAPPED : 0);
    out[q] = h;
  }
  return 0;
}
}  // namespace mgcm
int mgcm_halo_table(int sNx, int sNy, int OLx, int OLy, int Nr, int nTiles, const long *srcOf, int *out) {
  mgcm::Dims d{};
  d.sNx = sNx; d.sNy = sNy; d.OLx = OLx; d.OLy = OLy; d.Nr = Nr; d.nTiles = nTiles; d.nT = nTiles;
  d.nx = sNx + 2 * OLx; d.ny = sNy + 2 * OLy; d.n2 = (long)d.nx * d.ny; d.n3 = d.n2 * Nr;
  static_assert(sizeof(mgcm::HaloRec) == 4 * sizeof(int), "a HaloRec is four ints to the caller");
  return mgcm::mg_build_halo_table(d, srcOf, reinterpret_cast<mgcm::HaloRec *>(out));
}

static int upload_halo(mgcm_model *m) {
  if (m->d_halo) { hipFree(m->d_halo); m->d_halo = nullptr; }
  if (m->d_srcOf) { hipFree(m->d_srcOf); m->d_srcOf = nullptr; }
  if (m->d_haloRec) { hipFree(m->d_haloRec); m->d_haloRec = nullptr; }
  const long N2 = m->d.n2 * m->d.nTiles;
  std::vector<long> srcOf(N2, -1);
  for (size_t h = 0; h + 1 < m->h_halo.size(); h += 2) srcOf[m->h_halo[h]] = m->h_halo[h + 1];
  HIPCHK(hipMalloc(&m->d_srcOf, N2 * sizeof(long)));
  HIPCHK(hipMemcpy(m->d_srcOf, srcOf.data(), N2 * sizeof(long), hipMemcpyHostToDevice));
  // ... and the same map as records, for the end-of-step grid's riders (k_rstar_exch_phi); without
  // them (no 32-bit fit) plan_step keeps the plain end of step (StepPlan::phiPipeOk)
  std::vector<mgcm::HaloRec> rec(N2);
  if (mgcm::mg_build_halo_table(m->d, srcOf.data(), rec.data()) == 0) {
    HIPCHK(hipMalloc(&m->d_haloRec, N2 * sizeof(mgcm::HaloRec)));
    HIPCHK(hipMemcpy(m->d_haloRec, rec.data(), N2 * sizeof(mgcm::HaloRec), hipMemcpyHostToDevice));
  }
  // the 3-D exchange kernels refresh the halos of this process's tiles only
  // (tile-sharded runs receive the remote sources first, mgcm_halo_unpack)
  std::vector<long> loc;
  const long lo = (long)m->d.t0 * m->d.n2, hi = (long)(m->d.t0 + m->d.nT) * m->d.n2;
  for (size_t h = 0; h + 1 < m->h_halo.size(); h += 2)
    if (m->h_halo[h] >= lo && m->h_halo[h] < hi) { loc.push_back(m->h_halo[h]); loc.push_back(m->h_halo[h + 1]); }
  m->nHalo = (int)(loc.size() / 2);
  if (m->d_haloAll) { hipFree(m->d_haloAll); m->d_haloAll = nullptr; }
  m->nHaloAll = 0;
  if (m->d.nT < m->d.nTiles && !m->h_halo.empty()) {
    HIPCHK(hipMalloc(&m->d_haloAll, m->h_halo.size() * sizeof(long)));
    HIPCHK(hipMemcpy(m->d_haloAll, m->h_halo.data(), m->h_halo.size() * sizeof(long), hipMemcpyHostToDevice));
    m->nHaloAll = (int)(m->h_halo.size() / 2);
  }
  if (m->uvMap) {
    const long N2 = m->d.n2 * m->d.nTiles;
    for (int all = 0; all < 2; all++)
      for (int w = 0; w < 2; w++) {
        long *&dm = all ? m->d_uvAll[w] : m->d_uv[w];
        if (dm) { hipFree(dm); dm = nullptr; }
        const long l0 = all ? 0 : lo, l1 = all ? N2 : hi;
        const std::vector<long> &code = m->h_uv[w];   // [u | v], 0: the point is not written
        auto srcOfCode = [](long c) { return (c > 0 ? c : -c) - 1; };
        // early: the entry reads a point that the exchange writes (see uvPre)
        auto early = [&](long c) { return c != 0 && code[(size_t)srcOfCode(c)] != 0; };
        std::vector<long> e, pre;
        int nu = 0, nv = 0, pu = 0, pv = 0;
        for (int c = 0; c < 2; c++)
          for (long q = l0; q < l1; q++) {
            const long cd = code[(size_t)c * N2 + q];
            if (cd == 0) continue;
            if (early(cd)) {
              // one early launch is only right while no early entry reads another's target
              if (early(code[(size_t)srcOfCode(cd)]))
                return set_err("EXCH2 vector map: the halo of tile %ld copies a halo point that itself copies one "
                               "(tiles narrower than the halo are not supported on the device)", q / m->d.n2 + 1);
              if (m->d.nT < m->d.nTiles)
                return set_err("EXCH2 vector map: tiles as narrow as the halo are not supported in tile-sharded runs");
              pre.push_back(q); pre.push_back(cd);
              (c ? pv : pu)++;
              continue;
            }
            e.push_back(q); e.push_back(cd);
            (c ? nv : nu)++;
          }
        (all ? m->nUvUAll : m->nUvU)[w] = nu;
        (all ? m->nUvVAll : m->nUvV)[w] = nv;
        m->uvPre[all][w] = mgcm_model::UvPre{};
        const size_t nMain = e.size();
        e.insert(e.end(), pre.begin(), pre.end());
        if (!e.empty()) {
          HIPCHK(hipMalloc(&dm, e.size() * sizeof(long)));
          HIPCHK(hipMemcpy(dm, e.data(), e.size() * sizeof(long), hipMemcpyHostToDevice));
          m->uvPre[all][w].map = dm + nMain;
          m->uvPre[all][w].nU = pu;
          m->uvPre[all][w].nV = pv;
        }
      }
  }
  if (m->nHalo == 0) return 0;
  HIPCHK(hipMalloc(&m->d_halo, loc.size() * sizeof(long)));
  HIPCHK(hipMemcpy(m->d_halo, loc.data(), loc.size() * sizeof(long), hipMemcpyHostToDevice));
  return 0;
}

// ------------------------------------------------------------------ CG2D tables
// Each solver reads its own tables, and mgcm_init builds only those of the solver it selected:
// build_block (BlockRef), build_bxy (Bxy), build_mwg (Mwg, MwgRef).
template <typename T>
static int table_upload(T *&dptr, const std::vector<T> &h) {
  if (dptr) (void)hipFree(dptr);
  dptr = nullptr;
  HIPCHK(hipMalloc(&dptr, h.size() * sizeof(T)));
  HIPCHK(hipMemcpy(dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
// per 2-D point: the interior source of a halo point, -1 otherwise
static std::vector<long> halo_sources(const mgcm_model *m) {
  std::vector<long> srcOf((size_t)(m->d.n2 * m->d.nTiles), -1);
  for (size_t h = 0; h + 1 < m->h_halo.size(); h += 2) srcOf[m->h_halo[h]] = m->h_halo[h + 1];
  return srcOf;
}
// global lat-lon (I, J), 1-based -> tile-local point (i, j, t)
static void tile_point(const Dims &d, int I, int J, int &i, int &j, int &t) {
  const int bi = (I - 1) / d.sNx, bj = (J - 1) / d.sNy;
  t = bj * d.nSx + bi; i = (I - 1) % d.sNx + 1; j = (J - 1) % d.sNy + 1;
}
// Compact interior index (tile, j, i) of the point whose value a stencil finds at (i, j, t): the
// point itself, through the halo map the interior point a halo point is a copy of
// (EXCH_S3D_RL / EXCH_XY_RL), -1 where there is none.
static long value_point(const Dims &d, const std::vector<long> &srcOf, int i, int j, int t) {
  long g = MG_I2(d, i, j, t);
  if (i < 1 || i > d.sNx || j < 1 || j > d.sNy) g = srcOf[g];
  if (g < 0) return -1;
  const long tt = g / d.n2, l = g % d.n2;
  const int ii = (int)(l % d.nx) - d.OLx + 1, jj = (int)(l / d.nx) - d.OLy + 1;
  if (ii < 1 || ii > d.sNx || jj < 1 || jj > d.sNy) return -1;
  return tt * d.sNx * d.sNy + (long)(jj - 1) * d.sNx + (ii - 1);
}

// k_cg2d_block's tables: per interior point, in compact order, the compact indices of its W, E,
// S, N values packed as two 16-bit indices per word, and its 2-D offset; points are padded to
// NP = PPT*1024, and padding / missing neighbours point at the ZERO slot (index NP).
static int build_block(mgcm_model *m) {
  const Dims &d = m->d;
  const int NP = cg2d_block_ppt(m->nPts) * 1024;
  if (!NP) return set_err("build_block: %d points exceed k_cg2d_block's %d", m->nPts, cg2d_ref_max_points());
  const std::vector<long> srcOf = halo_sources(m);
  const unsigned ZERO = (unsigned)NP;
  auto slot = [&](int i, int j, int t) -> unsigned {
    const long c = value_point(d, srcOf, i, j, t);
    return c < 0 ? ZERO : (unsigned)c;
  };
  std::vector<unsigned> nb(2 * (size_t)NP, ZERO | (ZERO << 16));
  std::vector<int> gofs(NP, (int)MG_I2(d, 1, 1, 0));
  for (int t = 0; t < d.nTiles; t++)
    for (int j = 1; j <= d.sNy; j++)
      for (int i = 1; i <= d.sNx; i++) {
        const size_t pidx = (size_t)t * d.sNx * d.sNy + (size_t)(j - 1) * d.sNx + (i - 1);
        nb[2 * pidx] = slot(i - 1, j, t) | (slot(i + 1, j, t) << 16);
        nb[2 * pidx + 1] = slot(i, j - 1, t) | (slot(i, j + 1, t) << 16);
        gofs[pidx] = (int)MG_I2(d, i, j, t);
      }
  return table_upload(m->d_nbr, nb) || table_upload(m->d_gofs, gofs) ? -1 : 0;
}

// k_cg2d_bxy's tables (choose_bxy, build_bxy): BX x BY blocks formed on the global lat-lon
// index space, so they need the default EXCH1 lat-lon topology.
//
// Land-block compaction.  A block is left out of the tables when every point of it is a dry
// column with all four faces closed at every level -- decided from the static arrays
// INI_CG2D / UPDATE_CG2D build aW2d / aS2d from (h0FacW / h0FacS under the non-linear free
// surface, else hFacW / hFacS) and from hFacC.  Only the kept blocks are numbered; a left-out
// point's slot is the ZERO slot, so its neighbours read 0.0.  This is exact, not approximate, while cg2d_b and
// the first guess cg2d_x are 0.0 on those points, which holds by induction over the steps:
//   * cg2d_b: sfp_rhs_column (common.h) sums the fluxes through the point's faces, all 0.0
//     with the faces closed, the fresh-water term, masked by maskInC (0 on a dry column),
//     and the free-surface term, a multiple of etaH (etaN without exactConserv);
//   * cg2d_x, the first guess, is Bo_surf*etaN there; after the solve the epilogue (or
//     k_exch_eta) sets etaN = recip_Bo*cg2d_x, 0.0 where cg2d_x stayed 0.0;
//   * etaH: UPDATE_ETAH (k_corr_cont, k_calc_r_star) adds the masked divergence of the
//     transports through the same closed faces to etaN: 0.0 again.
// So the invariant can only be broken from outside: eta loaded from the host (checked by
// mgcm_init and mgcm_put*, land_eta_check) or b / x handed to mgcm_cg2d.  The solver's
// prologue scans the left-out points on every solve and records numIters = -1 on a
// non-zero (k_cg2d_bxy), which mgcm_cg2d answers by solving again on the full tables and a
// step reports as an error: a broken invariant is never a silently different answer.
//
// Selection: the first geometry of the preference list that the grid tiles into and that
// fits its thread count -- with every block where the full count fits (tables as without
// compaction), with the all-land blocks left out only where the full count does not fit
// but the kept count does.  MGCM_CG2D_BXY=<BX>x<BY>x<NT> (or the variant's index) forces a
// geometry; MGCM_CG2D_COMPACT=0 never leaves blocks out, =1 leaves them out wherever there
// are any.  After a broken invariant (noCompact) neither switch applies: the full tables of
// the first two geometries, as before compaction existed.
struct BxyChoice {
  int var = -1, bx = 0, by = 0, nt = 0;   // the geometry (kernels_solve.hip CGX[]); var -1: none fits
  int nBlk = 0;                           // blocks in the tables
  bool compacted = false;                 // the all-land blocks are left out
  int Nx = 0;
  std::vector<char> dry;                  // [global (J-1)*Nx + (I-1)]: the point may be left out; empty: no scan
  bool block_dry(int I0, int J0) const { return block_dry(I0, J0, bx, by); }
  bool block_dry(int I0, int J0, int bx_, int by_) const {
    if (dry.empty()) return false;
    for (int b = 0; b < by_; b++)
      for (int a = 0; a < bx_; a++)
        if (!dry[(size_t)(J0 + b - 1) * Nx + (I0 + a - 1)]) return false;
    return true;
  }
};
// A grid of more points than this gets no single-workgroup tables at all, whatever its land.
// It was the capacity of the generic one-workgroup kernel (retired) and is kept so that no
// grid's selection changes: lifting it would let large, mostly-land grids compact into
// k_cg2d_bxy, a change to measure on its own.
constexpr int CG2D_ONE_WG_MAX_POINTS = 8 * 1024;

static int choose_bxy(mgcm_model *m, BxyChoice &c) {
  const Dims &d = m->d;
  c = BxyChoice{};
  if (m->nPts > CG2D_ONE_WG_MAX_POINTS) return 0;
  const int Nx = d.sNx * d.nSx, Ny = d.sNy * d.nSy;
  c.Nx = Nx;
  // variants of kernels_solve.hip CGX[]: 3x2x512 first, the measured order (DESIGN.md "CG2D
  // on one CU", profiles/r07/cg2d_compact/); 3x4x256 (variant 2) fits no grid that 3x2x512
  // does not -- every 3x4 block is two 3x2 blocks -- and is reached by MGCM_CG2D_BXY only
  std::vector<int> pref = m->noCompact ? std::vector<int>{0, 1} : std::vector<int>{3, 0, 1};
  const char *envG = m->noCompact ? nullptr : getenv("MGCM_CG2D_BXY");
  const bool isForced = envG && *envG;
  if (isForced) {
    int forced = -1, fx = 0, fy = 0, ft = 0;
    if (sscanf(envG, "%dx%dx%d", &fx, &fy, &ft) == 3) {
      for (int v = 0; v < cg2d_bxy_variants(); v++) {
        int bx, by, nt;
        cg2d_bxy_geometry(v, &bx, &by, &nt);
        if (bx == fx && by == fy && nt == ft) forced = v;
      }
    } else if (envG[0] >= '0' && envG[0] <= '9' && atoi(envG) < cg2d_bxy_variants())
      forced = atoi(envG);
    if (forced < 0) return set_err("build_nbr: MGCM_CG2D_BXY=%s names no k_cg2d_bxy geometry", envG);
    pref.assign(1, forced);
  }
  if (!m->latlonTopology || getenv("MGCM_CG2D_NOBLOCKED")) return 0;
  const char *envC = m->noCompact ? nullptr : getenv("MGCM_CG2D_COMPACT");
  const int compactMode = m->noCompact ? 0 : (envC ? (atoi(envC) != 0 ? 2 : 0) : 1);   // 0 off, 1 where needed, 2 always
  if (compactMode > 0) {
    const bool nl = m->p.nonlinFreeSurf > 0;
    const size_t n3 = (size_t)d.n3 * d.nTiles;
    std::vector<double> hW(n3), hS(n3), hC(n3);
    HIPCHK(hipMemcpy(hW.data(), nl ? m->f.h0FacW : m->f.hFacW, n3 * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hS.data(), nl ? m->f.h0FacS : m->f.hFacS, n3 * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hC.data(), nl ? m->f.h0FacC : m->f.hFacC, n3 * sizeof(double), hipMemcpyDeviceToHost));
    c.dry.assign((size_t)Nx * Ny, 0);
    for (int J = 1; J <= Ny; J++)
      for (int I = 1; I <= Nx; I++) {
        int i, j, t;
        tile_point(d, I, J, i, j, t);
        bool closed = true;
        for (int k = 1; k <= d.Nr && closed; k++)
          closed = hC[MG_I3(d, i, j, k, t)] == 0.0 && hW[MG_I3(d, i, j, k, t)] == 0.0 &&
                   hW[MG_I3(d, i + 1, j, k, t)] == 0.0 && hS[MG_I3(d, i, j, k, t)] == 0.0 &&
                   hS[MG_I3(d, i, j + 1, k, t)] == 0.0;
        c.dry[(size_t)(J - 1) * Nx + (I - 1)] = closed;
      }
  }
  for (int v : pref) {
    int bx, by, nt;
    if (cg2d_bxy_geometry(v, &bx, &by, &nt)) continue;
    const int n = (Nx % bx == 0 && Ny % by == 0) ? (Nx / bx) * (Ny / by) : 0;
    if (n == 0) continue;
    int nDry = 0;
    for (int J0 = 1; J0 <= Ny; J0 += by)
      for (int I0 = 1; I0 <= Nx; I0 += bx) nDry += c.block_dry(I0, J0, bx, by) ? 1 : 0;
    const bool full = n <= nt && !(compactMode == 2 && nDry > 0);
    if (full || (nDry > 0 && n - nDry > 0 && n - nDry <= nt)) {
      c.var = v; c.bx = bx; c.by = by; c.nt = nt;
      c.nBlk = full ? n : n - nDry;
      c.compacted = !full;
      return 0;
    }
  }
  if (isForced)
    return set_err("build_nbr: the grid does not fit the k_cg2d_bxy geometry MGCM_CG2D_BXY=%s", envG);
  return 0;
}

// no k_cg2d_bxy tables: nothing is left out, so the land guards (land_eta_check, mgcm_cg2d) rest
static void clear_bxy(mgcm_model *m) {
  m->nBlkX = 0;
  m->bxyVar = -1;
  m->h_dropG.clear();
  m->nDropBlk = 0;
  if (m->d_dropG) { (void)hipFree(m->d_dropG); m->d_dropG = nullptr; }
}

static int build_bxy(mgcm_model *m, const BxyChoice &c) {
  const Dims &d = m->d;
  clear_bxy(m);
  const std::vector<long> srcOf = halo_sources(m);
  const int Nx = d.sNx * d.nSx, Ny = d.sNy * d.nSy;
  const int BX = c.bx, BY = c.by, NT = c.nt, NPT = BX * BY, NB = 2 * (BX + BY);
  const unsigned Z = (unsigned)(NPT * NT);   // the ZERO slot
  // LDS slot of an interior point: point-in-block major, block minor (p*NT + block),
  // so that consecutive threads touch consecutive doubles (no LDS bank conflicts)
  std::vector<unsigned> slotOf((size_t)m->nPts, Z);
  auto compact = [&](int i, int j, int t) { return (size_t)t * d.sNx * d.sNy + (size_t)(j - 1) * d.sNx + (i - 1); };
  int qb = 0;
  for (int J0 = 1; J0 <= Ny; J0 += BY)
    for (int I0 = 1; I0 <= Nx; I0 += BX) {
      const bool drop = c.compacted && c.block_dry(I0, J0);
      for (int b = 0; b < BY; b++)
        for (int a = 0; a < BX; a++) {
          int i, j, t;
          tile_point(d, I0 + a, J0 + b, i, j, t);
          if (drop) m->h_dropG.push_back((int)MG_I2(d, i, j, t));
          else slotOf[compact(i, j, t)] = (unsigned)((b * BX + a) * NT + qb);
        }
      if (drop) m->nDropBlk++;
      else qb++;
    }
  // slot of the value found at (i, j, t), through the halo map
  auto slot = [&](int i, int j, int t) -> unsigned {
    const long cp = value_point(d, srcOf, i, j, t);
    return cp < 0 ? Z : slotOf[cp];
  };
  std::vector<unsigned> nbx((size_t)(NB / 2) * NT, Z | (Z << 16));
  std::vector<int> blkx((size_t)NPT * NT, (int)MG_I2(d, 1, 1, 0));
  int q = 0;
  for (int J0 = 1; J0 <= Ny; J0 += BY)
    for (int I0 = 1; I0 <= Nx; I0 += BX) {
      if (c.compacted && c.block_dry(I0, J0)) continue;
      std::vector<int> ii(NPT), jj(NPT), tt(NPT);
      for (int b = 0; b < BY; b++)
        for (int a = 0; a < BX; a++) {
          tile_point(d, I0 + a, J0 + b, ii[b * BX + a], jj[b * BX + a], tt[b * BX + a]);
          blkx[(size_t)NPT * q + b * BX + a] = (int)MG_I2(d, ii[b * BX + a], jj[b * BX + a], tt[b * BX + a]);
        }
      // out-of-block neighbours, through each boundary point's own halo map
      std::vector<unsigned> v(NB);
      for (int b = 0; b < BY; b++) {
        const int w = b * BX, e = b * BX + BX - 1;
        v[b] = slot(ii[w] - 1, jj[w], tt[w]);
        v[BY + b] = slot(ii[e] + 1, jj[e], tt[e]);
      }
      for (int a = 0; a < BX; a++) {
        const int so = a, no = (BY - 1) * BX + a;
        v[2 * BY + a] = slot(ii[so], jj[so] - 1, tt[so]);
        v[2 * BY + BX + a] = slot(ii[no], jj[no] + 1, tt[no]);
      }
      for (int k = 0; k < NB / 2; k++) nbx[(size_t)(NB / 2) * q + k] = v[2 * k] | (v[2 * k + 1] << 16);
      q++;
    }
  if (table_upload(m->d_nbx, nbx) || table_upload(m->d_blkx, blkx)) return -1;
  m->bxyVar = c.var;
  m->nBlkX = c.nBlk;
  if (!m->h_dropG.empty()) {
    if (table_upload(m->d_dropG, m->h_dropG)) return -1;
    if (!m->h_guard) {
      HIPCHK(hipHostMalloc((void **)&m->h_guard, 64, hipHostMallocMapped));
      HIPCHK(hipHostGetDevicePointer((void **)&m->d_guard, m->h_guard, 0));
    }
    *m->h_guard = 0;
  }
  return 0;
}

// Multi-workgroup CG2D tables (kernels_cg2d_mwg.hip): every tile cut into row strips of
// <= OPT*NT points (one workgroup each), the two rings of neighbouring-part points each
// strip's stencils reach (through the halo map), LDS slot tables, export flags.
template <typename T>
static int mwg_upload(mgcm_model *m, const std::vector<T> &h, const T **out) {
  T *dptr = nullptr;
  HIPCHK(hipMalloc(&dptr, (h.empty() ? 1 : h.size()) * sizeof(T)));
  if (!h.empty()) HIPCHK(hipMemcpy(dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  m->mwgAllocs.push_back(dptr);
  *out = dptr;
  return 0;
}

static int mwg_block_realloc(mgcm_model *m, int mem, bool sys);
static int build_mwg(mgcm_model *m) {
  for (void *q : m->mwgAllocs) (void)hipFree(q);
  m->mwgAllocs.clear();
  const Dims &d = m->d;
  int NT, OPT, RPT;
  cg2d_mwg_geometry(&NT, &OPT, &RPT);
  const int NO = NT * OPT, NR = NT * RPT;
  if (d.sNx > NO) return set_err("build_mwg: sNx = %d > %d points per part", d.sNx, NO);
  const long N2 = d.n2 * d.nTiles;
  std::vector<long> srcOf(N2, -1);
  for (size_t h = 0; h + 1 < m->h_halo.size(); h += 2) srcOf[m->h_halo[h]] = m->h_halo[h + 1];
  const int ppTile = d.sNx * d.sNy;
  auto comp = [&](int i, int j, int t) { return t * ppTile + (j - 1) * d.sNx + (i - 1); };
  auto g2of = [&](int c) { const int t = c / ppTile, l = c % ppTile; return (int)MG_I2(d, l % d.sNx + 1, l / d.sNx + 1, t); };
  // neighbour (dir 0 W, 1 E, 2 S, 3 N) of compact point c, through the halo map; -1 = none
  auto nbr = [&](int c, int dir) -> int {
    const int t = c / ppTile, l = c % ppTile, i = l % d.sNx + 1, j = l / d.sNx + 1;
    const int ii = i + (dir == 0 ? -1 : dir == 1 ? 1 : 0), jj = j + (dir == 2 ? -1 : dir == 3 ? 1 : 0);
    if (ii >= 1 && ii <= d.sNx && jj >= 1 && jj <= d.sNy) return comp(ii, jj, t);
    const long src = srcOf[MG_I2(d, ii, jj, t)];
    if (src < 0) return -1;
    const int st = (int)(src / d.n2), sl = (int)(src % d.n2);
    const int si = sl % d.nx - d.OLx + 1, sj = sl / d.nx - d.OLy + 1;
    if (si < 1 || si > d.sNx || sj < 1 || sj > d.sNy) return -1;
    return comp(si, sj, st);
  };
  // parts: row strips of each tile
  int rows = NO / d.sNx;
  while (rows > 1 && 2 * (d.sNx + rows) > NR) rows--;
  if (rows > d.sNy) rows = d.sNy;
  const int nPartsTile = (d.sNy + rows - 1) / rows;
  std::vector<int> partOf((size_t)d.nTiles * ppTile);
  std::vector<std::vector<int>> own;
  for (int t = d.t0; t < d.t0 + d.nT; t++)
    for (int k = 0; k < nPartsTile; k++) {
      const int j0 = 1 + (k * d.sNy) / nPartsTile, j1 = ((k + 1) * d.sNy) / nPartsTile;
      std::vector<int> pts;
      for (int j = j0; j <= j1; j++)
        for (int i = 1; i <= d.sNx; i++) { pts.push_back(comp(i, j, t)); partOf[comp(i, j, t)] = (int)own.size(); }
      if ((int)pts.size() > NO) return set_err("build_mwg: part of %zu points > %d", pts.size(), NO);
      own.push_back(pts);
    }
  const int G = (int)own.size();
  std::vector<std::vector<int>> ring1(G), ring2(G);
  std::vector<std::vector<char>> inAnyRing(1);   // compact -> exported?
  std::vector<char> exported((size_t)d.nTiles * ppTile, 0);
  int r2max = 0;
  for (int g = 0; g < G; g++) {
    std::map<int, int> seen;   // compact -> 0 own, 1 ring1, 2 ring2
    for (int c : own[g]) seen[c] = 0;
    for (int c : own[g])
      for (int dir = 0; dir < 4; dir++) {
        const int nb = nbr(c, dir);
        if (nb >= 0 && !seen.count(nb)) { seen[nb] = 1; ring1[g].push_back(nb); }
      }
    for (int c : ring1[g])
      for (int dir = 0; dir < 4; dir++) {
        const int nb = nbr(c, dir);
        if (nb >= 0 && !seen.count(nb)) { seen[nb] = 2; ring2[g].push_back(nb); }
      }
    if ((int)ring1[g].size() > NR) return set_err("build_mwg: ring of %zu points > %d", ring1[g].size(), NR);
    for (int c : ring1[g]) exported[c] = 1;
    for (int c : ring2[g]) exported[c] = 1;
    r2max = std::max(r2max, (int)ring2[g].size());
  }
  const int IMAX = NR + ((r2max + 63) / 64) * 64, SZ = NO + IMAX;
  if (SZ >= 65535) return set_err("build_mwg: %d LDS slots exceed 16-bit indices", SZ);
  std::vector<int> ownG((size_t)G * NO, -1), ownC((size_t)G * NO, 0), ringG((size_t)G * NR, -1);
  std::vector<unsigned> ownNb((size_t)G * NO * 2, (unsigned)SZ | ((unsigned)SZ << 16)), ringNb((size_t)G * NR * 2,
                                                                                                 (unsigned)SZ | ((unsigned)SZ << 16));
  std::vector<unsigned> ownExp((size_t)G * NT, 0u);
  std::vector<int> impC((size_t)G * IMAX, 0), impG((size_t)G * IMAX, (int)MG_I2(d, 1, 1, d.t0)), nImp(G), ownN(G);
  m->mwgPlan.assign((size_t)G * NO, -1);
  // the exported points, numbered: their granules in the hand-off block
  std::vector<int> expSlot(exported.size(), -1);
  int nExp = 0;
  for (size_t c = 0; c < exported.size(); c++)
    if (exported[c]) expSlot[c] = nExp++;
  for (int g = 0; g < G; g++) {
    std::map<int, int> slot;
    ownN[g] = (int)own[g].size();
    for (size_t n = 0; n < own[g].size(); n++) {
      const int p = (int)n / NT, tid = (int)n % NT;
      slot[own[g][n]] = p * NT + tid;
    }
    for (size_t n = 0; n < ring1[g].size(); n++) slot[ring1[g][n]] = NO + (int)n;   // n = p*NT + tid
    for (size_t n = 0; n < ring2[g].size(); n++) slot[ring2[g][n]] = NO + NR + (int)n;
    auto sl = [&](int c) -> unsigned { if (c < 0) return (unsigned)SZ; auto it = slot.find(c); return it == slot.end() ? (unsigned)SZ : (unsigned)it->second; };
    for (size_t n = 0; n < own[g].size(); n++) {
      const int c = own[g][n], q = (int)n;   // slot p*NT + tid == n
      const size_t o = (size_t)g * NO + q;
      ownG[o] = g2of(c);
      ownC[o] = exported[c] ? expSlot[c] : 0;
      ownNb[2 * o] = sl(nbr(c, 0)) | (sl(nbr(c, 1)) << 16);
      ownNb[2 * o + 1] = sl(nbr(c, 2)) | (sl(nbr(c, 3)) << 16);
      if (exported[c]) ownExp[(size_t)g * NT + q % NT] |= 1u << (q / NT);
      m->mwgPlan[o] = ownG[o];
    }
    for (size_t n = 0; n < ring1[g].size(); n++) {
      const int c = ring1[g][n];
      const size_t o = (size_t)g * NR + n;
      ringG[o] = g2of(c);
      ringNb[2 * o] = sl(nbr(c, 0)) | (sl(nbr(c, 1)) << 16);
      ringNb[2 * o + 1] = sl(nbr(c, 2)) | (sl(nbr(c, 3)) << 16);
      impC[(size_t)g * IMAX + n] = expSlot[c];
      impG[(size_t)g * IMAX + n] = g2of(c);
    }
    for (size_t n = 0; n < ring2[g].size(); n++) {
      impC[(size_t)g * IMAX + NR + n] = expSlot[ring2[g][n]];
      impG[(size_t)g * IMAX + NR + n] = g2of(ring2[g][n]);
    }
    // the import slots run to the end of ring 2, or of ring 1 where there is no ring 2: the
    // unused ring-1 slots in front of a ring 2 poll export granule 0, which a part whose
    // stencils stay inside it (one part, periodic onto itself: no point exported) never gets.
    // This shortens the import sweep of every part without a ring 2 (e.g. the one-row parts
    // of a 126 x 3 box), not only of the lone part.  Their ring-1 slots past nImp keep the
    // value k_cg2d_mwg's prologue reads at impG's padding, cg2d_x(1,1,t0): it only ever meets
    // the zero coefficients of an inactive ring slot, and were it NaN or Inf the 0*NaN would
    // stay in r_l / s_l slots that no stencil of an active point names.
    nImp[g] = ring2[g].empty() ? (int)ring1[g].size() : NR + (int)ring2[g].size();
  }
  MwgTables &T = m->mwg;
  T = MwgTables{};
  if (mwg_upload(m, ownG, &T.ownG) || mwg_upload(m, ownC, &T.ownC) || mwg_upload(m, ownNb, &T.ownNb) ||
      mwg_upload(m, ownExp, &T.ownExp) || mwg_upload(m, ringG, &T.ringG) || mwg_upload(m, ringNb, &T.ringNb) ||
      mwg_upload(m, impC, &T.impC) || mwg_upload(m, impG, &T.impG) || mwg_upload(m, nImp, &T.nImp) ||
      mwg_upload(m, ownN, &T.ownN))
    return -1;
  T.G = G; T.IMAX = IMAX; T.SZ = SZ; T.nExp = nExp;
  T.pinned = (G <= 32 && !getenv("MGCM_CG2D_SPREAD")) ? 1 : 0;
  T.sys = 0;
  T.exclusive = 0;
  T.partsPerTile = (d.t0 == 0 && d.nT == d.nTiles) ? nPartsTile : 0;   // part ranges: whole-domain tables only
  // cg2dRefOrder: the sums chained along each tile's parts, then over the tiles (k_cg2d_mwg<.., REF>)
  T.ref = m->solver == Cg2dSolver::MwgRef ? 1 : 0;
  T.nTiles = d.nTiles;
  if (T.ref && T.partsPerTile <= 0)
    return set_err("mgcm_init: cg2dRefOrder in the multi-workgroup CG2D needs the whole domain's tiles, not the tile "
                   "range [%d, %d) of %d (mgcm_set_tile_range)", d.t0, d.t0 + d.nT, d.nTiles);
  // hand-off block: 64 B of words (launch epoch, timeout word), the partial granules, the
  // export granules, with cg2dRefOrder the carry and tile-partial granules (2 buffers x 3 values
  // x (G + nTiles) doubles); zeroed once here -- granule tags carry the launch epoch, so a launch
  // never matches an earlier launch's granules (a multiple of 16 B from the start)
  const size_t partGr = (size_t)2 * 3 * G * 2, refGr = T.ref ? (size_t)2 * 3 * (G + d.nTiles) * 2 : 0;
  const size_t hs = 64 + (partGr + (size_t)nExp * 4 + refGr) * sizeof(unsigned long long);
  char *blk = nullptr;
  HIPCHK(hipMalloc(&blk, hs));
  HIPCHK(hipMemset(blk, 0, hs));
  m->mwgAllocs.push_back(blk);
  m->mwgBlock = blk;
  // this process's launch epoch: its own word (not in the hand-off block an IPC import replaces)
  unsigned *ep = nullptr;
  HIPCHK(hipMalloc(&ep, 64));
  HIPCHK(hipMemset(ep, 0, 64));
  m->mwgAllocs.push_back(ep);
  T.epoch = ep;
  T.ctr = (unsigned *)blk;
  T.part = (unsigned long long *)(blk + 64);
  T.xs = T.part + partGr;
  T.refc = T.ref ? T.xs + (size_t)nExp * 4 : nullptr;
  T.hsBytes = hs;
  // The hand-off block's memory: where the parts spread over the XCDs (not pinned), uncached
  // device memory -- a granule store is then visible to the other XCDs' polls without an L2
  // round of its own: LLC-90 1.591 ms/step against 1.688 with the coarse-grained block, 117
  // parts, ~1 us per CG iteration (profiles/r04/mwgmem/); the XCD-pinned parts (cube, <= 32
  // parts, one XCD's L2) keep coarse-grained memory (cs32x15 0.416 against 0.421-0.455).
  // (fine-grained memory measured no better than coarse, system-scope accesses alike:
  // profiles/r04/mwgmem/)
  if (!T.pinned && mwg_block_realloc(m, 1, false)) return -1;
  return 0;
}

// ------------------------------------------------------------------ C-ABI
extern "C" {

const char *mgcm_last_error(void) { return g_err.c_str(); }

mgcm_model *mgcm_create(int sNx, int sNy, int OLx, int OLy, int Nr, int nSx, int nSy, int device) {
  if (sNx <= 0 || sNy <= 0 || Nr <= 0 || nSx <= 0 || nSy <= 0 || OLx < 2 || OLy < 2) {
    set_err("mgcm_create: invalid sizes (need OLx,OLy >= 2)");
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) {
    set_err("mgcm_create: no HIP device %d (found %d)", device, ndev);
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) { set_err("mgcm_create: hipSetDevice failed"); return nullptr; }
  mgcm_model *m = new mgcm_model();
  m->device = device;
  Dims &d = m->d;
  d.sNx = sNx; d.sNy = sNy; d.OLx = OLx; d.OLy = OLy; d.Nr = Nr; d.nSx = nSx; d.nSy = nSy; d.nTiles = nSx * nSy;
  d.nx = sNx + 2 * OLx; d.ny = sNy + 2 * OLy; d.n2 = (long)d.nx * d.ny; d.n3 = d.n2 * Nr;
  d.t0 = 0; d.nT = d.nTiles;
  // defaults (model/src/set_defaults.F, resolved by ini_parms.F)
  Params &p = m->p;
  p.abEps = 0.01; p.alph_AB = 0.5; p.beta_AB = 5.0 / 12.0; p.useAB3 = 0; p.rhoConst = 999.8; p.gBaro = 9.81; p.sideDragFactor = 2.0; p.freeSurfFac = 1.0;
  p.implicSurfPress = 1.0; p.implicDiv2DFlow = 1.0; p.rkSign = -1.0;
  p.afFacMom = p.vfFacMom = p.pfFacMom = p.cfFacMom = p.foFacMom = p.mtFacMom = 1.0;
  p.momAdvection = p.momViscosity = p.momForcing = p.useCoriolis = 1;
  p.no_slip_sides = p.no_slip_bottom = 1; p.momDissip_In_AB = 1; p.momForcingOutAB = 0;
  p.cg2dMaxIters = 150; p.cg2dNormaliseRHS = 1;
  // CG2D in fused multiply-adds where the kernel supports it (k_cg2d_bxy): 2.14 -> 1.83 us per
  // iteration on global_ocean.90x40x15; the device-order oracle evaluates the same fma chains
  p.cg2dUseFMA = 1;
  p.gravity = 9.81; p.gravitySign = -1.0; p.rhoNil = 999.8; p.tAlpha = 2.0e-4; p.tempAdvection = 1;
  p.tempForcing = 1; p.tempAdvScheme = 2; p.implicitDiffusion = 0;
  p.saltAdvection = 1; p.saltForcing = 1; p.saltAdvScheme = 2; p.multiDimAdvection = 1; p.momStepping = 1;
  p.HeatCapacity_Cp = 3994.0; p.convertFW2Salt = 35.0; p.temp_EvPrRn = 123456.7; p.salt_EvPrRn = 0.0;
  p.nForcRec = 12; p.GM_Small_Number = 1.0e-20; p.GM_slopeSqCutoff = 1.0e48; p.GM_skewflx = 1.0;
  if (hipStreamCreateWithFlags(&m->ownStream, hipStreamNonBlocking) != hipSuccess) {
    set_err("mgcm_create: stream");
    delete m;
    return nullptr;
  }
  m->stream = m->ownStream;
  if (hipStreamCreateWithFlags(&m->stream2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&m->evFork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&m->evHand, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&m->evJoin, hipEventDisableTiming) != hipSuccess ||
      hipEventCreate(&m->ovlEv[0]) != hipSuccess || hipEventCreate(&m->ovlEv[1]) != hipSuccess) {
    set_err("mgcm_create: second stream / events");
    delete m;
    return nullptr;
  }
  // MGCM_OVERLAP=1 forces the second stream on, =0 off; otherwise the graph path picks by timing
  const char *ov = getenv("MGCM_OVERLAP");
  m->overlap = !(ov && atoi(ov) == 0);
  m->ovlAuto = !ov;
  // one arena per kind for the 2-D and 3-D fields (MG_F2D_LIST / MG_F3D_LIST order, common.h)
  d.N2all = d.n2 * d.nTiles;
  d.N3all = d.n3 * d.nTiles;
  double *arena[2] = {nullptr, nullptr};
  const long arenaN[2] = {(long)F2_COUNT * d.N2all, (long)F3_COUNT * d.N3all};
  for (int q = 0; q < 2; q++) {
    if (hipMalloc(&arena[q], arenaN[q] * sizeof(double)) != hipSuccess ||
        hipMemset(arena[q], 0, arenaN[q] * sizeof(double)) != hipSuccess) {
      set_err("mgcm_create: hipMalloc of the %s arena (%ld doubles)", q ? "3-D" : "2-D", arenaN[q]);
      mgcm_destroy(m);
      return nullptr;
    }
    m->allocs.push_back(arena[q]);
  }
  m->f.a2 = arena[0];
  m->f.a3 = arena[1];
  int n2i = 0, n3i = 0;
  for (auto &fd : FIELDS) {
    const long n = field_count(m, fd.kind);
    double *ptr = nullptr;
    if (fd.kind == F2D) ptr = arena[0] + (long)(n2i++) * d.N2all;
    else if (fd.kind == F3D) ptr = arena[1] + (long)(n3i++) * d.N3all;
    else if (hipMalloc(&ptr, n * sizeof(double)) != hipSuccess || hipMemset(ptr, 0, n * sizeof(double)) != hipSuccess) {
      set_err("mgcm_create: hipMalloc %s (%ld doubles)", fd.name, n);
      mgcm_destroy(m);
      return nullptr;
    } else {
      m->allocs.push_back(ptr);
    }
    field_ptr(m, &fd) = ptr;
  }
  if (hipMalloc(&m->d_ctr, 2 * sizeof(int)) != hipSuccess || hipMemset(m->d_ctr, 0, 2 * sizeof(int)) != hipSuccess ||
      hipMalloc(&m->d_rec, m->maxRec * sizeof(SolveRecord)) != hipSuccess) {
    set_err("mgcm_create: counters");
    mgcm_destroy(m);
    return nullptr;
  }
  build_latlon_halo(m);
  // the zero fills above run on the null stream, which the model's non-blocking streams do
  // not wait for: finish them before any stream-ordered upload (mgcm_put) can start
  if (hipDeviceSynchronize() != hipSuccess) {
    set_err("mgcm_create: zero fill");
    mgcm_destroy(m);
    return nullptr;
  }
  return m;
}

void mgcm_destroy(mgcm_model *m) {
  if (!m) return;
  hipSetDevice(m->device);
  if (m->stream) hipStreamSynchronize(m->stream);
  ev_collect(m);
  ev_free(m);
  drop_graphs(m);
  for (void *p : m->allocs) hipFree(p);
  if (m->monBuf) hipFree(m->monBuf);
  if (m->d_halo) hipFree(m->d_halo);
  if (m->d_srcOf) hipFree(m->d_srcOf);
  if (m->d_haloRec) hipFree(m->d_haloRec);
  if (m->d_haloAll) hipFree(m->d_haloAll);
  for (int q = 0; q < 2; q++) {
    if (m->d_uv[q]) hipFree(m->d_uv[q]);
    if (m->d_uvAll[q]) hipFree(m->d_uvAll[q]);
  }
  if (m->d_tileInfo) hipFree(m->d_tileInfo);
  if (m->d_nbr) hipFree(m->d_nbr);
  if (m->d_gofs) hipFree(m->d_gofs);
  if (m->d_nbx) hipFree(m->d_nbx);
  if (m->d_blkx) hipFree(m->d_blkx);
  if (m->d_dropG) hipFree(m->d_dropG);
  if (m->h_guard) hipHostFree(m->h_guard);
  if (m->d_ctr) hipFree(m->d_ctr);
  for (auto &q : m->exchBuf)
    if (q) hipFree(q);
  if (m->d_rec) hipFree(m->d_rec);
  if (m->mwgShared) (void)hipIpcCloseMemHandle(m->mwgShared);
  for (void *q : m->mwgAllocs) hipFree(q);
  for (int q = 0; q < 2; q++) {
    if (m->stHost[q]) hipHostFree(m->stHost[q]);
    if (m->stEv[q]) hipEventDestroy(m->stEv[q]);
    if (m->stCopied[q]) hipEventDestroy(m->stCopied[q]);
    if (m->stDev[q]) hipFree(m->stDev[q]);
  }
  if (m->stCopy) hipStreamDestroy(m->stCopy);
  if (m->ownStream) hipStreamDestroy(m->ownStream);
  if (m->stream2) hipStreamDestroy(m->stream2);
  if (m->evFork) hipEventDestroy(m->evFork);
  if (m->evHand) hipEventDestroy(m->evHand);
  if (m->evJoin) hipEventDestroy(m->evJoin);
  for (auto &ev : m->ovlEv)
    if (ev) hipEventDestroy(ev);
  delete m;
}

int mgcm_set_param(mgcm_model *m, const char *name, double value) {
  drop_graphs(m);   // kernel arguments are captured by value
  m->ptrTabDirty = true;   // (the passive tracers' device table holds values derived from the parameters)
  if (!strcmp(name, "myIter")) {  // the device-side iteration counter (AB2 start, solve records)
    int it = (int)value;
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipMemcpyAsync(m->d_ctr, &it, sizeof(int), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
  }
  for (auto &pd : PARAMS)
    if (!strcmp(pd.name, name)) {
      char *ptr = reinterpret_cast<char *>(&m->p) + pd.off;
      if (pd.isint) *reinterpret_cast<int *>(ptr) = (int)value;
      else *reinterpret_cast<double *>(ptr) = value;
      return 0;
    }
  // options the kernels do not implement are accepted only at their default
  // (inert) value; anything else is an explicit error, never silently ignored.
  static const char *inert[] = {"implicitFreeSurface"};
  for (auto *n : inert)
    if (!strcmp(n, name)) {
      const bool isDefaultOff = (value == 0.0) || (!strcmp(n, "implicitFreeSurface") && value == 1.0);
      if (!isDefaultOff) return set_err("mgcm_set_param: option %s=%g is not supported by the device path yet", name, value);
      m->extra[name] = value;
      return 0;
    }
  m->extra[name] = value;
  return 0;
}

namespace mgcm {
__global__ void k_set_iter(int *ctr, int v) {
  if (threadIdx.x == 0) ctr[0] = v;
}
__global__ void k_add_iter(int *ctr, int inc) {
  if (threadIdx.x == 0) ctr[0] += inc;
}
}  // namespace mgcm

int mgcm_add_iter(mgcm_model *m, int inc) {
  HIPCHK(hipSetDevice(m->device));
  hipLaunchKernelGGL(mgcm::k_add_iter, dim3(1), dim3(64), 0, m->stream, m->d_ctr, inc);
  HIPCHK(hipGetLastError());
  return 0;
}

int mgcm_set_iter(mgcm_model *m, int myIter) {
  HIPCHK(hipSetDevice(m->device));
  hipLaunchKernelGGL(mgcm::k_set_iter, dim3(1), dim3(64), 0, m->stream, m->d_ctr, myIter);
  HIPCHK(hipGetLastError());
  return 0;
}

double mgcm_get_param(mgcm_model *m, const char *name) {
  if (!strcmp(name, "myIter")) {
    int it = 0;
    if (hipMemcpyAsync(&it, m->d_ctr, sizeof(int), hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess)
      return NAN;
    return it;
  }
  // 3: k_cg2d_bxy, 4: k_cg2d_mwg, 5: k_cg2d_block (reference order), 6: k_cg2d_mwg in the
  // reference order; 1 and 2 are retired (Cg2dSolver)
  if (!strcmp(name, "cg2dKernel")) return (double)(int)m->solver;
  if (!strcmp(name, "cg2dParts")) return m->useMwg() ? (double)m->mwg.G : 1.0;
  // 1 when the multi-workgroup solve's parts are placed on one XCD (one L2: ~1 us hand-offs)
  if (!strcmp(name, "cg2dPinned")) return m->useMwg() ? (double)m->mwg.pinned : 0.0;
  // THERMODYNAMICS on the second stream: 1 on, 0 off; -1 while the graph path is still timing
  // both (ovlMsOn / ovlMsOff: ovl_trial's event times of the two graphs, 8 steps each)
  if (!strcmp(name, "overlap")) return (m->ovlAuto && !m->ovlDecided) ? -1.0 : (m->overlap ? 1.0 : 0.0);
  if (!strcmp(name, "ovlMsOn")) return m->ovlMs[1];
  if (!strcmp(name, "ovlMsOff")) return m->ovlMs[0];
  if (!strcmp(name, "cg2dBxyVariant")) return (double)m->bxyVar;
  if (!strcmp(name, "cg2dDroppedBlocks")) return (double)(m->solver == Cg2dSolver::Bxy ? m->nDropBlk : 0);
  // the launch layout of the last FORWARD_STEP run (step_layout_bits of its plan)
  if (!strcmp(name, "stepLayout")) return (double)m->stepLayout;
  // the route of the last ptracers_on (0 no tracers, 1 functional, 2 batched) and its launches
  if (!strcmp(name, "ptrRoute")) return (double)m->ptrRoute;
  if (!strcmp(name, "ptrLaunches")) return (double)m->ptrLaunches;
  // 1 when the last THERMODYNAMICS formed GM_AdvForm's residual flow for its multi-dimensional tracers
  if (!strcmp(name, "gmResFlow")) return (double)m->gmResFlow;
  // whether the selected kernel solves with fused multiply-adds (k_cg2d_bxy honours cg2dUseFMA)
  if (!strcmp(name, "cg2dFMA")) return (m->solver == Cg2dSolver::Bxy && m->p.cg2dUseFMA) ? 1.0 : 0.0;
  for (auto &pd : PARAMS)
    if (!strcmp(pd.name, name)) {
      const char *ptr = reinterpret_cast<const char *>(&m->p) + pd.off;
      return pd.isint ? (double)*reinterpret_cast<const int *>(ptr) : *reinterpret_cast<const double *>(ptr);
    }
  auto it = m->extra.find(name);
  return it == m->extra.end() ? NAN : it->second;
}

// ---- pkg/ptracers: storage and parameters ------------------------------------------------
#define PTR_NF 7   // 3-D fields per tracer in the arena: the pair, gpTrNm1, T*, advScr1, advScr2, gAdv
int mgcm_ptracers_alloc(mgcm_model *m, int n) {
  if (n < 1 || n > 99) return set_err("mgcm_ptracers_alloc: %d tracers outside 1..99 (PTRACERS_num's two digits)", n);
  if (m->ready) return set_err("mgcm_ptracers_alloc: call before mgcm_init");
  if (!m->ptr.empty()) return set_err("mgcm_ptracers_alloc: the passive tracers are already allocated (%d)", (int)m->ptr.size());
  if (m->d.nT != m->d.nTiles)
    return set_err("mgcm_ptracers_alloc: passive tracers are not supported in tile-sharded runs (tile range [%d, %d) of %d)",
                   m->d.t0, m->d.t0 + m->d.nT, m->d.nTiles);
  HIPCHK(hipSetDevice(m->device));
  const size_t bytes = (size_t)n * PTR_NF * m->d.N3all * sizeof(double);
  HIPCHK(hipMalloc(&m->a4, bytes));
  m->allocs.push_back(m->a4);
  HIPCHK(hipMemset(m->a4, 0, bytes));
  HIPCHK(hipMalloc(&m->d_ptrTab, 2 * (size_t)n * sizeof(TracerArgs)));
  m->allocs.push_back(m->d_ptrTab);
  HIPCHK(hipMalloc(&m->d_ptrList, 2 * (size_t)n * sizeof(int)));
  m->allocs.push_back(m->d_ptrList);
  HIPCHK(hipDeviceSynchronize());   // (the zero fill ran on the null stream, as mgcm_create's)
  m->ptr.assign(n, mgcm_model::PTracer{});
  for (int i = 0; i < n; i++) {
    double *b = m->a4 + (size_t)i * PTR_NF * m->d.N3all;
    mgcm_model::PTracer &t = m->ptr[i];
    t.buf[0] = b; t.buf[1] = b + m->d.N3all; t.gNm1 = b + 2 * m->d.N3all; t.scr = b + 3 * m->d.N3all;
    t.adv1 = b + 4 * m->d.N3all; t.adv2 = b + 5 * m->d.N3all; t.gAdv = b + 6 * m->d.N3all;
  }
  m->ptrFlip = 0;
  m->ptrTabDirty = true;
  drop_graphs(m);
  return 0;
}
int mgcm_ptracers_count(mgcm_model *m) { return (int)m->ptr.size(); }

static double *ptracer_param_slot(mgcm_model::PTracer &t, const char *name, int **ip) {
  *ip = nullptr;
  if (!strcmp(name, "advScheme")) { *ip = &t.advScheme; return nullptr; }
  if (!strcmp(name, "useGMRedi")) { *ip = &t.useGMRedi; return nullptr; }
  if (!strcmp(name, "diffKh")) return &t.diffKh;
  if (!strcmp(name, "diffKr")) return &t.diffKr;
  if (!strcmp(name, "surfRelaxTau")) return &t.surfRelaxTau;
  if (!strcmp(name, "surfRelaxVal")) return &t.surfRelaxVal;
  if (!strcmp(name, "interiorSource")) return &t.interiorSource;
  if (!strcmp(name, "EvPrRn")) return &t.EvPrRn;
  return nullptr;
}
int mgcm_ptracer_param(mgcm_model *m, int iTracer, const char *name, double value) {
  if (iTracer < 1 || iTracer > (int)m->ptr.size())
    return set_err("mgcm_ptracer_param: tracer %d outside 1..%d", iTracer, (int)m->ptr.size());
  int *ip = nullptr;
  double *dp = ptracer_param_slot(m->ptr[iTracer - 1], name, &ip);
  if (!dp && !ip) return set_err("mgcm_ptracer_param: unknown parameter %s", name);
  if (ip) *ip = (int)value;
  else *dp = value;
  // (the scheme rules are mgcm_init's: a changed parameter needs a new mgcm_init)
  if (m->ready && (ip || !strcmp(name, "EvPrRn"))) m->ready = false;
  m->ptrTabDirty = true;
  drop_graphs(m);   // kernel arguments are captured by value
  return 0;
}
double mgcm_ptracer_param_get(mgcm_model *m, int iTracer, const char *name) {
  if (iTracer < 1 || iTracer > (int)m->ptr.size()) return NAN;
  int *ip = nullptr;
  double *dp = ptracer_param_slot(m->ptr[iTracer - 1], name, &ip);
  if (ip) return (double)*ip;
  return dp ? *dp : NAN;
}

int mgcm_put(mgcm_model *m, const char *name, const double *host, long count) {
  double *dev = nullptr;
  long n = 0;
  if (!lookup_field(m, name, &dev, &n)) return set_err("mgcm_put: unknown field %s", name);
  if (count > n || count <= 0) return set_err("mgcm_put: %s count %ld > %ld", name, count, n);
  if (m->ready && land_eta_check(m, name, host, count)) return -1;
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(mg_host_copy(dev, host, count * sizeof(double), hipMemcpyHostToDevice, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return 0;
}

namespace mgcm {
// The values of a staged batch to their fields: blockIdx.y = the field, its header entry
// (destination, start) read from the batch itself
__global__ void __launch_bounds__(256) k_put_scatter(const char *batch) {
  const long *hdr = reinterpret_cast<const long *>(batch);
  const long n = hdr[0];
  const int y = blockIdx.y;
  if (y >= n) return;
  double *dst = reinterpret_cast<double *>(hdr[1 + y]);
  const long o0 = hdr[1 + n + y], o1 = hdr[2 + n + y];
  const double *src = reinterpret_cast<const double *>(batch) + 2 + 2 * n;
  for (long i = o0 + blockIdx.x * 256L + threadIdx.x; i < o1; i += (long)gridDim.x * 256L) dst[i - o0] = src[i];
}
}  // namespace mgcm

// mgcm_put of n fields in stream order, without a host synchronisation: the host arrays are
// copied into a pinned slot as [n | destinations | starts | values], which goes up in one
// copy and is scattered to the fields by one launch.  A slot is reused only after its
// previous copy (two calls back) completed, so a step's upload never waits on the step before
// it; the host arrays may be reused as soon as the call returns.
int mgcm_put_batch_async(mgcm_model *m, int n, const char *const *names, const double *const *hosts,
                         const long *counts) {
  if (n <= 0) return 0;
  std::vector<double *> dst(n);
  long total = 0, maxc = 0;
  for (int i = 0; i < n; i++) {
    long lim = 0;
    if (!lookup_field(m, names[i], &dst[i], &lim)) return set_err("mgcm_put_batch_async: unknown field %s", names[i]);
    if (counts[i] > lim || counts[i] <= 0)
      return set_err("mgcm_put_batch_async: %s count %ld > %ld", names[i], counts[i], lim);
    if (m->ready && land_eta_check(m, names[i], hosts[i], counts[i])) return -1;
    total += counts[i];
    maxc = std::max(maxc, counts[i]);
  }
  HIPCHK(hipSetDevice(m->device));
  const size_t bytes = (size_t)(2 + 2 * n + total) * sizeof(double);
  if (m->stCap < bytes) {
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->stCopy) HIPCHK(hipStreamSynchronize(m->stCopy));
    else HIPCHK(hipStreamCreateWithFlags(&m->stCopy, hipStreamNonBlocking));
    for (int q = 0; q < 2; q++) {
      if (m->stHost[q]) HIPCHK(hipHostFree(m->stHost[q]));
      if (m->stDev[q]) HIPCHK(hipFree(m->stDev[q]));
      m->stHost[q] = nullptr;
      m->stDev[q] = nullptr;
      HIPCHK(hipHostMalloc((void **)&m->stHost[q], bytes, hipHostMallocDefault));
      HIPCHK(hipMalloc((void **)&m->stDev[q], bytes));
      if (!m->stEv[q]) HIPCHK(hipEventCreateWithFlags(&m->stEv[q], hipEventDisableTiming));
      if (!m->stCopied[q]) HIPCHK(hipEventCreateWithFlags(&m->stCopied[q], hipEventDisableTiming));
    }
    m->stCap = bytes;
  }
  const int q = m->stNext;
  m->stNext ^= 1;
  HIPCHK(hipEventSynchronize(m->stEv[q]));   // slot q's previous scatter (two calls back) is done
  long *hdr = reinterpret_cast<long *>(m->stHost[q]);
  double *vals = reinterpret_cast<double *>(m->stHost[q]) + 2 + 2 * n;
  hdr[0] = n;
  long o = 0;
  for (int i = 0; i < n; i++) {
    hdr[1 + i] = reinterpret_cast<long>(dst[i]);
    hdr[1 + n + i] = o;
    memcpy(vals + o, hosts[i], counts[i] * sizeof(double));
    o += counts[i];
  }
  hdr[1 + 2 * n] = o;
  // the copy on the copy stream (beside whatever the model stream still runs), the scatter
  // in the model stream's order after it
  HIPCHK(hipMemcpyAsync(m->stDev[q], m->stHost[q], bytes, hipMemcpyHostToDevice, m->stCopy));
  HIPCHK(hipEventRecord(m->stCopied[q], m->stCopy));
  HIPCHK(hipStreamWaitEvent(m->stream, m->stCopied[q], 0));
  const unsigned gx = (unsigned)std::min<long>(64, (maxc + 255) / 256);
  hipLaunchKernelGGL(mgcm::k_put_scatter, dim3(gx, n), dim3(256), 0, m->stream, m->stDev[q]);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(m->stEv[q], m->stream));
  return 0;
}

int mgcm_put_async(mgcm_model *m, const char *name, const double *host, long count) {
  return mgcm_put_batch_async(m, 1, &name, &host, &count);
}

int mgcm_get(mgcm_model *m, const char *name, double *host, long count) {
  double *dev = nullptr;
  long n = 0;
  if (!lookup_field(m, name, &dev, &n)) return set_err("mgcm_get: unknown field %s", name);
  if (count > n || count <= 0) return set_err("mgcm_get: %s count %ld > %ld", name, count, n);
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(mg_host_copy(host, dev, count * sizeof(double), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return 0;
}

double *mgcm_device_ptr(mgcm_model *m, const char *name) {
  double *dev = nullptr;
  long n = 0;
  if (!lookup_field(m, name, &dev, &n)) { set_err("mgcm_device_ptr: unknown field %s", name); return nullptr; }
  return dev;
}

int mgcm_set_halo_map(mgcm_model *m, const long *src_of_point, long count) {
  const long N2 = m->d.n2 * m->d.nTiles;
  if (count != N2) return set_err("mgcm_set_halo_map: count %ld != %ld", count, N2);
  m->h_halo.clear();
  // a map identical to the default lat-lon one keeps the global-index CG2D blocking
  build_latlon_halo(m);
  std::vector<long> ll = m->h_halo;
  m->h_halo.clear();
  for (long q = 0; q < N2; q++)
    if (src_of_point[q] >= 0 && src_of_point[q] != q) {
      m->h_halo.push_back(q);
      m->h_halo.push_back(src_of_point[q]);
    }
  m->latlonTopology = (ll == m->h_halo);
  m->ready = false;
  return 0;
}

int mgcm_set_uv_map(mgcm_model *m, const long *u1, const long *v1, const long *u0, const long *v0,
                    const int *tileFace, const int *tileEdge, long count) {
  const long N2 = m->d.n2 * m->d.nTiles;
  if (count != N2) return set_err("mgcm_set_uv_map: count %ld != %ld", count, N2);
  const long *src[2][2] = {{u0, v0}, {u1, v1}};
  for (int w = 0; w < 2; w++) {
    m->h_uv[w].assign((size_t)2 * N2, 0);
    for (int c = 0; c < 2; c++)
      for (long q = 0; q < N2; q++) {
        const long code = src[w][c][q];
        const long s = (code > 0 ? code : -code) - 1;
        if (code != 0 && (s < 0 || s >= 2 * N2)) return set_err("mgcm_set_uv_map: bad code %ld at %ld", code, q);
        m->h_uv[w][(size_t)c * N2 + q] = code;
      }
  }
  std::vector<int> info(2 * (size_t)m->d.nTiles);
  for (int t = 0; t < m->d.nTiles; t++) { info[t] = tileFace[t]; info[m->d.nTiles + t] = tileEdge[t]; }
  HIPCHK(hipSetDevice(m->device));
  if (m->d_tileInfo) (void)hipFree(m->d_tileInfo);
  HIPCHK(hipMalloc(&m->d_tileInfo, info.size() * sizeof(int)));
  HIPCHK(hipMemcpy(m->d_tileInfo, info.data(), info.size() * sizeof(int), hipMemcpyHostToDevice));
  m->f.tileFace = m->d_tileInfo;
  m->f.tileEdge = m->d_tileInfo + m->d.nTiles;
  m->p.cubeCorners = 1;
  m->uvMap = true;
  m->ready = false;
  drop_graphs(m);
  return 0;
}

// The early entries of the vector map (mgcm_model::uvPre) on u, v: to be launched ahead of
// every launch that applies d_uv / d_uvAll to the same pair; no launch where there are none.
static hipError_t uv_pre(mgcm_model *m, const Dims &d, double *u, double *v, int nz, int w, bool all = false) {
  const mgcm_model::UvPre &p = m->uvPre[all ? 1 : 0][w];
  return launch_exchange_uv(d, u, v, p.map, p.nU, p.nV, nz, m->stream);
}

// EXCH_UV_XYZ_RL / EXCH_UV_XY_RL of a C-grid vector pair: the EXCH2 vector map when one
// is installed, else the two components through the scalar (EXCH1) map.
static int exchange_uv(mgcm_model *m, double *u, double *v, int nz, bool withSigns) {
  if (!m->uvMap) {
    HIPCHK(launch_exchange(m->d, u, m->d_halo, m->nHalo, nz, m->stream));
    HIPCHK(launch_exchange(m->d, v, m->d_halo, m->nHalo, nz, m->stream));
    return 0;
  }
  const int w = withSigns ? 1 : 0;
  HIPCHK(uv_pre(m, m->d, u, v, nz, w));
  HIPCHK(launch_exchange_uv(m->d, u, v, m->d_uv[w], m->nUvU[w], m->nUvV[w], nz, m->stream));
  return 0;
}

// CALC_R_STAR (calc_r_star.F): on an EXCH2 topology k_calc_r_star evaluates the W/S
// factors in place and EXCH_UV_XY_RL(rStarFacW, rStarFacS, .FALSE.) (calc_r_star.F:256-257)
// refills their halos through the vector map; rStarDh*Dt and rStarExp* are pointwise
// functions of the new and old factors, so their halos are the same copies.
// In tile-sharded runs every process holds the whole 2-D state after the free-surface
// gathers, so the r* state (factors, hFac, CG2D operator) is recomputed on EVERY tile,
// redundantly and identically: no communication, and the replicated CG2D sees the global
// operator.
static Dims all_tiles(const Dims &d) { Dims a = d; a.t0 = 0; a.nT = d.nTiles; return a; }

// stagEx (cube/LLC maps, the whole domain): DO_STAGGER_FIELDS_EXCHANGES' u, v, w ride in
// CALC_R_STAR's grid (k_rstar_exmix, MG_FUSE_ENDS)
static hipError_t calc_r_star(mgcm_model *m, bool fuseEtaH = false, int fromX = 0, bool stagEx = false) {
  const Dims da = all_tiles(m->d);
  hipError_t e;
  if (stagEx) {
    XFields xw{};
    xw.p[0] = m->f.wVel; xw.nz[0] = m->d.Nr; xw.n = 1;
    e = uv_pre(m, m->d, m->f.uVel, m->f.vVel, m->d.Nr, 1);
    if (e != hipSuccess) return e;
    e = launch_rstar_exmix(da, m->p, m->f, m->d_srcOf, fuseEtaH, fromX, m->f.uVel, m->f.vVel, m->d.Nr, m->d_uv[1],
                           m->nUvU[1], m->nUvV[1], xw, m->d_halo, m->nHalo, m->stream);
  } else
    e = launch_calc_r_star(da, m->p, m->f, m->d_srcOf, m->stream, fuseEtaH, fromX);
  if (e != hipSuccess || !m->uvMap) return e;
  double *us[3] = {m->f.rStarFacW, m->f.rStarDhWDt, m->f.rStarExpW}, *vs[3] = {m->f.rStarFacS, m->f.rStarDhSDt,
                                                                                 m->f.rStarExpS};
  for (int q = 0; q < 3; q++)
    if ((e = uv_pre(m, da, us[q], vs[q], 1, 0, true)) != hipSuccess) return e;
  return launch_exchange_uv_pairs(da, us, vs, 3, m->d_uvAll[0], m->nUvUAll[0], m->nUvVAll[0], m->stream);
}
// sfp: k_sfp_rhs fused into the r* column pass (FORWARD_STEP on the whole domain only: in a
// tile-sharded run the r* pass covers every tile and the right-hand side this process's own)
static hipError_t update_r_star_cg2d(mgcm_model *m, bool sfp = false, bool opEarly = false, bool pcHere = false,
                                     const int *physNext = nullptr, bool keepFac = false, bool spec = false) {
  return launch_update_r_star_cg2d(all_tiles(m->d), m->p, m->f, m->d_srcOf, m->stream, sfp, opEarly, pcHere, physNext,
                                   keepFac, spec);
}

int mgcm_init(mgcm_model *m) {
  auto ext = [&](const char *n, double dflt) { auto it = m->extra.find(n); return it == m->extra.end() ? dflt : it->second; };
  HIPCHK(hipSetDevice(m->device));
  // a retired fusion bit is refused, never ignored: an A/B run must measure what it asked for
  const char *retired = nullptr;
  if (const int bit = mg_fuse_retired(&retired))
    return set_err("mgcm_init: MGCM_STEP_FUSE bit %d (%s) was measured slower than the default and removed in round 10 "
                   "(common.h); unset it", bit, retired);
  if (upload_halo(m)) return -1;
  // The CG2D solver, selected here and nowhere else:
  //   * cg2dRefOrder (parity runs on the reference's own tiling): the reference's summation
  //     order, in k_cg2d_block where the grid fits one workgroup, else in k_cg2d_mwg<.., REF>;
  //   * k_cg2d_bxy on a lat-lon grid that fits one of its geometries (choose_bxy);
  //   * otherwise, or with cg2dForceMwg (the tile-sharded device CG2D runs its parts in several
  //     processes), the multi-workgroup k_cg2d_mwg.  A generic point-per-thread kernel in one
  //     workgroup once took the grids k_cg2d_bxy does not; it measured 12.7 against 4.2
  //     us/iteration on the cube and was superseded in round 3.
  m->noCompact = false;
  m->nPts = m->d.nTiles * m->d.sNx * m->d.sNy;
  BxyChoice bxy;
  if (choose_bxy(m, bxy)) return -1;
  if (m->p.cg2dRefOrder) {
    if (m->p.useSRCGSolver) return set_err("mgcm_init: cg2dRefOrder with useSRCGSolver not implemented");
    m->solver = m->nPts > cg2d_ref_max_points() ? Cg2dSolver::MwgRef : Cg2dSolver::BlockRef;
  } else
    m->solver = (bxy.var < 0 || ext("cg2dForceMwg", 0.0) != 0.0) ? Cg2dSolver::Mwg : Cg2dSolver::Bxy;
  if (m->p.useSRCGSolver && m->solver == Cg2dSolver::BlockRef)
    return set_err("mgcm_init: useSRCGSolver (CG2D_SR) is implemented in the blocked single-workgroup and the "
                   "multi-workgroup CG2D only");
  clear_bxy(m);
  if (m->solver == Cg2dSolver::Bxy ? build_bxy(m, bxy) : m->solver == Cg2dSolver::BlockRef ? build_block(m) : build_mwg(m))
    return -1;
  if (!m->h_dropG.empty()) {
    // the state the fields were loaded with (a cold start, a pickup): eta must be 0.0 on the
    // points the compacted tables leave out, else the full tables (land_uncompact)
    const long n2a = m->d.n2 * m->d.nTiles;
    std::vector<double> eta((size_t)n2a);
    for (const char *nm : {"etaN", "etaH"}) {
      if (!strcmp(nm, "etaH") && m->p.nIter0 == 0) continue;   // INI_PSURF below: etaH = etaN
      HIPCHK(hipMemcpy(eta.data(), !strcmp(nm, "etaN") ? m->f.etaN : m->f.etaH, n2a * sizeof(double), hipMemcpyDeviceToHost));
      if (land_eta_check(m, nm, eta.data(), n2a)) return -1;
    }
  }
  if ((m->p.viscA4D != 0.0 || m->p.viscA4Z != 0.0) && (m->d.OLx < 3 || m->d.OLy < 3))
    return set_err("mgcm_init: biharmonic viscosity needs OLx, OLy >= 3 (del2u of the halo ring)");
  const bool rstar = m->p.nonlinFreeSurf > 0;
  if (rstar) {
    if (m->p.nonlinFreeSurf != 4 || m->p.select_rStar != 2)
      return set_err("mgcm_init: the non-linear free surface is implemented for nonlinFreeSurf=4, select_rStar=2 only");
    if (!m->p.exactConserv) return set_err("mgcm_init: nonlinFreeSurf needs exactConserv");
  }
  if (m->p.selectP_inEOS_Zc > 2) return set_err("mgcm_init: selectP_inEOS_Zc = 3 needs the non-hydrostatic pressure");
  if (m->p.selectP_inEOS_Zc == 2 && !m->p.storePhiHyd4Phys)
    return set_err("mgcm_init: selectP_inEOS_Zc = 2 needs storePhiHyd4Phys (set_parms.F:297)");
  // implicitViscosity: MOM_U/V_IMPLICIT_R (k_mom_impl); with the CD scheme also IMPLDIFF on
  // vVelD / uVelD (dynamics.F:614-634, k_impldiff_cd)
  if (m->p.implicitViscosity && (ext("momImplVertAdv", 0.0) != 0.0 || ext("selectImplicitDrag", 0.0) != 0.0))
    return set_err("mgcm_init: momImplVertAdv / selectImplicitDrag not implemented on the device");
  if (m->p.vectorInvariantMomentum) {
    // the MOM_VECINV subset k_mom_step implements (see kernels_dyn.hip)
    if (m->d.OLx < 2 || m->d.OLy < 2) return set_err("mgcm_init: vector-invariant momentum needs OLx, OLy >= 2");
    if (m->p.viscA4D != 0.0 || m->p.viscA4Z != 0.0)
      return set_err("mgcm_init: biharmonic viscosity with vectorInvariantMomentum not implemented on the device");
    if (m->p.useNHMTerms || m->p.select3dCoriScheme > 0 || m->p.useCDscheme)
      return set_err("mgcm_init: NH metric / 3-D Coriolis / CD scheme with vectorInvariantMomentum not implemented");
    if (m->p.selectVortScheme < 0 || m->p.selectVortScheme > 3 || m->p.selectKEscheme < 0 || m->p.selectKEscheme > 3 ||
        m->p.selectCoriScheme < 0 || m->p.selectCoriScheme > 3)
      return set_err("mgcm_init: selectVortScheme/selectKEscheme/selectCoriScheme outside 0..3");
    auto e = m->extra.find("useAbsVorticity");
    if (e != m->extra.end() && e->second != 0.0) return set_err("mgcm_init: useAbsVorticity not implemented");
  }
  if (m->uvMap && m->p.useCDscheme) return set_err("mgcm_init: CD scheme on an EXCH2 topology not implemented");
  if (m->p.implicSurfPress != 1.0 || m->p.implicDiv2DFlow != 1.0)
    return set_err("mgcm_init: implicSurfPress/implicDiv2DFlow != 1 not supported yet");
  const bool sph = ext("usingSphericalPolarGrid", 0.0) != 0.0;
  m->p.metricSphere = sph && ext("selectMetricTerms", 1.0) >= 1.0;
  m->p.recip_rSphere = sph ? 1.0 / ext("rSphere", 6370.0e3) : 0.0;   // ini_parms.F:1334
  if (ext("integr_GeoPot", 2.0) != 2.0) return set_err("mgcm_init: only integr_GeoPot = 2 is implemented");
  // tracer advection schemes implemented on the device: 2 (C2), 3 (U3) and 4 (C4) inside
  // GAD_CALC_RHS with Adams-Bashforth on the tendency; multi-dimensional 30 (DST3), 33 (DST3
  // flux-limited), 1 (upwind), 20 (DST2) and 7 (OS7MP); the vertical scheme must match the
  // horizontal one.  (77 and the other flux limiters, SOM, PPM / PQM: not restated.)
  auto mdScheme = [&](int s) { return s == 30 || s == 33 || s == 1 || s == 20 || s == 7; };
  auto okScheme = [&](int s, const char *vname) {
    return (s == 2 || s == 3 || s == 4 || (mdScheme(s) && m->p.multiDimAdvection)) && ext(vname, (double)s) == (double)s;
  };
  // OS7MP reaches 4 cells: GAD_CHECK wants an overlap of 4 (gad_init_fixed.F:52), 8 on the cube
  // (gad_init_fixed.F:178-181 doubles it), where the wider reach across face edges is not restated
  auto os7mpRefused = [&](int s, const char *who) {   // (0: accepted)
    if (s != 7 || !m->p.multiDimAdvection) return 0;
    if (m->uvMap)
      return set_err("mgcm_init: %s 7 (OS7MP) on an EXCH2 topology is not implemented: the cube needs OLx, OLy >= 8 "
                     "(gad_init_fixed.F:178-181) and the 4-cell reach across face edges is not restated", who);
    if (m->d.OLx < 4 || m->d.OLy < 4)
      return set_err("mgcm_init: %s 7 (OS7MP) needs OLx, OLy >= 4 (GAD_CHECK: Overlap Size too small)", who);
    return 0;
  };
  auto wideScheme = [&](int s) { return s == 3 || s == 4; };
  if (((m->p.tempStepping && wideScheme(m->p.tempAdvScheme)) || (m->p.saltStepping && wideScheme(m->p.saltAdvScheme))) &&
      (m->uvMap || m->d.OLx < 2 || m->d.OLy < 2))
    return set_err("mgcm_init: advection schemes 3 / 4 need OLx, OLy >= 2 and a lat-lon topology on the device");
  // ADAMS_BASHFORTH3 (ALLOW_ADAMSBASHFORTH_3) is restated for the tracers' tendencies only
  if (m->p.useAB3 && (m->p.momStepping || (m->p.nonlinFreeSurf > 0 && m->p.select_rStar > 0) || m->p.staggerTimeStep))
    return set_err("mgcm_init: ADAMS_BASHFORTH3 only for the tracers (momStepping off, no r*, not staggered)");
  // (a restart would need both history slots, gtNm(:,:,:,1:2), which the pickup path does not carry)
  if (m->p.useAB3 && m->p.nIter0 != 0) return set_err("mgcm_init: ADAMS_BASHFORTH3 from a pickup (nIter0 != 0) not supported");
  // the cube's multi-dimensional split (3 face-dependent passes with corner fills,
  // gad_advection.F:339-367) runs the general pass kernels (kernels_thermo.hip k_advg_*),
  // which need the tile face / edge table of the EXCH2 topology and OLx = OLy (corner fills)
  if (m->uvMap && ((m->p.tempStepping && mdScheme(m->p.tempAdvScheme)) || (m->p.saltStepping && mdScheme(m->p.saltAdvScheme)))) {
    if (!m->f.tileFace) return set_err("mgcm_init: multi-dimensional advection on EXCH2 needs the tile face table");
    if (m->d.OLx != m->d.OLy) return set_err("mgcm_init: cube multi-dimensional advection needs OLx = OLy");
    // GAD_CHECK (gad_check.F:115-130): minOlSize = GAD_OlMinSize(1) * GAD_OlMinSize(3), the scheme's
    // own 2 (DST3, DST3FL: gad_init_fixed.F:50-51) doubled under useCubedSphereExchange with
    // useMultiDimAdvec (gad_init_fixed.F:178-181) -- the overlap-only passes update the halo
    if (m->d.OLx < 4 || m->d.OLy < 4)
      return set_err("mgcm_init: multi-dimensional advection on the cube needs OLx, OLy >= 4 (GAD_CHECK: Overlap Size too small)");
  }
  if (m->p.tempStepping && !okScheme(m->p.tempAdvScheme, "tempVertAdvScheme"))
    return set_err("mgcm_init: tempAdvScheme %d not implemented on the device", m->p.tempAdvScheme);
  if (m->p.saltStepping && !okScheme(m->p.saltAdvScheme, "saltVertAdvScheme"))
    return set_err("mgcm_init: saltAdvScheme %d not implemented on the device", m->p.saltAdvScheme);
  if (m->p.tempStepping && os7mpRefused(m->p.tempAdvScheme, "tempAdvScheme")) return -1;
  if (m->p.saltStepping && os7mpRefused(m->p.saltAdvScheme, "saltAdvScheme")) return -1;
  if (m->p.useGMRedi && m->p.GM_AdvForm && m->p.GM_skewflx != 0.0)
    return set_err("mgcm_init: GM_AdvForm needs GM_skewflx = 0 (gmredi_readparms.F:243-244)");
  // pkg/ptracers: a tracer is accepted with exactly the options salt would be accepted with
  for (size_t it = 0; it < m->ptr.size(); it++) {
    const mgcm_model::PTracer &t = m->ptr[it];
    const int s = t.advScheme, no = (int)it + 1;
    if (!std::isnan(t.EvPrRn))
      return set_err("mgcm_init: pTracer%02d: PTRACERS_EvPrRn is not implemented on the device (only the unset case: "
                     "no fresh-water dilution of the tracer)", no);
    if (m->p.useAB3) return set_err("mgcm_init: passive tracers with ADAMS_BASHFORTH3 (useAB3) are not implemented");
    if (m->d.nT != m->d.nTiles) return set_err("mgcm_init: passive tracers are not supported in tile-sharded runs");
    if (wideScheme(s) && (m->uvMap || m->d.OLx < 2 || m->d.OLy < 2))
      return set_err("mgcm_init: pTracer%02d: advection schemes 3 / 4 need OLx, OLy >= 2 and a lat-lon topology on the device", no);
    if (m->uvMap && mdScheme(s)) {
      if (!m->f.tileFace) return set_err("mgcm_init: pTracer%02d: multi-dimensional advection on EXCH2 needs the tile face table", no);
      if (m->d.OLx != m->d.OLy) return set_err("mgcm_init: pTracer%02d: cube multi-dimensional advection needs OLx = OLy", no);
      if (m->d.OLx < 4 || m->d.OLy < 4)
        return set_err("mgcm_init: pTracer%02d: multi-dimensional advection on the cube needs OLx, OLy >= 4 (GAD_CHECK: Overlap Size too small)", no);
    }
    if (!okScheme(s, "PTRACERS_vertAdvScheme"))
      return set_err("mgcm_init: pTracer%02d: advScheme %d not implemented on the device", no, s);
    char who[32];
    snprintf(who, sizeof who, "pTracer%02d: advScheme", no);
    if (os7mpRefused(s, who)) return -1;
  }
  if (m->p.eosType != 0 && m->p.eosType != 1) return set_err("mgcm_init: eosType %d not implemented", m->p.eosType);
  if (m->d.Nr > 64) return set_err("mgcm_init: Nr = %d > 64 (column kernels hold a column in one workgroup)", m->d.Nr);
  if (m->p.periodicExternalForcing && (m->p.nForcRec < 1 || m->p.nForcRec > MG_MAXREC))
    return set_err("mgcm_init: nForcRec %d outside 1..%d", m->p.nForcRec, MG_MAXREC);
  drop_graphs(m);
  m->thetaA = m->f.theta;
  m->saltA = m->f.salt;
  m->useGraph = true;
  int it0 = m->p.nIter0;
  // every copy is ordered on the model's stream (a null-stream hipMemcpy does not wait for
  // the non-blocking streams)
  HIPCHK(hipMemcpyAsync(m->d_ctr, &it0, sizeof(int), hipMemcpyHostToDevice, m->stream));
  // INI_PSURF (ini_psurf.F:84) on a cold start: etaH = etaN (a pickup holds etaH)
  if (m->p.nIter0 == 0)
    HIPCHK(hipMemcpyAsync(m->f.etaH, m->f.etaN, m->d.n2 * m->d.nTiles * sizeof(double), hipMemcpyDeviceToDevice,
                          m->stream));
  if (rstar) {
    // INITIALISE_VARIA (initialise_varia.F:299-349): CALC_R_STAR(etaH) -> UPDATE_R_STAR ->
    // UPDATE_CG2D -> INTEGR_CONTINUITY(nIter0) (+ UPDATE_ETAH, EXCH w) -> CALC_R_STAR(etaH)
    HIPCHK(calc_r_star(m));
    HIPCHK(update_r_star_cg2d(m));
    HIPCHK(launch_corr_cont(m->d, m->p, m->f, 1, m->stream));
    HIPCHK(launch_exch_eta(m->d, m->p, m->f, m->d_srcOf, true, 1, m->stream));
    HIPCHK(launch_exchange(m->d, m->f.wVel, m->d_halo, m->nHalo, m->d.Nr, m->stream));
    HIPCHK(calc_r_star(m));
    HIPCHK(hipStreamSynchronize(m->stream));
  }
  m->ptrTabDirty = true;
  if (ptr_tables_sync(m)) return -1;
  m->ready = true;
  return 0;
}

static hipError_t launch_cg2d(mgcm_model *m, int maxIters, int nIterMin) {
  switch (m->solver) {
    case Cg2dSolver::Bxy:
      return launch_cg2d_bxy(m->bxyVar, m->d, m->p, m->f, m->d_nbx, m->d_blkx, m->nBlkX, maxIters, nIterMin, m->d_rec,
                             m->d_ctr + 1, m->d_dropG, (int)m->h_dropG.size(), m->h_dropG.empty() ? nullptr : m->d_guard,
                             m->stream);
    case Cg2dSolver::BlockRef:
      return launch_cg2d_block(m->d, m->p, m->f, m->d_nbr, m->d_gofs, m->nPts, maxIters, nIterMin, m->d_rec, m->d_ctr + 1,
                               m->stream);
    case Cg2dSolver::Mwg:
    case Cg2dSolver::MwgRef:
      return launch_cg2d_mwg(m->d, m->p, m->f, m->mwg, maxIters, nIterMin, m->d_rec, m->d_ctr + 1, m->stream);
  }
  return hipErrorInvalidValue;
}

// The zero-on-land invariant of the compacted k_cg2d_bxy tables (choose_bxy), on the host side;
// only the Bxy solver leaves blocks out (h_dropG), so only it comes here.
// land_uncompact: the full tables of the geometry used before compaction existed, from now on;
// the captured graphs hold the old tables' addresses and go.  The solver stays k_cg2d_bxy: a
// grid whose full tables fit no geometry is an error.
static int land_uncompact(mgcm_model *m) {
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  drop_graphs(m);
  m->noCompact = true;
  BxyChoice bxy;
  if (choose_bxy(m, bxy)) return -1;
  if (m->h_guard) *m->h_guard = 0;
  if (bxy.var < 0) {
    clear_bxy(m);
    return set_err("land_uncompact: no single-workgroup CG2D fits this grid without leaving the all-land blocks out");
  }
  return build_bxy(m, bxy);
}
// eta arriving from the host (n values of a 2-D field from its start): non-zero on a left-out point?
static int land_eta_check(mgcm_model *m, const char *name, const double *host, long n) {
  if (m->h_dropG.empty() || (strcmp(name, "etaN") && strcmp(name, "etaH"))) return 0;
  for (int g : m->h_dropG)
    if (g < n && !(host[g] == 0.0)) return land_uncompact(m);
  return 0;
}
// a step's solve found a non-zero on a left-out point (k_cg2d_bxy's guard): its results are
// not those of the full solve, and every later call says so
static int land_guard_check(mgcm_model *m, const char *who) {
  if (m->h_guard && *(volatile int *)m->h_guard)
    return set_err("%s: a CG2D solve of an earlier step found a non-zero cg2d_b or cg2d_x on a land point of a block left "
                   "out of the solver's tables (recorded as numIters = -1); its results are invalid -- load the state "
                   "through mgcm_put / mgcm_init, which check eta on those points, or set MGCM_CG2D_COMPACT=0", who);
  return 0;
}

static int check_ready(mgcm_model *m) {
  if (!m->ready) return set_err("model not initialised: call mgcm_init() after loading the fields");
  return 0;
}

#define TIMED(K, CALL)                      \
  do {                                      \
    int ev_ = ev_begin(m, K);               \
    hipError_t e_ = (CALL);                 \
    ev_end(m, K, ev_);                      \
    if (e_ != hipSuccess) return set_err("%s: %s", KNAMES[K], hipGetErrorString(e_)); \
  } while (0)

static int dynamics_on(mgcm_model *m, bool ring) {
  TIMED(K_PHI, launch_phi_hyd(m->d, m->p, m->f, m->stream));   // CALC_PHI_HYD (dynamics.F:462)
  TIMED(K_MOM, launch_mom_step(m->d, m->p, m->f, m->d_ctr, m->stream, ring));
  return 0;
}
int mgcm_dynamics(mgcm_model *m) {
  if (check_ready(m)) return -1;
  return dynamics_on(m, true);
}

// gad_init_fixed.F:126-162: multi-dimensional advection for the schemes that are not
// Adams-Bashforth ones; AB (2 or 3) on the tendency for C2, U3 and C4
static bool scheme_is_ab(int scheme) { return scheme == 2 || scheme == 3 || scheme == 4; }
static bool scheme_multi_dim(const Params &p, int advection, int scheme) {
  return p.multiDimAdvection && advection && !scheme_is_ab(scheme);
}
// Whether this model's THERMODYNAMICS takes GM_AdvForm's residual flow (k_gm_residual_flow ->
// uRes, vRes, wRes): some stepped tracer -- theta, salt or a passive one -- is multi-dimensional.
// From the parameters alone: plan_step launches the kernel by it (StepPlan::resFlow) and the two
// builders below point every tracer's passes at the flow by it.
static bool takes_res_flow(const mgcm_model *m) {
  const Params &p = m->p;
  if (!p.useGMRedi || !p.GM_AdvForm) return false;
  if (p.tempStepping && scheme_multi_dim(p, p.tempAdvection, p.tempAdvScheme)) return true;
  if (p.saltStepping && scheme_multi_dim(p, p.saltAdvection, p.saltAdvScheme)) return true;
  for (const auto &t : m->ptr)
    if (scheme_multi_dim(p, 1, t.advScheme)) return true;
  return false;
}
// what both builders derive from the model: the scheme's fields (a.advection is set) and the
// flow the multi-dimensional passes advect by
// res: takes_res_flow(m), evaluated once by the caller
static void tracer_args_common(const mgcm_model *m, int scheme, bool res, TracerArgs &a) {
  a.dT = m->p.deltaTtracer;
  a.multiDim = scheme_multi_dim(m->p, a.advection, scheme);
  a.useAB = scheme_is_ab(scheme);
  // the flux function the passes are compiled for, and its parameter: DST3 (30) without, DST3FL
  // (33) with the flux limiter; upwind (1) and DST2 (20) are GAD_DST2U1's xLimit = 0 / 1
  a.advFamily = scheme == 7 ? MG_ADV_OS7MP : (scheme == 1 || scheme == 20) ? MG_ADV_DST2U1 : MG_ADV_DST3;
  a.advParm = scheme == 33 || scheme == 20;
  a.scheme = scheme;
  a.advU = res ? m->f.uRes : m->f.uVel;
  a.advV = res ? m->f.vRes : m->f.vVel;
  a.advW = res ? m->f.wRes : m->f.wVel;
}

static TracerArgs tracer_args(const mgcm_model *m, bool salt) {
  const Params &p = m->p;
  TracerArgs a{};
  const int scheme = salt ? p.saltAdvScheme : p.tempAdvScheme;
  a.tr = salt ? m->f.salt : m->f.theta;
  a.trNext = salt ? m->f.saltNext : m->f.thetaNext;
  a.gNm1 = salt ? m->f.gsNm1 : m->f.gtNm1;
  a.scr = salt ? m->f.cpScr : m->f.gTscr;   // own scratch each: the two may run concurrently
  a.cp = salt ? m->f.advScr2 : m->f.advScr1;
  a.sfc = salt ? m->f.surfaceForcingS : m->f.surfaceForcingT;
  a.diffKh = salt ? p.diffKhS : p.diffKhT;
  a.diffKr = salt ? p.diffKrS : p.diffKrT;
  a.advection = salt ? p.saltAdvection : p.tempAdvection;
  a.forcing = salt ? p.saltForcing : p.tempForcing;
  a.gNm2 = salt ? m->f.gsNm2 : m->f.gtNm2;
  a.gm = p.useGMRedi;
  a.adv1 = m->f.advScr1; a.adv2 = m->f.advScr2; a.gAdv = m->f.gAdv;
  tracer_args_common(m, scheme, takes_res_flow(m), a);
  return a;
}

// Passive tracer i (0-based) of PTRACERS_INTEGRATE (ptracers_integrate.F:150-420): salt's
// sequence with the tracer's own parameters (PTRACERS_advScheme, _diffKh, _diffKr,
// _useGMRedi), its own buffers and scratch, and the forcing restated from the reference's
// experiment code (common.h TracerArgs).  flip: the parity the arguments are for.
static TracerArgs tracer_args_ptr(const mgcm_model *m, int i, int flip, bool res) {
  const Params &p = m->p;
  const mgcm_model::PTracer &t = m->ptr[i];
  TracerArgs a{};
  a.tr = t.buf[flip];
  a.trNext = t.buf[flip ^ 1];
  a.gNm1 = t.gNm1;
  a.scr = t.scr;
  a.cp = t.adv1;   // (the marches' c': unused with multi-dimensional advection, as salt's advScr2)
  a.sfc = nullptr;   // surfaceForcingPTr = 0 (PTRACERS_EvPrRn unset) unless the relaxation below
  a.diffKh = t.diffKh;
  a.diffKr = t.diffKr;
  a.advection = 1;
  a.forcing = 0;
  a.gNm2 = nullptr;   // (ADAMS_BASHFORTH3 is refused with passive tracers)
  a.relaxRate = t.surfRelaxTau != 0.0 ? 1.0 / t.surfRelaxTau : 0.0;
  a.relaxVal = t.surfRelaxVal;
  a.src = t.interiorSource;
  a.gm = p.useGMRedi && t.useGMRedi != 0;
  a.adv1 = t.adv1; a.adv2 = t.adv2; a.gAdv = t.gAdv;
  tracer_args_common(m, t.advScheme, res, a);
  return a;
}
// MGCM_PTR_BATCH=1: the batched kernels wherever they apply (kernels_ptracers.hip ptr_batch_ok:
// no k-march, no ADAMS_BASHFORTH3, and where the multi-dimensional tracers take the general form
// of GAD_ADVECTION -- every EXCH2 topology, multiDimCompressible -- a frame of at most 64 KiB);
// =0 and the default: one launch_tracer_step per tracer.  Read whenever
// ptracers_on runs, which for forward_step is when a step graph is captured: the graph caches
// are not keyed on the switch (nor on MGCM_STEP_FUSE), so a model that has captured its graphs
// keeps their route whatever the variable says later (tools/ptracers_ab.py, tools/ptracers_cube_ab.py:
// one model per route); mgcm_get_param "ptrRoute" / "ptrLaunches" say which route ran.
// The default is the lat-lon measurement's (tools/ptracers_ab.py, profiles/r09/ptracers/): on
// tutorial_global_oce_latlon the tracers run beside the 190 us pressure solve, where 4 tracers
// cost nothing either way and the batched launches measured 1 % above the per-tracer ones in
// every alternation (0.2575-0.2650 against 0.2547-0.2624 ms/step), although they take 57 us
// of kernel time in 5 launches against 134 us in 20; at 8 tracers the per-tracer launches
// outlast the solve (0.387 ms/step) and the batched ones do not (0.258): set it to 1 there.
// On the cube it is the faster route from the first tracer on (tools/ptracers_cube_ab.py,
// profiles/r11/ptracers_cube/): global_ocean.cs32x15 is staggered with r*, the tracers sit on the
// critical path before UPDATE_R_STAR, and a scheme-33 tracer is 28 launches there: 0.519 against
// 0.476 ms/step at 1 tracer, 0.843 against 0.485 at 4, 1.298 against 0.522 at 8 (0.391 without).
static bool ptr_batched(const mgcm_model *m) {
  const char *e = getenv("MGCM_PTR_BATCH");
  if (!e || atoi(e) == 0) return false;
  return ptr_batch_ok(m->d, m->p, m->ptrNMd > 0);
}
// The batched kernels' device tables, one per parity: uploaded by mgcm_init and, after a
// parameter change, by the next entry point that steps (never inside a graph capture).  An entry
// depends on the tracer's own parameters, on deltaTtracer, on what takes_res_flow reads --
// useGMRedi, GM_AdvForm, multiDimAdvection, temp / saltStepping, temp / saltAdvection,
// temp / saltAdvScheme and every tracer's advScheme -- and on device pointers fixed at
// allocation.  All of these change through mgcm_set_param, mgcm_ptracer_param or
// mgcm_ptracers_alloc, which mark the tables dirty (as mgcm_init does).
static int ptr_tables_sync(mgcm_model *m) {
  const int n = (int)m->ptr.size();
  if (!n || !m->ptrTabDirty) return 0;
  std::vector<TracerArgs> tab(2 * (size_t)n);
  const bool res = takes_res_flow(m);
  for (int q = 0; q < 2; q++)
    for (int i = 0; i < n; i++) tab[(size_t)q * n + i] = tracer_args_ptr(m, i, q, res);
  // launch order: the GM/Redi tracers first (their own kernel), and in each kind the longest
  // bodies first -- U3 / C4 inside GAD_CALC_RHS, then C2, then the multi-dimensional tracers
  // (their advection ran in the passes)
  std::vector<int> lists(2 * (size_t)n, 0);
  m->ptrNMd = 0;
  m->ptrNGM = 0;
  int na = 0;
  for (int cls = 0; cls < 6; cls++)
    for (int i = 0; i < n; i++) {
      const TracerArgs &a = tab[i];
      const int c = (a.gm ? 0 : 3) + (a.multiDim ? 2 : (a.scheme == 2 ? 1 : 0));
      if (c == cls) lists[n + na++] = i;
    }
  for (int fam = 0; fam < MG_ADV_NFAM; fam++) {   // one set of pass launches per family (launch_ptracers_batch)
    m->ptrNMdFam[fam] = 0;
    for (int i = 0; i < n; i++)
      if (tab[i].multiDim && tab[i].advFamily == fam) { lists[m->ptrNMd++] = i; m->ptrNMdFam[fam]++; }
  }
  for (int i = 0; i < n; i++)
    if (tab[i].gm) m->ptrNGM++;
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  HIPCHK(hipMemcpy(m->d_ptrTab, tab.data(), tab.size() * sizeof(TracerArgs), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->d_ptrList, lists.data(), lists.size() * sizeof(int), hipMemcpyHostToDevice));
  m->ptrTabDirty = false;
  return 0;
}
// PTRACERS_INTEGRATE on stream `st`, after salt, and the tracers' part of
// DO_FIELDS_BLOCKING_EXCHANGES right behind it on the same stream (nothing reads the new
// tracers before the next step, so the end-of-step kernels stay as they are); then all pairs
// swap together (CYCLE_TRACER)
static int ptracers_on(mgcm_model *m, hipStream_t st) {
  const int n = (int)m->ptr.size();
  m->ptrRoute = 0;
  m->ptrLaunches = 0;
  if (!n) return 0;
  if (m->ptrTabDirty) return set_err("ptracers_on: the passive tracers' device table is stale");
  if (ptr_batched(m)) {
    m->ptrRoute = 2;
    TIMED(K_TEMP, launch_ptracers_batch(m->d, m->p, m->f, m->d_ptrTab + (size_t)m->ptrFlip * n, m->d_ptrList, n, m->ptrNMdFam, n,
                                        m->ptrNGM, m->d_ctr, st, &m->ptrLaunches));
  } else {
    m->ptrRoute = 1;
    const bool res = takes_res_flow(m);
    for (int i = 0; i < n; i++)
      TIMED(K_TEMP, launch_tracer_step(m->d, m->p, m->f, tracer_args_ptr(m, i, m->ptrFlip, res), m->d_ctr, st, true, &m->ptrLaunches));
  }
  for (int i0 = 0; i0 < n; i0 += MG_XMAX) {
    XFields x{};
    for (int i = i0; i < n && i < i0 + MG_XMAX; i++) { x.p[x.n] = m->ptr[i].buf[m->ptrFlip ^ 1]; x.nz[x.n] = m->d.Nr; x.n++; }
    TIMED(K_EXCH, launch_exchange_multi(m->d, x, m->d_halo, m->nHalo, nullptr, st));
  }
  m->ptrFlip ^= 1;
  return 0;
}

// GMREDI_RESIDUAL_FLOW (thermodynamics.F:252-270) at the head of THERMODYNAMICS, where the model
// takes it (StepPlan::resFlow); gmResFlow: what mgcm_get_param reports, nothing here reads it
static int res_flow_on(mgcm_model *m, hipStream_t st) {
  m->gmResFlow = takes_res_flow(m) ? 1 : 0;
  if (m->gmResFlow) TIMED(K_TEMP, launch_gm_residual_flow(m->d, m->p, m->f, st));
  return 0;
}

// TEMP_INTEGRATE / SALT_INTEGRATE (and PTRACERS_INTEGRATE) on stream `st` (the ping-pong swaps are host-side)
static int tracers_on(mgcm_model *m, hipStream_t st) {
  if (res_flow_on(m, st)) return -1;
  const TracerArgs aT = tracer_args(m, false), aS = tracer_args(m, true);
  if (tracer_hpair_ok(m->d, m->p, aT, aS)) {   // small grids: both tracers per launch
    TIMED(K_TEMP, launch_tracer_hpair(m->d, m->p, m->f, aT, aS, m->d_ctr, st));
    std::swap(m->f.theta, m->f.thetaNext);
    std::swap(m->f.salt, m->f.saltNext);
    return ptracers_on(m, st);
  }
  if (m->p.tempStepping) {
    TIMED(K_TEMP, launch_tracer_step(m->d, m->p, m->f, aT, m->d_ctr, st));
    std::swap(m->f.theta, m->f.thetaNext);   // CYCLE_TRACER: the new theta is the other buffer
  }
  if (m->p.saltStepping) {
    TIMED(K_TEMP, launch_tracer_step(m->d, m->p, m->f, aS, m->d_ctr, st));
    std::swap(m->f.salt, m->f.saltNext);
  }
  return ptracers_on(m, st);
}

int mgcm_thermodynamics(mgcm_model *m) {
  if (check_ready(m) || ptr_tables_sync(m)) return -1;
  // forward_step.F:656 DO_OCEANIC_PHYS (every step: forcing records, EOS, GM tensor),
  // :732 THERMODYNAMICS (staggerTimeStep = F; the tracers only when stepped)
  TIMED(K_PHYS, launch_oceanic_phys(m->d, m->p, m->f, m->d_ctr, m->stream));
  return tracers_on(m, m->stream);
}

// The routine-level ops run the same kernels as one_step, split at the reference's
// routine boundaries (forward_step.F:925-976), so a host that calls them in FORWARD_STEP
// order reproduces mgcm_forward_step bit for bit.
static int solve_impl(mgcm_model *m) {
  TIMED(K_RHS, launch_sfp_rhs(m->d, m->p, m->f, m->stream));
  const int nIterMin = m->p.cg2dUseMinResSol - 1;
  TIMED(K_CG2D, launch_cg2d(m, m->p.cg2dMaxIters, nIterMin));
  // EXCH_XY_RL(cg2d_x) + etaN = recip_Bo*cg2d_x (solve_for_pressure.F:309-330)
  TIMED(K_ETA, launch_exch_eta(m->d, m->p, m->f, m->d_srcOf, false, 0, m->stream));
  return 0;
}

int mgcm_solve_for_pressure(mgcm_model *m) {
  if (check_ready(m)) return -1;
  return solve_impl(m);
}

int mgcm_momentum_correction_step(mgcm_model *m) {
  if (check_ready(m)) return -1;
  TIMED(K_CORR, launch_correction(m->d, m->p, m->f, m->stream));
  return 0;
}

int mgcm_integr_continuity(mgcm_model *m) {
  if (check_ready(m)) return -1;
  // integr_continuity.F:66-310 (exactConserv eta, INTEGRATE_FOR_W incl. r*) from the corrected
  // uVel, vVel; :324-350 EXCH etaN + UPDATE_ETAH (PmEpR under real fresh water)
  TIMED(K_CONT, launch_corr_cont(m->d, m->p, m->f, 2, m->stream));
  if (m->p.exactConserv) TIMED(K_ETA, launch_exch_eta(m->d, m->p, m->f, m->d_srcOf, true, 0, m->stream));
  return 0;
}

int mgcm_update_r_star(mgcm_model *m) {
  if (check_ready(m)) return -1;
  // UPDATE_R_STAR(.TRUE.) + UPDATE_CG2D (forward_step.F:829-877)
  if (m->p.nonlinFreeSurf > 0) TIMED(K_RSTAR, update_r_star_cg2d(m));
  return 0;
}

int mgcm_calc_r_star(mgcm_model *m) {
  if (check_ready(m)) return -1;
  // CALC_R_STAR(etaH) (forward_step.F:965-977)
  if (m->p.nonlinFreeSurf > 0) TIMED(K_RSTAR, calc_r_star(m));
  return 0;
}

static XFields blocking_fields(const mgcm_model *m, int tracers = 1, bool totPhi = true);

int mgcm_blocking_exchanges(mgcm_model *m) {
  if (check_ready(m)) return -1;
  // DO_FIELDS_BLOCKING_EXCHANGES (do_fields_blocking_exchanges.F:54-97): the set FORWARD_STEP
  // exchanges (one_step), without advancing the step counter
  if (m->uvMap) TIMED(K_EXCH, exchange_uv(m, m->f.uVel, m->f.vVel, m->d.Nr, true) ? hipErrorUnknown : hipSuccess);
  TIMED(K_EXCH, launch_exchange_multi(m->d, blocking_fields(m), m->d_halo, m->nHalo, nullptr, m->stream));
  return 0;
}

int mgcm_stagger_exchanges(mgcm_model *m) {
  if (check_ready(m)) return -1;
  // DO_STAGGER_FIELDS_EXCHANGES (do_stagger_fields_exchanges.F:37-43): EXCH_UV_3D_RL(uVel,
  // vVel, .TRUE.) and EXCH_3D_RL(wVel) before the staggered THERMODYNAMICS -- the exchange
  // one_step makes there
  if (m->uvMap) {
    XFields xw{};
    xw.p[0] = m->f.wVel; xw.nz[0] = m->d.Nr; xw.n = 1;
    HIPCHK(uv_pre(m, m->d, m->f.uVel, m->f.vVel, m->d.Nr, 1));
    TIMED(K_EXCH, launch_exchange_mixed(m->d, m->f.uVel, m->f.vVel, m->d.Nr, m->d_uv[1], m->nUvU[1], m->nUvV[1], xw,
                                        m->d_halo, m->nHalo, nullptr, m->stream));
  } else {
    TIMED(K_EXCH, exchange_uv(m, m->f.uVel, m->f.vVel, m->d.Nr, true) ? hipErrorUnknown : hipSuccess);
    TIMED(K_EXCH, launch_exchange(m->d, m->f.wVel, m->d_halo, m->nHalo, m->d.Nr, m->stream));
  }
  return 0;
}

int mgcm_oceanic_phys(mgcm_model *m) {
  if (check_ready(m)) return -1;
  TIMED(K_PHYS, launch_oceanic_phys(m->d, m->p, m->f, m->d_ctr, m->stream));
  return 0;
}

int mgcm_tracer_step(mgcm_model *m) {
  if (check_ready(m) || ptr_tables_sync(m)) return -1;
  return tracers_on(m, m->stream);
}

// EXCH_XY_RL / EXCH_XYZ_RL / EXCH_UV_*_RL on a caller's (host) array: staged through a
// device scratch pair, exchanged with the model's maps, copied back.
static int exch_scratch(mgcm_model *m, int nz) {
  const long need = (long)nz * m->d.n2 * m->d.nTiles;
  if (need <= m->exchCap) return 0;
  for (auto &q : m->exchBuf)
    if (q) { hipFree(q); q = nullptr; }
  HIPCHK(hipMalloc(&m->exchBuf[0], need * sizeof(double)));
  HIPCHK(hipMalloc(&m->exchBuf[1], need * sizeof(double)));
  m->exchCap = need;
  return 0;
}

int mgcm_exchange_host(mgcm_model *m, double *u, double *v, int nz, int vector, int withSigns) {
  // needs only the halo maps (usable before mgcm_init: the reference exchanges while
  // initialising, e.g. INI_FIELDS)
  if (!m->d_srcOf && upload_halo(m)) return -1;
  if (nz < 1 || nz > m->d.Nr) return set_err("mgcm_exchange_host: nz = %d outside 1..%d", nz, m->d.Nr);
  if (vector && !v) return set_err("mgcm_exchange_host: a vector exchange needs both components");
  if (exch_scratch(m, nz)) return -1;
  HIPCHK(hipSetDevice(m->device));
  const size_t bytes = (size_t)nz * m->d.n2 * m->d.nTiles * sizeof(double);
  double *host[2] = {u, v};
  for (int c = 0; c < 2; c++)
    if (host[c]) HIPCHK(mg_host_copy(m->exchBuf[c], host[c], bytes, hipMemcpyHostToDevice, m->stream));
  // every tile's halo, also when this model steps a tile subset (the host array is the domain)
  const long *hmap = m->d_haloAll ? m->d_haloAll : m->d_halo;
  const int nh = m->d_haloAll ? m->nHaloAll : m->nHalo;
  if (vector && m->uvMap) {
    const int w = withSigns ? 1 : 0;
    HIPCHK(uv_pre(m, m->d, m->exchBuf[0], m->exchBuf[1], nz, w, true));
    HIPCHK(launch_exchange_uv(m->d, m->exchBuf[0], m->exchBuf[1], m->d_uvAll[w], m->nUvUAll[w], m->nUvVAll[w], nz,
                              m->stream));
  } else {
    for (int c = 0; c < 2; c++)
      if (host[c]) HIPCHK(launch_exchange(m->d, m->exchBuf[c], hmap, nh, nz, m->stream));
  }
  for (int c = 0; c < 2; c++)
    if (host[c]) HIPCHK(mg_host_copy(host[c], m->exchBuf[c], bytes, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return 0;
}

const char *mgcm_param_name(int i) {
  const int n = (int)(sizeof(PARAMS) / sizeof(PARAMS[0]));
  return (i >= 0 && i < n) ? PARAMS[i].name : nullptr;
}

long mgcm_field_count(mgcm_model *m, const char *name) {
  double *dev = nullptr;
  long n = 0;
  if (!lookup_field(m, name, &dev, &n)) { set_err("mgcm_field_count: unknown field %s", name); return -1; }
  return n;
}

// tracers: 1 every field (the reference's set), 0 without theta/salt (exchanged beside the
// pressure solve, one_step), 2 theta/salt only
// totPhi = false: without totPhiHyd (a step whose last grid runs the next step's CALC_PHI_HYD, which
// stores totPhiHyd on exchange destinations; its halo is next read at the sources, one_step)
static XFields blocking_fields(const mgcm_model *m, int tracers, bool totPhi) {
  XFields x{};
  // do_fields_blocking_exchanges.F:54-97 (+ EXCH_UV_DGRID of uVelD/vVelD with the CD scheme,
  // totPhiHyd when the EOS reads it)
  // (on an EXCH2 topology u, v go through the vector map instead: exchange_uv)
  double *fl[] = {m->f.uVel, m->f.vVel, m->f.wVel, m->f.theta, m->f.salt, m->f.uVelD, m->f.vVelD, m->f.totPhiHyd};
  const bool use[] = {!m->uvMap, !m->uvMap, true, m->p.tempStepping != 0, m->p.saltStepping != 0, m->p.useCDscheme != 0,
                      m->p.useCDscheme != 0, m->p.storePhiHyd4Phys != 0 && totPhi};
  for (int q = 0; q < 8; q++) {
    const bool tr = q == 3 || q == 4;
    if (use[q] && (tracers == 1 || (tracers == 2) == tr)) { x.p[x.n] = fl[q]; x.nz[x.n] = m->d.Nr; x.n++; }
  }
  return x;
}

// One FORWARD_STEP with the fused end-of-step kernels: EXCH(cg2d_x)+etaN,
// correction+continuity, EXCH(eta)+UPDATE_ETAH, and every blocking exchange plus
// the counter bump in one launch.  Same arithmetic as the separate C-ABI ops.
//
// The pipelined step (MG_FUSE_PIPE, StepPlan::pipeOk): DO_OCEANIC_PHYS and GMREDI_CALC_TENSOR
// of a step read only the new theta and salt, totPhiHyd, the surface hFacC and EmPmR of the
// step before it -- nothing its pressure solve, correction step, CALC_R_STAR or velocity
// exchange produce -- so the step before runs them in two of its own grids, which are far from
// full (phys.h oceanic_phys_point_t<true>: in UPDATE_R_STAR's grid; the tensor in the
// correction step's), and the step itself starts at CALC_PHI_HYD: one launch fewer, and the
// fold's first grid without the tensor's blocks.  mgcm_forward_step runs the two stand-alone
// for the first step of a call (so a put between calls is honoured) and leaves the last step
// without the riders, so after a call every field holds what the plain steps leave.
//
// With MG_FUSE_PHIP (StepPlan::phiPipe) the next step's CALC_PHI_HYD and del2uv -- the first
// of DYNAMICS' grids, which from the step before needs only its last launch's halos of u, v and
// r* factors -- run in that last launch too (kernels_step.hip k_rstar_exch_phi), and the step
// starts at the momentum grid: six launches.  The head of a call then runs that grid stand-alone
// as well, after DO_OCEANIC_PHYS + tensor, from the halos as the caller left them.
enum StepMode {
  STEP_PLAIN = 0,   // the step runs its own DO_OCEANIC_PHYS + tensor
  STEP_HOIST = 1,   // its own are already done; it runs the next step's
  STEP_LAST = 2     // its own are already done; it runs nobody's (the last step of a call)
};
// a call of fewer steps keeps the plain step: the stand-alone head of a pipelined call costs
// two launches, each hoisting step saves one (profiles/r07/step_pipeline/threshold.md); with
// MG_FUSE_PHIP three launches, and every step saves two: the same threshold, a call of 3 gains
// less than three times what two processes differ by (profiles/r08/step_pipeline_phi/threshold.md)
#define MG_PIPE_MIN_STEPS 4

// The launch plan of one FORWARD_STEP: every layout decision of the step, made in plan_step
// from the model's parameters and the MGCM_STEP_FUSE mask and nowhere else.  one_step executes
// it; mgcm_forward_step, mgcm_prepare, ovl_trial and mgcm_step_phase read the same plan.
struct StepPlan {
  bool mom, rstar;   // momStepping; the non-linear free surface (r*)
  // staggerTimeStep (forward_step.F:1003-1036): THERMODYNAMICS after the pressure solve and
  // continuity, with the new velocities; DO_OCEANIC_PHYS still opens the step
  bool stagger;
  bool tracers;   // theta, salt or passive tracers are stepped
  // THERMODYNAMICS reads u, v, w, hFac and DO_OCEANIC_PHYS's outputs and writes only the
  // tracers' other buffers and AB histories; DYNAMICS reads none of those.  So once
  // DO_OCEANIC_PHYS is done the two run concurrently (second stream), joined before
  // UPDATE_R_STAR / SOLVE_FOR_PRESSURE (which rewrite hFac, then u, v, w).
  // canFork: the step has something to fork (ovl_trial: something to choose); forkable: and the
  // overlap is on (decided without the timing switch: one stream, so the eager timed pass runs
  // the layout the graph replays -- bench.py's per-kernel times and PMC attribution then
  // describe it); fork: the second stream is really used
  bool canFork, forkable, fork;
  // Under the linear free surface nothing between DYNAMICS and the correction step touches
  // what THERMODYNAMICS reads or writes (no r* rewrite of hFac; SOLVE_FOR_PRESSURE and CG2D
  // read gU, gV, hFac and eta, write the solver's vectors and etaN), so the tracers may run
  // beside the pressure solve too and join before MOMENTUM_CORRECTION_STEP rewrites u, v, w.
  // The fork comes after CALC_DIV_GHAT (beside the CG2D: the pressure solve leaves most CUs
  // idle while DYNAMICS and CALC_DIV_GHAT, alone, have the chip), under the linear free
  // surface only.  LLC-90 round 3 (profiles/r03/thermo_at/): 1.98 ms forked after
  // DO_OCEANIC_PHYS, 1.86 after DYNAMICS, 1.88 after CALC_DIV_GHAT; round 5, with the faster
  // solve, after CALC_DIV_GHAT wins: THERMODYNAMICS beside the CG2D only, CALC_DIV_GHAT (an HBM
  // stream, on the critical path) alone before it -- LLC-90 1.528-1.532 -> 1.474-1.476 ms/step,
  // alternating on one box (profiles/r05/thermo_at/); the tracers still finish inside the solve.
  // forkLate: where a fork of this model goes (the tile-sharded driver forks there too);
  // thermoLate: this step forks there; forkEarly: it forks right after DO_OCEANIC_PHYS and
  // joins before UPDATE_R_STAR; thermoInline: the tracers on the model's stream, after
  // DO_OCEANIC_PHYS (nothing forks, folds or staggers)
  bool forkLate, thermoLate, forkEarly, thermoInline;
  // With the late join (THERMODYNAMICS beside the pressure solve) the new tracers' halos are
  // filled on the tracers' stream right after them -- DO_FIELDS_BLOCKING_EXCHANGES' theta and
  // salt, which nothing before it reads -- so the end-of-step exchange carries only the
  // velocities (MG_FUSE_TREX)
  bool trEx;
  // the VI path's halo-ring AB2 (launch_mom_ring) on the tracers' stream with them, when they
  // fork right after DYNAMICS (MG_FUSE_RING; joined with them before the correction step).
  // ringLate: a late fork of this model takes the ring; ringAside: this step's does
  bool ringLate, ringAside;
  // Early fork on a small grid: THERMODYNAMICS' tracer kernels share DYNAMICS' launches
  // (kernels_step.hip, MG_FUSE_DT) instead of running on the second stream -- no fork, no join
  bool dtFused;
  // GMREDI_CALC_TENSOR beside CALC_PHI_HYD (launch_gm_phi) where THERMODYNAMICS, its reader,
  // runs after DYNAMICS (staggered, or forked after CALC_DIV_GHAT) and the fold does not apply
  bool gmPhi;
  // DO_OCEANIC_PHYS's launch runs GMREDI_CALC_TENSOR (not where launch_dyn_thermo's first grid
  // or launch_gm_phi takes it)
  bool physGm;
  // the VI path's halo-ring AB2 in DO_OCEANIC_PHYS's grid where it is not beside the solve
  // (k_phys_ring, MG_FUSE_RINGP: the staggered cube; the per-point form of the launch only,
  // phys_ring_ok); momRing: the momentum launch runs the ring itself
  bool ringPhys, momRing;
  // UPDATE_CG2D beside DYNAMICS (ucg2d.h, MG_FUSE_OPE): the operator from h0Fac*rStarFac in
  // the fold's first grid, the preconditioner in its second; UPDATE_R_STAR then rewrites hFac only
  // (round 4 measured the operator also in GMREDI_CALC_TENSOR + CALC_PHI_HYD's grid on the
  // staggered cube: slower, 0.4235-0.4257 against 0.4165-0.4234 ms/step, profiles/r04/ope_cs/;
  // removed in round 5)
  bool opEarly;
  // CALC_DIV_GHAT in the r* column pass (forward_step.F:829-877: UPDATE_R_STAR(.TRUE.) +
  // UPDATE_CG2D; MG_FUSE_SFP)
  bool sfpFused;
  // Under exactConserv the etaN of EXCH_XY_RL(cg2d_x) + etaN = recip_Bo*cg2d_x
  // (solve_for_pressure.F:309-330) is read only by MOMENTUM_CORRECTION_STEP's gradient before
  // INTEGR_CONTINUITY's EXCH(eta) + UPDATE_ETAH replaces it; k_corr_cont derives that eta from
  // cg2d_x at the exchange sources itself.
  // Under exactConserv nothing else reads that etaN either: INTEGR_CONTINUITY's EXCH(eta) +
  // UPDATE_ETAH overwrites it everywhere but at points neither interior nor mapped, where it
  // keeps recip_Bo*cg2d_x -- so with MG_FUSE_ETAX k_exch_eta is not launched at all: k_corr_cont
  // reads eta from cg2d_x as above and the UPDATE_ETAH pass forms those points' etaN itself
  // (fromX; cg2d_x's halo is left unexchanged: the next SOLVE_FOR_PRESSURE rewrites cg2d_x
  // everywhere before anything reads it)
  bool etaX;
  // forward_step.F:965-977: CALC_R_STAR(etaH(n+1)); the next step's RESET_NLFS_VARS +
  // UPDATE_R_STAR(.FALSE.) restore the hFac in place, so they are not repeated here.
  // Under r* the exactConserv EXCH(eta) + UPDATE_ETAH runs inside CALC_R_STAR's pass
  // (k_calc_r_star<FUSE>: fuseEtaH); etaHAlone: as a launch of its own (the linear free surface)
  bool fuseEtaH, etaHAlone;
  // CALC_R_STAR and the blocking exchanges in one grid on the small lat-lon grids
  // (k_rstar_exch; independent, and nothing between them in the non-staggered step; MG_FUSE_END)
  bool endFused;
  // CALC_R_STAR + the staggered exchanges in one launch (cube/LLC maps, the whole domain:
  // DO_STAGGER_FIELDS_EXCHANGES' u, v, w ride in CALC_R_STAR's grid, k_rstar_exmix, MG_FUSE_ENDS)
  bool stagEx;
  // The pipelined step.  pipeOk: the substitutions of the hoisted pass are exact (phys.h) and
  // its host grids run -- the fold with the tensor, the r* pass with the right-hand side and
  // CALC_R_STAR + the exchanges are the grids that carry the riders; phiPipeOk: and CALC_PHI_HYD
  // and del2uv of the next step ride in the step's last grid as well (phi_pipe_ok).
  // pipe / hoist: the mode asked for (StepMode); valid: it applies to this model; phiPipe: the
  // step's own CALC_PHI_HYD + del2uv are already done; phiNext: it runs the next step's;
  // empNext: the next step's DO_OCEANIC_PHYS left its EmPmR in EmPmRnext (rstar.h)
  bool pipeOk, phiPipeOk, pipe, hoist, valid, phiPipe, phiNext, empNext;
  // GMREDI_RESIDUAL_FLOW as a launch of its own (k_gm_residual_flow -> uRes, vRes, wRes): under
  // GM_AdvForm when a stepped tracer -- theta, salt or a passive one -- takes GAD_ADVECTION's
  // multi-dimensional passes (takes_res_flow; their TracerArgs then name those fields as the
  // flow to advect by).  It reads the step's whole
  // tensor (Psi at i+1, j+1) and u, v, w with the halos THERMODYNAMICS sees, so it opens
  // THERMODYNAMICS wherever that runs (tracers_on, on the tracers' stream: after the tensor's
  // grid, and on the staggered cube after DO_STAGGER_FIELDS_EXCHANGES); resFlowFold: where the
  // fold steps theta and salt (scheme 2) in DYNAMICS' grids, it opens PTRACERS_INTEGRATE instead.
  // Such a step keeps the plain plan (pipeOk): the pipelined step's hoisted tensor is checked
  // against the scheme-2 right-hand side, which reads Psi one point outside the interior at
  // most, and the residual flow reads it over the whole slab
  bool resFlow, resFlowFold;
  // the fold's second and third grid run the bodies compiled for the pinned option
  // set (common.h OptsGO90, MG_FUSE_SPEC): the model's options are that set and the fold's default
  // layout runs (dyn_thermo_spec_ok).  A choice of instantiation only: the same launches, the same bits
  bool spec;
  // ... and so do, in a pipelined call, the two grids on either side of the pressure solve: the
  // r* column pass with the next step's DO_OCEANIC_PHYS and the correction step with the next
  // step's tensor (MG_FUSE_SPEC2; the instantiations that exist are those of the hoisting step with
  // the operator built early and CALC_PHI_HYD pipelined as well)
  bool spec2;
};
static StepPlan plan_step(const mgcm_model *m, StepMode mode) {
  const Params &p = m->p;
  const Dims &d = m->d;
  const bool whole = d.nT == d.nTiles;   // every tile is this process's (not a tile-sharded run)
  StepPlan pl{};
  pl.mom = p.momStepping != 0;
  pl.rstar = p.nonlinFreeSurf > 0;
  pl.stagger = p.staggerTimeStep != 0 && pl.mom;
  pl.tracers = p.tempStepping || p.saltStepping || !m->ptr.empty();
  pl.canFork = !pl.stagger && pl.mom && pl.tracers;
  pl.forkable = pl.canFork && m->overlap;
  pl.fork = pl.forkable && !m->timing;
  pl.forkLate = !pl.rstar;
  pl.thermoLate = pl.fork && pl.forkLate;
  pl.trEx = pl.thermoLate && mg_fuse_on(MG_FUSE_TREX);
  const bool ringSep = mom_ring_separable(d, p);
  pl.ringLate = pl.forkLate && ringSep && mg_fuse_on(MG_FUSE_RING);
  pl.ringAside = pl.thermoLate && pl.ringLate;
  pl.resFlow = takes_res_flow(m);
  pl.dtFused = pl.forkable && pl.rstar && dyn_thermo_fusable(d, p, tracer_args(m, false), tracer_args(m, true));
  // (GMREDI_CALC_TENSOR in launch_dyn_thermo's first grid when it takes it)
  const bool gmFold = pl.dtFused && dyn_thermo_takes_gm(p);
  pl.spec = gmFold && dyn_thermo_spec_ok(p);
  pl.forkEarly = pl.fork && !pl.thermoLate && !pl.dtFused;
  pl.thermoInline = !pl.stagger && !pl.fork && !pl.dtFused;
  pl.gmPhi = (pl.stagger || pl.thermoLate) && !pl.dtFused && !m->timing && gm_phi_fusable(d, p);
  pl.physGm = !gmFold && !pl.gmPhi;
  pl.opEarly = gmFold && p.nonlinFreeSurf > 2 && whole && mg_fuse_on(MG_FUSE_OPE);
  pl.sfpFused = mg_fuse_on(MG_FUSE_SFP) && pl.rstar && whole;
  pl.etaX = p.exactConserv && mg_fuse_on(MG_FUSE_ETAX) && whole;
  pl.fuseEtaH = p.exactConserv && pl.rstar;
  pl.etaHAlone = p.exactConserv && !pl.fuseEtaH;
  pl.endFused = pl.mom && pl.rstar && !pl.stagger && !m->uvMap && whole && mg_hfuse(MG_FUSE_END, d.nx, d.ny, d.nT, d.Nr);
  pl.stagEx = pl.mom && pl.rstar && !pl.endFused && pl.stagger && pl.tracers && m->uvMap && whole &&
              mg_hfuse(MG_FUSE_ENDS, d.nx, d.ny, d.nT, d.Nr);
  // (JMD95P reads totPhiHyd's halo: exact at the exchange source only where it is exchanged)
  const bool totPhiHalo = p.eosType == 1 && p.selectP_inEOS_Zc == 2 && !p.storePhiHyd4Phys;
  pl.resFlowFold = pl.resFlow && pl.dtFused;
  pl.pipeOk = gmFold && pl.sfpFused && pl.endFused && mg_fuse_on(MG_FUSE_PIPE) && p.select_rStar > 0 &&
              p.useRealFreshWaterFlux && p.exactConserv && m->d_srcOf && !totPhiHalo && !pl.resFlow;
  pl.phiPipeOk = pl.pipeOk && phi_pipe_ok(d, p) && m->d_haloRec;
  pl.pipe = mode != STEP_PLAIN;
  pl.hoist = mode == STEP_HOIST;
  pl.valid = !pl.pipe || pl.pipeOk;
  pl.phiPipe = pl.pipe && pl.phiPipeOk;
  pl.phiNext = pl.hoist && pl.phiPipe;
  pl.empNext = pl.hoist && p.periodicExternalForcing;
  pl.spec2 = pl.spec && pl.phiPipe && pl.opEarly && pl.etaX && mg_fuse_on(MG_FUSE_SPEC2);
  // (a pipelined step's DO_OCEANIC_PHYS ran in the previous step's grids, or at the head of the call)
  pl.ringPhys = !pl.pipe && !pl.ringAside && ringSep && mg_fuse_on(MG_FUSE_RINGP) && phys_ring_ok(d, p, m->f);
  pl.momRing = !pl.ringAside && !pl.ringPhys;
  return pl;
}
// mgcm_get_param("stepLayout") (model.py step_layout): bit 0 THERMODYNAMICS folded into
// DYNAMICS' grids (k_dt_l1/l2/l3), 2 the tracers on the second stream, 3 joined only before the
// correction step, 4 pipelined, 5 with the next step's CALC_PHI_HYD too, 6 (value 64) the fold's
// bodies compiled for the pinned option set, 7 (value 128) the pipelined call's r* and
// correction-step grids too; bit 1 is retired
// (the graph's layout: the eager timed pass, one stream, serialises a fork it reports here)
static int step_layout_bits(const StepPlan &pl) {
  return (pl.dtFused ? 1 : 0) | (pl.forkable && !pl.dtFused ? 4 : 0) | (pl.forkable && pl.forkLate ? 8 : 0) |
         (pl.pipe ? 16 : 0) | (pl.phiPipe ? 32 : 0) | (pl.spec ? 64 : 0) | (pl.spec2 ? 128 : 0);
}

// THERMODYNAMICS onto the second stream (after the model stream's work so far), evJoin behind
// it; ring: the VI path's halo-ring AB2 ahead of it (StepPlan::ringAside), trEx: the new
// tracers' halo exchange behind it (StepPlan::trEx)
static int fork_thermo(mgcm_model *m, bool ring, bool trEx) {
  HIPCHK(hipEventRecord(m->evFork, m->stream));
  HIPCHK(hipStreamWaitEvent(m->stream2, m->evFork, 0));
  if (ring) HIPCHK(launch_mom_ring(m->d, m->p, m->f, m->d_ctr, m->stream2));
  if (tracers_on(m, m->stream2)) return -1;
  if (trEx) {
    const XFields xt = blocking_fields(m, 2);
    if (xt.n > 0) HIPCHK(launch_exchange_multi(m->d, xt, m->d_halo, m->nHalo, nullptr, m->stream2));
  }
  HIPCHK(hipEventRecord(m->evJoin, m->stream2));
  return 0;
}

// The executor of a StepPlan: launches, events and the CYCLE_TRACER swaps in FORWARD_STEP's order
static int one_step(mgcm_model *m, StepMode mode = STEP_PLAIN) {
  const StepPlan pl = plan_step(m, mode);
  if (!pl.valid) return set_err("one_step: the pipelined step does not apply to this model");
  const int fromX = pl.etaX ? 1 : 0;
  // the multi-workgroup CG2D keeps its CUs to itself while the tracers run beside it
  m->mwg.exclusive = pl.thermoLate ? 1 : 0;
  m->stepLayout = step_layout_bits(pl);
  m->gmResFlow = 0;
  if (!pl.pipe) TIMED(K_PHYS, launch_oceanic_phys(m->d, m->p, m->f, m->d_ctr, m->stream, pl.physGm, pl.ringPhys));
  if (pl.forkEarly && fork_thermo(m, false, false)) return -1;
  if (pl.thermoInline && tracers_on(m, m->stream)) return -1;
  if (pl.mom) {
    if (pl.dtFused) {
      TIMED(K_MOM, launch_dyn_thermo(m->d, m->p, m->f, tracer_args(m, false), tracer_args(m, true), m->d_ctr, m->stream,
                                     pl.opEarly ? m->d_srcOf : nullptr, !pl.pipe, !pl.phiPipe, pl.spec));
      std::swap(m->f.theta, m->f.thetaNext);   // CYCLE_TRACER: the new tracers are the other buffers
      std::swap(m->f.salt, m->f.saltNext);
      // PTRACERS_INTEGRATE where the fold replaced tracers_on: right behind it, before
      // UPDATE_R_STAR rewrites the hFac it reads
      if (pl.resFlowFold && res_flow_on(m, m->stream)) return -1;
      if (ptracers_on(m, m->stream)) return -1;
    } else if (pl.gmPhi) {
      TIMED(K_PHI, launch_gm_phi(m->d, m->p, m->f, m->stream));
      TIMED(K_MOM, launch_mom_step(m->d, m->p, m->f, m->d_ctr, m->stream, pl.momRing));
    } else if (dynamics_on(m, pl.momRing)) return -1;
    if (pl.forkEarly) HIPCHK(hipStreamWaitEvent(m->stream, m->evJoin, 0));
    if (pl.rstar)
      TIMED(K_RSTAR, update_r_star_cg2d(m, pl.sfpFused, pl.opEarly, false, pl.hoist ? m->d_ctr : nullptr, pl.phiNext,
                                        pl.spec2 && pl.hoist));
    if (!pl.sfpFused) TIMED(K_RHS, launch_sfp_rhs(m->d, m->p, m->f, m->stream));
    if (pl.thermoLate && fork_thermo(m, pl.ringAside, pl.trEx)) return -1;
    TIMED(K_CG2D, launch_cg2d(m, m->p.cg2dMaxIters, m->p.cg2dUseMinResSol - 1));
    if (!pl.etaX) TIMED(K_ETA, launch_exch_eta(m->d, m->p, m->f, m->d_srcOf, false, 0, m->stream));
    if (pl.thermoLate) HIPCHK(hipStreamWaitEvent(m->stream, m->evJoin, 0));
    TIMED(K_CONT, launch_corr_cont(m->d, m->p, m->f, 0, m->stream, pl.etaX ? m->d_srcOf : nullptr, pl.hoist,
                                   pl.spec2 && pl.hoist));
    if (pl.etaHAlone) TIMED(K_ETA, launch_exch_eta(m->d, m->p, m->f, m->d_srcOf, true, 0, m->stream, fromX));
    if (pl.endFused && pl.phiNext)
      TIMED(K_RSTAR, launch_rstar_exch_phi(m->d, m->p, m->f, m->d_haloRec, blocking_fields(m, 1, false), m->d_halo, m->nHalo,
                                           m->d_ctr, m->stream, fromX, pl.empNext ? 1 : 0));
    else if (pl.endFused)
      TIMED(K_RSTAR, launch_rstar_exch(m->d, m->p, m->f, m->d_srcOf, pl.fuseEtaH, blocking_fields(m), m->d_halo, m->nHalo,
                                       m->d_ctr, m->stream, fromX, pl.empNext ? 1 : 0));
    else if (pl.rstar)
      TIMED(K_RSTAR, calc_r_star(m, pl.fuseEtaH, fromX, pl.stagEx));
  } else {
    if (mgcm_integr_continuity(m)) return -1;
  }
  if (pl.stagger && pl.tracers) {
    // DO_STAGGER_FIELDS_EXCHANGES (do_stagger_fields_exchanges.F:37-43; in CALC_R_STAR's grid
    // with stagEx) + THERMODYNAMICS
    if (!pl.stagEx && mgcm_stagger_exchanges(m)) return -1;
    if (tracers_on(m, m->stream)) return -1;
  }
  if (pl.endFused) return 0;
  const XFields xEnd = blocking_fields(m, pl.trEx ? 0 : 1);
  if (m->uvMap) {   // the vector pair and the scalar fields in one launch
    HIPCHK(uv_pre(m, m->d, m->f.uVel, m->f.vVel, m->d.Nr, 1));
    TIMED(K_EXCH, launch_exchange_mixed(m->d, m->f.uVel, m->f.vVel, m->d.Nr, m->d_uv[1], m->nUvU[1], m->nUvV[1], xEnd,
                                        m->d_halo, m->nHalo, m->d_ctr, m->stream));
  } else
    TIMED(K_EXCH, launch_exchange_multi(m->d, xEnd, m->d_halo, m->nHalo, m->d_ctr, m->stream));
  return 0;
}

static void drop_graphs(mgcm_model *m) {
  for (auto &row : m->graphs)
    for (auto &col : row)
      for (auto &g : col)
        if (g.exec) { (void)hipGraphExecDestroy(g.exec); g = mgcm_model::StepGraph{}; }
}

// Which theta/salt ping-pong buffers are current (the kernels' arguments differ).
static int buffer_parity(const mgcm_model *m) {
  return (m->f.theta == m->thetaA ? 0 : 1) + (m->f.salt == m->saltA ? 0 : 2) + (m->ptrFlip ? 4 : 0);
}

// The step sequences replayed as hipGraphs, each captured once per THERMODYNAMICS overlap mode
// and tracer buffer parity (mgcm_model::graphs): no per-kernel host launch cost inside a batch.
// Two FORWARD_STEPs per graph inside a call (the tracer ping-pong swaps twice, so the pointers
// are back where they started); ONE for the odd step of a call and for a caller that steps one
// at a time -- the Fortran drop-ins, with host work between steps -- which still replays instead
// of launching (the ping-pong flips the parity, so consecutive single steps alternate between
// two of these graphs).
static const struct { int n; StepMode mode[2]; } STEP_SEQS[SEQ_N] = {
    {2, {STEP_PLAIN, STEP_PLAIN}},   // SEQ_PLAIN2
    {2, {STEP_HOIST, STEP_HOIST}},   // SEQ_HOIST2: inside a pipelined call
    {2, {STEP_HOIST, STEP_LAST}},    // SEQ_HOIST_LAST: its end
    {1, {STEP_PLAIN, STEP_PLAIN}},   // SEQ_PLAIN1
    {1, {STEP_LAST, STEP_LAST}},     // SEQ_LAST1: the odd last step of a pipelined call
};
static int step_graph(mgcm_model *m, StepSeq seq, mgcm_model::StepGraph **out = nullptr) {
  mgcm_model::StepGraph &sg = m->graphs[m->overlap ? 1 : 0][buffer_parity(m)][seq];
  if (!sg.exec) {
    double **tr[4] = {&m->f.theta, &m->f.thetaNext, &m->f.salt, &m->f.saltNext};
    double *pre[4];
    for (int k = 0; k < 4; k++) pre[k] = *tr[k];
    const int preFlip = m->ptrFlip;
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
    int rc = 0;
    for (int k = 0; k < STEP_SEQS[seq].n && !rc; k++) rc = one_step(m, STEP_SEQS[seq].mode[k]);
    hipError_t e = hipStreamEndCapture(m->stream, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return -1; }
    HIPCHK(e);
    e = hipGraphInstantiate(&sg.exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIPCHK(e);
    // the capture ran one_step's host side (CYCLE_TRACER's pointer swaps) without launching:
    // keep the pointers it leaves for every replay, and undo them until the replay
    for (int k = 0; k < 4; k++) { sg.tr[k] = *tr[k]; *tr[k] = pre[k]; }
    sg.flip = m->ptrFlip;
    m->ptrFlip = preFlip;
    sg.layout = m->stepLayout;
  }
  if (out) *out = &sg;
  return 0;
}
// replays the sequence (captured first where it is not yet) and leaves the host side as its
// steps would have: the tracer pointers, the passive tracers' parity, the layout it ran
static int step_graph_launch(mgcm_model *m, StepSeq seq) {
  mgcm_model::StepGraph *sg;
  if (step_graph(m, seq, &sg)) return -1;
  HIPCHK(hipGraphLaunch(sg->exec, m->stream));
  m->f.theta = sg->tr[0]; m->f.thetaNext = sg->tr[1]; m->f.salt = sg->tr[2]; m->f.saltNext = sg->tr[3];
  m->ptrFlip = sg->flip;
  m->stepLayout = sg->layout;
  return 0;
}
int mgcm_tracer_parity(mgcm_model *m, int set) {
  if (set < 0) return buffer_parity(m);
  const int top = m->ptr.empty() ? 3 : 7;   // bit 2: the passive tracers (all pairs swap together)
  if (set > top) return set_err("mgcm_tracer_parity: parity %d outside 0..%d", set, top);
  m->ptrFlip = (set & 4) ? 1 : 0;
  double *tB = m->f.theta == m->thetaA ? m->f.thetaNext : m->f.theta;
  double *sB = m->f.salt == m->saltA ? m->f.saltNext : m->f.salt;
  m->f.theta = (set & 1) ? tB : m->thetaA;
  m->f.thetaNext = (set & 1) ? m->thetaA : tB;
  m->f.salt = (set & 2) ? sB : m->saltA;
  m->f.saltNext = (set & 2) ? m->saltA : sB;
  return set;
}

static int ovl_trial(mgcm_model *m);

// Builds the graphs of the next batch and, when the THERMODYNAMICS overlap is still
// undecided, runs its trial now (on a copy of the state) so that no later timed batch
// contains the trial's 20 steps.
int mgcm_prepare(mgcm_model *m) {
  if (check_ready(m) || ptr_tables_sync(m)) return -1;
  if (!m->useGraph) return 0;
  HIPCHK(hipSetDevice(m->device));
  if (m->ovlAuto && !m->ovlDecided && ovl_trial(m)) return -1;
  if (plan_step(m, STEP_HOIST).valid && (step_graph(m, SEQ_HOIST2) || step_graph(m, SEQ_HOIST_LAST))) return -1;
  return step_graph(m, SEQ_PLAIN2);
}

// THERMODYNAMICS overlap auto-selection: the device state (both field arenas, the other
// fields, counters, solve records) is copied aside, 20 steps run through the two graphs --
// on, off (one two-step graph each: builds and warms them), then on, off, on, off of two
// graphs each, bracketed by events -- and the state is copied back, so the caller's steps
// are untouched; the faster graph is kept.  Both graphs compute identical results.
static int ovl_trial(mgcm_model *m) {
  if (!plan_step(m, STEP_PLAIN).canFork) { m->ovlDecided = true; return 0; }   // one_step never forks: nothing to choose
  std::vector<std::pair<void *, size_t>> parts = {
      {m->f.a2, (size_t)F2_COUNT * m->d.N2all * sizeof(double)},
      {m->f.a3, (size_t)F3_COUNT * m->d.N3all * sizeof(double)},
      {m->d_ctr, 2 * sizeof(int)},
      {m->d_rec, (size_t)m->maxRec * sizeof(SolveRecord)}};
  // (the passive tracers' arena too: the trial's steps must not leak into the caller's tracers)
  if (!m->ptr.empty()) parts.push_back({m->a4, m->ptr.size() * PTR_NF * (size_t)m->d.N3all * sizeof(double)});
  for (auto &fd : FIELDS)
    if (fd.kind != F2D && fd.kind != F3D && field_ptr(m, &fd))
      parts.push_back({field_ptr(m, &fd), (size_t)field_count(m, fd.kind) * sizeof(double)});
  size_t total = 0;
  for (auto &pr : parts) total += (pr.second + 255) & ~(size_t)255;
  char *save = nullptr;
  if (hipMalloc(&save, total) != hipSuccess) {   // no room for the copy: keep the overlap on, untimed
    (void)hipGetLastError();
    m->ovlDecided = true;
    return 0;
  }
  // one exit path: the copy is always restored and freed, the overlap mode always reset
  // when the trial fails
  const bool ovl0 = m->overlap;
  int rc = 0;
  size_t off = 0;
  for (auto &pr : parts) {
    if (!rc && hipMemcpyAsync(save + off, pr.first, pr.second, hipMemcpyDeviceToDevice, m->stream) != hipSuccess) rc = -1;
    off += (pr.second + 255) & ~(size_t)255;
  }
  for (int ph = 0; ph < 6 && !rc; ph++) {
    const int pairs = ph < 2 ? 1 : 2, mode = (ph & 1) ? 0 : 1;
    m->overlap = mode != 0;
    if (step_graph(m, SEQ_PLAIN2)) { rc = -1; break; }   // built before the events (same parity after a pair)
    if (hipEventRecord(m->ovlEv[0], m->stream) != hipSuccess) { rc = -1; break; }
    for (int r = 0; r < pairs && !rc; r++)
      if (step_graph_launch(m, SEQ_PLAIN2)) rc = -1;
    float ms = 0.f;
    if (rc || hipEventRecord(m->ovlEv[1], m->stream) != hipSuccess || hipEventSynchronize(m->ovlEv[1]) != hipSuccess ||
        hipEventElapsedTime(&ms, m->ovlEv[0], m->ovlEv[1]) != hipSuccess) { rc = -1; break; }
    if (ph >= 2) m->ovlMs[mode] += ms;
  }
  int rs = 0;
  off = 0;
  for (auto &pr : parts) {
    if (hipMemcpyAsync(pr.first, save + off, pr.second, hipMemcpyDeviceToDevice, m->stream) != hipSuccess) rs = -1;
    off += (pr.second + 255) & ~(size_t)255;
  }
  if (hipStreamSynchronize(m->stream) != hipSuccess) rs = -1;
  (void)hipFree(save);
  if (rc || rs) {
    m->overlap = ovl0;
    return set_err(rs ? "ovl_trial: restoring the saved state failed" : "ovl_trial: graph replay failed");
  }
  m->ovlDecided = true;
  m->overlap = m->ovlMs[1] <= m->ovlMs[0];
  return 0;
}

int mgcm_forward_step(mgcm_model *m, int nsteps) {
  if (check_ready(m) || ptr_tables_sync(m)) return -1;
  if (land_guard_check(m, "mgcm_forward_step")) return -1;
  if (nsteps <= 0 || nsteps > m->maxRec) return set_err("mgcm_forward_step: nsteps %d out of range", nsteps);
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipMemsetAsync(m->d_ctr + 1, 0, sizeof(int), m->stream));
  int s = 0;
  if (m->useGraph && !m->timing && m->ovlAuto && !m->ovlDecided && nsteps >= 2 && ovl_trial(m)) return -1;
  // the pipelined call (one_step's StepMode): DO_OCEANIC_PHYS + GMREDI_CALC_TENSOR of the first
  // step stand-alone, from the fields as the caller left them; every step but the last then
  // runs the next step's, and the last leaves every field as the plain step does
  const StepPlan hp = plan_step(m, STEP_HOIST);
  const bool pipe = nsteps >= MG_PIPE_MIN_STEPS && hp.valid;
  if (pipe) TIMED(K_PHYS, launch_oceanic_phys(m->d, m->p, m->f, m->d_ctr, m->stream));
  // ... and, where every step's CALC_PHI_HYD + del2uv run in the step before (MG_FUSE_PHIP), the
  // first step's: from the halos of u and v as the caller left them
  if (pipe && hp.phiPipe) TIMED(K_PHI, launch_phi_del2(m->d, m->p, m->f, m->stream));
  if (m->useGraph && !m->timing) {
    for (; s + 2 <= nsteps; s += 2)
      if (step_graph_launch(m, !pipe ? SEQ_PLAIN2 : s + 2 == nsteps ? SEQ_HOIST_LAST : SEQ_HOIST2)) return -1;
    // an odd step (a caller stepping one at a time): the one-step graph of this parity
    if (s < nsteps) {
      if (step_graph_launch(m, pipe ? SEQ_LAST1 : SEQ_PLAIN1)) return -1;
      s++;
    }
  }
  for (; s < nsteps; s++)
    if (one_step(m, pipe ? (s == nsteps - 1 ? STEP_LAST : STEP_HOIST) : STEP_PLAIN)) return -1;
  m->lastBatch = nsteps;
  return 0;
}

// ---- tile-sharded runs (mitgcm_amd/parallel.py drives the collectives) ----------
int mgcm_set_tile_range(mgcm_model *m, int t0, int nT) {
  if (t0 < 0 || nT < 1 || t0 + nT > m->d.nTiles)
    return set_err("mgcm_set_tile_range: tiles [%d, %d) outside [0, %d)", t0, t0 + nT, m->d.nTiles);
  if (!m->ptr.empty() && nT < m->d.nTiles)
    return set_err("mgcm_set_tile_range: passive tracers are not supported in tile-sharded runs (tile range [%d, %d) of %d)",
                   t0, t0 + nT, m->d.nTiles);
  if (m->solver == Cg2dSolver::MwgRef && nT < m->d.nTiles)
    return set_err("mgcm_set_tile_range: cg2dRefOrder in the multi-workgroup CG2D needs the whole domain's tiles, not the "
                   "tile range [%d, %d) of %d", t0, t0 + nT, m->d.nTiles);
  m->d.t0 = t0;
  m->d.nT = nT;
  drop_graphs(m);
  if (m->ready) {
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (upload_halo(m)) return -1;
  }
  return 0;
}

int mgcm_set_stream(mgcm_model *m, void *stream) {
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  drop_graphs(m);
  m->stream = stream ? (hipStream_t)stream : m->ownStream;
  return 0;
}

// The 3-D fields whose halo sources travel between processes: the blocking-exchange set
// with u and v always included (on an EXCH2 topology the vector map may read either
// component of a source point, exch2_uv_3d_rx.template).
// group 0: all of them; 1: the tracers (final once THERMODYNAMICS has run, so their
// exchange can travel while DYNAMICS and the solve compute); 2: the rest.
static XFields transfer_fields(const mgcm_model *m, int group = 0) {
  XFields x{};
  double *fl[] = {m->f.uVel, m->f.vVel, m->f.wVel, m->f.theta, m->f.salt, m->f.uVelD, m->f.vVelD, m->f.totPhiHyd};
  const bool use[] = {true, true, true, m->p.tempStepping != 0, m->p.saltStepping != 0, m->p.useCDscheme != 0,
                      m->p.useCDscheme != 0, m->p.storePhiHyd4Phys != 0};
  const bool tracer[] = {false, false, false, true, true, false, false, false};
  for (int q = 0; q < 8; q++)
    if (use[q] && (group == 0 || (group == 1) == tracer[q])) { x.p[x.n] = fl[q]; x.nz[x.n] = m->d.Nr; x.n++; }
  return x;
}

int mgcm_exchange_nfields(mgcm_model *m) { return transfer_fields(m).n; }
int mgcm_exchange_nfields_group(mgcm_model *m, int group) {
  if (group < 0 || group > 2) return -1;
  return transfer_fields(m, group).n;
}

int mgcm_halo_pack(mgcm_model *m, const long *idx, long n, double *buf, int unpack) {
  return mgcm_halo_pack_group(m, 0, idx, n, buf, unpack);
}

int mgcm_halo_pack_group(mgcm_model *m, int group, const long *idx, long n, double *buf, int unpack) {
  if (check_ready(m)) return -1;
  if (group < 0 || group > 2) return set_err("mgcm_halo_pack_group: no group %d", group);
  HIPCHK(launch_halo_pack(m->d, transfer_fields(m, group), idx, n, buf, unpack, m->stream));
  return 0;
}

// Cross-stream ordering for callers whose collectives run on another stream: direction 0
// makes `other` wait for the work issued on the model's stream so far (the model's outputs,
// e.g. a packed halo buffer or tile partials, are then safe to read there); 1 makes the
// model's stream wait for the work issued on `other` so far (e.g. a received buffer).
int mgcm_stream_handoff(mgcm_model *m, void *other, int direction) {
  hipStream_t o = (hipStream_t)other;
  if (o == m->stream) return 0;
  HIPCHK(hipSetDevice(m->device));
  if (direction == 0) {
    HIPCHK(hipEventRecord(m->evHand, m->stream));
    HIPCHK(hipStreamWaitEvent(o, m->evHand, 0));
  } else {
    HIPCHK(hipEventRecord(m->evHand, o));
    HIPCHK(hipStreamWaitEvent(m->stream, m->evHand, 0));
  }
  return 0;
}

int mgcm_tile_copy(mgcm_model *m, const char *name, int t0, int nT, void *buf, int toField) {
  const FieldDesc *fd = find_field(name);
  if (!fd || fd->kind == F1D) return set_err("mgcm_tile_copy: no 2-D/3-D field '%s'", name);
  if (t0 < 0 || nT < 0 || t0 + nT > m->d.nTiles) return set_err("mgcm_tile_copy: bad tile range");
  const long per = fd->kind == F2D ? m->d.n2 : m->d.n3;
  double *f = field_ptr(m, fd) + t0 * per;
  const size_t bytes = (size_t)nT * per * sizeof(double);
  HIPCHK(hipMemcpyAsync(toField ? f : buf, toField ? buf : f, bytes, hipMemcpyDeviceToDevice, m->stream));
  return 0;
}

static int mwg_block_uncached(mgcm_model *m);

// cg2dRefOrder in the multi-workgroup CG2D chains the parts of every tile inside ONE launch of
// the whole domain: no sub-launch of a tile range, no hand-off block shared between processes
// or models
static int mwg_ref_refuse(const mgcm_model *m, const char *who) {
  if (m->solver != Cg2dSolver::MwgRef) return 0;
  return set_err("%s: cg2dRefOrder in the multi-workgroup CG2D runs the whole domain in one launch of one model "
                 "(no tile ranges, no shared hand-off block)", who);
}

// Everyone sharing a hand-off block must tag with the same launch epoch: the epoch words
// (each process's / model's own, T.epoch) restart at 0 wherever a block is shared, and the
// block itself is zeroed by its owner then, so granules an earlier solve of one sharer left
// (tagged with that sharer's epochs) match no tag of the shared solves.  A hand-off that
// times out in a shared solve is fatal for the run (the epochs may then diverge: each sharer's
// first part reads the shared timeout word at its own time): ShardedModel.check_solves raises,
// the Fortran drop-ins die (fortran_abi.hip); re-sharing restarts both words.
static int mwg_restart_epoch(mgcm_model *m, bool zeroBlock) {
  if (zeroBlock) HIPCHK(hipMemset(m->mwg.ctr, 0, m->mwg.hsBytes));
  HIPCHK(hipMemset(m->mwg.epoch, 0, 64));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

// The tile-sharded device CG2D: every process launches the multi-workgroup solver's parts
// of its own tiles, all on ONE hand-off block (granules, epoch, timeout word), which the
// first process exports by IPC and the others map; every granule access is then at system
// scope.  The sums keep the single-launch order, so the solve is the 1-process solve.
int mgcm_cg2d_shared_export(mgcm_model *m, void *handle) {
  if (!m->useMwg() || m->mwg.partsPerTile <= 0)
    return set_err("mgcm_cg2d_shared_export: needs the multi-workgroup CG2D on whole-domain tables (cg2dForceMwg)");
  if (mwg_ref_refuse(m, "mgcm_cg2d_shared_export")) return -1;
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  // the importers' launches may run on other GPUs: an uncached block (mwg_block_uncached)
  if (mwg_block_uncached(m) || mwg_restart_epoch(m, true)) return -1;
  hipIpcMemHandle_t h;
  HIPCHK(hipIpcGetMemHandle(&h, (void *)m->mwg.ctr));
  memcpy(handle, &h, sizeof h);
  return 0;
}

int mgcm_cg2d_shared_import(mgcm_model *m, const void *handle) {
  if (!m->useMwg() || m->mwg.partsPerTile <= 0)
    return set_err("mgcm_cg2d_shared_import: needs the multi-workgroup CG2D on whole-domain tables (cg2dForceMwg)");
  if (mwg_ref_refuse(m, "mgcm_cg2d_shared_import")) return -1;
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  if (m->mwgShared) { (void)hipIpcCloseMemHandle(m->mwgShared); m->mwgShared = nullptr; }
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof h);
  void *p = nullptr;
  HIPCHK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
  m->mwgShared = p;
  const size_t partGr = (size_t)2 * 3 * m->mwg.G * 2;
  m->mwg.ctr = (unsigned *)p;
  m->mwg.part = (unsigned long long *)((char *)p + 64);
  m->mwg.xs = m->mwg.part + partGr;
  m->mwg.sys = 1;
  if (mwg_restart_epoch(m, false)) return -1;
  drop_graphs(m);
  return 0;
}

int mgcm_cg2d_shared_bytes(mgcm_model *m) { return m->useMwg() ? (int)sizeof(hipIpcMemHandle_t) : -1; }

// After a caller replays its own captured steps (ShardedModel.replay): the number of steps
// the batch recorded, so mgcm_solve_stats finds them.
int mgcm_end_steps(mgcm_model *m, int nsteps) {
  if (nsteps < 0 || nsteps > m->maxRec) return set_err("mgcm_end_steps: nsteps %d out of range", nsteps);
  m->lastBatch = nsteps;
  return 0;
}

int mgcm_begin_steps(mgcm_model *m) {
  if (check_ready(m)) return -1;
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipMemsetAsync(m->d_ctr + 1, 0, sizeof(int), m->stream));
  m->lastBatch = 0;
  return 0;
}

// FORWARD_STEP split at its exchange points (tile-sharded runs, mitgcm_amd/parallel.py
// drives the collectives in between):
//   1: DO_OCEANIC_PHYS, THERMODYNAMICS (staggerTimeStep = F), DYNAMICS, UPDATE_R_STAR +
//      UPDATE_CG2D (r*, every tile), the SOLVE_FOR_PRESSURE right-hand side;
//      [all-gather cg2d_b, cg2d_x]
//   2: CG2D on the whole domain (replicated), EXCH + etaN everywhere, correction +
//      continuity on this process's tiles;  [all-gather the new eta (exactConserv)]
//   3: EXCH eta + UPDATE_ETAH everywhere, CALC_R_STAR (r*, every tile);
//      [send/recv the 3-D halo sources]
//   5: staggerTimeStep only: DO_STAGGER_FIELDS_EXCHANGES on this process's tiles, then
//      THERMODYNAMICS with the new velocities;  [send/recv the 3-D halo sources again]
//   4: DO_FIELDS_BLOCKING_EXCHANGES of this process's tiles, step counters.
// the join of THERMODYNAMICS on the second stream (fork_thermo)
static int shard_join_thermo(mgcm_model *m) {
  if (m->shardFork == 1 || m->shardFork == 3) HIPCHK(hipStreamWaitEvent(m->stream, m->evJoin, 0));
  m->shardFork = 0;
  m->mwg.exclusive = 0;
  return 0;
}

int mgcm_step_phase(mgcm_model *m, int phase) {
  if (check_ready(m)) return -1;
  if (!m->p.momStepping) return set_err("mgcm_step_phase: requires momStepping");
  if (!m->ptr.empty()) return set_err("mgcm_step_phase: passive tracers are not supported by the tile-sharded driver");
  // (the resident step's plan: where it forks, the sharded step forks, whatever the overlap switch says)
  const StepPlan pl = plan_step(m, STEP_PLAIN);
  const bool stagger = pl.stagger;
  switch (phase) {
    case 16:  // DO_OCEANIC_PHYS, THERMODYNAMICS on the second stream as the resident step forks it
              // (one_step): beside DYNAMICS under r* (joined before UPDATE_R_STAR, which rewrites
              // hFac), beside the pressure solve under the linear free surface (forked after
              // DYNAMICS, joined before MOMENTUM_CORRECTION_STEP rewrites u, v, w)
      if (!pl.canFork || m->timing) {   // nothing to fork (the timed pass: one stream)
        phase = 8;
      } else {
        if (m->shardFork) return set_err("mgcm_step_phase(16): the previous step's THERMODYNAMICS not joined");
        TIMED(K_PHYS, launch_oceanic_phys(m->d, m->p, m->f, m->d_ctr, m->stream));
        if (!pl.forkLate) {
          if (fork_thermo(m, false, false)) return -1;
          m->shardFork = 1;
        } else {
          m->shardFork = 2;
        }
        return 0;
      }
      [[fallthrough]];
    case 1:   // = 8 then 9
    case 8:   // DO_OCEANIC_PHYS + THERMODYNAMICS (non-staggered): the tracers are final
      TIMED(K_PHYS, launch_oceanic_phys(m->d, m->p, m->f, m->d_ctr, m->stream));
      if (!stagger && tracers_on(m, m->stream)) return -1;
      if (phase == 8) return 0;
      [[fallthrough]];
    case 9: {   // DYNAMICS, UPDATE_R_STAR + UPDATE_CG2D, CALC_DIV_GHAT
      const bool ringAside = m->shardFork == 2 && pl.ringLate;
      if (dynamics_on(m, !ringAside)) return -1;
      if (m->shardFork == 1 && shard_join_thermo(m)) return -1;
      if (m->p.nonlinFreeSurf > 0) TIMED(K_RSTAR, update_r_star_cg2d(m));
      TIMED(K_RHS, launch_sfp_rhs(m->d, m->p, m->f, m->stream));
      if (m->shardFork == 2) {   // after CALC_DIV_GHAT, as one_step forks it
        if (fork_thermo(m, ringAside, false)) return -1;
        m->shardFork = 3;
        m->mwg.exclusive = 1;   // the multi-workgroup CG2D keeps its CUs while the tracers run
      }
      return 0;
    }
    case 2:
      TIMED(K_CG2D, launch_cg2d(m, m->p.cg2dMaxIters, m->p.cg2dUseMinResSol - 1));
      TIMED(K_ETA, launch_exch_eta(m->d, m->p, m->f, m->d_srcOf, false, 0, m->stream));
      if (shard_join_thermo(m)) return -1;
      TIMED(K_CONT, launch_corr_cont(m->d, m->p, m->f, 0, m->stream));
      return 0;
    case 10:  // the device CG2D over this process's parts (hand-off block shared by IPC)
      if (!m->useMwg() || m->mwg.partsPerTile <= 0)
        return set_err("mgcm_step_phase(10): needs the multi-workgroup CG2D on whole-domain tables (cg2dForceMwg)");
      if (m->d.nT < m->d.nTiles && mwg_ref_refuse(m, "mgcm_step_phase(10) on a tile subset")) return -1;
      if (m->d.nT < m->d.nTiles && !m->mwg.sys)
        return set_err("mgcm_step_phase(10): a tile subset needs the shared hand-off block (mgcm_cg2d_shared_*)");
      TIMED(K_CG2D, launch_cg2d_mwg(m->d, m->p, m->f, m->mwg, m->p.cg2dMaxIters, m->p.cg2dUseMinResSol - 1, m->d_rec, m->d_ctr + 1, m->stream,
                                    m->d.t0 * m->mwg.partsPerTile, m->d.nT * m->mwg.partsPerTile));
      return 0;
    case 6:   // phase 2 after a CG2D driven by the caller (mgcm_cg2d_op: distributed CG2D)
      TIMED(K_ETA, launch_exch_eta(m->d, m->p, m->f, m->d_srcOf, false, 0, m->stream));
      if (shard_join_thermo(m)) return -1;
      TIMED(K_CONT, launch_corr_cont(m->d, m->p, m->f, 0, m->stream));
      return 0;
    // phase 2 / 6 split at the THERMODYNAMICS join, so the caller can send the new tracers'
    // halo sources while the correction step runs: 19 the replicated CG2D alone, 17 EXCH(x) +
    // etaN and the join, 18 the correction + continuity pass
    case 19:
      TIMED(K_CG2D, launch_cg2d(m, m->p.cg2dMaxIters, m->p.cg2dUseMinResSol - 1));
      return 0;
    case 17:
      TIMED(K_ETA, launch_exch_eta(m->d, m->p, m->f, m->d_srcOf, false, 0, m->stream));
      return shard_join_thermo(m);
    case 18:
      TIMED(K_CONT, launch_corr_cont(m->d, m->p, m->f, 0, m->stream));
      return 0;
    case 3:
      if (shard_join_thermo(m)) return -1;
      if (m->p.exactConserv) TIMED(K_ETA, launch_exch_eta(m->d, m->p, m->f, m->d_srcOf, true, 0, m->stream));
      if (m->p.nonlinFreeSurf > 0) TIMED(K_RSTAR, calc_r_star(m));
      return 0;
    case 5:
      if (!stagger) return 0;
      TIMED(K_EXCH, exchange_uv(m, m->f.uVel, m->f.vVel, m->d.Nr, true) ? hipErrorUnknown : hipSuccess);
      TIMED(K_EXCH, launch_exchange(m->d, m->f.wVel, m->d_halo, m->nHalo, m->d.Nr, m->stream));
      return tracers_on(m, m->stream);
    case 4:
      if (m->uvMap) TIMED(K_EXCH, exchange_uv(m, m->f.uVel, m->f.vVel, m->d.Nr, true) ? hipErrorUnknown : hipSuccess);
      TIMED(K_EXCH, launch_exchange_multi(m->d, blocking_fields(m), m->d_halo, m->nHalo, m->d_ctr, m->stream));
      m->lastBatch++;
      return 0;
    // the routine-level split of a sharded step (one Fortran host stepping several models,
    // fortran_abi.hip: the reference's routine boundaries with the cross-model copies between)
    case 11:  // SOLVE_FOR_PRESSURE's right-hand side (CALC_DIV_GHAT) on this model's tiles
      TIMED(K_RHS, launch_sfp_rhs(m->d, m->p, m->f, m->stream));
      return 0;
    case 12:  // CG2D on the whole (gathered) domain + EXCH_XY_RL(cg2d_x) + etaN everywhere
      TIMED(K_CG2D, launch_cg2d(m, m->p.cg2dMaxIters, m->p.cg2dUseMinResSol - 1));
      [[fallthrough]];
    case 13:  // EXCH_XY_RL(cg2d_x) + etaN everywhere, after a CG2D done by phase 10 / mgcm_cg2d_tiles
      TIMED(K_ETA, launch_exch_eta(m->d, m->p, m->f, m->d_srcOf, false, 0, m->stream));
      return 0;
    case 14:  // INTEGR_CONTINUITY's column pass (after MOMENTUM_CORRECTION_STEP) on this model's tiles
      TIMED(K_CONT, launch_corr_cont(m->d, m->p, m->f, 2, m->stream));
      return 0;
    case 15:  // INTEGR_CONTINUITY's EXCH(eta) + UPDATE_ETAH everywhere (exactConserv; gathered eta)
      if (m->p.exactConserv) TIMED(K_ETA, launch_exch_eta(m->d, m->p, m->f, m->d_srcOf, true, 0, m->stream));
      return 0;
  }
  return set_err("mgcm_step_phase: no phase %d", phase);
}

// ---- the box's HBM reference rate (bench.py: SURVEY.md 8(d)'s roofline denominator) ---------
namespace mgcm {
__global__ void __launch_bounds__(256) k_triad(double2 *__restrict__ a, const double2 *__restrict__ b,
                                               const double2 *__restrict__ c, double s, long n2) {
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n2; q += (long)gridDim.x * 256) {
    const double2 x = b[q], y = c[q];
    a[q] = make_double2(x.x + s * y.x, x.y + s * y.y);
  }
}
}  // namespace mgcm
// STREAM triad a = b + s*c over three fp64 arrays of n doubles on `device`, 16 B per lane,
// best of `reps` (event-timed): GB/s at 24 bytes per element.
int mgcm_stream_triad(int device, long n, int reps, double *gbs) {
  if (n <= 0 || (n & 1) || reps <= 0 || !gbs) return set_err("mgcm_stream_triad: bad arguments");
  HIPCHK(hipSetDevice(device));
  double *a = nullptr, *b = nullptr, *c = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = 0;
  float best = 1e30f;
  if (hipMalloc(&a, n * sizeof(double)) != hipSuccess || hipMalloc(&b, n * sizeof(double)) != hipSuccess ||
      hipMalloc(&c, n * sizeof(double)) != hipSuccess || hipStreamCreate(&st) != hipSuccess ||
      hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess ||
      hipMemsetAsync(b, 0, n * sizeof(double), st) != hipSuccess || hipMemsetAsync(c, 0, n * sizeof(double), st) != hipSuccess)
    rc = set_err("mgcm_stream_triad: allocation");
  const unsigned grid = 256 * 16;   // 16 workgroups per CU, grid-stride
  for (int r = -1; rc == 0 && r < reps; r++) {   // r = -1: warm-up
    hipEventRecord(e0, st);
    hipLaunchKernelGGL(mgcm::k_triad, dim3(grid), dim3(256), 0, st, (double2 *)a, (const double2 *)b, (const double2 *)c, 3.0,
                       n / 2);
    hipEventRecord(e1, st);
    if (hipEventSynchronize(e1) != hipSuccess) { rc = set_err("mgcm_stream_triad: kernel"); break; }
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    if (r >= 0 && ms < best) best = ms;
  }
  if (rc == 0) *gbs = 24.0 * (double)n / (best * 1e-3) / 1e9;
  if (e0) hipEventDestroy(e0);
  if (e1) hipEventDestroy(e1);
  if (st) hipStreamDestroy(st);
  if (a) hipFree(a);
  if (b) hipFree(b);
  if (c) hipFree(c);
  return rc;
}

// ---- several models stepped by one host (fortran_abi.hip's tile-sharded drop-ins) ---------
void *mgcm_get_stream(mgcm_model *m) { return (void *)m->stream; }

// The interior points whose values the halos of tiles [t0, t0+nT) copy (the scalar EXCH map
// and, on EXCH2 topologies, both vector maps), outside those tiles: what another model that
// steps them must deliver before this one's local halo fill (the in-process HaloPlan).
long mgcm_halo_sources(mgcm_model *m, int t0, int nT, long *out, long cap) {
  if (t0 < 0 || nT < 1 || t0 + nT > m->d.nTiles) return set_err("mgcm_halo_sources: bad tile range");
  const long n2 = m->d.n2, N2 = n2 * m->d.nTiles, lo = (long)t0 * n2, hi = (long)(t0 + nT) * n2;
  std::vector<long> src;
  for (size_t h = 0; h + 1 < m->h_halo.size(); h += 2)
    if (m->h_halo[h] >= lo && m->h_halo[h] < hi) src.push_back(m->h_halo[h + 1]);
  if (m->uvMap)
    for (int w = 0; w < 2; w++)
      for (int c = 0; c < 2; c++)
        for (long q = lo; q < hi; q++) {
          const long code = m->h_uv[w][(size_t)c * N2 + q];
          if (code != 0) src.push_back(((code < 0 ? -code : code) - 1) % N2);
        }
  std::sort(src.begin(), src.end());
  src.erase(std::unique(src.begin(), src.end()), src.end());
  long n = 0;
  for (long v : src)
    if (v < lo || v >= hi) {
      if (out && n < cap) out[n] = v;
      n++;
    }
  return n;
}

// The device CG2D's parts of tiles [t0, t0+nT) on this model's stream and arrays (its
// cg2d_b, cg2d_x and operator must hold those tiles' values): a host stepping several models
// on one GPU launches one model's arrays for all of them (the gathered right-hand side), on
// several GPUs one launch per GPU on one shared hand-off block (mgcm_cg2d_share).
int mgcm_cg2d_tiles(mgcm_model *m, int t0, int nT) {
  if (check_ready(m)) return -1;
  if (!m->useMwg() || m->mwg.partsPerTile <= 0)
    return set_err("mgcm_cg2d_tiles: needs the multi-workgroup CG2D on whole-domain tables (cg2dForceMwg)");
  if (t0 < 0 || nT < 1 || t0 + nT > m->d.nTiles) return set_err("mgcm_cg2d_tiles: bad tile range");
  if (nT < m->d.nTiles && mwg_ref_refuse(m, "mgcm_cg2d_tiles on a tile subset")) return -1;
  if (nT < m->d.nTiles && !m->mwg.sys)
    return set_err("mgcm_cg2d_tiles: a tile subset needs the shared hand-off block (mgcm_cg2d_share)");
  HIPCHK(hipSetDevice(m->device));
  TIMED(K_CG2D, launch_cg2d_mwg(m->d, m->p, m->f, m->mwg, m->p.cg2dMaxIters, m->p.cg2dUseMinResSol - 1, m->d_rec, m->d_ctr + 1, m->stream,
                                t0 * m->mwg.partsPerTile, nT * m->mwg.partsPerTile));
  return 0;
}

// The hand-off block re-allocated as uncached (mem 1) or fine-grained (mem 2) device memory,
// its granules accessed at system scope (sys) or agent scope.
static int mwg_block_realloc(mgcm_model *m, int mem, bool sys) {
  const size_t partGr = (size_t)2 * 3 * m->mwg.G * 2;
  char *blk = nullptr;
  if (mem != 2 && hipExtMallocWithFlags((void **)&blk, m->mwg.hsBytes, hipDeviceMallocUncached) != hipSuccess) blk = nullptr;
  if (!blk) HIPCHK(hipExtMallocWithFlags((void **)&blk, m->mwg.hsBytes, hipDeviceMallocFinegrained));
  HIPCHK(hipMemset(blk, 0, m->mwg.hsBytes));
  HIPCHK(hipDeviceSynchronize());
  for (auto &q : m->mwgAllocs)
    if (q == m->mwgBlock) { (void)hipFree(q); q = blk; }
  m->mwgBlock = blk;
  m->mwg.ctr = (unsigned *)blk;
  m->mwg.part = (unsigned long long *)(blk + 64);
  m->mwg.xs = m->mwg.part + partGr;
  m->mwg.refc = m->mwg.ref ? m->mwg.xs + (size_t)m->mwg.nExp * 4 : nullptr;
  m->mwg.sys = sys ? 1 : 0;
  drop_graphs(m);
  return 0;
}

// A hand-off block that other launches poll from another GPU: uncached device memory, so no
// GPU's L2 holds a stale copy of a granule (coarse-grained hipMalloc memory is coherent only at
// kernel boundaries); every granule access is then at system scope (T.sys).
static int mwg_block_uncached(mgcm_model *m) {
  if (m->mwg.sys) return 0;
  return mwg_block_realloc(m, 1, true);
}

// In-process sharing of `owner`'s hand-off block by m (another model of the same host, on
// another GPU): the block becomes uncached device memory of the owner's GPU, m's launches map
// it by peer access, and both poll at system scope.  m == owner prepares the owner only.
int mgcm_cg2d_share(mgcm_model *m, mgcm_model *owner) {
  if (!m->useMwg() || !owner->useMwg() || m->mwg.partsPerTile <= 0 || m->mwg.G != owner->mwg.G)
    return set_err("mgcm_cg2d_share: both models need the same whole-domain multi-workgroup CG2D (cg2dForceMwg)");
  if (mwg_ref_refuse(m, "mgcm_cg2d_share") || mwg_ref_refuse(owner, "mgcm_cg2d_share")) return -1;
  HIPCHK(hipSetDevice(owner->device));
  HIPCHK(hipStreamSynchronize(owner->stream));
  if (mwg_block_uncached(owner)) return -1;
  if (m == owner) return mwg_restart_epoch(owner, true);
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  if (m->device != owner->device) {
    hipError_t e = hipDeviceEnablePeerAccess(owner->device, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return set_err("mgcm_cg2d_share: peer access %d -> %d: %s",
                                                                                  m->device, owner->device, hipGetErrorString(e));
    (void)hipGetLastError();
  }
  m->mwg.ctr = owner->mwg.ctr;
  m->mwg.part = owner->mwg.part;
  m->mwg.xs = owner->mwg.xs;
  m->mwg.sys = 1;
  if (mwg_restart_epoch(m, false)) return -1;
  drop_graphs(m);
  return 0;
}

// Distributed CG2D building blocks (kernels_cg2d_dist.hip): one op of cg2d.F over this
// process's tiles, per-tile partial sums into the device buffer part[2*nTiles].
int mgcm_cg2d_op(mgcm_model *m, int op, double a0, double *part) {
  if (check_ready(m)) return -1;
  if (op < 0 || op > 15) return set_err("mgcm_cg2d_op: no op %d", op);
  const bool sums = op == 0 || op == 2 || op == 3 || op == 5 || op == 6 || op == 10 || op == 13 || op == 14;
  if (!part && sums) return set_err("mgcm_cg2d_op: op %d needs the partials buffer", op);
  HIPCHK(launch_cgd(m->d, m->p, m->f, op, a0, part, m->stream));
  return 0;
}

int mgcm_cg2d_record(mgcm_model *m, double firstResidual, double lastResidual, double rhsMax, double sumRHS,
                     int numIters, double minResidualSq, int nIterMin) {
  if (check_ready(m)) return -1;
  HIPCHK(launch_cgd_record(m->d_rec, m->d_ctr + 1, firstResidual, lastResidual, rhsMax, sumRHS, numIters, minResidualSq,
                           nIterMin, m->stream));
  return 0;
}

int mgcm_field_pack(mgcm_model *m, const char *name, const long *idx, long n, double *buf, int unpack) {
  const FieldDesc *fd = find_field(name);
  if (!fd || fd->kind != F2D) return set_err("mgcm_field_pack: no 2-D field '%s'", name);
  HIPCHK(launch_field_pack(field_ptr(m, fd), idx, n, buf, unpack, m->stream));
  return 0;
}

int mgcm_exchange_field(mgcm_model *m, const char *name) {
  const FieldDesc *fd = find_field(name);
  if (!fd || fd->kind == F1D) return set_err("mgcm_exchange_field: no 2-D/3-D field '%s'", name);
  HIPCHK(launch_exchange(m->d, field_ptr(m, fd), m->d_halo, m->nHalo, fd->kind == F2D ? 1 : m->d.Nr, m->stream));
  return 0;
}

int mgcm_sync(mgcm_model *m) {
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  ev_collect(m);
  return land_guard_check(m, "mgcm_sync");
}

int mgcm_solve_stats(mgcm_model *m, int back, double *firstResidual, double *lastResidual, int *numIters,
                     double *rhsMax) {
  HIPCHK(hipStreamSynchronize(m->stream));
  int slot = m->lastBatch - 1 - back;
  if (m->lastBatch == 0) slot = 0;
  if (slot < 0) return set_err("mgcm_solve_stats: no such step");
  SolveRecord r;
  HIPCHK(hipMemcpy(&r, m->d_rec + slot, sizeof r, hipMemcpyDeviceToHost));
  if (firstResidual) *firstResidual = r.firstResidual;
  if (lastResidual) *lastResidual = r.lastResidual;
  if (numIters) *numIters = r.numIters;
  if (rhsMax) *rhsMax = r.rhsMax;
  return 0;
}

// The min-residual bookkeeping of a step's solve (cg2dUseMinResSol): the lowest squared
// residual reached and its iteration (cg2d.F minResidualSq, nIterMin; -1 / -1 when off).
int mgcm_solve_minres(mgcm_model *m, int back, double *minResidualSq, int *nIterMin) {
  HIPCHK(hipStreamSynchronize(m->stream));
  int slot = m->lastBatch - 1 - back;
  if (m->lastBatch == 0) slot = 0;
  if (slot < 0) return set_err("mgcm_solve_minres: no such step");
  SolveRecord r;
  HIPCHK(hipMemcpy(&r, m->d_rec + slot, sizeof r, hipMemcpyDeviceToHost));
  if (minResidualSq) *minResidualSq = r.minResidualSq;
  if (nIterMin) *nIterMin = r.nIterMin;
  return 0;
}

// The last n steps' solve records in one copy (oldest first): what a caller checks after a
// batch without a device-to-host transfer per step.
int mgcm_solve_history(mgcm_model *m, int n, int *numIters, double *firstResidual, double *lastResidual) {
  HIPCHK(hipStreamSynchronize(m->stream));
  if (n < 0 || n > m->lastBatch) return set_err("mgcm_solve_history: %d steps asked, %d in the last batch", n, m->lastBatch);
  if (n == 0) return 0;
  std::vector<SolveRecord> r((size_t)n);
  HIPCHK(hipMemcpy(r.data(), m->d_rec + (m->lastBatch - n), (size_t)n * sizeof(SolveRecord), hipMemcpyDeviceToHost));
  for (int q = 0; q < n; q++) {
    if (numIters) numIters[q] = r[q].numIters;
    if (firstResidual) firstResidual[q] = r[q].firstResidual;
    if (lastResidual) lastResidual[q] = r[q].lastResidual;
  }
  return 0;
}

// MONITOR's dynstat block (pkg/monitor/monitor.F:103-129, MON_CALC_STATS_RL) on the device:
// plane partials by k_mon_stats, added here in (tile, level) order; out[6][5] = (max, min,
// mean, sd, del2) of eta, uvel, vvel, wvel, theta, salt over this process's tiles.
int mgcm_monitor(mgcm_model *m, double *out) {
  if (check_ready(m)) return -1;
  HIPCHK(hipSetDevice(m->device));
  const Dims &d = m->d;
  const Fields &f = m->f;
  const int nzmax = d.Nr;
  const size_t nval = (size_t)MON_NF * d.nT * nzmax * MON_NV;
  if (m->monCap < nval) {
    if (m->monBuf) (void)hipFree(m->monBuf);
    m->monBuf = nullptr;
    HIPCHK(hipMalloc(&m->monBuf, nval * sizeof(double)));
    m->monCap = nval;
  }
  MonSpecs S{};
  S.s[0] = MonSpec{f.etaN, f.maskInC, f.maskInC, f.rA, f.drF, 1, 0, 0};
  S.s[1] = MonSpec{f.uVel, f.hFacW, f.maskInW, f.rAw, f.drF, d.Nr, 1, 1};
  S.s[2] = MonSpec{f.vVel, f.hFacS, f.maskInS, f.rAs, f.drF, d.Nr, 1, 1};
  S.s[3] = MonSpec{f.wVel, f.maskC, f.maskInC, f.rA, f.drC, d.Nr, 1, 1};
  S.s[4] = MonSpec{f.theta, f.hFacC, f.maskInC, f.rA, f.drF, d.Nr, 1, 1};
  S.s[5] = MonSpec{f.salt, f.hFacC, f.maskInC, f.rA, f.drF, d.Nr, 1, 1};
  std::vector<double> h(nval);
  double nb[MON_NF], d2[MON_NF], vol[MON_NF], sum[MON_NF], mn[MON_NF], mx[MON_NF], sd[MON_NF];
  for (int pass = 0; pass < 2; pass++) {
    HIPCHK(launch_mon_stats(d, S, nzmax, m->monBuf, pass, m->stream));
    HIPCHK(hipMemcpyAsync(h.data(), m->monBuf, nval * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    for (int fi = 0; fi < MON_NF; fi++) {
      double a[MON_NV] = {0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY};
      for (int t = 0; t < d.nT; t++)
        for (int k = 0; k < S.s[fi].nz; k++) {
          const double *v = &h[(((size_t)fi * d.nT + t) * nzmax + k) * MON_NV];
          for (int q = 0; q < 4; q++) a[q] = a[q] + v[q];
          a[4] = fmin(a[4], v[4]);
          a[5] = fmax(a[5], v[5]);
        }
      if (pass == 0) {
        nb[fi] = a[0]; d2[fi] = a[1]; vol[fi] = a[2]; sum[fi] = a[3]; mn[fi] = a[4]; mx[fi] = a[5];
        S.mean[fi] = vol[fi] > 0.0 ? sum[fi] / vol[fi] : 0.0;
      } else {
        sd[fi] = vol[fi] > 0.0 ? sqrt(a[3] / vol[fi]) : 0.0;
      }
    }
  }
  for (int fi = 0; fi < MON_NF; fi++) {
    const bool any = nb[fi] > 0.0;   // mon_calc_stats_rl.F: min = max = 0 with no wet point
    out[fi * 5 + 0] = any ? mx[fi] : 0.0;
    out[fi * 5 + 1] = any ? mn[fi] : 0.0;
    out[fi * 5 + 2] = S.mean[fi];
    out[fi * 5 + 3] = sd[fi];
    out[fi * 5 + 4] = any ? sqrt(d2[fi]) / nb[fi] : 0.0;
  }
  return 0;
}

void mgcm_kernel_timing(mgcm_model *m, int enable) {
  hipStreamSynchronize(m->stream);
  ev_collect(m);
  for (int k = 0; k < K_N; k++) { m->kms[k] = 0; m->kcnt[k] = 0; }
  m->timing = enable != 0;
}

double mgcm_kernel_ms(mgcm_model *m, const char *name, int *launches) {
  hipStreamSynchronize(m->stream);
  ev_collect(m);
  for (int k = 0; k < K_N; k++)
    if (!strcmp(KNAMES[k], name)) {
      if (launches) *launches = m->kcnt[k];
      return m->kcnt[k] ? m->kms[k] / m->kcnt[k] : 0.0;
    }
  if (launches) *launches = 0;
  return -1.0;
}

// The order in which the selected CG2D kernel forms its global sums (GLOBAL_SUM_TILE_RL's
// replacement), for the oracle to restate it: thread tid accumulates the per-point terms of
// plan[p*NT + tid] (2-D flat offsets; -1 = padding) for p = 0..PPT-1 in order, starting from
// 0.0; the NT thread partials are then combined by the pairwise tree the DPP row sums,
// row broadcasts and the cross-wave slot tree implement (block_sum_nw: lanes
// (2i, 2i+1), then pairs of pairs, ..., in thread order, zero-padded to a power of two).
int mgcm_cg2d_sum_plan(mgcm_model *m, int *plan, long capacity, int *NT, int *PPT, int *NG) {
  if (!m->ready) return set_err("mgcm_cg2d_sum_plan: model not initialised");
  int nt = 0, ppt = 0, ng = 1;
  std::vector<int> tab;
  switch (m->solver) {
    case Cg2dSolver::Mwg:
    case Cg2dSolver::MwgRef: {
      int rpt;
      cg2d_mwg_geometry(&nt, &ppt, &rpt);
      ng = m->mwg.G;
      tab = m->mwgPlan;
      break;
    }
    case Cg2dSolver::Bxy: {
      int BX, BY;
      if (cg2d_bxy_geometry(m->bxyVar, &BX, &BY, &nt)) return set_err("mgcm_cg2d_sum_plan: no k_cg2d_bxy tables");
      ppt = BX * BY;
      std::vector<int> blkx((size_t)ppt * nt);
      HIPCHK(hipMemcpy(blkx.data(), m->d_blkx, blkx.size() * sizeof(int), hipMemcpyDeviceToHost));
      tab.assign((size_t)ppt * nt, -1);
      for (int t = 0; t < m->nBlkX; t++)
        for (int q = 0; q < ppt; q++) tab[(size_t)q * nt + t] = blkx[(size_t)ppt * t + q];
      break;
    }
    case Cg2dSolver::BlockRef: {
      nt = 1024; ppt = cg2d_block_ppt(m->nPts);
      std::vector<int> gofs((size_t)ppt * nt);
      HIPCHK(hipMemcpy(gofs.data(), m->d_gofs, gofs.size() * sizeof(int), hipMemcpyDeviceToHost));
      tab.assign((size_t)ppt * nt, -1);
      for (int q = 0; q < ppt; q++)
        for (int t = 0; t < nt; t++)
          if (t + q * nt < m->nPts) tab[(size_t)q * nt + t] = gofs[(size_t)t + (size_t)q * nt];
      break;
    }
  }
  *NT = nt;
  *PPT = ppt;
  *NG = ng;
  if ((long)tab.size() > capacity) return set_err("mgcm_cg2d_sum_plan: capacity %ld < %zu", capacity, tab.size());
  memcpy(plan, tab.data(), tab.size() * sizeof(int));
  return 0;
}

int mgcm_cg2d(mgcm_model *m, double *cg2d_b, double *cg2d_x, double *firstResidual, double *minResidualSq,
              double *lastResidual, int *numIters, int *nIterMin) {
  if (check_ready(m)) return -1;
  const long n = m->d.n2 * m->d.nTiles;
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(mg_host_copy(m->f.cg2d_b, cg2d_b, n * sizeof(double), hipMemcpyHostToDevice, m->stream));
  HIPCHK(mg_host_copy(m->f.cg2d_x, cg2d_x, n * sizeof(double), hipMemcpyHostToDevice, m->stream));
  HIPCHK(hipMemsetAsync(m->d_ctr + 1, 0, sizeof(int), m->stream));
  // CG2D itself (cg2d.F): useSRCGSolver selects CG2D_SR only in SOLVE_FOR_PRESSURE
  const int sr = m->p.useSRCGSolver;
  m->p.useSRCGSolver = 0;
  const int ev = ev_begin(m, K_CG2D);
  const hipError_t le = launch_cg2d(m, *numIters, *nIterMin);
  ev_end(m, K_CG2D, ev);
  m->p.useSRCGSolver = sr;
  HIPCHK(le);
  SolveRecord r;
  if (!m->h_dropG.empty()) {
    // compacted tables: the record first, before the caller's arrays are overwritten.  A
    // solve the kernel's guard marked failed had a non-zero b or first guess on a point of a
    // left-out all-land block: the full tables from now on, and the same solve again
    HIPCHK(hipMemcpyAsync(&r, m->d_rec, sizeof r, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (r.numIters == -1) {
      if (land_uncompact(m)) return -1;
      return mgcm_cg2d(m, cg2d_b, cg2d_x, firstResidual, minResidualSq, lastResidual, numIters, nIterMin);
    }
  }
  HIPCHK(mg_host_copy(cg2d_b, m->f.cg2d_b, n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(mg_host_copy(cg2d_x, m->f.cg2d_x, n * sizeof(double), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipMemcpyAsync(&r, m->d_rec, sizeof r, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  *firstResidual = r.firstResidual;
  *minResidualSq = r.minResidualSq;
  *lastResidual = r.lastResidual;
  *numIters = r.numIters;
  *nIterMin = r.nIterMin;
  return 0;
}

}  // extern "C"
