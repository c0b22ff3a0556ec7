// myriad_hip.hip -- C-ABI (include/myriad_hip.h) over the gfx950 kernels.  No CPU fallback exists:
// every entry point either runs the HIP kernels or fails with an error code.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <thread>
#include <atomic>
#include <chrono>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/myriad_hip.h"
#include "dbg_regfill.h"
#include "hs_eval.h"
#include "colloc_products.h"
#include "hs_solver.h"
#include "hs_solver_wave.h"
#include "hs_solver_fused.h"
#include "shoot_solver_wave.h"
#include "os_solver.h"
#include "shoot_eval.h"
#include "rollout.h"
#include "fit.h"
#include "fit_gn.h"
#include "exgd_grad.h"
#include "exgd_jac.h"
#include "node_exgd_grad.h"
#include "colloc_hvp.h"
#include "shoot_hvp.h"
#include "shoot_exgd_grad.h"
#include "node_shoot_products.h"
#include "node_shoot_exgd_grad.h"
#include "node_hvp.h"
#include "fbsm.h"
#include "systems_gen.h"
#include "node_system.h"
#include "host_stage.h"

// closed-form systems (tools/gen_systems.py): X(NAME) expands once per system; the enum values are MYR_SYS_<NAME>
#define MYR_CLOSED_FORM_SYSTEMS(X)                                                                               \
  X(CARTPOLE) X(VANDERPOL) X(CANCERTREATMENT) X(SIMPLECASE) X(BIOREACTOR) X(GLUCOSE) X(MOULDFUNGICIDE)           \
  X(SIMPLECASEWITHBOUNDS) X(HIVTREATMENT) X(EPIDEMICSEIRN) X(SEIR) X(BEARPOPULATIONS) X(PENDULUM) X(MOUNTAINCAR)     \
  X(ROCKETLANDING) X(BACTERIA) X(TUMOUR) X(HARVEST) X(TIMBERHARVEST) X(PREDATORPREY)                               \
  X(PENDULUM_ELASTIC) X(ROCKETLANDING_ELASTIC) X(CARTPOLE_ELASTIC) X(VANDERPOL_ELASTIC) X(MOUNTAINCAR_ELASTIC)


using namespace myriad;

// Translation units (see __graft_entry__.build): the library is either this one file compiled as is, or -- to build in
// parallel -- one object with -DMYR_TU_MAIN (C-ABI + dispatch, no per-system kernels) plus one object per system with
// -DMYR_TU_SYSTEM=<Sys...> (explicit instantiation of that system's entry points, nothing else exported).
#if defined(MYR_TU_SYSTEM)
extern thread_local std::string g_err;
#else
thread_local std::string g_err;
#endif
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(MYR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));            \
  } while (0)

// The one switch over the systems: f(SysTag<Sys>{}) for a closed-form system, for the network system where `node` says so; unknown() for every other id
// (each caller has its own answer).  A caller names the type as SYS_OF(tag).
template <class S> struct SysTag { using type = S; };
#define SYS_OF(tag) typename decltype(tag)::type
template <class F, class U>
static auto for_system(int id, bool node, F&& f, U&& unknown) -> decltype(unknown()) {
  switch (id) {
#define X(N) case MYR_SYS_##N: return f(SysTag<Sys##N>{});
    MYR_CLOSED_FORM_SYSTEMS(X)
#undef X
    case MYR_SYS_NODE_CARTPOLE: if (node) return f(SysTag<SysNODE_CARTPOLE>{}); break;
  }
  return unknown();
}

struct SysInfo { int ns, nu, np; bool cost_dep_x; };
static bool sys_info(int id, SysInfo* s) {
  if (id == MYR_SYS_INVASIVEPLANT) { *s = {DiscINVASIVEPLANT::NS, DiscINVASIVEPLANT::NU, DiscINVASIVEPLANT::NP, false}; return true; }   // myr_fbsm only
  return for_system(id, true, [&](auto t) { using S = SYS_OF(t); *s = {S::NS, S::NU, S::NP, S::COST_DEP_X}; return true; }, [] { return false; });
}

struct KTimer {
  hipEvent_t a = nullptr, b = nullptr;
  double sum_ms = 0.0;
  int launches = 0;
};

struct myr_handle_s {
  myr_problem_desc d;
  myr_dims dims;
  SysInfo si;
  hipStream_t stream = nullptr;
  KTimer kt[MYR_K_COUNT];
  // staging for MYR_MEM_HOST calls
  void* dbuf = nullptr;
  size_t dbuf_bytes = 0;
  int eval_wpt = 8;
  int eval_nt = 1;      // non-temporal stores for the c / J-block streams
  int solve_mode = 1;   // 1: one trajectory per wavefront (hs_solver_fused.h / hs_solver_wave.h); 0: one trajectory per lane (hs_solver.h)
  int solve_fused = 1;  // 1: the fused-phase wavefront kernel where it is built (MYRIAD_SOLVE_MODE=wave1 selects round 2's HsWave)
  int solve_lpw = 16;   // trajectories (active lanes) per wavefront in the solve kernel
  // solver scratch (batch-minor / SoA)
  void* sbuf = nullptr;
  size_t sbuf_bytes = 0;
  int* ticket = nullptr;      // work counter of the persistent solve kernel (one int)
  int solve_slots = 0;        // MYRIAD_SOLVE_SLOTS: resident wavefronts of the solve kernel (0 = what the device holds)
  std::map<std::tuple<const void*, int, size_t>, int> occ;   // kernel_slots(): workgroups per CU of (kernel, block size, dynamic LDS)
  size_t eval_attr_lds[6] = {0, 0, 0, 0, 0, 0};   // dynamic-LDS attribute already set for the eval kernel variants (W = 1 / 4 / 8, nt)
  int fused_waves = 0;        // MYRIAD_FUSED_WAVES: wavefronts per trajectory (0 = by batch size)
  // two-phase launch of the one-wavefront fused kernel (hs_solver_fused.h: ParkArgs): records of the parked trajectories, resume order
  void* park_state = nullptr; size_t park_bytes = 0;
  int* park_perm = nullptr; size_t park_n = 0;      // [park_n] resume order, then PARK_BUCKETS + 2 counters: buckets, parked in all, `reached`
  int park_iter = -1;         // MYRIAD_PARK_ITER: iterations of phase 1 (-1 = by batch size, 0 = whole solves only)
  int park_fill = 1;          // MYRIAD_PARK_FILL: 0 = every trajectory parks at k1 (phase 1 without the fill, hs_solver_fused.h: ParkArgs)
  int park_shift = 3;         // MYRIAD_PARK_SHIFT: resume buckets per iteration a trajectory was parked after k1 (hs_solver_fused.h: park_bucket_late)
  // restoration inside myr_solve (myr_solve_opts.restoration): the twin handle, device scratch, and the account of the last call
  myr_handle_s* twin = nullptr;
  bool twin_unavailable = false;
  void* rbuf = nullptr; size_t rbuf_bytes = 0;      // copy of the caller's guess + status / iters when the caller passed none
  void* fbuf = nullptr; size_t fbuf_bytes = 0;      // working set of the failed instances
  int32_t* nfail_host = nullptr;                    // pinned: instances the first attempt left without a KKT point (copied from nfail_dev)
  int32_t* nfail_dev = nullptr;                     // the device word the count kernel adds to (device-scope atomics on device memory: no PCIe atomics needed)
  std::vector<int32_t> info_start, info_attempts, info_restored;
  int last_solve_form = 1;         // kernel form of the last solve launch on this handle: 1 = a wavefront kernel, 0 = the lane kernel
  unsigned long long poison = 0;   // MYRIAD_POISON: bit pattern written over a slot's LDS and scratch at every trajectory hand-over (tests)
  int cus = 0;                // compute units of the device (cached)
  // variable scaling of the solve path (myr_set_var_scale): the solver kernels see z/s, lb/s, ub/s
  VarScale vscale{{1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}};
  bool vscale_on = false;
  void* vbuf = nullptr;       // scaled copies of lb, ub
  size_t vbuf_bytes = 0;
  // helper workgroups of the network kernel (hs_solver_fused.h: NodeBoard): boards | abort word | published vectors
  void* coop_buf = nullptr; size_t coop_bytes = 0;
  int node_exgd_wpi = 4;      // MYRIAD_NODE_EXGD_WPI: wavefronts per instance of node_exgd_grad_kernel (1, 2 or 4: 8 spills; profiles/r18_node_exgd_grad)
  int node_helpers = -1;      // MYRIAD_NODE_HELPERS: helper workgroups per trajectory (-1 = by batch size)
  int32_t plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // myr_solve_plan: how the last first-attempt solve was launched
  bool plan_frozen = false;                     //   (second starts re-launch on this handle: they leave the first attempt's record alone)
  int reg_fill = 0;                    // MYRIAD_REG_FILL (tests): pattern left in every VGPR / AGPR of every SIMD before every solver launch (1 nan, 2 finite, 3 big, 4 zero)
  unsigned long long stack_fill = 0;   // MYRIAD_STACK_FILL (tests / experiments): bit pattern left in the queue's private-segment memory before every solver launch
  int prod_lane = 0;                   // MYRIAD_PROD_MODE=lane (developer switch): the products of a NODE system under SHOOTING by the per-lane kernels (cross-check, timing baseline)
};

static int device_cus(myr_handle h) {
  if (h->cus <= 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) h->cus = cus;
    else h->cus = 256;
  }
  return h->cus;
}

// MYRIAD_STACK_FILL: what a kernel's spill slots and stack objects inherit.  The private segment ("scratch") of a queue is not cleared between
// launches: a kernel that reads a stack slot before writing it gets what the previous kernel ON THIS QUEUE left there -- the same leftovers call after
// call on one handle, something else on a fresh handle (new stream, new queue, new backing memory).  This kernel overwrites 4 KB of private memory per
// lane of every resident wavefront slot with one pattern (MYRIAD_POISON does the same for the LDS and the solver's global scratch slots).
template <int WORDS>
static __global__ __launch_bounds__(64) void stack_fill_kernel(unsigned long long pat, int salt, unsigned long long* sink) {
  volatile unsigned long long a[WORDS];
  for (int i = 0; i < WORDS; ++i) a[i] = pat == 2 ? (0x3ff0000000000000ULL + ((unsigned long long)(i * 2654435761u + threadIdx.x * 40503u + salt) << 20)) : pat;
  unsigned long long acc = 0;
  for (int i = threadIdx.x & 7; i < WORDS; i += 61) acc ^= a[i];
  if (acc == 0x1234567ULL) sink[0] = acc;
}
// ... and the form for locating ONE slot: exactly `BYTES` of private memory per lane (the solver kernel's own private-segment size, so that the wave
// slots of the two kernels coincide), every dword the NaN pattern except dwords [z0, z1), which are zero
template <int DWORDS>
static __global__ __launch_bounds__(64) void stack_fill_window_kernel(int z0, int z1, unsigned* sink) {
  volatile unsigned a[DWORDS];
  for (int i = 0; i < DWORDS; ++i) a[i] = (i >= z0 && i < z1) ? 0u : ((i & 1) ? 0x7ff40000u : 0x00000001u);
  unsigned acc = 0;
  for (int i = threadIdx.x & 7; i < DWORDS; i += 61) acc ^= a[i];
  if (acc == 0x1234567u) sink[0] = acc;
}
static int stack_fill(myr_handle h) {
  if (const char* w = getenv("MYRIAD_STACK_FILL_WINDOW")) {      // "bytes:z0:z1"
    int bytes = 0, z0 = 0, z1 = 0;
    if (sscanf(w, "%d:%d:%d", &bytes, &z0, &z1) == 3) {
      if (!h->ticket) HIPCHK(hipMalloc(&h->ticket, sizeof(int)));
      for (int rep = 0; rep < 3; ++rep) {
        if (bytes == 528) hipLaunchKernelGGL((stack_fill_window_kernel<132>), dim3((unsigned)(device_cus(h) * 16)), dim3(64), 0, h->stream, z0, z1, (unsigned*)h->ticket);
        else hipLaunchKernelGGL((stack_fill_window_kernel<512>), dim3((unsigned)(device_cus(h) * 16)), dim3(64), 0, h->stream, z0, z1, (unsigned*)h->ticket);
      }
      HIPCHK(hipGetLastError());
      return MYR_OK;
    }
  }
  if (h->reg_fill) {      // MYRIAD_REG_FILL: what the registers inherit (dbg_regfill.h)
    const unsigned rp = h->reg_fill == 1 ? 0x7ff40000u : (h->reg_fill == 3 ? 0x4415af1du : (h->reg_fill == 4 ? 0u : 0x3ff12345u));
    for (int rep = 0; rep < 3; ++rep) hipLaunchKernelGGL(myriad::reg_fill_kernel, dim3((unsigned)(device_cus(h) * 16)), dim3(64), 0, h->stream, rp);
    HIPCHK(hipGetLastError());
  }
  if (!h->stack_fill) return MYR_OK;
  if (!h->ticket) HIPCHK(hipMalloc(&h->ticket, sizeof(int)));
  const unsigned long long pat = h->stack_fill == 1 ? 0x7ff4000000000000ULL /* signalling NaN */ : (h->stack_fill == 3 ? 0x4415af1d78b58c40ULL /* 1e20 */ : (h->stack_fill == 4 ? 0ULL : 2ULL));
  for (int rep = 0; rep < 3; ++rep)
    hipLaunchKernelGGL((stack_fill_kernel<512>), dim3((unsigned)(device_cus(h) * 16)), dim3(64), 0, h->stream, pat, rep, (unsigned long long*)h->ticket);
  HIPCHK(hipGetLastError());
  return MYR_OK;
}

// Workgroups of `kern` a CU keeps resident at this block size and dynamic-LDS size; sets the kernel's dynamic-LDS limit on the
// way.  Asked of the runtime once per handle and configuration, not on every solve call.
static int kernel_blocks_per_cu(myr_handle h, const void* kern, int threads, size_t lds, int* out) {
  auto key = std::make_tuple(kern, threads, lds);
  auto it = h->occ.find(key);
  if (it == h->occ.end()) {
    int per_cu = 0;
    // (the limit is a property of the FUNCTION, shared by every handle of the process: raise it to the hardware's 160 KB once
    // instead of to this handle's size, which a handle with a shorter horizon would lower again)
    HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds));
    it = h->occ.emplace(key, per_cu).first;
  }
  *out = it->second;
  return MYR_OK;
}

// every growing device buffer of a handle (sbuf, vbuf, dbuf, rbuf, fbuf, coop_buf): at least `need` bytes, contents not kept
static int ensure_buf(void** buf, size_t* have, size_t need) {
  if (need <= *have) return MYR_OK;
  if (*buf) HIPCHK(hipFree(*buf));
  *buf = nullptr; *have = 0;
  HIPCHK(hipMalloc(buf, need));
  *have = need;
  return MYR_OK;
}

// Stage (host_stage.h) on the HIP runtime: the arrays of one call in one of the handle's growing buffers, copies on the handle's stream
struct HipStage {
  myr_handle h; void** buf; size_t* have;
  int grow(size_t need, void** base) { const int rc = ensure_buf(buf, have, need); *base = *buf; return rc; }
  int upload(void* dev, const void* host, size_t bytes) { HIPCHK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, h->stream)); return MYR_OK; }
  int download(void* host, const void* dev, size_t bytes) { HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream)); return MYR_OK; }
  int sync() { HIPCHK(hipStreamSynchronize(h->stream)); return MYR_OK; }
};
using DevStage = Stage<HipStage>;
// the arrays of a C-ABI call of memory kind `mem`, in dbuf
static DevStage call_stage(myr_handle h, int mem) { return DevStage(HipStage{h, &h->dbuf, &h->dbuf_bytes}, mem == MYR_MEM_HOST); }
// device scratch of a launcher in `buf`: scratch items only
static DevStage scratch_stage(myr_handle h, void** buf, size_t* have) { return DevStage(HipStage{h, buf, have}, false); }

// grid of an elementwise kernel with a grid-stride loop, 256 threads per workgroup: one thread per element up to 64 workgroups per CU
static unsigned grid_for(long total) { long b = (total + 255) / 256; if (b > 16384) b = 16384; if (b < 1) b = 1; return (unsigned)b; }
// leading dimension of a batch-minor array: whole wavefronts of 64 lanes, an ODD number of them, so that consecutive elements of a trajectory
// (stride Bp * 8 bytes) rotate over the HBM channels / L2 sets instead of camping on one (a power-of-two stride would)
static long padded_lanes(int B) {
  long Bp = ((long)B + 63) / 64 * 64;
  if (((Bp / 64) & 1) == 0) Bp += 64;
  return Bp;
}

// ---- the steps the launchers share -----------------------------------------------------------------------------------------
// A timed launch on KTimer slot `k` (MYR_K_*): timed_begin -- the test fills, then the start event -- directly in front of the kernels,
// timed_end behind them.  A launcher that has work between the stop event and the account calls the parts of timed_end itself.
static int timed_begin(myr_handle h, int k) {
  KTimer& kt = h->kt[k];
  if (int rc_fill = stack_fill(h)) return rc_fill;
  HIPCHK(hipEventRecord(kt.a, h->stream));
  return MYR_OK;
}
static int timed_stop(myr_handle h, int k) {
  KTimer& kt = h->kt[k];
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(kt.b, h->stream));
  return MYR_OK;
}
static int timed_account(myr_handle h, int k) {      // (the stream has been synchronised)
  KTimer& kt = h->kt[k];
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, kt.a, kt.b));
  kt.sum_ms += ms;
  kt.launches += 1;
  return MYR_OK;
}
static int timed_end(myr_handle h, int k) {
  if (int rc = timed_stop(h, k)) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return timed_account(h, k);
}

// Persistent solver kernels: resident workgroups pull trajectories from a ticket counter, scratch belongs to the slot.
// Slot stride in doubles: whole 256-byte lines, an ODD number of them, so that the slots rotate over the HBM channels
static long slot_stride(long doubles) {
  long stride = (doubles + 31) / 32 * 32;
  if (((stride / 32) & 1) == 0) stride += 32;
  return stride;
}
// the ticket: allocated once per handle, cleared on the stream in front of every launch
static int reset_ticket(myr_handle h) {
  if (!h->ticket) HIPCHK(hipMalloc(&h->ticket, sizeof(int)));
  HIPCHK(hipMemsetAsync(h->ticket, 0, sizeof(int), h->stream));
  return MYR_OK;
}
// slots of a launch before the cap at the batch size: MYRIAD_SOLVE_SLOTS, else what the device keeps resident -- per_cu workgroups on every CU
// by the occupancy query (`guess` where that gave none), `per_group` slots in each
static int default_slots(myr_handle h, int per_cu, int guess, int per_group = 1) {
  return h->solve_slots > 0 ? h->solve_slots : (per_cu > 0 ? per_cu : guess) * device_cus(h) * per_group;
}
// myr_solve_plan's record of this launch: {form, wavefronts per trajectory, k1, phases, slots, helpers}
static void set_plan(myr_handle h, int form, int waves, int k1, int phases, int slots, int helpers) {
  const int32_t pl[8] = {form, waves, k1, phases, slots, helpers, 0, 0};
  if (!h->plan_frozen) memcpy(h->plan, pl, sizeof(pl));      // (second starts re-launch on this handle: they leave the first attempt's record alone)
}

// ---- one record per entry point: the batch in device memory, as the launchers see it ------------------------------------------
struct EvalArgs { int B; const double *z, *params; int pstride; double *f, *g, *c, *j; };      // each output may be null
enum { PRODOP_VJP = 0, PRODOP_JVP = 1, PRODOP_EXGD = 2 };
struct ProdArgs {
  int op, B;
  const double *z, *w, *params; int pstride;     // w: lam (vjp) or v (jvp)
  double* out; int add_gradf;
  double *zio, *lamio; const double *lb, *ub; double eta_x, eta_v; int nsteps;   // exgd
};
struct SolveCall {
  int B; double* z; const double *lb, *ub, *params; int pstride; myr_solve_opts so;
  double *lam, *cost; int32_t *status, *iters; double* kkt;      // each may be null
};
struct RolloutArgs { int B, num_steps, u_rows; const double *x0, *us, *params; int pstride; double *xs, *cost; };      // xs, cost may be null
struct FitArgs {      // E parameter sets of R trajectories each (myr_fit_grad: E = 1, R = B).  xh: [num_steps+1][NS][Bp] state scratch; loss [E][R] or null;
  // grad [E][R][NP] rows or null (the loss only); data_shared: xs_obs, us are [R][...], read by every set; params: [E][NP] (a closed-form system: may be
  // null = the defaults), or with per_row -- myr_fit_grad with params_stride == np on a closed-form system, E = 1 -- [R][NP], a row per trajectory
  int E, R, data_shared; long Bp; int num_steps, u_rows; const double *xs_obs, *us, *wt, *params; int per_row; double *xh, *loss, *grad;
  // myr_fit_gn*: gn non-null -- [E][R][NP][NP], the Gauss-Newton matrices; fit_gn_lane_kernel runs, without xh.  grad_ld, gn_ld: doubles from one
  // trajectory's row to the next (dispatch_fit sets them)
  double* gn; long grad_ld, gn_ld;
  // myr_fit_gnvp* (mode FIT_GNVP; the network system only): v [E][NP], a direction per set; jv [E][R][num_steps+1][NS] or null; grad is the product --
  // rows, sums or null (the forward tangent only); dxh: the tangent's scratch, of xh's shape (dispatch_fit sets it); loss stays null
  int mode; const double* v; double *jv, *dxh;
};
enum { FIT_GRAD = 0, FIT_GN = 1, FIT_GNVP = 2 };
struct ExgdGradArgs {      // rows: [B][NP] gradient rows; hist: the history of one chunk of `chunk` instances; seed_lam, dz0, dlam0 may be null
  int B; const double *z, *lam, *lb, *ub, *params; int pstride; double eta_x, eta_v; int nsteps; const double *seed_z, *seed_lam;
  double *rows, *dz0, *dlam0, *hist; int chunk;
  double* work; long Pp;      // SHOOTING (closed form) only: the scratch of one chunk (launch_shoot_exgd_grad carves it) and its pair columns
  int R, inst0;               // R: instances to a weight set (the network routes: params [B / R][NP], pstride 0; else B); inst0: the chunk's first instance
  // myr_exgd_jac (route EXGD_JAC; no seeds, rows or history): the start's tangents jz0 [B][NP][n], jlam0 [B][NP][m] and the outputs zn [B][n],
  // lamn [B][m], jz, jlam (the tangents' shapes); each may be null, jz and jlam not both
  const double *jz0, *jlam0; double *zn, *lamn, *jz, *jlam;
};
struct HvpArgs {      // lam, out_z, rows ([B][NP] parameter rows) may be null; hist, side: shooting scratch, batch-minor with Pp columns (one per pair)
  int B; const double *z, *lam, *v, *params; int pstride, with_cost; double *out_z, *rows, *hist, *side; long Pp;
  int R;                      // myr_hvp_node*: instances to a weight set (params [B / R][NP])
};
struct FbsmArgs {      // X, A [N+1][NS][Bp], U [N+1 | N][NU][Bp]: batch-minor
  int B; long Bp; int N; const double *x0, *adjT, *params; int pstride; VarScale lo, hi; double bang, delta; int max_sweeps;
  double *X, *U, *A; int32_t* sweeps;
};

// ------------------------------------------------------------------------------------------------
// eval
// ------------------------------------------------------------------------------------------------
template <class Sys, int SCHEME>
static int launch_hs_eval(myr_handle h, const EvalArgs& a) {
  const int N = h->d.intervals;
  const double hstep = h->d.T / N;
  int wpt = h->eval_wpt;
  // LDS is sized for the number of wavefronts ACTUALLY launched (the non-NT fallback always runs 4 per workgroup): when the
  // preferred width does not fit a CU the launch steps down (8 -> 4 -> 1) before it gives up
  const bool nt_ = h->eval_nt != 0;
  auto launched = [&](int w) { return nt_ ? (w == 1 ? 1 : (w == 8 ? 8 : 4)) : 4; };
  while (hs_eval_lds_bytes<Sys, SCHEME>(N, launched(wpt)) > 160 * 1024 && nt_ && wpt > 1) wpt = wpt == 8 ? 4 : 1;
  if (hs_eval_lds_bytes<Sys, SCHEME>(N, launched(wpt)) > 160 * 1024) return fail(MYR_E_CAPACITY, "hs_eval: intervals too large for the 160 KiB LDS record");
  // the start event is recorded after the host-side attribute call, directly in front of the launch: the interval
  // between the two events is the kernel plus its dispatch, not host work
#define MYR_EVAL_LAUNCH(W, NTV)                                                                                   \
  {                                                                                                               \
    auto kern = hs_eval_kernel<Sys, W, NTV, SCHEME>;                                                                   \
    const size_t lds = hs_eval_lds_bytes<Sys, SCHEME>(N, W);                                                      \
    if (h->eval_attr_lds[(W == 1 ? 0 : (W == 4 ? 1 : 2)) + (NTV ? 3 : 0)] == 0) {      /* function-wide limit: the hardware's, once */ \
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
      h->eval_attr_lds[(W == 1 ? 0 : (W == 4 ? 1 : 2)) + (NTV ? 3 : 0)] = 1;                                     \
    }                                                                                                             \
    if (int rc = timed_begin(h, MYR_K_EVAL)) return rc;                                                           \
    hipLaunchKernelGGL(kern, dim3(a.B), dim3(64 * W), lds, h->stream, N, hstep, a.z, a.params, a.pstride, a.f, a.g, a.c, a.j); \
  }
  const bool nt = h->eval_nt != 0;
  switch (wpt) {
    case 1: if (nt) MYR_EVAL_LAUNCH(1, true) else MYR_EVAL_LAUNCH(4, false) break;
    case 8: if (nt) MYR_EVAL_LAUNCH(8, true) else MYR_EVAL_LAUNCH(4, false) break;
    default: if (nt) MYR_EVAL_LAUNCH(4, true) else MYR_EVAL_LAUNCH(4, false) break;
  }
#undef MYR_EVAL_LAUNCH
  return timed_end(h, MYR_K_EVAL);
}

template <class Sys>
static int launch_shoot_eval(myr_handle h, const EvalArgs& a) {
  const int I = h->d.intervals, cpi = h->d.controls_per_interval, method = h->d.integration_method, B = a.B;
  if (int rc = ensure_buf(&h->sbuf, &h->sbuf_bytes, (size_t)B * (size_t)(cpi + 1) * Sys::NS * 8)) return rc;
  if (int rc = timed_begin(h, MYR_K_EVAL)) return rc;
  if (method == MYR_INT_RK4)
    hipLaunchKernelGGL((shoot_eval_kernel<Sys, 2>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, B, I, cpi, method, h->d.T,
                       a.z, a.params, a.pstride, a.f, a.g, a.c, a.j, (double*)h->sbuf, (const double*)nullptr, 1);
  else
    hipLaunchKernelGGL((shoot_eval_kernel<Sys, 1>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, B, I, cpi, method, h->d.T,
                       a.z, a.params, a.pstride, a.f, a.g, a.c, a.j, (double*)h->sbuf, (const double*)nullptr, 1);
  return timed_end(h, MYR_K_EVAL);
}

template <class Sys>
int eval_for_system(myr_handle h, const EvalArgs& a) {
  if constexpr (Sys::PARAMS_BY_POINTER) {   // neural-ODE systems: Hermite-Simpson (config 5) and shooting (the reference's default route for a NodeSystem,
                                            // config.py:66 + shooting.py:144-167, 212-228); its parametrised trapezoid is dead code (trapezoidal.py:204-206, quirk Q8)
    if (h->d.transcription == MYR_TR_SHOOTING) return launch_shoot_eval<Sys>(h, a);
    if (h->d.transcription != MYR_TR_HERMITE_SIMPSON) return fail(MYR_E_UNSUPPORTED, "myr_eval: NODE systems are built for HERMITE_SIMPSON and SHOOTING");
    return launch_hs_eval<Sys, EVAL_HS>(h, a);
  } else {
    switch (h->d.transcription) {
      case MYR_TR_HERMITE_SIMPSON: return launch_hs_eval<Sys, EVAL_HS>(h, a);
      case MYR_TR_TRAPEZOIDAL: return launch_hs_eval<Sys, EVAL_TRAP>(h, a);
      case MYR_TR_SHOOTING: return launch_shoot_eval<Sys>(h, a);
    }
  }
  return fail(MYR_E_ARG, "eval: unknown transcription");
}

// ------------------------------------------------------------------------------------------------
// Lagrangian products and the extragradient step (collocation transcriptions)
// ------------------------------------------------------------------------------------------------
template <class Sys, int SCHEME>
static int launch_products(myr_handle h, const ProdArgs& a) {
  const int N = h->d.intervals;
  const double hstep = h->d.T / N;
  using P = CollocProducts<Sys, SCHEME>;
  if (int rc = timed_begin(h, MYR_K_PROD)) return rc;
  if (a.op == PRODOP_EXGD) {
    const size_t lds = colloc_exgd_lds_bytes<Sys, SCHEME>(N);
    if (lds > 160 * 1024) return fail(MYR_E_CAPACITY, "myr_exgd: intervals too large for the LDS-resident iterate");
    auto kern = colloc_exgd_kernel<Sys, SCHEME>;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)a.B), dim3(64), lds, h->stream, a.B, N, hstep, a.zio, a.lamio, a.lb, a.ub,
                       a.params, a.pstride, a.eta_x, a.eta_v, a.nsteps);
  } else {
    const long units = (long)a.B * (a.op == PRODOP_VJP ? P::points(N) : N);
    const unsigned blocks = grid_for(units);
    if (a.op == PRODOP_VJP)
      hipLaunchKernelGGL((colloc_vjp_kernel<Sys, SCHEME>), dim3(blocks), dim3(256), 0, h->stream, a.B, N, hstep, a.z, a.w,
                         a.params, a.pstride, a.out, a.add_gradf);
    else
      hipLaunchKernelGGL((colloc_jvp_kernel<Sys, SCHEME>), dim3(blocks), dim3(256), 0, h->stream, a.B, N, hstep, a.z, a.w,
                         a.params, a.pstride, a.out);
  }
  return timed_end(h, MYR_K_PROD);
}

// count doubles from one device array of the handle's stream to another
static int copy_doubles(myr_handle h, double* dst, const double* src, long count) {
  HIPCHK(hipMemcpyAsync(dst, src, (size_t)count * 8, hipMemcpyDeviceToDevice, h->stream));
  return MYR_OK;
}

// `nsteps` extragradient steps of a shooting problem as a launch sequence (the iterate of a shooting problem is small: no LDS-resident variant), in place
// in (zio, lamio).  scr: B (cpi + 1) NS doubles of sweep scratch; g, zbar [B][n]; cbuf [B][m].  hist (or null; ShootExgdGrad's layout for a chunk of
// B instances): x_s, x_bar_s, lam_s of every step and the final x are copied out as the steps go.  myr_exgd and myr_exgd_grad_shoot both run this.
template <class Sys, int M>
static int shoot_exgd_steps(myr_handle h, int B, double* zio, double* lamio, const double* lb, const double* ub, const double* params, int pstride,
                             double eta_x, double eta_v, int nsteps, double* scr, double* g, double* zbar, double* cbuf, double* hist) {
  const int I = h->d.intervals, cpi = h->d.controls_per_interval, method = h->d.integration_method;
  const myr_dims& dm = h->dims;
  const dim3 grid((unsigned)((B + 63) / 64)), blk(64);
  const long tz = (long)B * dm.n, tl = (long)B * dm.m;
  const unsigned ub_ = grid_for(tz);
  for (int s = 0; s < nsteps; ++s) {
    double* hs = hist ? hist + (size_t)s * (size_t)(2 * tz + tl) : nullptr;
    if (hs) {
      if (int rc = copy_doubles(h, hs, zio, tz)) return rc;
      if (int rc = copy_doubles(h, hs + 2 * tz, lamio, tl)) return rc;
    }
    hipLaunchKernelGGL((shoot_eval_kernel<Sys, M>), grid, blk, 0, h->stream, B, I, cpi, method, h->d.T, (const double*)zio, params, pstride,
                       (double*)nullptr, g, (double*)nullptr, (double*)nullptr, scr, (const double*)lamio, 1);
    hipLaunchKernelGGL(exgd_update_kernel, dim3(ub_), dim3(256), 0, h->stream, tz, (const double*)zio, (const double*)g, lb, ub, eta_x, zbar);
    if (hs)
      if (int rc = copy_doubles(h, hs + tz, zbar, tz)) return rc;
    hipLaunchKernelGGL((shoot_eval_kernel<Sys, M>), grid, blk, 0, h->stream, B, I, cpi, method, h->d.T, (const double*)zbar, params, pstride,
                       (double*)nullptr, g, (double*)nullptr, (double*)nullptr, scr, (const double*)lamio, 1);
    hipLaunchKernelGGL(exgd_update_kernel, dim3(ub_), dim3(256), 0, h->stream, tz, (const double*)zio, (const double*)g, lb, ub, eta_x, zio);
    hipLaunchKernelGGL((shoot_eval_kernel<Sys, M>), grid, blk, 0, h->stream, B, I, cpi, method, h->d.T, (const double*)zio, params, pstride,
                       (double*)nullptr, (double*)nullptr, cbuf, (double*)nullptr, scr, (const double*)nullptr, 1);
    hipLaunchKernelGGL(axpy_kernel, dim3((unsigned)((tl + 255) / 256)), dim3(256), 0, h->stream, tl, eta_v, (const double*)cbuf, lamio);
  }
  return hist ? copy_doubles(h, hist + (size_t)nsteps * (size_t)(2 * tz + tl), zio, tz) : (int)MYR_OK;
}

// shooting: J^T lam / grad L by the reverse sweep of shoot_eval_kernel seeded with lam, J v by forward tangents, and the
// extragradient step (shoot_exgd_steps)
template <class Sys, int M>
static int launch_shoot_products_m(myr_handle h, const ProdArgs& a) {
  const int I = h->d.intervals, cpi = h->d.controls_per_interval, method = h->d.integration_method;
  const myr_dims& dm = h->dims;
  const size_t sweep = (size_t)a.B * (size_t)(cpi + 1) * Sys::NS * 8;
  const size_t extra = a.op == PRODOP_EXGD ? ((size_t)2 * a.B * dm.n + (size_t)a.B * dm.m) * 8 : 0;   // g, zbar, c
  if (int rc = ensure_buf(&h->sbuf, &h->sbuf_bytes, sweep + extra)) return rc;
  double* scr = (double*)h->sbuf;
  const dim3 grid((unsigned)((a.B + 63) / 64)), blk(64);
  if (int rc = timed_begin(h, MYR_K_PROD)) return rc;
  int rc = MYR_OK;
  if (a.op == PRODOP_VJP) {
    hipLaunchKernelGGL((shoot_eval_kernel<Sys, M>), grid, blk, 0, h->stream, a.B, I, cpi, method, h->d.T, a.z, a.params, a.pstride,
                       (double*)nullptr, a.out, (double*)nullptr, (double*)nullptr, scr, a.w, a.add_gradf);
  } else if (a.op == PRODOP_JVP) {
    hipLaunchKernelGGL((shoot_jvp_kernel<Sys, M>), grid, blk, 0, h->stream, a.B, I, cpi, method, h->d.T, a.z, a.w, a.params, a.pstride, a.out);
  } else {
    double* g = scr + sweep / 8; double* zbar = g + (size_t)a.B * dm.n; double* cbuf = zbar + (size_t)a.B * dm.n;
    rc = shoot_exgd_steps<Sys, M>(h, a.B, a.zio, a.lamio, a.lb, a.ub, a.params, a.pstride, a.eta_x, a.eta_v, a.nsteps, scr, g, zbar, cbuf, nullptr);
  }
  const int rc_end = timed_end(h, MYR_K_PROD);
  return rc ? rc : rc_end;
}

template <class Sys>
static int launch_shoot_products(myr_handle h, const ProdArgs& a) {
  return h->d.integration_method == MYR_INT_RK4 ? launch_shoot_products_m<Sys, 2>(h, a) : launch_shoot_products_m<Sys, 1>(h, a);
}

// NODE systems under shooting: ONE launch per call, lane = (instance, interval) pair, the network by matrix-core passes (node_shoot_products.h).
// G instances per workgroup from I, cpi and params_stride alone -- never from the batch size: an instance's bits do not depend on its batch.
template <class Sys, int M>
static int launch_node_shoot_products(myr_handle h, const ProdArgs& a) {
  if constexpr (NodeTraits<Sys>::mlp) {
    using P = NodeShootProd<Sys, M>;
    using L = NspLds<Sys, M>;
    const int I = h->d.intervals, cpi = h->d.controls_per_interval;
    const long lds_max = 160 * 1024 / 8;
    const long fixed = L::fixed_doubles(I), per = L::iter_doubles(I, cpi);
    if (fixed > lds_max) return fail(MYR_E_CAPACITY, "products: intervals too large for the LDS slots of the shared control rows");
    NspArgs k{};
    k.op = a.op == PRODOP_VJP ? NSP_VJP : (a.op == PRODOP_JVP ? NSP_JVP : NSP_EXGD);
    k.B = a.B; k.I = I; k.cpi = cpi; k.method = h->d.integration_method; k.T = h->d.T;
    k.z = a.z; k.w = a.w; k.params = a.params; k.pstride = a.pstride; k.out = a.out; k.add_gradf = a.add_gradf;
    k.zio = a.zio; k.lamio = a.lamio; k.lb = a.lb; k.ub = a.ub; k.eta_x = a.eta_x; k.eta_v = a.eta_v; k.nsteps = a.nsteps;
    int G = (a.pstride != 0 || I > 64) ? 1 : 64 / I;
    bool iter_global = false;
    if (a.op == PRODOP_EXGD) {      // z, x_bar, g, lam of the group in LDS: fewer instances per workgroup where 64 lanes' worth do not fit, global scratch where one does not
      const long fit = (lds_max - fixed) / per;
      if (fit < 1) iter_global = true;
      else if (fit < G) G = (int)fit;
    }
    k.G = G;
    const long groups = ((long)a.B + G - 1) / G;
    const long pairs = (long)a.B * I;
    k.Pp = (pairs + 63) / 64 * 64;
    const size_t scr_bytes = (size_t)P::pair_doubles(cpi) * (size_t)k.Pp * 8;
    const size_t iter_bytes = iter_global ? (size_t)groups * (size_t)G * (size_t)per * 8 : 0;
    if (int rc = ensure_buf(&h->sbuf, &h->sbuf_bytes, scr_bytes + iter_bytes)) return rc;
    k.scr = (double*)h->sbuf;
    k.iter = iter_global ? k.scr + scr_bytes / 8 : nullptr;
    k.lds_doubles = fixed + (a.op == PRODOP_EXGD && !iter_global ? (long)G * per : 0);
    k.poison = h->poison;
    auto kern = node_shoot_products_kernel<Sys, M>;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (int rc = timed_begin(h, MYR_K_PROD)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)groups), dim3(64), (size_t)k.lds_doubles * 8, h->stream, k);
    return timed_end(h, MYR_K_PROD);
  } else {
    (void)a;
    return fail(MYR_E_UNSUPPORTED, "products: this NODE system has no matrix-core passes");
  }
}

template <class Sys>
int products_for_system(myr_handle h, const ProdArgs& a) {
  if constexpr (Sys::PARAMS_BY_POINTER) {
    if (h->d.transcription == MYR_TR_SHOOTING) {      // the reference's default route for a NodeSystem (config.py:66): matrix-core passes over pairs (node_shoot_products.h)
      if (h->prod_lane) return launch_shoot_products<Sys>(h, a);
      return h->d.integration_method == MYR_INT_RK4 ? launch_node_shoot_products<Sys, 2>(h, a) : launch_node_shoot_products<Sys, 1>(h, a);
    }
    if (h->d.transcription != MYR_TR_HERMITE_SIMPSON) return fail(MYR_E_UNSUPPORTED, "products: NODE systems are built for HERMITE_SIMPSON and SHOOTING");
    return launch_products<Sys, PROD_HS>(h, a);
  } else {
    switch (h->d.transcription) {
      case MYR_TR_HERMITE_SIMPSON: return launch_products<Sys, PROD_HS>(h, a);
      case MYR_TR_TRAPEZOIDAL: return launch_products<Sys, PROD_TRAP>(h, a);
      case MYR_TR_SHOOTING: return launch_shoot_products<Sys>(h, a);
      default: return fail(MYR_E_ARG, "products: unknown transcription");
    }
  }
}

// ------------------------------------------------------------------------------------------------
// solve
// ------------------------------------------------------------------------------------------------
// [rows][cols] row-major  ->  [cols][ld] (ld >= rows): instance-major <-> batch-minor, 32x32 LDS tiles
static __global__ __launch_bounds__(256) void transpose_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                        int rows, int cols, long ld) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 32; i += 8) {
    const int r = r0 + ty + i, c = c0 + tx;
    if (r < rows && c < cols) tile[ty + i][tx] = src[(long)r * cols + c];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 32; i += 8) {
    const int c = c0 + ty + i, r = r0 + tx;
    if (r < rows && c < cols) dst[(long)c * ld + r] = tile[tx][ty + i];
  }
}
// [cols][ld] -> [rows][cols]
static __global__ __launch_bounds__(256) void transpose_back_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                             int rows, int cols, long ld) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 32; i += 8) {
    const int c = c0 + ty + i, r = r0 + tx;
    if (r < rows && c < cols) tile[ty + i][tx] = src[(long)c * ld + r];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 32; i += 8) {
    const int r = r0 + ty + i, c = c0 + tx;
    if (r < rows && c < cols) dst[(long)r * cols + c] = tile[tx][ty + i];
  }
}

// One trajectory per lane; every per-trajectory array is batch-minor (element i of trajectory b at a[i*Bp + b]),
// so the 64 lanes of a wavefront always touch 64 consecutive doubles (one 512-byte coalesced access).
template <class Core, class Sys>
__global__ __launch_bounds__(64, 1)
void lane_solve_kernel(int B, long Bp, int lanes_per_wave, HsSolveOpts o, VarScale vs, double* z, double* lb, double* ub, double* zL, double* zU,
                     double* lam, double* dz, double* st, const double* __restrict__ params, int params_stride,
                     double* cost, int32_t* status, int32_t* iters, double* kkt) {
  // The kernel is latency-bound (long dependent fp64 chains, one wave per SIMD at best), so a wavefront may be
  // launched partially populated: fewer trajectories per wave -> more waves in flight and a shorter wait for
  // the slowest trajectory of each wave.
  if ((int)threadIdx.x >= lanes_per_wave) return;
  const long b = (long)blockIdx.x * lanes_per_wave + threadIdx.x;
  if (b >= B) return;
  SysParams<Sys> pp;
  pp.load(params, b, params_stride);
  pp.set_scale(vs.s);
  const double* p = pp.get();
  HsWork w{{z + b, Bp}, {lb + b, Bp}, {ub + b, Bp}, {zL + b, Bp}, {zU + b, Bp}, {lam + b, Bp}, {dz + b, Bp}, {st + b, Bp}};
  HsSolveResult r;
  Core::solve(w, o, p, r);
  if (cost) cost[b] = r.cost;
  if (status) status[b] = r.status;
  if (iters) iters[b] = r.iters;
  if (kkt) { kkt[3 * b] = r.feas; kkt[3 * b + 1] = r.stat; kkt[3 * b + 2] = r.compl_; }
}

static HsSolveOpts make_opts(myr_handle h, const myr_solve_opts& so) {
  HsSolveOpts o;
  o.N = h->d.intervals; o.h = h->d.T / h->d.intervals; o.max_iter = so.max_iter; o.tol_feas = so.tol_feas;
  o.tol_stat = so.tol_stat; o.tol_compl = so.tol_compl; o.mu_init = so.mu_init;
  o.cpi = h->d.controls_per_interval; o.method = h->d.integration_method;
  o.restarts = so.restarts < 0 ? MYR_SHOOT_RESTARTS : (so.restarts > 4 ? 4 : so.restarts);
  // warm-started inertia correction: trades factorisation sweeps for (slightly more) iterations, which pays when a
  // sweep costs more than a linearisation -- collocation with closed-form dynamics; not shooting (the rollout
  // linearisation dominates, and the correction decays too slowly for its stragglers) nor network dynamics
  o.delta_warm = (h->d.transcription != MYR_TR_SHOOTING && h->d.system_id != MYR_SYS_NODE_CARTPOLE) ? 1 : 0;
  if (const char* e = getenv("MYRIAD_NONMONO")) o.nonmono = atoi(e);      // developer knobs (globalisation ablations)
  if (const char* e = getenv("MYRIAD_RECENTER")) o.recenter = atoi(e);
  if (const char* e = getenv("MYRIAD_DELTA_WARM")) o.delta_warm = atoi(e);
  if (const char* e = getenv("MYRIAD_DELTA_WARM_MIN")) o.delta_warm_min = atof(e);
  if (const char* e = getenv("MYRIAD_KAPPA_MU")) o.kappa_mu = atof(e);    // barrier schedule ablations
  if (const char* e = getenv("MYRIAD_THETA_MU")) o.theta_mu = atof(e);
  if (const char* e = getenv("MYRIAD_KAPPA_EPS")) o.kappa_eps = atof(e);
  if (const char* e = getenv("MYRIAD_MU_INIT")) o.mu_init = atof(e);
  if (o.nonmono < 0) o.nonmono = 0;
  if (o.nonmono > 8) o.nonmono = 8;
  return o;
}

template <class Core, class Sys>
static int launch_lane_solve(myr_handle h, const SolveCall& a, long nst);
// the lane kernels of the collocation solvers as an entry point of their own (objects of their own in a split build: MYR_TU_PART 5, 6)
template <class Sys, int SCHEME>
int solve_lane_colloc_for_system(myr_handle h, const SolveCall& a);
#if defined(MYR_TU_SYSTEM) && defined(MYR_TU_PART)
#if MYR_TU_PART != 5
extern template int solve_lane_colloc_for_system<myriad::MYR_TU_SYSTEM, 0>(myr_handle, const SolveCall&);
#endif
#if MYR_TU_PART != 6
extern template int solve_lane_colloc_for_system<myriad::MYR_TU_SYSTEM, 1>(myr_handle, const SolveCall&);
#endif
#endif

// Resume order of a two-phase launch (hs_solver_fused.h: park_bucket): the trajectories counted themselves into `cnt` when they parked; ONE workgroup
// turns the 256 counts into start offsets, largest bucket first, and places every parked trajectory (the order inside a bucket is whatever the atomics give).
using myriad::PARK_BUCKETS;
// `late`: the iterations a trajectory was parked after k1, from its record (`state` + pk_it, HsFused::PK_IT).
static __global__ __launch_bounds__(1024) void park_order_kernel(int B, const int32_t* __restrict__ status, const double* __restrict__ kkt, int* __restrict__ cnt, int* __restrict__ perm,
                                                                 const double* __restrict__ state, long stride, int pk_it, int k1, int shift) {
  __shared__ int off[PARK_BUCKETS];
  if (threadIdx.x < PARK_BUCKETS) off[threadIdx.x] = cnt[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int k = PARK_BUCKETS - 1; k >= 0; --k) { const int c = off[k]; off[k] = run; run += c; }
    cnt[PARK_BUCKETS] = run;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += blockDim.x)
    if (status[b] == myriad::MYR_STATUS_PARKED_) {
      const int late = (int)state[(long)b * stride + pk_it] - k1;
      const int p = atomicAdd(&off[myriad::park_bucket_late(kkt[3 * b + 1], kkt[3 * b + 2], late, shift)], 1);
      if (p < B) perm[p] = b;
    }
}

// fused-phase wavefront kernel (hs_solver_fused.h): Hermite-Simpson, closed-form systems with one control and <= 4 states.
// NWAVES wavefronts per trajectory: 1 for throughput (four trajectories per CU), 2 when the batch leaves CUs idle otherwise
// (B <= 2 trajectories per CU: the parallel phases of an iteration take half the time, the launch lasts as long as one solve).
template <class Sys, int NWAVES, int SCHEME>
static int launch_hs_fused_w(myr_handle h, const SolveCall& a) {
  using W = HsFused<Sys, NWAVES, SCHEME>;
  const int N = h->d.intervals, B = a.B;
  const myr_solve_opts& so = a.so;
  const size_t lds = W::lds_bytes(N);
  auto kern = hs_solve_fused_kernel<Sys, NWAVES, SCHEME>;
  int per_cu = 0;       // (attributes and occupancy once per handle and configuration, not per call)
  if (int rc = kernel_blocks_per_cu(h, reinterpret_cast<const void*>(kern), 64 * NWAVES, lds, &per_cu)) return rc;
  const int slots_full = default_slots(h, per_cu, 4 / NWAVES);
  const int slots = slots_full > B ? B : slots_full;
  const long stride = slot_stride(W::scratch_doubles(N));
  const size_t need = (size_t)slots * (size_t)stride * 8;
  if (int rc = ensure_buf(&h->sbuf, &h->sbuf_bytes, need)) return rc;
  if (int rc = reset_ticket(h)) return rc;
  HsSolveOpts o = make_opts(h, so);
  if (int rc = timed_begin(h, MYR_K_SOLVE)) return rc;
  h->last_solve_form = 1;
  if (getenv("MYRIAD_DEBUG_PTRS"))
    fprintf(stderr, "[myriad] fused W=%d N=%d B=%d slots=%d lds=%zu stride=%ld doubles: scratch [%p, %p) z %p lb %p ub %p lam %p ticket %p\n", NWAVES, N, B, slots, lds, stride,
            h->sbuf, (char*)h->sbuf + need, (void*)a.z, (const void*)a.lb, (const void*)a.ub, (void*)a.lam, (void*)h->ticket);
  // Two phases when a slot would take at least two whole solves (B >= 2 x resident wavefronts): k1 iterations for every trajectory, the
  // unfinished ones parked, then resumed longest-first (hs_solver_fused.h: ParkArgs).  Needs the per-instance status and residuals.
  int k1 = 0;
  if constexpr (NWAVES == 1 || W::MLP) {        // the one-wavefront kernels and the network kernel (four wavefronts, one trajectory per CU: B = 1024 is four rounds)
    k1 = so.park_iter != 0 ? so.park_iter : h->park_iter;
    if (k1 < 0 && so.park_iter < 0) k1 = 0;                     // opts.park_iter = -1: whole solves
    else if (k1 < 0) {
      // by the number of solves a resident wavefront gets (measured on the headline workload, tools/dev/exp/exp47.sh: B = 1536 +4 %, 2048 +7 %,
      // 3072 +16 %, 4096 +9 %, 8192 +7 %; below one and a half solves per wavefront whole solves are faster)
      const double per_slot = (double)B / (double)slots_full;
      k1 = (SCHEME != 0 || W::MLP) ? 0 : (per_slot >= 3.0 ? 12 : (per_slot >= 2.0 ? 10 : (per_slot >= 1.5 ? 8 : 0)));
    }       // a little more than half of a typical interior-point solve (20-25 iterations);
                                                                               // (trapezoidal solves are shorter and closer together: two phases cost them 2.5 %;
                                                                               //  the network system's longest solves -- 75 iterations against a median of 24 -- have SMALL
                                                                               //  residuals at the parking point and would come last: 41 -> 52 ms at B = 1024, exp42 / exp43)
    if (k1 >= o.max_iter || !a.status || !a.kkt) k1 = 0;
    if (W::ZLU_GLOBAL && W::MLP) k1 = 0;        // (the network kernel's throughput form: its helper protocol and activation store are not part of a parked record;
                                                //  the closed-form systems that keep the bound multipliers in the slot's scratch park them with the solver's LDS)
  }
  // Helper workgroups for the network passes (hs_solver_fused.h: NodeBoard): a batch of at most half the CUs (config 5's share of an 8-GPU node is 128
  // trajectories) gets nh = #CU / B - 1 <= 3 more workgroups per trajectory; whole solves with one shared weight set only.
  myriad::CoopArgs co{nullptr, nullptr, 0, 0, nullptr};
  unsigned grid = (unsigned)slots;
  if constexpr (W::MLP) {
    const int cus = device_cus(h);
    const int resident = per_cu * cus;                               // workgroups the device holds: 1 per CU (four wavefronts), 2 per CU (two)
    int maxh = NWAVES == 2 ? 5 : 3;                                  // 13 tiles over 4 (nh + 1) resp. 2 (nh + 1) wavefronts
    if (B <= resident / 2 && resident / B - 1 < maxh) maxh = resident / B - 1;      // a small batch: spread the idle workgroups evenly
    if (h->node_helpers >= 0 && h->node_helpers < maxh) maxh = h->node_helpers;
    // whole solves with one shared weight set; every workgroup of the launch must be resident: owners wait for their helpers
    if (a.pstride != 0 || k1 > 0 || per_cu < 1 || per_cu != 4 / NWAVES || h->solve_slots > 0) maxh = 0;
    if (maxh > 0) {
      grid = (unsigned)((long)B * (maxh + 1) < (long)resident ? B * (maxh + 1) : resident);
      const int nboards = B <= (int)grid ? B : (int)grid;      // workgroups that can own a trajectory (hs_solve_fused_kernel: `fixed`)
      const long pub = ((long)h->dims.n + (long)W::MLAM * N * W::NS + (long)W::npoints(N) * W::NS + 15) / 16 * 16;
      const size_t head = ((size_t)nboards * sizeof(myriad::NodeBoard) + 128 + 127) / 128 * 128;
      if (int rc = ensure_buf(&h->coop_buf, &h->coop_bytes, head + (size_t)nboards * (size_t)pub * 8)) return rc;
      HIPCHK(hipMemsetAsync(h->coop_buf, 0, head, h->stream));
      co.boards = (myriad::NodeBoard*)h->coop_buf;
      co.abort = (int*)((char*)h->coop_buf + (size_t)nboards * sizeof(myriad::NodeBoard));
      co.pub = (double*)((char*)h->coop_buf + head);
      co.pub_stride = pub; co.maxh = maxh;
    }
  }
  myriad::ParkArgs pk{0, 0, nullptr, nullptr, nullptr, 0};
  if (k1 > 0) {
    const long pstr = (W::park_doubles(N) + 31) / 32 * 32;
    const size_t pneed = (size_t)B * (size_t)pstr * 8;
    if (pneed > h->park_bytes) {
      if (h->park_state) HIPCHK(hipFree(h->park_state));
      h->park_state = nullptr; h->park_bytes = 0;
      if (hipMalloc(&h->park_state, pneed) == hipSuccess) h->park_bytes = pneed;
      else { (void)hipGetLastError(); h->park_state = nullptr; k1 = 0; }      // no room for the records (41 KB per instance): whole solves
    }
  }
  if (k1 > 0) {
    const long pstr = (W::park_doubles(N) + 31) / 32 * 32;
    if ((size_t)B > h->park_n) {
      if (h->park_perm) HIPCHK(hipFree(h->park_perm));
      h->park_perm = nullptr; h->park_n = 0;
      HIPCHK(hipMalloc(&h->park_perm, ((size_t)B + PARK_BUCKETS + 2) * sizeof(int)));
      h->park_n = (size_t)B;
    }
    int* cnt = h->park_perm + h->park_n;        // [PARK_BUCKETS] per bucket, then the number parked, then `reached`
    pk = myriad::ParkArgs{1, k1, h->park_perm, cnt + PARK_BUCKETS, (double*)h->park_state, pstr, h->park_fill, h->park_shift, cnt + PARK_BUCKETS + 1, cnt};
    HIPCHK(hipMemsetAsync(cnt, 0, (PARK_BUCKETS + 2) * sizeof(int), h->stream));       // (launch 1 counts into them)
#ifdef MYR_SLOT_STAMPS
    // developer instrument (-DMYR_SLOT_STAMPS, tools/dev/slot_stamps.py): wall clock of every slot at entry, after each ticket and at exit, both launches;
    // one buffer per process (the handle's layout is shared with objects built without the flag)
    static void* stamp_buf = nullptr; static size_t stamp_bytes = 0;
    const size_t stamp_need = 2 * (size_t)slots * myriad::SLOT_STAMP_WORDS * sizeof(long long);
    if (int rc = ensure_buf(&stamp_buf, &stamp_bytes, stamp_need)) return rc;
    HIPCHK(hipMemsetAsync(stamp_buf, 0, stamp_need, h->stream));
    pk.stamps = (long long*)stamp_buf;
#endif
    hipLaunchKernelGGL(kern, dim3((unsigned)slots), dim3(64 * NWAVES), lds, h->stream, B, h->ticket, o, h->vscale, a.z, a.lb, a.ub, a.lam, (double*)h->sbuf, stride,
                       a.params, a.pstride, a.cost, a.status, a.iters, a.kkt, h->poison, pk, co);
    HIPCHK(hipGetLastError());
    if (int rc = reset_ticket(h)) return rc;
    hipLaunchKernelGGL(park_order_kernel, dim3(1), dim3(1024), 0, h->stream, B, a.status, a.kkt, cnt, h->park_perm,
                       (const double*)h->park_state, pstr, (int)W::PK_IT, k1, h->park_shift);
    pk.mode = 2;
#ifdef MYR_SLOT_STAMPS
    pk.stamps += (size_t)slots * myriad::SLOT_STAMP_WORDS;
#endif
  }
#ifdef MYR_COOP_TRACE
  static int* trace_host = nullptr;
  if (!trace_host) { HIPCHK(hipHostMalloc((void**)&trace_host, 256 * 16 * sizeof(int), hipHostMallocMapped)); }
  for (int i = 0; i < 256 * 16; ++i) trace_host[i] = 0;
  if (co.maxh > 0) {
    int* dev = nullptr; HIPCHK(hipHostGetDevicePointer((void**)&dev, trace_host, 0));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(myriad::g_coop_trace), &dev, sizeof(dev)));
    static std::atomic<int> launch_no{0};
    const int my = ++launch_no; const int ng = (int)grid;
    std::thread([my, ng]() {
      std::this_thread::sleep_for(std::chrono::seconds(8));
      if (launch_no.load() != my) return;
      fprintf(stderr, "[coop trace] launch %d still running after 8 s; per workgroup: t0 seq target mode expect to hid lastcmd hstate ostate quit w1 w2 w3\n", my);
      for (int w = 0; w < ng; ++w) { fprintf(stderr, "  wg %3d:", w); for (int k = 0; k < 16; ++k) fprintf(stderr, " %d", trace_host[w * 16 + k]); fprintf(stderr, "\n"); }
      fflush(stderr);
    }).detach();
  }
#endif
  set_plan(h, 1, NWAVES, k1, k1 > 0 ? 2 : 1, slots, co.maxh);      // (the plan of THIS handle's last launch; a restoration twin is a handle of its own)
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NWAVES), lds, h->stream, B, h->ticket, o, h->vscale, a.z, a.lb, a.ub, a.lam, (double*)h->sbuf, stride,
                     a.params, a.pstride, a.cost, a.status, a.iters, a.kkt, h->poison, pk, co);
  if (int rc = timed_stop(h, MYR_K_SOLVE)) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (co.maxh > 0) {
    int ab = 0;
    HIPCHK(hipMemcpy(&ab, co.abort, sizeof(int), hipMemcpyDeviceToHost));
    if (ab) return fail(MYR_E_HIP, "network kernel: a wait between a trajectory's workgroups ran into its bound (MYRIAD_NODE_HELPERS=0 runs without helper workgroups)");
  }
  if (k1 > 0) {
    if (const char* path = getenv("MYRIAD_PARK_DUMP")) {      // developer knob: the loop scalars of every record as parked ([B][NSCAL] doubles), for the study of resume orders;
      std::vector<double> sc((size_t)B * W::NSCAL + 4);       // then four doubles: NSCAL, the index of the parking iteration (PK_IT), trajectories parked, `reached`
      HIPCHK(hipMemcpy2D(sc.data(), W::NSCAL * sizeof(double), h->park_state, (size_t)pk.stride * sizeof(double), W::NSCAL * sizeof(double), (size_t)B, hipMemcpyDeviceToHost));
      int tail[2] = {0, 0};
      HIPCHK(hipMemcpy(tail, pk.count, sizeof(tail), hipMemcpyDeviceToHost));
      double* t = sc.data() + (size_t)B * W::NSCAL;
      t[0] = (double)W::NSCAL; t[1] = (double)W::PK_IT; t[2] = (double)tail[0]; t[3] = (double)tail[1];
      if (FILE* f = fopen(path, "wb")) { fwrite(sc.data(), sizeof(double), sc.size(), f); fclose(f); }
    }
#ifdef MYR_SLOT_STAMPS
    if (const char* path = getenv("MYRIAD_SLOT_STAMPS")) {      // [2 launches][slots][SLOT_STAMP_WORDS] int64 behind a header {slots, SLOT_STAMP_WORDS}
      const long long head[2] = {(long long)slots, (long long)myriad::SLOT_STAMP_WORDS};
      std::vector<long long> st(2 * (size_t)slots * myriad::SLOT_STAMP_WORDS);
      HIPCHK(hipMemcpy(st.data(), pk.stamps - (size_t)slots * myriad::SLOT_STAMP_WORDS, st.size() * sizeof(long long), hipMemcpyDeviceToHost));
      if (FILE* f = fopen(path, "wb")) { fwrite(head, sizeof(long long), 2, f); fwrite(st.data(), sizeof(long long), st.size(), f); fclose(f); }
    }
#endif
  }
  return timed_account(h, MYR_K_SOLVE);      // (a launch the helper protocol aborted is not counted)
}
template <class Sys, int SCHEME>
static int launch_hs_fused(myr_handle h, const SolveCall& a) {
  if constexpr (NodeTraits<Sys>::mlp) {
    // network dynamics.  Up to one trajectory per CU: four wavefronts share a trajectory (the LATENCY form: a launch is one solve long, idle CUs attach as
    // helpers).  Beyond: two wavefronts per trajectory, two trajectories per CU (the THROUGHPUT form: one trajectory's sequential sweep and interval
    // passes overlap the other's matrix-core passes on the CU's other two SIMDs; bound multipliers in global scratch so that two workgroups fit the LDS).
    // MYRIAD_FUSED_WAVES=2|4 overrides.
    int waves = (a.B > device_cus(h)) ? 2 : 4;
    if (h->fused_waves == 2 || h->fused_waves == 4) waves = h->fused_waves;
    if (waves == 2 && a.pstride == 0 && 2 * HsFused<Sys, 2, 0>::lds_bytes(h->d.intervals) <= 160 * 1024)
      return launch_hs_fused_w<Sys, 2, 0>(h, a);
    return launch_hs_fused_w<Sys, 4, 0>(h, a);
  } else {
    // W = 2: two wavefronts per trajectory for batches of at most two trajectories per CU (a launch then lasts as long as one solve,
    // and the parallel passes of an iteration take half the time: +15 % at B = 512).  Round 3 switched it off -- its build returned
    // results that differed from launch to launch; round 4 found the form of the sweep that does it
    // (hs_solver_fused.h: sweep) and gates every build with tests/test_gpu_poison.py.  MYRIAD_FUSED_WAVES=1|2 overrides the choice.
    int waves = (a.B <= 2 * device_cus(h)) ? 2 : 1;
    // (Four wavefronts per trajectory for batches of at most one trajectory per CU -- chunks of N / 4 stages -- were built and measured in round 6,
    // tools/dev/exp/exp84.sh: same iterates, and NO gain over two wavefronts -- B = 128 50.6 k against 50.4 k solves/s, B = 256 97.5 k against 96.6 k: what the
    // shorter chunks save, the three interface joins, one after the other on wavefront 0, cost.  Not instantiated: 160 KB of code per system.)
    // Four wavefronts running two chunks and TWO RUNGS of the inertia ladder at a time for batches of at most one trajectory per CU: +3 %, not in (the code
    // is in the history at 2373201).
    // Systems whose solver LDS lets at most two one-wavefront workgroups onto a CU (ROCKETLANDING's Hermite-Simpson form: 64 KB; the wider twins) leave two
    // SIMDs of every CU idle in that form: when as many two-wavefront workgroups fit, those run at EVERY batch size (round 6, tools/dev/exp/exp96.sh, B = 4096:
    // ROCKETLANDING 94.5 -> 70.4 ms, CARTPOLE's twin 192 -> 146 ms, ROCKETLANDING's twin 397 -> 311 ms; with four one-wavefront workgroups per CU the
    // one-wavefront form wins as before -- BEARPOPULATIONS 9.6 against 14.9 ms).
    // The same holds for every system once the horizon is long enough (exp100.sh, the headline system, B = 4096: N = 150 -- two workgroups per CU in either form --
    // 34.1 -> 27.2 ms; N = 300 -- one -- 130.9 -> 88.2 ms; N = 200, where two one-wavefront workgroups fit but only one of two wavefronts, stays: 46.3 against 57.7 ms).
    if constexpr (HsFused<Sys, 2, SCHEME>::SUPPORTED) {
      const int N = h->d.intervals;
      if (HsFused<Sys, 2, SCHEME>::lds_bytes(N) <= 160 * 1024) {
        int pc1 = 0, pc2 = 0;
        if (int rc = kernel_blocks_per_cu(h, reinterpret_cast<const void*>(hs_solve_fused_kernel<Sys, 1, SCHEME>), 64, HsFused<Sys, 1, SCHEME>::lds_bytes(N), &pc1)) return rc;
        if (int rc = kernel_blocks_per_cu(h, reinterpret_cast<const void*>(hs_solve_fused_kernel<Sys, 2, SCHEME>), 128, HsFused<Sys, 2, SCHEME>::lds_bytes(N), &pc2)) return rc;
        if (pc1 >= 1 && pc1 <= 2 && pc2 >= pc1) waves = 2;
      }
    }
    if (a.so.park_iter > 0) waves = 1;                // an explicit two-phase launch: only the one-wavefront form parks (include/myriad_hip.h: park_iter)
    if (h->fused_waves > 0) waves = h->fused_waves;
    if (waves > 2) waves = 2;
    if (waves == 2 && HsFused<Sys, 2, SCHEME>::lds_bytes(h->d.intervals) <= 160 * 1024)
      return launch_hs_fused_w<Sys, 2, SCHEME>(h, a);
    return launch_hs_fused_w<Sys, 1, SCHEME>(h, a);
  }
}

template <class Sys, int SCHEME = 0>
static int launch_hs_solve(myr_handle h, const SolveCall& a) {
  const int N = h->d.intervals, B = a.B;
  // one trajectory per wavefront while its LDS working set fits a CU (N <= ~480 for CARTPOLE); beyond that the
  // lane-per-trajectory form, which keeps everything in global scratch, takes over
  if constexpr (HsFused<Sys, 1, SCHEME>::SUPPORTED && !(SCHEME == 1 && NodeTraits<Sys>::mlp)) {
    if (h->solve_mode == 1 && h->solve_fused && HsFused<Sys, (NodeTraits<Sys>::mlp ? 4 : 1), SCHEME>::lds_bytes(N) <= 160 * 1024)
      return launch_hs_fused<Sys, SCHEME>(h, a);
  }
  // (Round 3 kept the trapezoidal scheme with more than one control or more than four states off the wavefront kernel: its general
  // sweep read the end point's Hessian record at the Hermite-Simpson stride -- point 2k + 2 instead of k + 1 -- and BEARPOPULATIONS
  // ended in NaN.  Fixed in HsWave::riccati (H_PTS); MYRIAD_TRAP_GENERAL_WAVE=0 sends those systems to the lane form again.)
  static const bool trap_general_wave = [] { const char* e = getenv("MYRIAD_TRAP_GENERAL_WAVE"); return !(e && atoi(e) == 0); }();
  const bool wave_ok = !(SCHEME == 1 && !(Sys::NU == 1 && Sys::NS <= 4)) || trap_general_wave;
  // (ROCKETLANDING's twin, 14 variables per point: round 2's kernel -- minutes of build time, a 16 x 16 factor per lane and stage -- is not built any more
  //  now that the fused kernel serves it; beyond the fused kernel's LDS limit it runs on the lane kernel)
  constexpr bool round2_built = !(Sys::ID >= 100 && Sys::NW > 9 && HsFused<Sys, 1, SCHEME>::SUPPORTED);
  if constexpr (round2_built)
  if (wave_ok)
  if (h->solve_mode == 1 && HsWave<Sys, SCHEME>::lds_bytes(N) <= 160 * 1024) {
    using W = HsWave<Sys, SCHEME>;
    // wavefronts per workgroup: 1, except network systems -- independent solves that share the 40 KB of weights in LDS, four to a
    // workgroup (4 x 24 + 40 KB), or, for batches smaller than the number of CUs, ONE solve whose network passes the four share
    int wpb = 1, coop = 0;
    if (W::MLP) {
      const int cus = device_cus(h);
      // Small batches: the wavefronts of a workgroup share one trajectory's network passes (cooperative mode) -- four per
      // trajectory up to one trajectory per CU, two up to two per CU (two such workgroups fit a CU), four again up to four per
      // CU (the workgroup takes its trajectories one after the other); beyond that independent solves, four per workgroup.
      // Measured on one box (B: independent / coop 2 / coop 4 ms): 512: 50.8 / 34.5 / 42.3, 1024: 91.3 / 84.6 / 82.5,
      // 2048: 104.4 / 113.5 / 144.8.
      coop = (B <= 4 * cus) ? 1 : 0;
      int coop_wpb = (B > cus && B <= 2 * cus) ? 2 : W::WPB_MAX;
      if (const char* e = getenv("MYRIAD_NODE_COOP")) coop = atoi(e) != 0;
      if (coop || a.pstride == 0) {
        wpb = coop ? coop_wpb : W::WPB_MAX;
        if (const char* e = getenv("MYRIAD_NODE_WPB")) { wpb = atoi(e); if (wpb < 1) wpb = 1; if (wpb > W::WPB_MAX) wpb = W::WPB_MAX; }
        while (!coop && wpb > 1 && ((size_t)wpb * W::lds_solver_doubles(N) + NodeTraits<Sys>::lds_doubles) * 8 > 160 * 1024) --wpb;
      }
      if (wpb == 1) coop = 0;
    }
    const int lwaves = coop ? 1 : wpb;                          // solves per workgroup
    const size_t lds = ((size_t)lwaves * W::lds_solver_doubles(N) + NodeTraits<Sys>::lds_doubles + (coop ? W::COOP_CMD_DOUBLES : 0)) * 8;
    auto kern = hs_solve_wave_kernel<Sys, SCHEME>;
    int per_cu = 0;
    if (int rc = kernel_blocks_per_cu(h, reinterpret_cast<const void*>(kern), 64 * wpb, lds, &per_cu)) return rc;
    // Persistent form: as many workgroups as the device keeps resident (registers and LDS allow 4 wavefronts per CU), each
    // pulling trajectories from a ticket counter.  Scratch belongs to the SLOT, not to the trajectory: the working set of
    // a launch is slots x 273 KB (280 MB for CARTPOLE N=100) instead of B x 273 KB (1.1 GB at B = 4096) and is re-used
    // trajectory after trajectory, i.e. it stays in the 256 MB Infinity Cache instead of streaming through HBM.
    int slots = default_slots(h, per_cu, 4, lwaves);             // wavefronts
    if (slots > B) slots = B;
    slots = (slots + lwaves - 1) / lwaves * lwaves;              // whole workgroups (surplus wavefronts find the ticket counter exhausted)
    const long stride = slot_stride(W::scratch_doubles(N));
    const size_t need = (size_t)slots * (size_t)stride * 8;
    if (getenv("MYRIAD_DEBUG_PTRS"))
      fprintf(stderr, "[myriad] wave kernel N=%d B=%d slots=%d wpb=%d coop=%d per_cu=%d lds=%zu stride=%ld doubles need=%zu\n", N, B, slots, wpb, coop, per_cu, lds, stride, need);
    if (int rc = ensure_buf(&h->sbuf, &h->sbuf_bytes, need)) return rc;
    if (int rc = reset_ticket(h)) return rc;
    HsSolveOpts o = make_opts(h, a.so);
    if (int rc = timed_begin(h, MYR_K_SOLVE)) return rc;
    h->last_solve_form = 1;
    set_plan(h, 2, coop ? wpb : 1, 0, 1, slots, 0);
    hipLaunchKernelGGL(kern, dim3((unsigned)(slots / lwaves)), dim3(64 * wpb), lds, h->stream, B, h->ticket, o, h->vscale, a.z, a.lb, a.ub, a.lam, (double*)h->sbuf, stride,
                       a.params, a.pstride, a.cost, a.status, a.iters, a.kkt, coop, h->poison);
    return timed_end(h, MYR_K_SOLVE);
  }
  return solve_lane_colloc_for_system<Sys, SCHEME>(h, a);
}

// lane-per-trajectory path, any sweep core (Hermite-Simpson, trapezoidal, shooting)
template <class Core, class Sys>
static int launch_lane_solve(myr_handle h, const SolveCall& a, long nst) {
  const myr_dims& dm = h->dims;
  const int B = a.B;
  const long Bp = padded_lanes(B);
  const long n = dm.n, m = dm.m;
  if (int rc = ensure_buf(&h->sbuf, &h->sbuf_bytes, (size_t)Bp * (size_t)(6 * n + m + nst) * 8)) return rc;
  double* sz = (double*)h->sbuf;
  double* slb = sz + n * Bp;
  double* sub = slb + n * Bp;
  double* szL = sub + n * Bp;
  double* szU = szL + n * Bp;
  double* sdz = szU + n * Bp;
  double* slam = sdz + n * Bp;
  double* sst = slam + m * Bp;
  // padded lanes read garbage-free memory
  HIPCHK(hipMemsetAsync(h->sbuf, 0, (size_t)Bp * (size_t)(3 * n) * 8, h->stream));
  dim3 tb(256), tg((unsigned)((n + 31) / 32), (unsigned)((B + 31) / 32));
  hipLaunchKernelGGL(transpose_kernel, tg, tb, 0, h->stream, (const double*)a.z, sz, B, (int)n, Bp);
  hipLaunchKernelGGL(transpose_kernel, tg, tb, 0, h->stream, a.lb, slb, B, (int)n, Bp);
  hipLaunchKernelGGL(transpose_kernel, tg, tb, 0, h->stream, a.ub, sub, B, (int)n, Bp);
  HsSolveOpts o = make_opts(h, a.so);
  if (int rc = timed_begin(h, MYR_K_SOLVE)) return rc;
  const int lpw = h->solve_lpw;
  h->last_solve_form = 0;
  set_plan(h, 0, 0, 0, 1, B, 0);
  hipLaunchKernelGGL((lane_solve_kernel<Core, Sys>), dim3((unsigned)((B + lpw - 1) / lpw)), dim3(64), 0, h->stream, B, Bp, lpw, o, h->vscale, sz, slb, sub, szL,
                     szU, slam, sdz, sst, a.params, a.pstride, a.cost, a.status, a.iters, a.kkt);
  if (int rc = timed_stop(h, MYR_K_SOLVE)) return rc;      // the kernel alone is timed: the transposes back come behind the stop event
  hipLaunchKernelGGL(transpose_back_kernel, tg, tb, 0, h->stream, (const double*)sz, a.z, B, (int)n, Bp);
  if (a.lam) {
    dim3 tgl((unsigned)((m + 31) / 32), (unsigned)((B + 31) / 32));
    hipLaunchKernelGGL(transpose_back_kernel, tgl, tb, 0, h->stream, (const double*)slam, a.lam, B, (int)m, Bp);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return timed_account(h, MYR_K_SOLVE);
}

// shooting, one trajectory per wavefront (shoot_solver_wave.h) while the iterate fits the LDS of a CU; else the lane form
template <class Sys, int M>
static int launch_shoot_solve(myr_handle h, const SolveCall& a) {
  const int N = h->d.intervals, cpi = h->d.controls_per_interval;
  using W = ShootWave<Sys, M>;
  const size_t lds = W::lds_bytes(N, cpi);
  if (h->solve_mode != 1 || lds > 160 * 1024)
    return launch_lane_solve<ShootCore<Sys, M>, Sys>(h, a, ShootCore<Sys, M>::stage_doubles(N, cpi));
  auto kern = shoot_solve_wave_kernel<Sys, M>;
  int per_cu = 0;
  if (int rc = kernel_blocks_per_cu(h, reinterpret_cast<const void*>(kern), 64, lds, &per_cu)) return rc;
  int slots = default_slots(h, per_cu, 4);
  if (slots > a.B) slots = a.B;
  if (int rc = reset_ticket(h)) return rc;
  HsSolveOpts o = make_opts(h, a.so);
  // network systems: records, activations and tangents of the matrix-core passes, per resident workgroup (shoot_solver_wave.h: mlp_scratch_doubles)
  const long sdoubles = W::mlp_scratch_doubles(N, cpi);
  const long sstride = sdoubles > 0 ? slot_stride(sdoubles) : 0;
  if (sstride > 0)
    if (int rc = ensure_buf(&h->sbuf, &h->sbuf_bytes, (size_t)slots * (size_t)sstride * 8)) return rc;
  if (int rc = timed_begin(h, MYR_K_SOLVE)) return rc;
  h->last_solve_form = 1;
  set_plan(h, 3, 1, 0, 1, slots, 0);
  hipLaunchKernelGGL(kern, dim3((unsigned)slots), dim3(64), lds, h->stream, a.B, h->ticket, o, h->vscale, a.z, a.lb, a.ub, a.lam, a.params, a.pstride,
                     a.cost, a.status, a.iters, a.kkt, h->poison, sstride > 0 ? (double*)h->sbuf : (double*)nullptr, sstride);
  return timed_end(h, MYR_K_SOLVE);
}

// One function template per transcription, so that the build can give each its own object (MYR_TU_PART below: the solver kernels of a wide system
// are minutes of compile time per scheme).
template <class Sys, int SCHEME>
int solve_lane_colloc_for_system(myr_handle h, const SolveCall& a) {
  const int N = h->d.intervals;
  if constexpr (SCHEME == 1) {
    if constexpr (Sys::PARAMS_BY_POINTER) return fail(MYR_E_UNSUPPORTED, "myr_solve: NODE systems are built for HERMITE_SIMPSON");
    else return launch_lane_solve<TrapCore<Sys>, Sys>(h, a, TrapCore<Sys>::stage_doubles(N));
  } else
    return launch_lane_solve<HsSolver<Sys>, Sys>(h, a, HsSol<Sys>::stage_doubles(N));
}
template <class Sys>
int solve_hs_for_system(myr_handle h, const SolveCall& a) {
  return launch_hs_solve<Sys>(h, a);
}
template <class Sys>
int solve_trap_for_system(myr_handle h, const SolveCall& a) {      // wavefront form (falls back to the lane form for MYRIAD_SOLVE_MODE=lane / very large N)
  if constexpr (Sys::PARAMS_BY_POINTER) return fail(MYR_E_UNSUPPORTED, "myr_solve: NODE systems are built for HERMITE_SIMPSON");
  // (a twin too wide for the fused kernel's block sweep would cost minutes of build time per solver on round 2's kernel: refused; no twin is, since round 5)
  else if constexpr (Sys::ID >= 100 && Sys::NW > 9 && !HsFused<Sys, 1, 1>::SUPPORTED) return fail(MYR_E_UNSUPPORTED, "myr_solve: the trapezoidal solver of this elastic twin is not built");
  else return launch_hs_solve<Sys, 1>(h, a);
}
template <class Sys>
int solve_shoot_for_system(myr_handle h, const SolveCall& a) {
  // elastic twins (id >= 100) exist for the collocation solvers, whose restoration device they are; their shooting solver is not built
  if constexpr (Sys::ID >= 100) return fail(MYR_E_UNSUPPORTED, "myr_solve: elastic twins are built for the collocation transcriptions");
  else {
    if (h->d.integration_method == MYR_INT_RK4)
      return launch_shoot_solve<Sys, 2>(h, a);
    return launch_shoot_solve<Sys, 1>(h, a);
  }
}
#if defined(MYR_TU_SYSTEM) && defined(MYR_TU_PART)      // the scheme solvers this object does not hold: no implicit instantiation
#if MYR_TU_PART != 1
extern template int solve_hs_for_system<myriad::MYR_TU_SYSTEM>(myr_handle, const SolveCall&);
#endif
#if MYR_TU_PART != 3
extern template int solve_trap_for_system<myriad::MYR_TU_SYSTEM>(myr_handle, const SolveCall&);
#endif
#if MYR_TU_PART != 4
extern template int solve_shoot_for_system<myriad::MYR_TU_SYSTEM>(myr_handle, const SolveCall&);
#endif
#endif
template <class Sys>
int solve_for_system(myr_handle h, const SolveCall& a) {
  switch (h->d.transcription) {
    case MYR_TR_HERMITE_SIMPSON: return solve_hs_for_system<Sys>(h, a);
    case MYR_TR_TRAPEZOIDAL: return solve_trap_for_system<Sys>(h, a);
    case MYR_TR_SHOOTING: return solve_shoot_for_system<Sys>(h, a);
  }
  return fail(MYR_E_ARG, "solve: unknown transcription");
}

// ------------------------------------------------------------------------------------------------
// rollout
// ------------------------------------------------------------------------------------------------
template <class Sys>
__global__ __launch_bounds__(64)
void rollout_kernel(int B, int method, int num_steps, double h, int u_rows, const double* __restrict__ x0,
                    const double* __restrict__ us, const double* __restrict__ params, int params_stride,
                    double* __restrict__ xs, double* __restrict__ cost) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  SysParams<Sys> pp;
  pp.load(params, b, params_stride);
  const double* p = pp.get();
  const double c = Rollout<Sys>::run(method, num_steps, h, u_rows, x0 + b * Sys::NS, us + b * (long)u_rows * Sys::NU, p,
                                     xs ? xs + b * (long)(num_steps + 1) * Sys::NS : nullptr);
  if (cost) cost[b] = c;
}

// ------------------------------------------------------------------------------------------------
// batched Forward-Backward Sweep (indirect method)
// ------------------------------------------------------------------------------------------------
template <class Sys>
int launch_fbsm(myr_handle h, const FbsmArgs& a) {
  if constexpr (!Indirect<Sys>::SUPPORTED) {
    return fail(MYR_E_UNSUPPORTED, "myr_fbsm: this system has no adjoint dynamics (not an IndirectFHCS on the path)");
  } else {
    if (int rc = timed_begin(h, MYR_K_FBSM)) return rc;
    hipLaunchKernelGGL(fbsm_kernel<Sys>, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, h->stream, a.B, a.Bp, a.N, h->d.T, a.x0, a.adjT, a.params,
                       a.pstride, a.lo, a.hi, a.bang, a.delta, a.max_sweeps, a.X, a.U, a.A, a.sweeps);
    return timed_end(h, MYR_K_FBSM);
  }
}

template <class Sys>
int rollout_for_system(myr_handle h, const RolloutArgs& a) {
  hipLaunchKernelGGL(rollout_kernel<Sys>, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, h->stream, a.B, (int)h->d.integration_method, a.num_steps,
                     h->d.T / a.num_steps, a.u_rows, a.x0, a.us, a.params, a.pstride, a.xs, a.cost);
  return MYR_OK;
}

// ------------------------------------------------------------------------------------------------
// trajectory-matching loss and its parameter gradient (fit.h: fit_lane_kernel, node_fit_kernel)
// ------------------------------------------------------------------------------------------------
// A system without generated parameter derivatives (the elastic twins): the one text for it.  The entry points refuse such a handle before anything is
// launched (check_fit_has_derivatives); the two launchers below keep the branch because FitLane does not compile for such a system.
static inline int fit_no_derivatives() { return fail(MYR_E_UNSUPPORTED, "myr_fit_grad: no parameter derivatives are generated for this system"); }

template <class Sys>
int fit_for_system(myr_handle h, const FitArgs& a) {
  if constexpr (std::is_same<Sys, SysNODE_CARTPOLE>::value) {      // a set of weights per workgroup (never per trajectory: myr_fit_grad has checked), one wavefront per trajectory
    const unsigned per_set = (unsigned)((a.R + NodeFit::WPB - 1) / NodeFit::WPB);
    if (a.mode == FIT_GNVP)
      hipLaunchKernelGGL(node_fit_gnvp_kernel<NodeFit>, dim3((unsigned)a.E * per_set), dim3(64 * NodeFit::WPB), 0, h->stream, a.R, a.data_shared, a.Bp,
                         (int)h->d.integration_method, a.num_steps, h->d.T / a.num_steps, a.u_rows, a.xs_obs, a.us, a.wt, a.params, a.v, a.xh, a.dxh, a.jv,
                         a.grad);
    else
      hipLaunchKernelGGL(node_fit_kernel<NodeFit>, dim3((unsigned)a.E * per_set), dim3(64 * NodeFit::WPB), 0, h->stream, a.R, a.data_shared, a.Bp,
                         (int)h->d.integration_method, a.num_steps, h->d.T / a.num_steps, a.u_rows, a.xs_obs, a.us, a.wt, a.params, a.xh, a.loss, a.grad);
    return MYR_OK;
  } else if constexpr (!SysDp<Sys>::SUPPORTED) {
    return fit_no_derivatives();
  } else {
    const long B = (long)a.E * a.R;
    hipLaunchKernelGGL(fit_lane_kernel<Sys>, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, (int)B, a.R, a.per_row ? 1 : a.R, a.data_shared, a.Bp,
                       (int)h->d.integration_method, a.num_steps, h->d.T / a.num_steps, a.u_rows, a.xs_obs, a.us, a.wt, a.params, a.xh, a.loss, a.grad);
    return MYR_OK;
  }
}

// ... and with the Gauss-Newton matrix, by forward sensitivities (fit_gn.h: fit_gn_lane_kernel).  myr_fit_gn* have refused the network system
// (check_fit_gn_not_node), which has no SysDp either
template <class Sys>
int fit_gn_for_system(myr_handle h, const FitArgs& a) {
  if constexpr (!SysDp<Sys>::SUPPORTED) {
    return fit_no_derivatives();
  } else {
    const long B = (long)a.E * a.R;
    hipLaunchKernelGGL(fit_gn_lane_kernel<Sys>, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, (int)B, a.R, a.per_row ? 1 : a.R, a.data_shared,
                       (int)h->d.integration_method, a.num_steps, h->d.T / a.num_steps, a.u_rows, a.xs_obs, a.us, a.wt, a.params, a.loss, a.grad, a.grad_ld,
                       a.gn, a.gn_ld);
    return MYR_OK;
  }
}

// ------------------------------------------------------------------------------------------------
// derivative of the unrolled extragradient steps in the model parameters (exgd_grad.h: colloc_exgd_grad_kernel)
// ------------------------------------------------------------------------------------------------
// The batch in chunks of a.chunk instances that share one history buffer (launches on one stream: a chunk starts when the one before has ended).
// `launch` gets the chunk's record: B its instances, inst0 the number of its first one in the call, every batch pointer at that instance (null stays
// null; params advances by pstride -- the network routes pass pstride 0 and find an instance's weight set from inst0 and R: blockIdx.x restarts at 0
// in every chunk, and a chunk may begin and end inside a set)
template <class F>
static int for_exgd_grad_chunks(myr_handle h, const ExgdGradArgs& a, F launch) {
  const myr_dims& dm = h->dims;
  for (long b0 = 0; b0 < a.B; b0 += a.chunk) {
    auto at = [b0](auto* p, long stride) { return p ? p + b0 * stride : nullptr; };
    ExgdGradArgs c = a;
    c.B = (int)(a.B - b0 < a.chunk ? a.B - b0 : a.chunk);
    c.inst0 = (int)b0;
    c.z = at(a.z, dm.n); c.lam = at(a.lam, dm.m); c.lb = at(a.lb, dm.n); c.ub = at(a.ub, dm.n); c.params = at(a.params, a.pstride);
    c.seed_z = at(a.seed_z, dm.n); c.seed_lam = at(a.seed_lam, dm.m);
    c.rows = at(a.rows, dm.np); c.dz0 = at(a.dz0, dm.n); c.dlam0 = at(a.dlam0, dm.m);
    if (int rc = launch(c)) return rc;
  }
  return MYR_OK;
}

template <class Sys, int SCHEME>
static int launch_exgd_grad(myr_handle h, const ExgdGradArgs& a) {
  const int N = h->d.intervals;
  const size_t lds = colloc_exgd_grad_lds_bytes<Sys, SCHEME>(N);
  if (lds > 160 * 1024) return fail(MYR_E_CAPACITY, "myr_exgd_grad: intervals too large for the LDS-resident reverse sweep");
  auto kern = colloc_exgd_grad_kernel<Sys, SCHEME>;
  // (the limit is a property of the FUNCTION, shared by every handle of the process: the hardware's 160 KB, not this handle's size -- kernel_blocks_per_cu)
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return for_exgd_grad_chunks(h, a, [&](const ExgdGradArgs& c) {
    hipLaunchKernelGGL(kern, dim3((unsigned)c.B), dim3(64), lds, h->stream, c.B, N, h->d.T / N, c.z, c.lam, c.lb, c.ub, c.params, c.pstride, c.eta_x,
                       c.eta_v, c.nsteps, c.seed_z, c.seed_lam, c.hist, c.rows, c.dz0, c.dlam0);
    return (int)MYR_OK;
  });
}

template <class Sys>
int exgd_grad_for_system(myr_handle h, const ExgdGradArgs& a) {
  // myr_exgd_grad has refused the twins, the network system and SHOOTING, each with its own message; the constexpr keeps their kernels out of the build
  if constexpr (SysDpw<Sys>::SUPPORTED) {
    if (h->d.transcription == MYR_TR_HERMITE_SIMPSON) return launch_exgd_grad<Sys, PROD_HS>(h, a);
    if (h->d.transcription == MYR_TR_TRAPEZOIDAL) return launch_exgd_grad<Sys, PROD_TRAP>(h, a);
  }
  return fail(MYR_E_UNSUPPORTED, "myr_exgd_grad: not built for this system and transcription");
}

// the forward-mode Jacobian of the same steps (exgd_jac.h: colloc_exgd_jac_kernel), one launch: a wavefront per (instance, group of columns).  The
// columns run in the fewest groups of equal size whose LDS record -- the iterate's and one of the same size per column -- fits the budget: the
// hardware's 160 KB, or less where MYRIAD_EXGD_JAC_LDS_BYTES says so (tests: the grouped path)
template <class Sys, int SCHEME>
static int launch_exgd_jac(myr_handle h, const ExgdGradArgs& a) {
  const int N = h->d.intervals, NP = Sys::NP;
  size_t budget = 160 * 1024;
  if (const char* e = getenv("MYRIAD_EXGD_JAC_LDS_BYTES")) { const long long v = atoll(e); if (v > 0 && (size_t)v < budget) budget = (size_t)v; }
  int cap = 0;
  while (cap < NP && colloc_exgd_jac_lds_bytes<Sys, SCHEME>(N, cap + 1) <= budget) ++cap;
  if (cap < 1)
    return fail(MYR_E_CAPACITY, "myr_exgd_jac: the iterate and one tangent column do not fit in LDS (" +
                                    std::to_string(colloc_exgd_jac_lds_bytes<Sys, SCHEME>(N, 1)) + " bytes of " + std::to_string(budget) +
                                    "); use fewer intervals, or myr_exgd_grad for seeded rows");
  const int groups = (NP + cap - 1) / cap, gcols = (NP + groups - 1) / groups;
  auto kern = colloc_exgd_jac_kernel<Sys, SCHEME>;
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  const size_t lds = colloc_exgd_jac_lds_bytes<Sys, SCHEME>(N, gcols);
  hipLaunchKernelGGL(kern, dim3((unsigned)a.B, (unsigned)((NP + gcols - 1) / gcols)), dim3(64), lds, h->stream,
                     a.B, N, h->d.T / N, a.z, a.lam, a.lb, a.ub, a.params, a.pstride, a.eta_x, a.eta_v, a.nsteps, a.jz0, a.jlam0, a.zn, a.lamn, a.jz,
                     a.jlam, gcols);
  return MYR_OK;
}

template <class Sys>
int exgd_jac_for_system(myr_handle h, const ExgdGradArgs& a) {
  // myr_exgd_jac has refused the twins, the network system and SHOOTING, each with its own message; the constexpr keeps their kernels out of the build
  if constexpr (SysDpw<Sys>::SUPPORTED) {
    if (h->d.transcription == MYR_TR_HERMITE_SIMPSON) return launch_exgd_jac<Sys, PROD_HS>(h, a);
    if (h->d.transcription == MYR_TR_TRAPEZOIDAL) return launch_exgd_jac<Sys, PROD_TRAP>(h, a);
  }
  return fail(MYR_E_UNSUPPORTED, "myr_exgd_jac: not built for this system and transcription");
}

// the same derivative in the weights of the network system (node_exgd_grad.h: node_exgd_grad_kernel; myr_exgd_grad_node has checked system and transcription)
template <int WPI>
static int launch_node_exgd_grad(myr_handle h, const ExgdGradArgs& a) {
  const int N = h->d.intervals;
  const size_t lds = node_exgd_grad_lds_bytes(N);
  auto kern = node_exgd_grad_kernel<WPI>;
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return for_exgd_grad_chunks(h, a, [&](const ExgdGradArgs& c) {      // (params: the call's weight sets, pstride 0)
    hipLaunchKernelGGL(kern, dim3((unsigned)c.B), dim3(64 * WPI), lds, h->stream, c.B, N, h->d.T / N, c.z, c.lam, c.lb, c.ub, c.params, c.eta_x, c.eta_v,
                       c.nsteps, c.seed_z, c.seed_lam, c.hist, c.rows, c.dz0, c.dlam0, c.inst0, c.R);
    return (int)MYR_OK;
  });
}

template <class Sys>
int exgd_grad_node_for_system(myr_handle h, const ExgdGradArgs& a) {
  if constexpr (std::is_same<Sys, SysNODE_CARTPOLE>::value) {      // the kernel lives in the network system's object only
    switch (h->node_exgd_wpi) {      // (myr_exgd_grad_node has checked that the LDS record fits)
      case 1: return launch_node_exgd_grad<1>(h, a);
      case 2: return launch_node_exgd_grad<2>(h, a);
      default: return launch_node_exgd_grad<4>(h, a);
    }
  }
  return fail(MYR_E_UNSUPPORTED, "myr_exgd_grad_node: the network system only; use myr_exgd_grad");
}

// ------------------------------------------------------------------------------------------------
// Lagrangian Hessian-vector product (colloc_hvp.h: colloc_hvp_kernel; shoot_hvp.h: shoot_hvp_kernel, shoot_hvp_gather_kernel)
// ------------------------------------------------------------------------------------------------
// myr_hvp has refused the twins and the network system, each with its own message; the constexpr keeps their kernels out of the build
template <class Sys>
int hvp_colloc_for_system(myr_handle h, const HvpArgs& a) {
  if constexpr (SysDpw<Sys>::SUPPORTED) {
    const int N = h->d.intervals;
    if (h->d.transcription == MYR_TR_HERMITE_SIMPSON)
      hipLaunchKernelGGL((colloc_hvp_kernel<Sys, PROD_HS>), dim3((unsigned)a.B), dim3(64), 0, h->stream, a.B, N, h->d.T / N, a.z, a.lam, a.v, a.params,
                         a.pstride, a.with_cost, a.out_z, a.rows);
    else
      hipLaunchKernelGGL((colloc_hvp_kernel<Sys, PROD_TRAP>), dim3((unsigned)a.B), dim3(64), 0, h->stream, a.B, N, h->d.T / N, a.z, a.lam, a.v, a.params,
                         a.pstride, a.with_cost, a.out_z, a.rows);
    return MYR_OK;
  }
  return fail(MYR_E_UNSUPPORTED, "myr_hvp: not built for this system");
}

template <class Sys, int M>
static int launch_shoot_hvp(myr_handle h, const HvpArgs& a) {
  const int I = h->d.intervals, cpi = h->d.controls_per_interval;
  const long P = (long)a.B * I;
  hipLaunchKernelGGL((shoot_hvp_kernel<Sys, M>), dim3((unsigned)((P + 63) / 64)), dim3(64), 0, h->stream, a.B, a.Pp, I, cpi, (int)h->d.integration_method,
                     h->d.T, a.z, a.lam, a.v, a.params, a.pstride, a.with_cost, a.hist, a.side);
  hipLaunchKernelGGL((shoot_hvp_gather_kernel<Sys, M>), dim3(grid_for((long)a.B * (h->dims.n + h->dims.np))), dim3(256), 0, h->stream, a.B, a.Pp, I, cpi,
                     (const double*)a.side, a.out_z, a.rows);
  return MYR_OK;
}

template <class Sys>
int hvp_shoot_for_system(myr_handle h, const HvpArgs& a) {
  if constexpr (SysDpw<Sys>::SUPPORTED)
    return h->d.integration_method == MYR_INT_RK4 ? launch_shoot_hvp<Sys, 2>(h, a) : launch_shoot_hvp<Sys, 1>(h, a);
  return fail(MYR_E_UNSUPPORTED, "myr_hvp: not built for this system");
}

// ------------------------------------------------------------------------------------------------
// derivative of the unrolled extragradient steps under SHOOTING (shoot_exgd_grad.h: the seeded pair pass and the mask pass behind it)
// ------------------------------------------------------------------------------------------------
template <class Sys, int M>
static int launch_shoot_exgd_grad(myr_handle h, const ExgdGradArgs& a) {
  using HV = ShootHvp<Sys, M>;
  using G = ShootExgdGrad<Sys, M>;
  const int I = h->d.intervals, cpi = h->d.controls_per_interval, method = h->d.integration_method;
  const long n = h->dims.n, m = h->dims.m, np = h->dims.np, C = a.chunk, Pp = a.Pp;
  // the chunk's scratch: the iterate of the forward steps and what they need, a_x, the direction, and a column per pair of a_lam, history and side record
  double* zio = a.work;            double* lamio = zio + C * n;     double* g = lamio + C * m;      double* zbar = g + C * n;
  double* cbuf = zbar + C * n;     double* scr = cbuf + C * m;      double* ax = scr + C * (long)(cpi + 1) * Sys::NS;
  double* dir = ax + C * n;        double* al = dir + C * n;        double* phist = al + Pp * Sys::NS;
  double* side = phist + Pp * HV::hist_doubles(cpi);
  return for_exgd_grad_chunks(h, a, [&](const ExgdGradArgs& c) {
    const int nb = c.B;
    const long P = (long)nb * I, tz = (long)nb * n, tl = (long)nb * m, hs = 2 * tz + tl;
    if (int rc = copy_doubles(h, zio, c.z, tz)) return rc;
    if (int rc = copy_doubles(h, lamio, c.lam, tl)) return rc;
    if (int rc = shoot_exgd_steps<Sys, M>(h, nb, zio, lamio, c.lb, c.ub, c.params, c.pstride, c.eta_x, c.eta_v, c.nsteps, scr, g, zbar, cbuf, c.hist)) return rc;
    if (int rc = copy_doubles(h, ax, c.seed_z, tz)) return rc;
    hipLaunchKernelGGL(shoot_exgd_grad_lam_kernel, dim3(grid_for(Pp * Sys::NS + tz + nb * np)), dim3(256), 0, h->stream, 1, nb, Pp, I, (int)Sys::NS, n, (int)np,
                       c.seed_lam, al, dir, c.rows, (double*)nullptr);
    for (int ps = 0; ps < G::passes(c.nsteps); ++ps) {      // (the pass at x_n runs on the direction the kernel above has cleared)
      const typename G::Pass q = G::pass_of(ps, c.nsteps, c.eta_v);
      const double* H = c.hist + q.s * hs;
      const double* pt = q.at_bar ? H + tz : H;
      hipLaunchKernelGGL((shoot_exgd_grad_pair_kernel<Sys, M>), dim3((unsigned)((P + 63) / 64)), dim3(64), 0, h->stream, nb, Pp, I, cpi, method, h->d.T, pt,
                         q.alone ? (const double*)nullptr : H + 2 * tz, (const double*)dir, c.params, c.pstride, q.scale, al, phist, side);
      hipLaunchKernelGGL((shoot_exgd_grad_mask_kernel<Sys, M>), dim3(grid_for(tz + nb * np)), dim3(256), 0, h->stream, nb, Pp, I, cpi, q.mode, q.scale,
                         c.eta_x, (const double*)side, (const double*)al, pt, c.lb, c.ub, ax, dir, c.rows);
    }
    if (c.dz0)
      if (int rc = copy_doubles(h, c.dz0, ax, tz)) return rc;
    if (c.dlam0)
      hipLaunchKernelGGL(shoot_exgd_grad_lam_kernel, dim3(grid_for(P * Sys::NS)), dim3(256), 0, h->stream, 0, nb, Pp, I, (int)Sys::NS, n, (int)np,
                         (const double*)nullptr, al, (double*)nullptr, (double*)nullptr, c.dlam0);
    return (int)MYR_OK;
  });
}

// doubles of `work` for a chunk of C instances with Pp pair columns (the carve of launch_shoot_exgd_grad)
static size_t shoot_exgd_grad_work_doubles(myr_handle h, size_t C, size_t Pp) {
  const myr_dims& dm = h->dims;
  const size_t cpi = h->d.controls_per_interval, Mr = h->d.integration_method == MYR_INT_RK4 ? 2 : 1;
  return C * (5 * (size_t)dm.n + 2 * (size_t)dm.m + (cpi + 1) * dm.ns) + Pp * (dm.ns + cpi * 2 * dm.ns + dm.ns + (Mr * cpi + 1) * dm.nu + dm.np);
}

// myr_exgd_grad_shoot has refused the twins, the network system and the collocation transcriptions, each with its own message
template <class Sys>
int exgd_grad_shoot_for_system(myr_handle h, const ExgdGradArgs& a) {
  if constexpr (SysDpw<Sys>::SUPPORTED)
    return h->d.integration_method == MYR_INT_RK4 ? launch_shoot_exgd_grad<Sys, 2>(h, a) : launch_shoot_exgd_grad<Sys, 1>(h, a);
  return fail(MYR_E_UNSUPPORTED, "myr_exgd_grad_shoot: not built for this system");
}

// ------------------------------------------------------------------------------------------------
// derivative of the unrolled extragradient steps in the weights of the network system under SHOOTING (node_shoot_exgd_grad.h: one launch per chunk;
// myr_exgd_grad_node_shoot has checked system, transcription and that the LDS carve fits)
// ------------------------------------------------------------------------------------------------
template <int M>
static int launch_node_shoot_exgd_grad(myr_handle h, const ExgdGradArgs& a) {
  const int I = h->d.intervals, cpi = h->d.controls_per_interval;
  const size_t lds = node_shoot_exgd_grad_lds_bytes<M>(I, cpi);
  const int wpi = node_shoot_exgd_grad_wpi(I);
  auto kern = node_shoot_exgd_grad_kernel<M>;
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return for_exgd_grad_chunks(h, a, [&](const ExgdGradArgs& c) {
    NseArgs k{};
    k.B = c.B; k.I = I; k.cpi = cpi; k.method = (int)h->d.integration_method; k.nsteps = c.nsteps; k.inst0 = c.inst0; k.R = c.R;
    k.T = h->d.T; k.eta_x = c.eta_x; k.eta_v = c.eta_v;
    k.z = c.z; k.lam = c.lam; k.lb = c.lb; k.ub = c.ub; k.params = c.params; k.seed_z = c.seed_z; k.seed_lam = c.seed_lam;
    k.hist = c.hist; k.grad = c.rows; k.dz0 = c.dz0; k.dlam0 = c.dlam0;
    hipLaunchKernelGGL(kern, dim3((unsigned)k.B), dim3(64 * wpi), lds, h->stream, k);
    return (int)MYR_OK;
  });
}

template <class Sys>
int exgd_grad_node_shoot_for_system(myr_handle h, const ExgdGradArgs& a) {
  if constexpr (std::is_same<Sys, SysNODE_CARTPOLE>::value)      // the kernel lives in the network system's object only
    return h->d.integration_method == MYR_INT_RK4 ? launch_node_shoot_exgd_grad<2>(h, a) : launch_node_shoot_exgd_grad<1>(h, a);
  return fail(MYR_E_UNSUPPORTED, "myr_exgd_grad_node_shoot: the network system only; use myr_exgd_grad_shoot");
}

// ------------------------------------------------------------------------------------------------
// Lagrangian Hessian-vector product of the network system (node_hvp.h: node_hvp_colloc_kernel, node_hvp_shoot_kernel; myr_hvp_node has checked
// system, transcription and that the SHOOTING carve fits).  a.params [B / R][np]: a weight set for every R instances; a.pstride is not read
// ------------------------------------------------------------------------------------------------
template <class Sys>
int hvp_node_colloc_for_system(myr_handle h, const HvpArgs& a) {
  if constexpr (std::is_same<Sys, SysNODE_CARTPOLE>::value) {      // the kernel lives in the network system's object only
    constexpr int WPI = 4;
    const int N = h->d.intervals;
    hipLaunchKernelGGL(node_hvp_colloc_kernel<WPI>, dim3((unsigned)a.B), dim3(64 * WPI), node_hvp_colloc_lds_bytes(), h->stream, a.B, N, h->d.T / N, a.z,
                       a.lam, a.v, a.params, a.with_cost, a.out_z, a.rows, a.R);
    return MYR_OK;
  }
  return fail(MYR_E_UNSUPPORTED, "myr_hvp_node: the network system only; use myr_hvp");
}

template <int M>
static int launch_node_hvp_shoot(myr_handle h, const HvpArgs& a) {
  const int I = h->d.intervals, cpi = h->d.controls_per_interval;
  const size_t lds = node_hvp_shoot_lds_bytes<M>(I, cpi);
  auto kern = node_hvp_shoot_kernel<M>;
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  NodeHvpArgs k{};
  k.B = a.B; k.I = I; k.cpi = cpi; k.method = (int)h->d.integration_method; k.with_cost = a.with_cost; k.R = a.R; k.T = h->d.T;
  k.z = a.z; k.lam = a.lam; k.v = a.v; k.params = a.params; k.out_z = a.out_z; k.rows = a.rows;
  hipLaunchKernelGGL(kern, dim3((unsigned)k.B), dim3(64 * node_hvp_shoot_wpi(I)), lds, h->stream, k);
  return MYR_OK;
}

template <class Sys>
int hvp_node_shoot_for_system(myr_handle h, const HvpArgs& a) {
  if constexpr (std::is_same<Sys, SysNODE_CARTPOLE>::value)
    return h->d.integration_method == MYR_INT_RK4 ? launch_node_hvp_shoot<2>(h, a) : launch_node_hvp_shoot<1>(h, a);
  return fail(MYR_E_UNSUPPORTED, "myr_hvp_node: the network system only; use myr_hvp");
}

// ---- per-system entry points: explicit instantiation (system objects) / extern declaration (main object) -----------------
#define MYR_SYSTEM_ENTRY_POINTS(LINK, S)                                                                                          \
  LINK template int eval_for_system<S>(myr_handle, const EvalArgs&);          \
  LINK template int products_for_system<S>(myr_handle, const ProdArgs&);      \
  LINK template int solve_for_system<S>(myr_handle, const SolveCall&);        \
  LINK template int rollout_for_system<S>(myr_handle, const RolloutArgs&);    \
  LINK template int fit_for_system<S>(myr_handle, const FitArgs&);            \
  LINK template int fit_gn_for_system<S>(myr_handle, const FitArgs&);         \
  LINK template int exgd_grad_for_system<S>(myr_handle, const ExgdGradArgs&); \
  LINK template int exgd_grad_node_for_system<S>(myr_handle, const ExgdGradArgs&); \
  LINK template int exgd_jac_for_system<S>(myr_handle, const ExgdGradArgs&);  \
  LINK template int hvp_colloc_for_system<S>(myr_handle, const HvpArgs&);     \
  LINK template int hvp_shoot_for_system<S>(myr_handle, const HvpArgs&);      \
  LINK template int exgd_grad_shoot_for_system<S>(myr_handle, const ExgdGradArgs&); \
  LINK template int exgd_grad_node_shoot_for_system<S>(myr_handle, const ExgdGradArgs&); \
  LINK template int hvp_node_colloc_for_system<S>(myr_handle, const HvpArgs&); \
  LINK template int hvp_node_shoot_for_system<S>(myr_handle, const HvpArgs&); \
  LINK template int launch_fbsm<S>(myr_handle, const FbsmArgs&);
#if defined(MYR_TU_SYSTEM) && defined(MYR_TU_PART)
// a system's object in parts (the build splits the slow ones): -DMYR_TU_PART=1 the Hermite-Simpson wavefront solvers and the dispatch, 3 the trapezoidal
// wavefront solvers, 4 the shooting solvers, the shooting Hessian-vector products (closed-form and network) and the shooting derivatives of the extragradient steps (closed-form and network), 5 / 6 the lane kernels of the two collocation solvers, 2 everything else
#if MYR_TU_PART == 1
template int solve_hs_for_system<myriad::MYR_TU_SYSTEM>(myr_handle, const SolveCall&);
template int solve_for_system<myriad::MYR_TU_SYSTEM>(myr_handle, const SolveCall&);
#elif MYR_TU_PART == 3
template int solve_trap_for_system<myriad::MYR_TU_SYSTEM>(myr_handle, const SolveCall&);
#elif MYR_TU_PART == 4
template int solve_shoot_for_system<myriad::MYR_TU_SYSTEM>(myr_handle, const SolveCall&);
template int hvp_shoot_for_system<myriad::MYR_TU_SYSTEM>(myr_handle, const HvpArgs&);
template int exgd_grad_shoot_for_system<myriad::MYR_TU_SYSTEM>(myr_handle, const ExgdGradArgs&);
template int exgd_grad_node_shoot_for_system<myriad::MYR_TU_SYSTEM>(myr_handle, const ExgdGradArgs&);
template int hvp_node_shoot_for_system<myriad::MYR_TU_SYSTEM>(myr_handle, const HvpArgs&);
#elif MYR_TU_PART == 5
template int solve_lane_colloc_for_system<myriad::MYR_TU_SYSTEM, 0>(myr_handle, const SolveCall&);
#elif MYR_TU_PART == 6
template int solve_lane_colloc_for_system<myriad::MYR_TU_SYSTEM, 1>(myr_handle, const SolveCall&);
#else
#define MYR_SYSTEM_ENTRY_POINTS_REST(S)                                                                                            \
  template int eval_for_system<S>(myr_handle, const EvalArgs&);               \
  template int products_for_system<S>(myr_handle, const ProdArgs&);           \
  template int rollout_for_system<S>(myr_handle, const RolloutArgs&);         \
  template int fit_for_system<S>(myr_handle, const FitArgs&);                 \
  template int fit_gn_for_system<S>(myr_handle, const FitArgs&);              \
  template int exgd_grad_for_system<S>(myr_handle, const ExgdGradArgs&);      \
  template int exgd_grad_node_for_system<S>(myr_handle, const ExgdGradArgs&); \
  template int exgd_jac_for_system<S>(myr_handle, const ExgdGradArgs&);       \
  template int hvp_colloc_for_system<S>(myr_handle, const HvpArgs&);          \
  template int hvp_node_colloc_for_system<S>(myr_handle, const HvpArgs&);     \
  template int launch_fbsm<S>(myr_handle, const FbsmArgs&);
MYR_SYSTEM_ENTRY_POINTS_REST(myriad::MYR_TU_SYSTEM)
#endif
#elif defined(MYR_TU_SYSTEM)
MYR_SYSTEM_ENTRY_POINTS(, myriad::MYR_TU_SYSTEM)
#elif defined(MYR_TU_MAIN)
#define X(N) MYR_SYSTEM_ENTRY_POINTS(extern, Sys##N)
MYR_CLOSED_FORM_SYSTEMS(X)
#undef X
MYR_SYSTEM_ENTRY_POINTS(extern, SysNODE_CARTPOLE)
#endif

#if !defined(MYR_TU_SYSTEM)   // ===== C-ABI and dispatch: the main object only ============================================
extern "C" const char* myr_last_error(void) { return g_err.c_str(); }
extern "C" const char* myr_version(void) { return "myriad_hip 0.10 (gfx950)"; }
extern "C" int32_t myr_abi_sizeof(int32_t which) {
  switch (which) {
    case 0: return (int32_t)sizeof(myr_solve_opts);
    case 1: return (int32_t)sizeof(myr_problem_desc);
    case 2: return (int32_t)sizeof(myr_dims);
  }
  return -1;
}
extern "C" int myr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

extern "C" void myr_default_solve_opts(myr_solve_opts* o) {
  if (!o) return;
  o->max_iter = 1000;   // config.py:70
  o->restarts = -1;     // library default, see the header
  o->tol_feas = 1e-8;
  o->tol_stat = 1e-6;
  o->tol_compl = 1e-7;
  o->mu_init = 0.1;
  o->restoration = -1;  // library default: elastic phase + second starts, see the header
  o->park_iter = 0;     // the library decides, see the header
}

extern "C" int myr_create(const myr_problem_desc* desc, myr_handle* out) {
  if (!desc || !out) return fail(MYR_E_ARG, "myr_create: null argument");
  SysInfo si;
  if (!sys_info(desc->system_id, &si)) return fail(MYR_E_ARG, "myr_create: unknown system_id");
  if (desc->intervals < 1 || desc->controls_per_interval < 1 || !(desc->T > 0.0))
    return fail(MYR_E_ARG, "myr_create: intervals, controls_per_interval and T must be positive");
  myr_dims dm;
  memset(&dm, 0, sizeof(dm));
  dm.ns = si.ns; dm.nu = si.nu; dm.np = si.np;
  const int N = desc->intervals;
  switch (desc->transcription) {
    case MYR_TR_HERMITE_SIMPSON: {
      const int K = 2 * N + 1;
      dm.x_rows = K; dm.u_rows = K;
      dm.n = K * (si.ns + si.nu);
      dm.m = 2 * N * si.ns;
      dm.jblk = N * (5 * si.ns * si.ns + 5 * si.ns * si.nu);
      dm.ngrad = si.cost_dep_x ? dm.n : K * si.nu;
      break;
    }
    case MYR_TR_TRAPEZOIDAL: {
      dm.x_rows = N + 1; dm.u_rows = N + 1;
      dm.n = (N + 1) * (si.ns + si.nu);
      dm.m = N * si.ns;
      dm.jblk = N * (2 * si.ns * si.ns + 2 * si.ns * si.nu);
      dm.ngrad = si.cost_dep_x ? dm.n : (N + 1) * si.nu;
      break;
    }
    case MYR_TR_SHOOTING: {
      const int mc = desc->integration_method == MYR_INT_RK4 ? 2 : 1;
      dm.x_rows = N + 1; dm.u_rows = mc * N * desc->controls_per_interval + 1;
      dm.n = dm.x_rows * si.ns + dm.u_rows * si.nu;
      dm.m = N * si.ns;
      dm.jblk = N * (si.ns * si.ns + si.ns * (mc * desc->controls_per_interval + 1) * si.nu);   // Ju spans the interval's mc*cpi+1 control rows
      dm.ngrad = dm.n;
      break;
    }
    default:
      return fail(MYR_E_ARG, "myr_create: unknown transcription");
  }
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (desc->device < 0 || desc->device >= ndev) return fail(MYR_E_ARG, "myr_create: bad device ordinal");
  HIPCHK(hipSetDevice(desc->device));
  myr_handle h = new myr_handle_s();
  h->d = *desc;
  h->dims = dm;
  h->si = si;
  HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  for (int i = 0; i < MYR_K_COUNT; ++i) {
    HIPCHK(hipEventCreate(&h->kt[i].a));
    HIPCHK(hipEventCreate(&h->kt[i].b));
  }
  const char* w = getenv("MYRIAD_EVAL_WPT");
  if (w) { int v = atoi(w); if (v == 1 || v == 4 || v == 8) h->eval_wpt = v; }
  if (const char* e = getenv("MYRIAD_EVAL_NT")) h->eval_nt = atoi(e);
  const char* md = getenv("MYRIAD_SOLVE_MODE");
  if (md) { h->solve_mode = (strcmp(md, "lane") == 0) ? 0 : 1; h->solve_fused = (strcmp(md, "wave1") == 0) ? 0 : 1; }
  const char* l = getenv("MYRIAD_SOLVE_LPW");
  if (l) { int v = atoi(l); if (v >= 1 && v <= 64) h->solve_lpw = v; }
  if (const char* e = getenv("MYRIAD_REG_FILL")) h->reg_fill = !strcmp(e, "nan") ? 1 : (!strcmp(e, "random") ? 2 : (!strcmp(e, "big") ? 3 : (!strcmp(e, "zero") ? 4 : 0)));
  if (const char* e = getenv("MYRIAD_STACK_FILL")) h->stack_fill = !strcmp(e, "nan") ? 1 : (!strcmp(e, "random") ? 2 : (!strcmp(e, "big") ? 3 : (!strcmp(e, "zero") ? 4 : 0)));
  if (const char* e = getenv("MYRIAD_PROD_MODE")) h->prod_lane = !strcmp(e, "lane");      // developer switch: see prod_lane
  if (const char* e = getenv("MYRIAD_NODE_EXGD_WPI")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) h->node_exgd_wpi = v; }      // developer knob
  if (const char* e = getenv("MYRIAD_NODE_HELPERS")) h->node_helpers = atoi(e);   // developer knob: helper workgroups per trajectory of the network kernel (0 = none)
  if (const char* e = getenv("MYRIAD_PARK_ITER")) h->park_iter = atoi(e);         // developer knob: iterations of phase 1 of the two-phase launch (0 = off)
  if (const char* e = getenv("MYRIAD_PARK_FILL")) h->park_fill = atoi(e) != 0;    // developer knob: 0 = phase 1 without the fill (every trajectory parks at k1)
  if (const char* e = getenv("MYRIAD_PARK_SHIFT")) { const int v = atoi(e); h->park_shift = v < 0 ? 0 : (v > 64 ? 64 : v); }      // developer knob: see park_shift
  if (const char* e = getenv("MYRIAD_FUSED_WAVES")) h->fused_waves = atoi(e);     // developer knob: wavefronts per trajectory of the fused kernel
  if (const char* e = getenv("MYRIAD_SOLVE_SLOTS")) h->solve_slots = atoi(e);   // developer knob: resident wavefronts of the solve kernel
  if (const char* e = getenv("MYRIAD_POISON")) {      // test knob: "nan" (signalling NaN), "big", "random", or a 64-bit pattern in hex
    if (strcmp(e, "nan") == 0) h->poison = 0x7ff4dead0000beefULL;
    else if (strcmp(e, "big") == 0) h->poison = 0x4415af1d78b58c40ULL;      // 1e20
    else if (strcmp(e, "random") == 0) h->poison = MYR_POISON_RANDOM;       // finite values of order one, different in every word
    else h->poison = strtoull(e, nullptr, 16);
  }
  *out = h;
  return MYR_OK;
}

extern "C" int myr_destroy(myr_handle h) {
  if (!h) return MYR_OK;
  (void)hipSetDevice(h->d.device);
  if (h->dbuf) (void)hipFree(h->dbuf);
  if (h->sbuf) (void)hipFree(h->sbuf);
  if (h->ticket) (void)hipFree(h->ticket);
  if (h->park_state) (void)hipFree(h->park_state);
  if (h->park_perm) (void)hipFree(h->park_perm);
  if (h->vbuf) (void)hipFree(h->vbuf);
  if (h->rbuf) (void)hipFree(h->rbuf);
  if (h->fbuf) (void)hipFree(h->fbuf);
  if (h->nfail_host) (void)hipHostFree(h->nfail_host);
  if (h->nfail_dev) (void)hipFree(h->nfail_dev);
  if (h->coop_buf) (void)hipFree(h->coop_buf);
  if (h->twin) { (void)myr_destroy(h->twin); h->twin = nullptr; }
  for (int i = 0; i < MYR_K_COUNT; ++i) {
    if (h->kt[i].a) (void)hipEventDestroy(h->kt[i].a);
    if (h->kt[i].b) (void)hipEventDestroy(h->kt[i].b);
  }
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return MYR_OK;
}

extern "C" int myr_get_dims(myr_handle h, myr_dims* out) {
  if (!h || !out) return fail(MYR_E_ARG, "myr_get_dims: null argument");
  *out = h->dims;
  return MYR_OK;
}

extern "C" int myr_kernel_time(myr_handle h, int32_t kernel_id, double* avg_ms, int32_t* launches) {
  if (!h || kernel_id < 0 || kernel_id >= MYR_K_COUNT) return fail(MYR_E_ARG, "myr_kernel_time: bad argument");
  const KTimer& k = h->kt[kernel_id];
  if (avg_ms) *avg_ms = k.launches ? k.sum_ms / k.launches : 0.0;
  if (launches) *launches = k.launches;
  return MYR_OK;
}

extern "C" int myr_kernel_time_reset(myr_handle h) {
  if (!h) return fail(MYR_E_ARG, "myr_kernel_time_reset: null handle");
  for (int i = 0; i < MYR_K_COUNT; ++i) { h->kt[i].sum_ms = 0.0; h->kt[i].launches = 0; }
  return MYR_OK;
}

// systems without a direct-transcription path: INVASIVEPLANT is discrete-time (the reference refuses it in its direct
// optimisers too, trajectory_optimizers/base.py:66-67) and only has the discrete FBSM
static int arg_fail(const char* who, int code, const char* what) { return fail(code, std::string(who) + ": " + what); }
static int no_such_path(myr_handle h, const char* who) {
  if (h->d.system_id == MYR_SYS_INVASIVEPLANT)
    return arg_fail(who, MYR_E_UNSUPPORTED, "INVASIVEPLANT is a discrete-time system; only myr_fbsm is available for it");
  return arg_fail(who, MYR_E_ARG, "unknown system");
}

// ---- the argument checks the entry points share: one text each; every entry point makes them in its own order ------------------
static int check_batch(const char* who, int B) { return B < 0 ? arg_fail(who, MYR_E_ARG, "negative batch") : MYR_OK; }
static int check_stride(myr_handle h, const char* who, const double* params, int stride) {
  return params && stride != 0 && stride != h->dims.np ? arg_fail(who, MYR_E_ARG, "params_stride must be 0 (shared) or np") : MYR_OK;
}
static int check_node_weights(myr_handle h, const char* who, const double* params) {
  return !params && h->d.system_id == MYR_SYS_NODE_CARTPOLE ? arg_fail(who, MYR_E_ARG, "a NODE system needs its weights in `params`") : MYR_OK;
}
static int check_mem(const char* who, int mem) { return mem != MYR_MEM_HOST && mem != MYR_MEM_DEVICE ? arg_fail(who, MYR_E_ARG, "bad mem kind") : MYR_OK; }
// ... and those of the derivative family (myr_exgd_grad*, myr_hvp*, myr_fit_grad*)
static int check_handle_and_arrays(const char* who, myr_handle h, const void* p0, const void* p1, const void* p2) {
  return !h || !p0 || !p1 || !p2 ? arg_fail(who, MYR_E_ARG, "null handle or array") : MYR_OK;
}
static int check_ub(const char* who, const void* ub) { return !ub ? arg_fail(who, MYR_E_ARG, "null ub") : MYR_OK; }
static int check_steps_and_seed(const char* who, int nsteps, const void* seed_z, const void* grad) {
  if (nsteps < 0) return arg_fail(who, MYR_E_ARG, "negative nsteps");
  return !seed_z || !grad ? arg_fail(who, MYR_E_ARG, "null seed_z or grad") : MYR_OK;
}
// the stride of a result with np entries to a row (`name`: grad_stride, p_stride): np, a row per `unit`, or 0 -- `zero` says what the rows are summed to
static int check_row_stride(myr_handle h, const char* who, const char* name, int stride, const char* zero, const char* unit) {
  if (stride == 0 || stride == h->dims.np) return MYR_OK;
  return arg_fail(who, MYR_E_ARG, (std::string(name) + " must be 0 (" + zero + ") or np (a row per " + unit + ")").c_str());
}
static const char *const ROW_SUM_BATCH = "one row: the sum over the batch", *const ROW_SUM_SETS = "a row per set: the sum over its instances";
static int check_sets(const char* who, int E, int R) {
  return E < 0 || R < 1 || (long)E * R > 0x7fffffffL ? arg_fail(who, MYR_E_ARG, "bad sizes (E >= 0 sets of R >= 1 instances, E * R an int)") : MYR_OK;
}
static int check_weight_sets(const char* who, const double* params) {
  return !params ? arg_fail(who, MYR_E_ARG, "null params (the [E][np] weight sets)") : MYR_OK;
}
// the network calls: another system is sent to `use`; the transcriptions they have are named in `built`
static int check_is_node(myr_handle h, const char* who, const char* use) {
  if (h->d.system_id == MYR_SYS_NODE_CARTPOLE) return MYR_OK;
  return arg_fail(who, MYR_E_UNSUPPORTED, (std::string("this handle's system is not the network system; use ") + use).c_str());
}
static int check_node_not_trapezoidal(myr_handle h, const char* who, const char* built) {
  if (h->d.transcription == MYR_TR_HERMITE_SIMPSON || h->d.transcription == MYR_TR_SHOOTING) return MYR_OK;
  return arg_fail(who, MYR_E_UNSUPPORTED, (std::string("TRAPEZOIDAL is not built for the network system; ") + built + " only").c_str());
}
// does the LDS carve of the network kernel this handle would run fit?  The SHOOTING kernels come in two forms, <2> for RK4 (two control rows a step)
// and <1>; Hermite-Simpson has a bound for the reverse sweep only
enum { NODE_LDS_EXGD_GRAD = 0, NODE_LDS_HVP = 1 };
static int check_node_lds(myr_handle h, const char* who, int which) {
  const int I = h->d.intervals, cpi = h->d.controls_per_interval;
  const bool shoot = h->d.transcription == MYR_TR_SHOOTING, rk4 = h->d.integration_method == MYR_INT_RK4;
  size_t lds = 0;
  const char* what = "";
  if (which == NODE_LDS_HVP && shoot) {
    lds = rk4 ? node_hvp_shoot_lds_bytes<2>(I, cpi) : node_hvp_shoot_lds_bytes<1>(I, cpi);
    what = "intervals x controls_per_interval too large for the LDS-resident pair records beside the weight copy";
  } else if (which == NODE_LDS_EXGD_GRAD && shoot) {
    lds = rk4 ? node_shoot_exgd_grad_lds_bytes<2>(I, cpi) : node_shoot_exgd_grad_lds_bytes<1>(I, cpi);
    what = "intervals x controls_per_interval too large for the LDS-resident sweep beside the weight copy";
  } else if (which == NODE_LDS_EXGD_GRAD) {
    lds = node_exgd_grad_lds_bytes(I);
    what = "intervals too large for the LDS-resident reverse sweep beside the weight copy";
  }
  return lds > 160 * 1024 ? arg_fail(who, MYR_E_CAPACITY, what) : MYR_OK;
}
// ... and those of the fit family (myr_fit_grad, myr_fit_grad_sets, myr_fit_gn, myr_fit_gn_sets).  `sets`: E, or B for the single-set calls (which
// pass R = 1 here); rows_an_int: E * R is bounded too (myr_fit_gn_sets only: its sibling never has been)
static const char* const ROW_SUM_FIT_SETS = "a row per set: the sum over its trajectories";
static int check_fit_sizes(const char* who, int sets, int R, int num_steps, int u_rows, bool rows_an_int = false) {
  const bool bad = sets < 0 || R < 1 || num_steps < 1 || u_rows < 1 || (rows_an_int && (long)sets * R > 0x7fffffffL);
  return bad ? arg_fail(who, MYR_E_ARG, "bad sizes") : MYR_OK;
}
static int check_data_shared(const char* who, int data_shared) {
  return data_shared != 0 && data_shared != 1 ? arg_fail(who, MYR_E_ARG, "data_shared must be 0 (data per set) or 1 (one set of data, read by every set)") : MYR_OK;
}
// the systems no fit call serves.  A twin, and a system without derivatives, are answered in myr_fit_grad's name by all four
static int check_fit_not_plant(myr_handle h, const char* who) { return h->d.system_id == MYR_SYS_INVASIVEPLANT ? no_such_path(h, who) : MYR_OK; }
static int check_fit_not_twin(myr_handle h) {
  return h->d.system_id >= 100 ? fail(MYR_E_UNSUPPORTED, "myr_fit_grad: an elastic twin has no model of its own to fit; use the handle of its system") : MYR_OK;
}
static bool fit_supported(int id) {
  return for_system(id, true, [](auto t) { using S = SYS_OF(t); return std::is_same<S, SysNODE_CARTPOLE>::value || SysDp<S>::SUPPORTED; }, [] { return false; });
}
static int check_fit_has_derivatives(myr_handle h, const char* who) {
  if (fit_supported(h->d.system_id)) return MYR_OK;
  SysInfo si;
  return sys_info(h->d.system_id, &si) ? fit_no_derivatives() : no_such_path(h, who);
}
static int check_fit_gn_not_node(myr_handle h, const char* who) {
  if (h->d.system_id != MYR_SYS_NODE_CARTPOLE) return MYR_OK;
  return arg_fail(who, MYR_E_UNSUPPORTED, "the network system's 4 804 x 4 804 Gauss-Newton matrix is not formed; use myr_fit_grad for its loss and gradient");
}
// doubles behind `params`: none, one shared set, or a set per instance
static size_t n_params(myr_handle h, const double* params, int stride, int B) { return params ? (stride ? (size_t)B * h->dims.np : (size_t)h->dims.np) : 0; }

static int dispatch_eval(myr_handle h, const EvalArgs& a) {
  return for_system(h->d.system_id, true, [&](auto t) { return eval_for_system<SYS_OF(t)>(h, a); }, [&] { return no_such_path(h, "eval"); });
}

extern "C" int myr_eval(myr_handle h, int32_t B, const double* z, const double* params, int32_t params_stride,
                        double* f, double* gradf, double* c, double* jblk, int32_t mem) {
  const char* who = "myr_eval";
  if (!h || !z) return fail(MYR_E_ARG, "myr_eval: null handle or z");
  if (h->d.system_id == MYR_SYS_INVASIVEPLANT) return no_such_path(h, who);
  if (int rc = check_batch(who, B)) return rc;
  if (B == 0) return MYR_OK;
  if (int rc = check_stride(h, who, params, params_stride)) return rc;
  if (int rc = check_node_weights(h, who, params)) return rc;
  HIPCHK(hipSetDevice(h->d.device));
  if (int rc = check_mem(who, mem)) return rc;
  const myr_dims& dm = h->dims;
  const size_t nB = (size_t)B;
  EvalArgs a{B, nullptr, nullptr, params_stride, nullptr, nullptr, nullptr, nullptr};
  DevStage st = call_stage(h, mem);
  st.in(a.z, z, nB * dm.n);
  st.in(a.params, params, n_params(h, params, params_stride, B));
  st.out(a.f, f, nB);
  st.out(a.g, gradf, nB * dm.ngrad);
  st.out(a.c, c, nB * dm.m);
  st.out(a.j, jblk, nB * dm.jblk);
  if (int rc = st.commit()) return rc;
  if (int rc = dispatch_eval(h, a)) return rc;
  return st.finish();
}

static int dispatch_products(myr_handle h, const ProdArgs& a) {
  return for_system(h->d.system_id, true, [&](auto t) { return products_for_system<SYS_OF(t)>(h, a); }, [&] { return no_such_path(h, "products"); });
}

static int check_products_args(myr_handle h, const char* who, int32_t B, const void* p0, const void* p1, const void* p2,
                               const double* params, int32_t params_stride) {
  if (int rc = check_handle_and_arrays(who, h, p0, p1, p2)) return rc;
  if (h->d.system_id == MYR_SYS_INVASIVEPLANT) return no_such_path(h, who);
  if (int rc = check_batch(who, B)) return rc;
  if (int rc = check_stride(h, who, params, params_stride)) return rc;
  return check_node_weights(h, who, params);
}

// one implementation for J^T lam / grad L (in_w = m, out = n) and J v (in_w = n, out = m)
static int products_call(myr_handle h, int op, const char* who, int32_t B, const double* z, const double* w, const double* params,
                         int32_t params_stride, double* out, int32_t add_gradf, int32_t mem) {
  if (int rc = check_products_args(h, who, B, z, w, out, params, params_stride)) return rc;
  if (B == 0) return MYR_OK;
  HIPCHK(hipSetDevice(h->d.device));
  if (int rc = check_mem(who, mem)) return rc;
  const myr_dims& dm = h->dims;
  ProdArgs a{};
  a.op = op; a.B = B; a.pstride = params_stride; a.add_gradf = add_gradf;
  DevStage st = call_stage(h, mem);
  st.in(a.z, z, (size_t)B * dm.n);
  st.in(a.w, w, (size_t)B * (op == PRODOP_VJP ? dm.m : dm.n));
  st.out(a.out, out, (size_t)B * (op == PRODOP_VJP ? dm.n : dm.m));
  st.in(a.params, params, n_params(h, params, params_stride, B));
  if (int rc = st.commit()) return rc;
  if (int rc = dispatch_products(h, a)) return rc;
  return st.finish();
}

extern "C" int myr_vjp(myr_handle h, int32_t B, const double* z, const double* lam, const double* params, int32_t params_stride,
                       double* out, int32_t add_gradf, int32_t mem) {
  return products_call(h, PRODOP_VJP, "myr_vjp", B, z, lam, params, params_stride, out, add_gradf, mem);
}

extern "C" int myr_jvp(myr_handle h, int32_t B, const double* z, const double* v, const double* params, int32_t params_stride,
                       double* out, int32_t mem) {
  return products_call(h, PRODOP_JVP, "myr_jvp", B, z, v, params, params_stride, out, 0, mem);
}

extern "C" int myr_exgd(myr_handle h, int32_t B, double* z, double* lam, const double* lb, const double* ub, const double* params,
                        int32_t params_stride, double eta_x, double eta_v, int32_t nsteps, int32_t mem) {
  if (int rc = check_products_args(h, "myr_exgd", B, z, lam, lb, params, params_stride)) return rc;
  if (!ub) return fail(MYR_E_ARG, "myr_exgd: null ub");
  if (nsteps < 0) return fail(MYR_E_ARG, "myr_exgd: negative nsteps");
  if (B == 0 || nsteps == 0) return MYR_OK;
  HIPCHK(hipSetDevice(h->d.device));
  if (int rc = check_mem("myr_exgd", mem)) return rc;
  const size_t nz = (size_t)B * h->dims.n;
  ProdArgs a{};
  a.op = PRODOP_EXGD; a.B = B; a.pstride = params_stride; a.eta_x = eta_x; a.eta_v = eta_v; a.nsteps = nsteps;
  DevStage st = call_stage(h, mem);
  st.inout(a.zio, z, nz);
  st.in(a.lb, lb, nz);
  st.in(a.ub, ub, nz);
  st.inout(a.lamio, lam, (size_t)B * h->dims.m);
  st.in(a.params, params, n_params(h, params, params_stride, B));
  if (int rc = st.commit()) return rc;
  if (int rc = dispatch_products(h, a)) return rc;
  return st.finish();
}

static int dispatch_solve(myr_handle h, const SolveCall& a) {
  return for_system(h->d.system_id, true, [&](auto t) { return solve_for_system<SYS_OF(t)>(h, a); }, [&] { return no_such_path(h, "solve"); });
}

// ---- variable scaling of the solve path ----------------------------------------------------------------------
// z / lb / ub -> scaled variables (z in place, bounds into handle scratch); afterwards z back and lam / s_state
__global__ __launch_bounds__(256)
void scale_in_kernel(long total, int n, int xcount, int ns, int nu, VarScale vs, double* z, const double* __restrict__ lb,
                     const double* __restrict__ ub, double* lbs, double* ubs) {
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
    const int i = (int)(g % n);
    const double inv = 1.0 / vs.s[i < xcount ? i % ns : ns + (i - xcount) % nu];
    z[g] *= inv; lbs[g] = lb[g] * inv; ubs[g] = ub[g] * inv;
  }
}
__global__ __launch_bounds__(256)
void scale_out_kernel(long total_z, long total_l, int n, int xcount, int ns, int nu, int m, VarScale vs, double* z, double* lam) {
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total_z + total_l; g += (long)gridDim.x * blockDim.x) {
    if (g < total_z) {
      const int i = (int)(g % n);
      z[g] *= vs.s[i < xcount ? i % ns : ns + (i - xcount) % nu];
    } else if (lam) {
      const long q = g - total_z;
      lam[q] /= vs.s[(int)((q % m) % ns)];       // every constraint row is a state-component row (defect / interpolation)
    }
  }
}

static int dispatch_solve_scaled(myr_handle h, const SolveCall& a) {
  if (!h->vscale_on) return dispatch_solve(h, a);
  const myr_dims& dm = h->dims;
  if (int rc = ensure_buf(&h->vbuf, &h->vbuf_bytes, 2 * (size_t)a.B * dm.n * 8)) return rc;
  double* lbs = (double*)h->vbuf;
  double* ubs = lbs + (size_t)a.B * dm.n;
  SolveCall scaled = a;      // z is scaled in place; the bounds are not the caller's to change
  scaled.lb = lbs; scaled.ub = ubs;
  const long tz = (long)a.B * dm.n, tl = a.lam ? (long)a.B * dm.m : 0;
  const int xcount = dm.x_rows * dm.ns;
  const unsigned blocks = grid_for(tz);
  hipLaunchKernelGGL(scale_in_kernel, dim3(blocks), dim3(256), 0, h->stream, tz, dm.n, xcount, dm.ns, dm.nu, h->vscale, a.z, a.lb, a.ub, lbs, ubs);
  HIPCHK(hipGetLastError());
  int rc = dispatch_solve(h, scaled);
  // unscale even after a failed launch sequence is pointless: return the error as is
  if (rc) return rc;
  hipLaunchKernelGGL(scale_out_kernel, dim3(blocks), dim3(256), 0, h->stream, tz, tl, dm.n, xcount, dm.ns, dm.nu, dm.m, h->vscale, a.z, a.lam);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return MYR_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Restoration inside the solve call (myr_solve_opts.restoration): what the reference gets from inside its one minimize_ipopt call
// (/root/reference/myriad/nlp_solvers/__init__.py:57-58 -- IPOPT falls back to a feasibility-restoration phase when its line search
// fails) happens here for the instances the first attempt leaves without a KKT point, for EVERY binding of the C-ABI:
//   1. elastic phase  -- the system's elastic twin (x' = f(x,u) + s, cost g + rho/2 |s|^2) solved for rho = 1, 1e2, 1e4, each from the
//                        previous solution; its trajectory starts the problem itself;
//   2. second starts  -- excitation guesses (oscillating controls, states by a rollout of the true dynamics), c = 2, 3, 5 cycles.
// Host logic over device arrays: the failed rows are gathered into a working set, solved, and scattered back where they converged.
// (Rounds 2-3 had this in the Python host only: myriad_amd/trajectory_optimizers/__init__.py, removed in round 4.)
// ------------------------------------------------------------------------------------------------------------------------------
static int dispatch_rollout(myr_handle h, const RolloutArgs& a);
extern "C" int myr_set_var_scale(myr_handle h, const double* scale);

__global__ void gather_rows_kernel(long total, int w, const int32_t* __restrict__ idx, const double* __restrict__ src, double* __restrict__ dst) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long r = t / w; const int c = (int)(t - r * w);
    dst[t] = src[(long)idx[r] * w + c];
  }
}
__global__ void scatter_rows_kernel(long total, int w, const int32_t* __restrict__ idx, const int32_t* __restrict__ take, const double* __restrict__ src,
                                    double* __restrict__ dst) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long r = t / w; const int c = (int)(t - r * w);
    if (take[r]) dst[(long)idx[r] * w + c] = src[t];
  }
}
// z of the problem -> z of its twin: the state rows as they are, every control row widened by ns slack controls (= fill)
__global__ void twin_widen_kernel(long total, int nx, int nu, int ns, double fill, const double* __restrict__ src, double* __restrict__ dst, int n, int nt) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long b = t / nt; const int i = (int)(t - b * nt);
    double v;
    if (i < nx) v = src[b * n + i];
    else { const int row = (i - nx) / (nu + ns), c = (i - nx) % (nu + ns); v = c < nu ? src[b * n + nx + row * nu + c] : fill; }
    dst[t] = v;
  }
}
// the twin's states and controls -> a start of the problem itself; zt is first clipped into its bounds (non-finite entries -> 0 / +-1e6),
// as a start must be; slack[b] = max |s| of the clipped twin solution
__global__ void twin_clip_kernel(long total, const double* __restrict__ lb, const double* __restrict__ ub, double* __restrict__ z) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    double v = z[t];
    if (v != v) v = 0.0; else if (v > 1e300) v = 1e6; else if (v < -1e300) v = -1e6;
    v = v < lb[t] ? lb[t] : v; v = v > ub[t] ? ub[t] : v;
    z[t] = v;
  }
}
__global__ __launch_bounds__(256) void twin_slack_kernel(int nx, int rows_u, int nu, int ns, int nt, const double* __restrict__ zt, double* __restrict__ slack) {
  __shared__ double red[256];
  const long b = blockIdx.x;
  double m = 0.0;
  for (int i = threadIdx.x; i < rows_u * ns; i += blockDim.x) {
    const int row = i / ns, c = i % ns;
    const double v = fabs(zt[b * nt + nx + row * (nu + ns) + nu + c]);
    m = v > m ? v : m;
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] > red[threadIdx.x + o] ? red[threadIdx.x] : red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) slack[b] = red[0];
}
__global__ void twin_narrow_kernel(long total, int nx, int nu, int ns, const double* __restrict__ zt, double* __restrict__ z, int n, int nt) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long b = t / n; const int i = (int)(t - b * n);
    z[t] = i < nx ? zt[b * nt + i] : zt[b * nt + nx + ((i - nx) / nu) * (nu + ns) + (i - nx) % nu];
  }
}
__global__ void twin_params_kernel(int B, int np, const double* __restrict__ params, int pstride, const double* __restrict__ defaults, double rho, double* __restrict__ out) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < (long)B * (np + 1); t += (long)gridDim.x * blockDim.x) {
    const long b = t / (np + 1); const int i = (int)(t - b * (np + 1));
    out[t] = i == np ? rho : (params ? params[b * (long)pstride + i] : defaults[i]);
  }
}
// excitation guess, controls: us[b][j][a] = centre_a + 0.95 amp_a sin(2 pi c t_j / T), t_j = T j / (rr - 1); centre / amplitude from control a's own
// bounds.  The reference writes control bounds control-major (quirk Q1: hermite_simpson.py:71-74, trapezoidal.py:58-61, shooting.py:264-267 -- flat
// entries [a rr, (a + 1) rr) of the control part hold control a's bounds) while the variables are time-major, so control a's bounds are read at flat
// index a * u_rows (u_rows = control rows of the decision vector), NOT at the variable's own entry (for nu > 1 the first row holds control 0's bounds in every component).  x0[b] = the pinned start
// state, else the guess's
__global__ void excitation_controls_kernel(int B, int rr, int u_rows, int nu, int ns, int nx, int n, double cycles, const double* __restrict__ lb, const double* __restrict__ ub,
                                           const double* __restrict__ z0, double* __restrict__ us, double* __restrict__ x0) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < (long)B * rr * nu; t += (long)gridDim.x * blockDim.x) {
    const long b = t / ((long)rr * nu); const int j = (int)((t / nu) % rr), a = (int)(t % nu);
    const double lo = lb[b * n + nx + (long)a * u_rows], hi = ub[b * n + nx + (long)a * u_rows];
    const bool fin = lo > -1e300 && hi < 1e300;
    const double centre = fin ? 0.5 * (lo + hi) : 0.0, amp = fin ? 0.5 * (hi - lo) : 1.0;
    us[t] = centre + 0.95 * amp * sin(2.0 * 3.14159265358979323846 * cycles * ((double)j / (double)(rr - 1)));
    if (j == 0 && a == 0) {
      for (int q = 0; q < ns; ++q) { const double l = lb[b * n + q], u = ub[b * n + q]; x0[b * ns + q] = (l == u) ? l : z0[b * n + q]; }
    }
  }
}
// ... and the guess itself: states = every `xstride`-th state of the rollout, controls = every `ustride`-th row, clipped into the bounds
__global__ void excitation_pack_kernel(long total, int n, int nx, int ns, int nu, int steps, int xstride, int rr, int ustride, const double* __restrict__ xs,
                                       const double* __restrict__ us, const double* __restrict__ lb, const double* __restrict__ ub, double* __restrict__ z) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long b = t / n; const int i = (int)(t - b * n);
    double v;
    if (i < nx) { const int row = i / ns, c = i % ns; v = xs[(b * (steps + 1) + (long)row * xstride) * ns + c]; }
    else { const int row = (i - nx) / nu, c = (i - nx) % nu; v = us[(b * rr + (long)row * ustride) * nu + c]; }
    if (v != v) v = 0.0; else if (v > 1e300) v = 1e6; else if (v < -1e300) v = -1e6;
    v = v < lb[t] ? lb[t] : v; v = v > ub[t] ? ub[t] : v;
    z[t] = v;
  }
}

// how many instances ended without a KKT point -> a device word, copied to a pinned host word (the common answer, none, costs no status download)
__global__ void count_failed_kernel(int B, const int32_t* __restrict__ status, int32_t* __restrict__ out) {
  int n = 0;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) n += status[b] != MYR_STATUS_CONVERGED ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, n);
}

static bool twin_defaults(int twin_id, double* buf) {
  return for_system(twin_id, false, [&](auto t) { using S = SYS_OF(t); S::default_params(buf); return true; }, [] { return false; });
}

struct RestoreCfg { bool elastic, starts; std::vector<int> cycles; };
static RestoreCfg restore_cfg(const myr_solve_opts& so) {
  RestoreCfg c;
  int mode = so.restoration < 0 ? 3 : so.restoration;
  c.elastic = (mode & 1) != 0; c.starts = (mode & 2) != 0;
  c.cycles = {2, 3, 5};
  if (so.restoration < 0) {      // the library default listens to the environment (the explicit values do not)
    if (const char* e = getenv("MYRIAD_ELASTIC")) { if (atoi(e) == 0) c.elastic = false; }
    if (const char* e = getenv("MYRIAD_SECOND_STARTS")) {
      c.cycles.clear();
      for (const char* q = e; *q;) { char* end = nullptr; long v = strtol(q, &end, 10); if (end == q) { ++q; continue; } if (v > 0) c.cycles.push_back((int)v); q = end; }
      if (c.cycles.empty()) c.starts = false;
    }
  }
  return c;
}

// the twin handle of a collocation problem whose system has one (lazily; nullptr when there is none or its solver is not built)
static myr_handle twin_of(myr_handle h) {
  if (h->twin_unavailable) return nullptr;
  if (h->twin) return h->twin;
  SysInfo si;
  if (h->d.transcription == MYR_TR_SHOOTING || h->d.system_id >= 100 || !sys_info(h->d.system_id + 100, &si)) { h->twin_unavailable = true; return nullptr; }
  myr_problem_desc d = h->d;
  d.system_id += 100;
  myr_handle t = nullptr;
  if (myr_create(&d, &t) != MYR_OK) { h->twin_unavailable = true; return nullptr; }
  if (h->vscale_on) {          // a slack is a rate of its state: it takes the state's scale
    double sc[16];
    const int nw = h->dims.ns + h->dims.nu;
    for (int i = 0; i < nw; ++i) sc[i] = h->vscale.s[i];
    for (int i = 0; i < h->dims.ns && nw + i < 16; ++i) sc[nw + i] = h->vscale.s[i];
    if (myr_set_var_scale(t, sc) != MYR_OK) { (void)myr_destroy(t); h->twin_unavailable = true; return nullptr; }
  }
  t->solve_mode = h->solve_mode; t->solve_fused = h->solve_fused;
  h->twin = t;
  return t;
}

static int solve_restored(myr_handle h, const SolveCall& a) {
  const int B = a.B, pstride = a.pstride;
  double* const z = a.z; const double *lb = a.lb, *ub = a.ub, *params = a.params;
  h->info_start.assign(B, 0); h->info_attempts.assign(B, 1); h->info_restored.assign(B, 0);
  h->plan_frozen = false;
  struct Thaw { myr_handle h; ~Thaw() { h->plan_frozen = false; } } thaw{h};
  const RestoreCfg cfg = restore_cfg(a.so);
  if (!cfg.elastic && !cfg.starts) return dispatch_solve_scaled(h, a);
  const myr_dims& dm = h->dims;
  const int n = dm.n, m = dm.m, ns = dm.ns, nu = dm.nu, np = dm.np;
  // the caller's guess is overwritten by the first attempt: keep it
  double* z0c = nullptr;
  int32_t *dstat = a.status, *dit = a.iters;
  DevStage keep = scratch_stage(h, &h->rbuf, &h->rbuf_bytes);
  keep.scratch(z0c, (size_t)B * n);
  if (!a.status) keep.scratch(dstat, (size_t)B);
  if (!a.iters) keep.scratch(dit, (size_t)B);
  if (int rc = keep.commit()) return rc;
  HIPCHK(hipMemcpyAsync(z0c, z, (size_t)B * n * 8, hipMemcpyDeviceToDevice, h->stream));
  SolveCall first = a;      // status and iterations are needed here whether the caller asked for them or not
  first.status = dstat; first.iters = dit;
  if (int rc = dispatch_solve_scaled(h, first)) return rc;
  h->plan_frozen = true;
  if (!h->nfail_host) HIPCHK(hipHostMalloc((void**)&h->nfail_host, 64, hipHostMallocDefault));
  if (!h->nfail_dev) HIPCHK(hipMalloc((void**)&h->nfail_dev, 64));
  *h->nfail_host = -1;
  HIPCHK(hipMemsetAsync(h->nfail_dev, 0, 4, h->stream));
  hipLaunchKernelGGL(count_failed_kernel, dim3((unsigned)((B + 255) / 256 > 64 ? 64 : (B + 255) / 256)), dim3(256), 0, h->stream, B, dstat, h->nfail_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h->nfail_host, h->nfail_dev, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (*h->nfail_host < 0) return fail(MYR_E_HIP, "restoration: the count of failed instances did not arrive");
  if (*h->nfail_host == 0) return MYR_OK;
  std::vector<int32_t> hstat(B), hit(B);
  HIPCHK(hipMemcpyAsync(hstat.data(), dstat, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::vector<int32_t> fail_;
  for (int b = 0; b < B; ++b) if (hstat[b] != MYR_STATUS_CONVERGED) fail_.push_back(b);
  if (fail_.empty()) return MYR_OK;
  myr_handle twin = cfg.elastic ? twin_of(h) : nullptr;
  if (!twin && !cfg.starts) return MYR_OK;
  HIPCHK(hipMemcpyAsync(hit.data(), dit, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));

  // working set of the failed rows (device): idx | take | z0f zf lbf ubf | pf | lamf costf kktf statf itf | twin: zt lbt ubt pt slack | excitation: us x0 xs
  const int nf0 = (int)fail_.size();
  const int nt = twin ? twin->dims.n : 0;
  const int mc = (h->d.transcription == MYR_TR_SHOOTING && h->d.integration_method == MYR_INT_RK4) ? 2 : 1;
  const int steps = (dm.u_rows - 1) / mc;
  const int rr = (h->d.integration_method == MYR_INT_RK4) ? 2 * steps + 1 : steps + 1;
  const size_t F = (size_t)nf0;
  int32_t *didx, *dtake, *statf, *itf;
  double *z0f, *zf, *lbf, *ubf, *pf, *lamf, *costf, *kktf;
  double *zt = nullptr, *lbt = nullptr, *ubt = nullptr, *pt = nullptr, *dslack = nullptr, *ddef = nullptr;
  double *dus = nullptr, *dx0 = nullptr, *dxs = nullptr;
  DevStage ws = scratch_stage(h, &h->fbuf, &h->fbuf_bytes);
  ws.scratch(didx, F); ws.scratch(dtake, F);
  ws.scratch(z0f, F * n); ws.scratch(zf, F * n); ws.scratch(lbf, F * n); ws.scratch(ubf, F * n);
  ws.scratch(pf, F * (np > 0 ? np : 1));
  ws.scratch(lamf, F * m); ws.scratch(costf, F); ws.scratch(kktf, F * 3); ws.scratch(statf, F); ws.scratch(itf, F);
  if (twin) { ws.scratch(zt, F * nt); ws.scratch(lbt, F * nt); ws.scratch(ubt, F * nt); ws.scratch(pt, F * (np + 1)); ws.scratch(dslack, F); ws.scratch(ddef, 64); }
  if (cfg.starts) { ws.scratch(dus, F * rr * nu); ws.scratch(dx0, F * ns); ws.scratch(dxs, F * (steps + 1) * ns); }
  if (int rc = ws.commit()) return rc;
  const bool per_row_params = params && pstride != 0;
  const int nx = dm.x_rows * ns;

  // rows `rows` (indices into the batch) -> the working set
  auto gather = [&](const std::vector<int32_t>& rows) -> int {
    const int nf = (int)rows.size();
    HIPCHK(hipMemcpyAsync(didx, rows.data(), (size_t)nf * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for((long)nf * n)), dim3(256), 0, h->stream, (long)nf * n, n, didx, z0c, z0f);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for((long)nf * n)), dim3(256), 0, h->stream, (long)nf * n, n, didx, lb, lbf);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for((long)nf * n)), dim3(256), 0, h->stream, (long)nf * n, n, didx, ub, ubf);
    if (per_row_params) hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for((long)nf * np)), dim3(256), 0, h->stream, (long)nf * np, np, didx, params, pf);
    HIPCHK(hipGetLastError());
    return MYR_OK;
  };
  const double* pfp = per_row_params ? pf : params;
  // rows of the working set with take[r] != 0 -> the caller's arrays
  auto scatter = [&](const std::vector<int32_t>& take, int nf) -> int {
    HIPCHK(hipMemcpyAsync(dtake, take.data(), (size_t)nf * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(grid_for((long)nf * n)), dim3(256), 0, h->stream, (long)nf * n, n, didx, dtake, zf, z);
    if (a.lam) hipLaunchKernelGGL(scatter_rows_kernel, dim3(grid_for((long)nf * m)), dim3(256), 0, h->stream, (long)nf * m, m, didx, dtake, lamf, a.lam);
    if (a.cost) hipLaunchKernelGGL(scatter_rows_kernel, dim3(grid_for((long)nf)), dim3(256), 0, h->stream, (long)nf, 1, didx, dtake, costf, a.cost);
    if (a.kkt) hipLaunchKernelGGL(scatter_rows_kernel, dim3(grid_for((long)nf * 3)), dim3(256), 0, h->stream, (long)nf * 3, 3, didx, dtake, kktf, a.kkt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));     // (`take` is a host vector of the caller's frame)
    return MYR_OK;
  };
  std::vector<int32_t> st2, it2;
  auto read_back = [&](int nf) -> int {
    st2.resize(nf); it2.resize(nf);
    HIPCHK(hipMemcpyAsync(st2.data(), statf, (size_t)nf * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(it2.data(), itf, (size_t)nf * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return MYR_OK;
  };
  // every further attempt solves the working set of the failed rows, with no restoration of its own: on this handle ...
  SolveCall again = a;
  again.z = zf; again.lb = lbf; again.ub = ubf; again.params = pfp; again.pstride = per_row_params ? np : pstride;
  again.so.restoration = 0;
  again.lam = lamf; again.cost = costf; again.status = statf; again.iters = itf; again.kkt = kktf;

  if (twin) {      // ---- elastic phase -----------------------------------------------------------------------------------------
    const int nf = (int)fail_.size();
    if (int rc = gather(fail_)) return rc;
    double defs[64];
    for (int i = 0; i < 64; ++i) defs[i] = 0.0;
    if (!twin_defaults(twin->d.system_id - 100, defs)) return fail(MYR_E_ARG, "restoration: no default parameters for the system");
    HIPCHK(hipMemcpyAsync(ddef, defs, 64 * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(twin_widen_kernel, dim3(grid_for((long)nf * nt)), dim3(256), 0, h->stream, (long)nf * nt, nx, nu, ns, 0.0, z0f, zt, n, nt);
    hipLaunchKernelGGL(twin_widen_kernel, dim3(grid_for((long)nf * nt)), dim3(256), 0, h->stream, (long)nf * nt, nx, nu, ns, -INFINITY, lbf, lbt, n, nt);
    hipLaunchKernelGGL(twin_widen_kernel, dim3(grid_for((long)nf * nt)), dim3(256), 0, h->stream, (long)nf * nt, nx, nu, ns, INFINITY, ubf, ubt, n, nt);
    HIPCHK(hipGetLastError());
    // ... and on the twin handle: the widened rows, rho as one more parameter of every row, status and iterations only
    SolveCall tw = again;
    tw.z = zt; tw.lb = lbt; tw.ub = ubt; tw.params = pt; tw.pstride = np + 1;
    if (tw.so.max_iter > 500) tw.so.max_iter = 500;      // per twin solve (the ones that help take 30-300 iterations)
    tw.lam = nullptr; tw.cost = nullptr; tw.kkt = nullptr;
    const double rhos[3] = {1.0, 1e2, 1e4};
    std::vector<double> slack_prev(nf, 0.0), slack_last(nf, 0.0);
    std::vector<int64_t> it_acc(nf, 0);
    std::vector<int32_t> twin_stat(nf, 1);
    bool twin_ok = true;
    for (int k = 0; k < 3 && twin_ok; ++k) {
      hipLaunchKernelGGL(twin_params_kernel, dim3(grid_for((long)nf * (np + 1))), dim3(256), 0, h->stream, nf, np, pfp, per_row_params ? np : 0, ddef, rhos[k], pt);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(h->stream));      // the twin runs on a stream of its own
      tw.B = nf;
      const int rc = dispatch_solve_scaled(twin, tw);
      if (rc == MYR_E_UNSUPPORTED) {      // (a twin whose solver is not built for this scheme): drop the handle -- its stream and buffers -- for good, and do not
        twin_ok = false;                  // leave "... not built" behind as the last error of a myr_solve that returns MYR_OK
        h->twin_unavailable = true;
        (void)myr_destroy(h->twin); h->twin = nullptr; twin = nullptr;
        g_err.clear();
        break;
      }
      if (rc) return rc;
      hipLaunchKernelGGL(twin_clip_kernel, dim3(grid_for((long)nf * nt)), dim3(256), 0, h->stream, (long)nf * nt, lbt, ubt, zt);
      hipLaunchKernelGGL(twin_slack_kernel, dim3((unsigned)nf), dim3(256), 0, h->stream, nx, dm.u_rows, nu, ns, nt, zt, dslack);
      HIPCHK(hipGetLastError());
      if (int rc2 = read_back(nf)) return rc2;
      slack_prev = slack_last;
      HIPCHK(hipMemcpy(slack_last.data(), dslack, (size_t)nf * 8, hipMemcpyDeviceToHost));
      for (int r = 0; r < nf; ++r) { it_acc[r] += it2[r]; twin_stat[r] = st2[r]; }
      if (getenv("MYRIAD_DEBUG_ELASTIC"))
        for (int r = 0; r < nf && r < 8; ++r)
          fprintf(stderr, "[myriad] elastic phase: instance %d, rho %g: twin status %d after %d iterations, slack %.3e\n", (int)fail_[r], rhos[k], (int)st2[r], (int)it2[r], slack_last[r]);
    }
    if (twin_ok) {
      hipLaunchKernelGGL(twin_narrow_kernel, dim3(grid_for((long)nf * n)), dim3(256), 0, h->stream, (long)nf * n, nx, nu, ns, zt, zf, n, nt);
      HIPCHK(hipGetLastError());
      again.B = nf;
      if (int rc = dispatch_solve_scaled(h, again)) return rc;
      if (int rc = read_back(nf)) return rc;
      std::vector<int32_t> take(nf, 0), left;
      for (int r = 0; r < nf; ++r) {
        const int b = fail_[r];
        const bool ok = st2[r] == MYR_STATUS_CONVERGED;
        take[r] = ok ? 1 : 0;
        hit[b] += (int32_t)(it2[r] + it_acc[r]);
        h->info_attempts[b] += 4;
        if (ok) { hstat[b] = MYR_STATUS_CONVERGED; h->info_restored[b] = 1; }
        else {
          // stationary point of the infeasibility: the twin converged for the largest rho and its slack neither vanished nor shrank.
          // (A twin that ran on the lane kernel gives no verdict: its instantiations with many variables per point are not covered by the
          // wave / lane agreement tests -- and ROCKETLANDING's own lane kernel was once miscompiled)
          if (twin->last_solve_form == 1 && twin_stat[r] == MYR_STATUS_CONVERGED && slack_last[r] > 1e-3 && slack_last[r] > 0.1 * slack_prev[r])
            hstat[b] = MYR_STATUS_INFEASIBLE;
          left.push_back(b);
        }
      }
      if (int rc = scatter(take, nf)) return rc;
      fail_.swap(left);
    }
  }
  if (cfg.starts) {      // ---- second starts: excitation guesses --------------------------------------------------------------
    const int xstride = steps / (dm.x_rows - 1 > 0 ? dm.x_rows - 1 : 1), ustride = (rr - 1) / (dm.u_rows - 1 > 0 ? dm.u_rows - 1 : 1);
    for (size_t ci = 0; ci < cfg.cycles.size() && !fail_.empty(); ++ci) {
      const int nf = (int)fail_.size(), c = cfg.cycles[ci];
      if (int rc = gather(fail_)) return rc;
      hipLaunchKernelGGL(excitation_controls_kernel, dim3(grid_for((long)nf * rr * nu)), dim3(256), 0, h->stream, nf, rr, dm.u_rows, nu, ns, nx, n, (double)c, lbf, ubf, z0f, dus, dx0);
      HIPCHK(hipGetLastError());
      if (int rc = dispatch_rollout(h, RolloutArgs{nf, steps, rr, dx0, dus, pfp, per_row_params ? np : pstride, dxs, nullptr})) return rc;
      hipLaunchKernelGGL(excitation_pack_kernel, dim3(grid_for((long)nf * n)), dim3(256), 0, h->stream, (long)nf * n, n, nx, ns, nu, steps, xstride, rr, ustride, dxs, dus, lbf, ubf, zf);
      HIPCHK(hipGetLastError());
      again.B = nf;
      if (int rc = dispatch_solve_scaled(h, again)) return rc;
      if (int rc = read_back(nf)) return rc;
      std::vector<int32_t> take(nf, 0), left;
      for (int r = 0; r < nf; ++r) {
        const int b = fail_[r];
        const bool ok = st2[r] == MYR_STATUS_CONVERGED;
        take[r] = ok ? 1 : 0;
        hit[b] += it2[r];
        h->info_attempts[b] += 1;
        if (ok) { hstat[b] = MYR_STATUS_CONVERGED; h->info_restored[b] = 0; h->info_start[b] = c; }
        else left.push_back(b);
      }
      if (int rc = scatter(take, nf)) return rc;
      fail_.swap(left);
    }
  }
  HIPCHK(hipMemcpyAsync(dstat, hstat.data(), (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dit, hit.data(), (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return MYR_OK;
}

extern "C" int myr_solve_info(myr_handle h, int32_t B, int32_t* start, int32_t* attempts, int32_t* restored) {
  if (!h) return fail(MYR_E_ARG, "myr_solve_info: null handle");
  if (B != (int32_t)h->info_start.size()) return fail(MYR_E_ARG, "myr_solve_info: B is not the batch size of the last solve on this handle");
  if (start) memcpy(start, h->info_start.data(), (size_t)B * 4);
  if (attempts) memcpy(attempts, h->info_attempts.data(), (size_t)B * 4);
  if (restored) memcpy(restored, h->info_restored.data(), (size_t)B * 4);
  return MYR_OK;
}

extern "C" int myr_solve_plan(myr_handle h, int32_t* plan) {
  if (!h || !plan) return fail(MYR_E_ARG, "myr_solve_plan: null argument");
  memcpy(plan, h->plan, sizeof(h->plan));
  return MYR_OK;
}

extern "C" int myr_set_var_scale(myr_handle h, const double* scale) {
  if (!h) return fail(MYR_E_ARG, "myr_set_var_scale: null handle");
  if (h->d.system_id == MYR_SYS_NODE_CARTPOLE && scale) return fail(MYR_E_UNSUPPORTED, "myr_set_var_scale: not available for NODE systems");
  const int nw = h->dims.ns + h->dims.nu;
  if (nw > 16) return fail(MYR_E_CAPACITY, "myr_set_var_scale: more than 16 variables per point");
  // every entry is checked before anything changes: a refused vector leaves the previous scales (and the twin made under them) in force
  if (scale) {
    for (int i = 0; i < nw; ++i) {
      if (!(scale[i] > 0.0) || !(scale[i] < 1e300)) return fail(MYR_E_ARG, "myr_set_var_scale: scales must be positive and finite");
    }
  }
  if (h->twin) { (void)myr_destroy(h->twin); h->twin = nullptr; }      // (the twin of the restoration phase takes its scales from here: made again on demand)
  bool on = false;
  for (int i = 0; i < 16; ++i) h->vscale.s[i] = 1.0;
  if (scale) {
    for (int i = 0; i < nw; ++i) {
      h->vscale.s[i] = scale[i];
      on = on || scale[i] != 1.0;
    }
  }
  h->vscale_on = on;
  return MYR_OK;
}

// ---- myr_solve / myr_solve_x0: what the two entry points share ---------------------------------------------------------------
// The argument checks, in the order both make them, on the call as the user passed it (`c`; c->so is filled from `opts` here).  `who` names the
// entry point, `arrays` its pointers that must not be null (`null`: one is); mem_early: the memory kind where it is tested at this point
// (myr_solve_x0; myr_solve tests it after hipSetDevice).  *empty: a batch of zero instances -- nothing to do, and nothing further is checked.
static int check_solve_args(myr_handle h, const char* who, const char* arrays, bool null, const int32_t* mem_early, const myr_solve_opts* opts,
                            SolveCall* c, bool* empty) {
  *empty = false;
  if (!h || null) return arg_fail(who, MYR_E_ARG, (std::string("null handle, ") + arrays).c_str());
  if (h->d.system_id == MYR_SYS_INVASIVEPLANT) return no_such_path(h, who);
  if (int rc = check_batch(who, c->B)) return rc;
  if (c->B == 0) { h->info_start.clear(); h->info_attempts.clear(); h->info_restored.clear(); *empty = true; return MYR_OK; }
  if (int rc = check_stride(h, who, c->params, c->pstride)) return rc;
  if (int rc = check_node_weights(h, who, c->params)) return rc;
  if (mem_early)
    if (int rc = check_mem(who, *mem_early)) return rc;
  myr_solve_opts& so = c->so;
  if (opts) so = *opts; else myr_default_solve_opts(&so);
  if (so.max_iter < 0 || !(so.tol_feas > 0) || !(so.tol_stat > 0) || !(so.tol_compl > 0) || !(so.mu_init > 0))
    return arg_fail(who, MYR_E_ARG, "bad options");
  return MYR_OK;
}
// What the two entry points stage alike behind their own inputs: lam, the parameters, and the four per-instance results.  Those four are device arrays
// whether or not a host caller asked for them (the two-phase launch orders its resume by kkt; solve_restored reads status and iterations), downloaded when asked.
static void stage_solve_tail(DevStage& st, myr_handle h, SolveCall& d, const SolveCall& user) {
  const size_t B = (size_t)user.B;
  st.out(d.lam, user.lam, B * h->dims.m);
  st.in(d.params, user.params, n_params(h, user.params, user.pstride, user.B));
  st.out(d.cost, user.cost, B, true);
  st.out(d.status, user.status, B, true);
  st.out(d.iters, user.iters, B, true);
  st.out(d.kkt, user.kkt, 3 * B, true);
}

extern "C" int myr_solve(myr_handle h, int32_t B, double* z, const double* lb, const double* ub,
                         const double* params, int32_t params_stride, const myr_solve_opts* opts,
                         double* lam, double* cost, int32_t* status, int32_t* iters, double* kkt, int32_t mem) {
  SolveCall user{B, z, lb, ub, params, params_stride, {}, lam, cost, status, iters, kkt};
  bool empty = false;
  if (int rc = check_solve_args(h, "myr_solve", "z, lb or ub", !z || !lb || !ub, nullptr, opts, &user, &empty)) return rc;
  if (empty) return MYR_OK;
  HIPCHK(hipSetDevice(h->d.device));
  if (int rc = check_mem("myr_solve", mem)) return rc;
  const size_t nz = (size_t)B * h->dims.n;
  SolveCall d = user;      // the batch the solver sees: a device caller's own arrays, a host caller's staged
  DevStage st = call_stage(h, mem);
  st.inout(d.z, z, nz);
  st.in(d.lb, lb, nz);
  st.in(d.ub, ub, nz);
  stage_solve_tail(st, h, d, user);
  if (int rc = st.commit()) return rc;
  if (int rc = solve_restored(h, d)) return rc;
  return st.finish();
}

// ---- myr_solve_x0: B instances that differ in their START STATE only ------------------------------------------------
// The reference builds guess and bounds of an instance from system.x_0 in the optimiser's constructor
// (hermite_simpson.py:37-48 guess, :55-81 bounds; trapezoidal.py:36-50, 55-77; shooting.py:56-74, 247-275).  For a batch
// of start states that is B x 3 n doubles of host packing and PCIe traffic carrying B x ns doubles of information: the
// expansion runs on the device instead.  z0[b][i] = g0[i] + g1[i] * x0s[b][i mod ns] on the state rows (two roundings, the
// product and the sum: bit for bit what numpy's x0 * (1 - lin) + x_T * lin gives with g1 = 1 - lin, g0 = x_T * lin), g0[i]
// elsewhere; lb / ub = the templates with the first point's state rows replaced by x0s[b].
__global__ void pack_x0_kernel(long total, int n, int ns, int xcount, const double* __restrict__ x0s, const double* __restrict__ g0,
                               const double* __restrict__ g1, const double* __restrict__ lbt, const double* __restrict__ ubt,
                               double* __restrict__ z, double* __restrict__ lb, double* __restrict__ ub) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long b = t / n;
    const int i = (int)(t - b * n);
    double zi = g0[i], l = lbt[i], u = ubt[i];
    if (i < xcount) {
      const double x = x0s[b * ns + i % ns];
      double prod = x * g1[i];
      asm volatile("" : "+v"(prod));     // a rounded product of its own: the compiler must not contract it into an fma with the sum
      zi = prod + zi;
      if (i < ns) { l = x; u = x; }
    }
    z[t] = zi; lb[t] = l; ub[t] = u;
  }
}

extern "C" int myr_solve_x0(myr_handle h, int32_t B, const double* x0s, const double* g0, const double* g1, const double* lb,
                            const double* ub, const double* params, int32_t params_stride, const myr_solve_opts* opts,
                            double* z, double* lam, double* cost, int32_t* status, int32_t* iters, double* kkt, int32_t mem) {
  SolveCall user{B, z, nullptr, nullptr, params, params_stride, {}, lam, cost, status, iters, kkt};      // (lb, ub are templates here: the batch's bounds are made below)
  bool empty = false;
  if (int rc = check_solve_args(h, "myr_solve_x0", "x0s, g0, g1, lb, ub or z", !x0s || !g0 || !g1 || !lb || !ub || !z, &mem, opts, &user, &empty)) return rc;
  if (empty) return MYR_OK;
  HIPCHK(hipSetDevice(h->d.device));
  const myr_dims& dm = h->dims;
  const size_t nz = (size_t)B * dm.n, n1 = (size_t)dm.n;
  // the expanded bounds are device scratch for every caller; a host caller's iterate, inputs and results are staged too
  SolveCall d = user;
  double *dlb = nullptr, *dub = nullptr;
  const double *dx0 = nullptr, *dg0 = nullptr, *dg1 = nullptr, *dlt = nullptr, *dut = nullptr;
  DevStage st = call_stage(h, mem);
  st.scratch(dlb, nz);
  st.scratch(dub, nz);
  st.out(d.z, z, nz);
  st.in(dx0, x0s, (size_t)B * dm.ns);
  st.in(dg0, g0, n1); st.in(dg1, g1, n1); st.in(dlt, lb, n1); st.in(dut, ub, n1);
  stage_solve_tail(st, h, d, user);
  if (int rc = st.commit()) return rc;
  d.lb = dlb; d.ub = dub;
  hipLaunchKernelGGL(pack_x0_kernel, dim3(grid_for((long)nz)), dim3(256), 0, h->stream, (long)nz, dm.n, dm.ns, dm.x_rows * dm.ns, dx0, dg0, dg1, dlt, dut, d.z, dlb, dub);
  HIPCHK(hipGetLastError());
  if (int rc = solve_restored(h, d)) return rc;
  return st.finish();
}

static int dispatch_rollout(myr_handle h, const RolloutArgs& a) {
  if (int rc = timed_begin(h, MYR_K_ROLLOUT)) return rc;
  if (int rc = for_system(h->d.system_id, true, [&](auto t) { return rollout_for_system<SYS_OF(t)>(h, a); }, [&] { return no_such_path(h, "rollout"); })) return rc;
  return timed_end(h, MYR_K_ROLLOUT);
}

extern "C" int myr_rollout(myr_handle h, int32_t B, int32_t num_steps, int32_t u_rows, const double* x0, const double* us,
                           const double* params, int32_t params_stride, double* xs, double* cost, int32_t mem) {
  const char* who = "myr_rollout";
  if (!h || !x0 || !us) return fail(MYR_E_ARG, "myr_rollout: null handle, x0 or us");
  if (h->d.system_id == MYR_SYS_INVASIVEPLANT) return no_such_path(h, who);
  if (B < 0 || num_steps < 1 || u_rows < 1) return fail(MYR_E_ARG, "myr_rollout: bad sizes");
  if (B == 0) return MYR_OK;
  if (int rc = check_stride(h, who, params, params_stride)) return rc;
  if (int rc = check_node_weights(h, who, params)) return rc;
  HIPCHK(hipSetDevice(h->d.device));
  if (int rc = check_mem(who, mem)) return rc;
  const myr_dims& dm = h->dims;
  RolloutArgs a{B, num_steps, u_rows, nullptr, nullptr, nullptr, params_stride, nullptr, nullptr};
  DevStage st = call_stage(h, mem);
  st.in(a.x0, x0, (size_t)B * dm.ns);
  st.in(a.us, us, (size_t)B * u_rows * dm.nu);
  st.in(a.params, params, n_params(h, params, params_stride, B));
  st.out(a.xs, xs, (size_t)B * (num_steps + 1) * dm.ns);
  st.out(a.cost, cost, (size_t)B);
  if (int rc = st.commit()) return rc;
  if (int rc = dispatch_rollout(h, a)) return rc;
  return st.finish();
}

// Sum of the per-trajectory gradient rows in a fixed order, for each of E parameter sets of R rows (rows [E][R][np] -> out [E][np]; grid np * E): block
// (k, e) owns entry k of set e; thread t adds rows t, t + 256, ... of that set in ascending order, then the 256 partial sums meet in a fixed tree.  No
// atomics: the same bits on every call, and a set's sums have the bits of a call on that set alone.  The sum over a whole batch is the call with one set
// (E = 1, R = B): block k then runs the additions of the one-set kernel this replaces (out[k] = sum over b of rows[b * np + k], thread t taking b = t,
// t + 256, ..., the same tree) in the same order, so those bits are unchanged.  (Neighbouring threads read rows np apart -- not coalesced: the kernel
// reads E * R * np doubles once, and the rows keep the layout the caller gets with grad_stride == np.)
static __global__ __launch_bounds__(256) void fit_reduce_sets_kernel(int R, int np, const double* __restrict__ rows, double* __restrict__ out) {
  __shared__ double part[256];
  const int k = (int)(blockIdx.x % (unsigned)np), t = threadIdx.x;
  const long e = blockIdx.x / (unsigned)np;
  rows += e * (long)R * np;
  double a = 0.0;
  for (long b = t; b < R; b += 256) a += rows[b * np + k];
  part[t] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  if (t == 0) out[e * np + k] = part[0];
}

// parameter sets one launch of dispatch_fit takes: all of them, unless the per-set sums are asked for and the row scratch (E R np doubles) would pass
// 1 GiB -- then whole sets, at least one; and never more than 2^30 trajectories (the kernels count them in an int)
static int fit_sets_chunk(int E, int R, bool row_scratch, size_t width) {      // width: doubles of one trajectory's row (np; myr_fit_gn*: np + np^2)
  size_t chunk = (size_t)E;
  if (row_scratch) {
    size_t bound = (size_t)1 << 30;
    if (const char* e = getenv("MYRIAD_FIT_ROWS_BYTES")) { const long long v = atoll(e); if (v > 0) bound = (size_t)v; }      // tests: force the chunked path
    chunk = bound / ((size_t)R * (width > 0 ? width : 1) * 8);
  }
  const size_t cap = ((size_t)1 << 30) / (size_t)R;
  if (chunk > cap) chunk = cap;
  return (int)(chunk < 1 ? 1 : (chunk > (size_t)E ? (size_t)E : chunk));
}

// sums [E][np + np^2] (the packed per-set sums fit_reduce_sets_kernel leaves for myr_fit_gn*) -> grad [E][np] (or null) and gn [E][np][np]: a copy, one
// thread per entry
static __global__ __launch_bounds__(256) void fit_gn_unpack_kernel(long n, int np, const double* __restrict__ sums, double* __restrict__ grad,
                                                                   double* __restrict__ gn) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int ng = np + np * np;
  const long e = i / ng;
  const int k = (int)(i - e * ng);
  if (k < np) {
    if (grad) grad[e * np + k] = sums[i];
  } else {
    gn[e * (long)np * np + (k - np)] = sums[i];
  }
}

// device pointers throughout (a.Bp, a.xh are set here); a.grad: [E][R][np] rows (grad_stride == np), the [E][np] per-set sums (grad_stride == 0, rows in
// sbuf) or null (the loss only).  The sets run in chunks of fit_sets_chunk (launches on one stream: a chunk starts when the one before has ended); a
// trajectory's arithmetic does not depend on the chunk it runs in.
// With a.gn (myr_fit_gn*) the forward-sensitivity kernel runs instead: no state scratch; a.gn is [E][R][np][np] beside a.grad (which may then be null
// with either stride), or -- grad_stride == 0 -- [E][np][np] beside [E][np]: the lanes write packed rows [np + np^2], grad then gn, ONE reduction of
// that width sums them per set in the same fixed order, and a copy takes the sums apart into the two arrays.
// With FIT_GNVP (myr_fit_gnvp*) a.grad is the product, with the strides and the reduction of the gradient; a second scratch of xh's shape (a.dxh) holds
// the tangent, and a.v, a.jv advance with the sets of a chunk.
static int launch_fit(myr_handle h, const FitArgs& a) {      // the kernel by a.mode
  return for_system(h->d.system_id, true, [&](auto t) { return a.mode == FIT_GN ? fit_gn_for_system<SYS_OF(t)>(h, a) : fit_for_system<SYS_OF(t)>(h, a); },
                    [] { return (int)MYR_OK; });
}
static int dispatch_fit(myr_handle h, FitArgs a, int grad_stride) {
  const myr_dims& dm = h->dims;
  const bool gnm = a.mode == FIT_GN, gnvp = a.mode == FIT_GNVP;
  // refused before anything is sized by the system's np, and before the timer starts: begin and end stay paired
  if (int rc = check_fit_has_derivatives(h, gnm ? "myr_fit_gn" : "myr_fit_grad")) return rc;
  const size_t np = (size_t)dm.np, width = gnm ? np + np * np : np;
  const bool sums = (a.grad || gnm) && !grad_stride;
  const int E = a.E, chunk = fit_sets_chunk(E, a.R, sums, width);
  const size_t S1 = (size_t)a.num_steps + 1;
  const double *xs_obs = a.xs_obs, *us = a.us, *params = a.params, *v = a.v;
  double *const loss = a.loss, *const out = a.grad, *const out_gn = a.gn, *const jv = a.jv, *rows = nullptr, *packed = nullptr;
  a.Bp = padded_lanes((int)((long)chunk * a.R));
  DevStage st = scratch_stage(h, &h->sbuf, &h->sbuf_bytes);
  if (!gnm) st.scratch(a.xh, S1 * dm.ns * (size_t)a.Bp);
  if (gnvp) st.scratch(a.dxh, S1 * dm.ns * (size_t)a.Bp);
  if (sums) st.scratch(rows, (size_t)chunk * a.R * width);
  if (sums && gnm) st.scratch(packed, (size_t)chunk * width);
  if (int rc = st.commit()) return rc;
  if (int rc = timed_begin(h, MYR_K_FIT)) return rc;
  int rc = MYR_OK;
  for (int e0 = 0; e0 < E && !rc; e0 += chunk) {
    const size_t r0 = (size_t)e0 * a.R, d0 = a.data_shared ? 0 : r0;
    a.E = E - e0 < chunk ? E - e0 : chunk;
    a.xs_obs = xs_obs + d0 * S1 * dm.ns;
    a.us = us + d0 * a.u_rows * dm.nu;
    a.params = params ? params + (size_t)e0 * dm.np : nullptr;      // (per_row: one set, e0 = 0)
    a.loss = loss ? loss + r0 : nullptr;
    a.v = v ? v + (size_t)e0 * dm.np : nullptr;
    a.jv = jv ? jv + r0 * S1 * dm.ns : nullptr;
    a.grad = sums ? rows : (out ? out + r0 * np : nullptr);
    a.gn = !gnm ? nullptr : (sums ? rows + np : out_gn + r0 * np * np);
    a.grad_ld = (long)(sums ? width : np);               // (the two row lengths: read by the Gauss-Newton kernel only)
    a.gn_ld = (long)(sums ? width : np * np);
    rc = launch_fit(h, a);
    if (!rc && sums)      // one reduction of a row's whole width; the Gauss-Newton sums come out packed ...
      hipLaunchKernelGGL(fit_reduce_sets_kernel, dim3((unsigned)width * (unsigned)a.E), dim3(256), 0, h->stream, a.R, (int)width, (const double*)rows,
                         gnm ? packed : out + (size_t)e0 * np);
    if (!rc && sums && gnm) {      // ... and a copy takes them apart
      const long n = (long)a.E * (long)width;
      hipLaunchKernelGGL(fit_gn_unpack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, (int)np, (const double*)packed,
                         out ? out + (size_t)e0 * np : nullptr, out_gn + (size_t)e0 * np * np);
    }
  }
  const int rc_end = timed_end(h, MYR_K_FIT);          // on every path
  return rc ? rc : rc_end;
}

// What the four fit entry points do behind their checks: E parameter sets of R trajectories each (the single-set calls: E = 1, R = B).  params holds
// n_par doubles -- [E][np], or for a single-set call whatever its stride says: nothing, one set, or with per_row a row per trajectory.  row_stride is
// grad_stride / out_stride (np: a row of results per trajectory, 0: their sum per set); gn is null for myr_fit_grad*.
// myr_fit_gnvp*: v ([E][np], non-null: the mode) and jv ([E][R][num_steps+1][ns] or null) beside them; grad is then the product and may be null.
static int run_fit(myr_handle h, int32_t mem, int E, int R, int data_shared, int num_steps, int u_rows, const double* xs_obs, const double* us,
                   const double* wt, const double* params, size_t n_par, bool per_row, double* loss, double* grad, double* gn, int row_stride,
                   const double* v = nullptr, double* jv = nullptr) {
  HIPCHK(hipSetDevice(h->d.device));
  const myr_dims& dm = h->dims;
  const size_t np = (size_t)dm.np, rows = (size_t)E * R, drows = data_shared ? (size_t)R : rows, nout = row_stride ? rows : (size_t)E;
  FitArgs a{};
  a.E = E; a.R = R; a.data_shared = data_shared; a.num_steps = num_steps; a.u_rows = u_rows; a.per_row = per_row;
  a.mode = v ? FIT_GNVP : (gn ? FIT_GN : FIT_GRAD);
  DevStage st = call_stage(h, mem);
  st.in(a.xs_obs, xs_obs, drows * (num_steps + 1) * dm.ns);
  st.in(a.us, us, drows * u_rows * dm.nu);
  st.in(a.wt, wt, (size_t)num_steps + 1);
  st.in(a.params, params, n_par);
  st.in(a.v, v, (size_t)E * np);
  st.out(a.loss, loss, rows);
  st.out(a.grad, grad, nout * np);
  st.out(a.gn, gn, nout * np * np);
  st.out(a.jv, jv, rows * (num_steps + 1) * dm.ns);
  if (int rc = st.commit()) return rc;
  if (int rc = dispatch_fit(h, a, row_stride)) return rc;
  return st.finish();
}

// The four entry points: each its checks, in its own order -- myr_fit_grad looks at the system before its sizes, the other three at every argument
// first (tests/test_gpu_api.py holds the order of each, fault by fault) --, then run_fit.
extern "C" int myr_fit_grad(myr_handle h, int32_t B, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us,
                            const double* wt, const double* params, int32_t params_stride, double* loss, double* grad,
                            int32_t grad_stride, int32_t mem) {
  const char* who = "myr_fit_grad";
  if (!h || !xs_obs || !us || !grad) return arg_fail(who, MYR_E_ARG, "null handle, xs_obs, us or grad");
  if (int rc = check_fit_not_plant(h, who)) return rc;
  if (int rc = check_fit_not_twin(h)) return rc;
  if (int rc = check_fit_sizes(who, B, 1, num_steps, u_rows)) return rc;
  if (int rc = check_row_stride(h, who, "grad_stride", grad_stride, ROW_SUM_BATCH, "trajectory")) return rc;
  if (int rc = check_stride(h, who, params, params_stride)) return rc;
  if (int rc = check_node_weights(h, who, params)) return rc;
  if (h->d.system_id == MYR_SYS_NODE_CARTPOLE && params_stride != 0)
    return arg_fail(who, MYR_E_UNSUPPORTED, "a NODE system takes one shared set of weights (params_stride 0)");
  if (int rc = check_mem(who, mem)) return rc;
  if (B == 0) return MYR_OK;                          // (nothing is written)
  return run_fit(h, mem, 1, B, 0, num_steps, u_rows, xs_obs, us, wt, params, n_params(h, params, params_stride, B), params && params_stride != 0,
                 loss, grad, nullptr, grad_stride);
}

extern "C" int myr_fit_grad_sets(myr_handle h, int32_t E, int32_t R, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us,
                                 int32_t data_shared, const double* wt, const double* params, double* loss, double* grad, int32_t grad_stride,
                                 int32_t mem) {
  const char* who = "myr_fit_grad_sets";
  if (!h || !xs_obs || !us || !params) return arg_fail(who, MYR_E_ARG, "null handle, xs_obs, us or params");
  if (!loss && !grad) return arg_fail(who, MYR_E_ARG, "loss and grad are both null");
  if (int rc = check_fit_sizes(who, E, R, num_steps, u_rows)) return rc;
  if (int rc = check_row_stride(h, who, "grad_stride", grad_stride, ROW_SUM_FIT_SETS, "trajectory")) return rc;
  if (int rc = check_data_shared(who, data_shared)) return rc;
  if (int rc = check_mem(who, mem)) return rc;
  if (int rc = check_fit_not_plant(h, who)) return rc;
  if (int rc = check_fit_not_twin(h)) return rc;
  if (int rc = check_fit_has_derivatives(h, who)) return rc;
  if (E == 0) return MYR_OK;                          // (nothing is written)
  return run_fit(h, mem, E, R, data_shared, num_steps, u_rows, xs_obs, us, wt, params, (size_t)E * h->dims.np, false, loss, grad, nullptr, grad_stride);
}

// the refusals myr_fit_gn and myr_fit_gn_sets share, behind their argument checks: the network system, then myr_fit_grad_sets's
static int check_fit_gn_system(myr_handle h, const char* who) {
  if (int rc = check_fit_gn_not_node(h, who)) return rc;
  if (int rc = check_fit_not_twin(h)) return rc;
  if (int rc = check_fit_not_plant(h, who)) return rc;
  return check_fit_has_derivatives(h, who);
}

extern "C" int myr_fit_gn(myr_handle h, int32_t B, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us,
                          const double* wt, const double* params, int32_t params_stride, double* loss, double* grad, double* gn,
                          int32_t out_stride, int32_t mem) {
  const char* who = "myr_fit_gn";
  if (!h || !xs_obs || !us || !gn) return arg_fail(who, MYR_E_ARG, "null handle, xs_obs, us or gn");
  if (int rc = check_fit_sizes(who, B, 1, num_steps, u_rows)) return rc;
  if (int rc = check_row_stride(h, who, "out_stride", out_stride, ROW_SUM_BATCH, "trajectory")) return rc;
  if (int rc = check_stride(h, who, params, params_stride)) return rc;
  if (int rc = check_mem(who, mem)) return rc;
  if (int rc = check_fit_gn_system(h, who)) return rc;
  if (B == 0) return MYR_OK;                          // (nothing is written)
  return run_fit(h, mem, 1, B, 0, num_steps, u_rows, xs_obs, us, wt, params, n_params(h, params, params_stride, B), params && params_stride != 0,
                 loss, grad, gn, out_stride);
}

extern "C" int myr_fit_gn_sets(myr_handle h, int32_t E, int32_t R, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us,
                               int32_t data_shared, const double* wt, const double* params, double* loss, double* grad, double* gn,
                               int32_t out_stride, int32_t mem) {
  const char* who = "myr_fit_gn_sets";
  if (!h || !xs_obs || !us || !gn || !params) return arg_fail(who, MYR_E_ARG, "null handle, xs_obs, us, gn or params");
  if (int rc = check_fit_sizes(who, E, R, num_steps, u_rows, true)) return rc;
  if (int rc = check_row_stride(h, who, "out_stride", out_stride, ROW_SUM_FIT_SETS, "trajectory")) return rc;
  if (int rc = check_data_shared(who, data_shared)) return rc;
  if (int rc = check_mem(who, mem)) return rc;
  if (int rc = check_fit_gn_system(h, who)) return rc;
  if (E == 0) return MYR_OK;                          // (nothing is written)
  return run_fit(h, mem, E, R, data_shared, num_steps, u_rows, xs_obs, us, wt, params, (size_t)E * h->dims.np, false, loss, grad, gn, out_stride);
}

// The Gauss-Newton product of the network fit (fit.h: node_fit_gnvp_kernel).  The checks the two calls share, in the order the header gives: the
// arguments, then the system -- every handle but the network's is sent to myr_fit_gn, where gn is formed and the caller can multiply.
static int check_fit_gnvp(myr_handle h, const char* who, const void* xs_obs, const void* us, const void* params, const void* v, const void* jv,
                          const void* out, int sets, int R, int num_steps, int u_rows, int out_stride, const char* zero, int data_shared, int mem) {
  if (!h || !xs_obs || !us || !params || !v) return arg_fail(who, MYR_E_ARG, "null handle, xs_obs, us, params or v");
  if (!jv && !out) return arg_fail(who, MYR_E_ARG, "jv and out are both null");
  if (int rc = check_fit_sizes(who, sets, R, num_steps, u_rows, true)) return rc;
  if (int rc = check_row_stride(h, who, "out_stride", out_stride, zero, "trajectory")) return rc;
  if (int rc = check_data_shared(who, data_shared)) return rc;
  if (int rc = check_mem(who, mem)) return rc;
  if (h->d.system_id != MYR_SYS_NODE_CARTPOLE)
    return arg_fail(who, MYR_E_UNSUPPORTED, "the network system only: the matrix-free product lives here because its 4 804 x 4 804 matrix is not formed.  "
                                            "For a closed-form system use myr_fit_gn, which forms gn, and multiply");
  return MYR_OK;
}

extern "C" int myr_fit_gnvp(myr_handle h, int32_t B, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us, const double* wt,
                            const double* params, const double* v, double* jv, double* out, int32_t out_stride, int32_t mem) {
  const char* who = "myr_fit_gnvp";
  if (int rc = check_fit_gnvp(h, who, xs_obs, us, params, v, jv, out, B, 1, num_steps, u_rows, out_stride, ROW_SUM_BATCH, 0, mem)) return rc;
  if (B == 0) return MYR_OK;                          // (nothing is written)
  return run_fit(h, mem, 1, B, 0, num_steps, u_rows, xs_obs, us, wt, params, (size_t)h->dims.np, false, nullptr, out, nullptr, out_stride, v, jv);
}

extern "C" int myr_fit_gnvp_sets(myr_handle h, int32_t E, int32_t R, int32_t num_steps, int32_t u_rows, const double* xs_obs, const double* us,
                                 int32_t data_shared, const double* wt, const double* params, const double* v, double* jv, double* out,
                                 int32_t out_stride, int32_t mem) {
  const char* who = "myr_fit_gnvp_sets";
  if (int rc = check_fit_gnvp(h, who, xs_obs, us, params, v, jv, out, E, R, num_steps, u_rows, out_stride, ROW_SUM_FIT_SETS, data_shared, mem)) return rc;
  if (E == 0) return MYR_OK;                          // (nothing is written)
  return run_fit(h, mem, E, R, data_shared, num_steps, u_rows, xs_obs, us, wt, params, (size_t)E * h->dims.np, false, nullptr, out, nullptr, out_stride, v, jv);
}

// history of one instance of myr_exgd_grad*: x_s, x_bar_s, lam_s of every step and the final x (`per` doubles); the batch runs in chunks of the
// returned number of instances where the whole would pass the bound
static int exgd_grad_chunk(myr_handle h, int B, int nsteps, size_t* per) {
  const myr_dims& dm = h->dims;
  *per = (size_t)nsteps * (2 * (size_t)dm.n + dm.m) + dm.n;
  size_t bound = (size_t)1 << 30;
  if (const char* e = getenv("MYRIAD_EXGD_GRAD_HIST_BYTES")) { const long long v = atoll(e); if (v > 0) bound = (size_t)v; }      // tests: force the chunked path
  const size_t chunk = bound / (*per * 8);
  return (int)(chunk < 1 ? 1 : (chunk > (size_t)B ? (size_t)B : chunk));
}

// device pointers throughout (a.hist, a.chunk, under EXGD_GRAD_SHOOT a.work and a.Pp and, for the batch sum, a.rows are set here); grad: [B][np] rows
// (grad_stride == np) or, per weight set of a.R instances, the sum of its rows in fit_reduce_sets_kernel's fixed order: [B / R][np] (the closed-form
// routes and the single-set network calls have R = B: one row, the sum over the batch)
// EXGD_JAC (myr_exgd_jac: forward mode) has no history, rows or reduction: one launch between the timers
enum { EXGD_GRAD_CLOSED_FORM = 0, EXGD_GRAD_NODE = 1, EXGD_GRAD_NODE_SHOOT = 2, EXGD_GRAD_SHOOT = 3, EXGD_JAC = 4 };      // which kernel family runs the sweep
static int dispatch_exgd_grad(myr_handle h, ExgdGradArgs a, double* grad, int grad_stride, int route) {
  const myr_dims& dm = h->dims;
  const long I = h->d.intervals;
  if (route == EXGD_JAC) {
    if (int rc = timed_begin(h, MYR_K_PROD)) return rc;
    const int rc = for_system(h->d.system_id, true, [&](auto t) { return exgd_jac_for_system<SYS_OF(t)>(h, a); }, [] { return (int)MYR_OK; });
    const int rc_end = timed_end(h, MYR_K_PROD);          // on every path
    return rc ? rc : rc_end;
  }
  if (route == EXGD_GRAD_SHOOT && (long)a.B * I > (1L << 30))
    return fail(MYR_E_CAPACITY, "myr_exgd_grad_shoot: more than 2^30 (instance, interval) pairs in one call");
  size_t per;
  a.chunk = exgd_grad_chunk(h, a.B, a.nsteps, &per);
  DevStage st = scratch_stage(h, &h->sbuf, &h->sbuf_bytes);
  st.scratch(a.hist, (size_t)a.chunk * per);
  if (route == EXGD_GRAD_SHOOT) {      // a column per pair of the chunk
    a.Pp = ((long)a.chunk * I + 63) / 64 * 64;
    if (((a.Pp / 64) & 1) == 0) a.Pp += 64;      // an odd number of wavefronts, as padded_lanes
    st.scratch(a.work, shoot_exgd_grad_work_doubles(h, (size_t)a.chunk, (size_t)a.Pp));
  }
  if (grad_stride) a.rows = grad;
  else st.scratch(a.rows, (size_t)a.B * dm.np);
  if (int rc = st.commit()) return rc;
  if (int rc = timed_begin(h, MYR_K_PROD)) return rc;
  const int rc = route == EXGD_GRAD_NODE_SHOOT ? exgd_grad_node_shoot_for_system<SysNODE_CARTPOLE>(h, a)
                 : route == EXGD_GRAD_NODE ? exgd_grad_node_for_system<SysNODE_CARTPOLE>(h, a)
                 : route == EXGD_GRAD_SHOOT
                     ? for_system(h->d.system_id, true, [&](auto t) { return exgd_grad_shoot_for_system<SYS_OF(t)>(h, a); }, [] { return (int)MYR_OK; })
                     : for_system(h->d.system_id, true, [&](auto t) { return exgd_grad_for_system<SYS_OF(t)>(h, a); }, [] { return (int)MYR_OK; });
  if (!rc && !grad_stride)
    hipLaunchKernelGGL(fit_reduce_sets_kernel, dim3((unsigned)dm.np * (unsigned)(a.B / a.R)), dim3(256), 0, h->stream, a.R, (int)dm.np, (const double*)a.rows,
                       grad);
  const int rc_end = timed_end(h, MYR_K_PROD);          // on every path
  return rc ? rc : rc_end;
}

// what the five myr_exgd_grad* entry points and myr_exgd_jac share behind their own checks: the staging, the sweep of `route`, the copies back.
// n_param_doubles: what `params` holds (a row per instance, or one shared set; the network routes: a set for every R instances, B / R sets)
// jac (route EXGD_JAC only; then seeds, grad, dz0, dlam0 are null): the caller's tangent inputs and outputs, staged like the rest
struct ExgdJacIO { const double *jz0, *jlam0; double *zn, *lamn, *jz, *jlam; };
static int run_exgd_grad(myr_handle h, int route, int mem, int B, int R, const double* z, const double* lam, const double* lb, const double* ub,
                         const double* params, size_t n_param_doubles, int pstride, double eta_x, double eta_v, int nsteps, const double* seed_z,
                         const double* seed_lam, double* grad, int grad_stride, double* dz0, double* dlam0, const ExgdJacIO* jac = nullptr) {
  if (B == 0) return MYR_OK;                          // (nothing is written)
  HIPCHK(hipSetDevice(h->d.device));
  const myr_dims& dm = h->dims;
  const size_t nz = (size_t)B * dm.n, nl = (size_t)B * dm.m;
  ExgdGradArgs a{};
  a.B = B; a.R = R; a.pstride = pstride; a.eta_x = eta_x; a.eta_v = eta_v; a.nsteps = nsteps;
  double* g = nullptr;
  DevStage st = call_stage(h, mem);
  st.in(a.z, z, nz);
  st.in(a.lb, lb, nz);
  st.in(a.ub, ub, nz);
  st.in(a.lam, lam, nl);
  st.in(a.params, params, n_param_doubles);
  st.in(a.seed_z, seed_z, nz);
  st.in(a.seed_lam, seed_lam, nl);
  st.out(g, grad, grad_stride ? (size_t)B * dm.np : (size_t)(B / R) * dm.np);
  st.out(a.dz0, dz0, nz);
  st.out(a.dlam0, dlam0, nl);
  if (jac) {
    st.in(a.jz0, jac->jz0, nz * dm.np);
    st.in(a.jlam0, jac->jlam0, nl * dm.np);
    st.out(a.zn, jac->zn, nz);
    st.out(a.lamn, jac->lamn, nl);
    st.out(a.jz, jac->jz, nz * dm.np);
    st.out(a.jlam, jac->jlam, nl * dm.np);
  }
  if (int rc = st.commit()) return rc;
  if (int rc = dispatch_exgd_grad(h, a, g, grad_stride, route)) return rc;
  return st.finish();
}

extern "C" int myr_exgd_grad(myr_handle h, int32_t B, const double* z, const double* lam, const double* lb, const double* ub, const double* params,
                             int32_t params_stride, double eta_x, double eta_v, int32_t nsteps, const double* seed_z, const double* seed_lam,
                             double* grad, int32_t grad_stride, double* dz0, double* dlam0, int32_t mem) {
  const char* who = "myr_exgd_grad";
  if (int rc = check_products_args(h, who, B, z, lam, lb, params, params_stride)) return rc;
  if (int rc = check_ub(who, ub)) return rc;
  if (int rc = check_steps_and_seed(who, nsteps, seed_z, grad)) return rc;
  if (int rc = check_row_stride(h, who, "grad_stride", grad_stride, ROW_SUM_BATCH, "instance")) return rc;
  if (h->d.system_id >= 100) return fail(MYR_E_UNSUPPORTED, "myr_exgd_grad: an elastic twin has no model of its own to differentiate; use the handle of its system");
  if (h->d.system_id == MYR_SYS_NODE_CARTPOLE)
    return fail(MYR_E_UNSUPPORTED, "myr_exgd_grad: the network system is not built (second derivatives in 4 804 weights)");
  if (h->d.transcription == MYR_TR_SHOOTING)
    return fail(MYR_E_UNSUPPORTED, "myr_exgd_grad: SHOOTING is not built (it needs the second-order adjoint of the rollout); use a collocation transcription");
  if (int rc = check_mem(who, mem)) return rc;
  return run_exgd_grad(h, EXGD_GRAD_CLOSED_FORM, mem, B, B, z, lam, lb, ub, params, n_params(h, params, params_stride, B), params_stride, eta_x, eta_v, nsteps,
                       seed_z, seed_lam, grad, grad_stride, dz0, dlam0);
}

// the forward-mode Jacobian of the same steps (exgd_jac.h): every argument check first, then the refusals of myr_exgd_grad, then the LDS bound
extern "C" int myr_exgd_jac(myr_handle h, int32_t B, const double* z, const double* lam, const double* lb, const double* ub, const double* params,
                            int32_t params_stride, double eta_x, double eta_v, int32_t nsteps, const double* jz0, const double* jlam0, double* zn,
                            double* lamn, double* jz, double* jlam, int32_t mem) {
  const char* who = "myr_exgd_jac";
  if (int rc = check_handle_and_arrays(who, h, z, lam, lb)) return rc;
  if (int rc = check_ub(who, ub)) return rc;
  if (!jz && !jlam) return arg_fail(who, MYR_E_ARG, "jz and jlam are both null");
  if (int rc = check_batch(who, B)) return rc;
  if (nsteps < 0) return arg_fail(who, MYR_E_ARG, "negative nsteps");
  if (int rc = check_stride(h, who, params, params_stride)) return rc;
  if (int rc = check_mem(who, mem)) return rc;
  if (h->d.transcription == MYR_TR_SHOOTING && h->d.system_id != MYR_SYS_INVASIVEPLANT)
    return arg_fail(who, MYR_E_UNSUPPORTED, "SHOOTING is not built; use myr_exgd_grad_shoot (myr_exgd_grad_node_shoot for the network system) for seeded rows, or a collocation transcription");
  if (h->d.system_id == MYR_SYS_NODE_CARTPOLE)
    return arg_fail(who, MYR_E_UNSUPPORTED, "the network system is not built (4 804 tangent columns are reverse mode's case); use myr_exgd_grad_node");
  if (h->d.system_id >= 100) return arg_fail(who, MYR_E_UNSUPPORTED, "an elastic twin has no model of its own to differentiate; use the handle of its system");
  if (h->d.system_id == MYR_SYS_INVASIVEPLANT) return no_such_path(h, who);
  if (!for_system(h->d.system_id, false, [](auto t) { return (int)SysDpw<SYS_OF(t)>::SUPPORTED; }, [] { return 0; }))
    return arg_fail(who, MYR_E_UNSUPPORTED, "this system has no generated parameter derivatives; myr_exgd and differences in the parameters remain");
  const ExgdJacIO io{jz0, jlam0, zn, lamn, jz, jlam};
  return run_exgd_grad(h, EXGD_JAC, mem, B, B, z, lam, lb, ub, params, n_params(h, params, params_stride, B), params_stride, eta_x, eta_v, nsteps, nullptr,
                       nullptr, nullptr, h->dims.np, nullptr, nullptr, &io);
}

// the same call for the weights of the network system: one shared weight set (no params_stride), Hermite-Simpson
extern "C" int myr_exgd_grad_node(myr_handle h, int32_t B, const double* z, const double* lam, const double* lb, const double* ub, const double* params,
                                  double eta_x, double eta_v, int32_t nsteps, const double* seed_z, const double* seed_lam, double* grad,
                                  int32_t grad_stride, double* dz0, double* dlam0, int32_t mem) {
  const char* who = "myr_exgd_grad_node";
  if (int rc = check_handle_and_arrays(who, h, z, lam, lb)) return rc;
  if (int rc = check_ub(who, ub)) return rc;
  if (int rc = check_batch(who, B)) return rc;
  if (int rc = check_steps_and_seed(who, nsteps, seed_z, grad)) return rc;
  if (int rc = check_is_node(h, who, "myr_exgd_grad")) return rc;
  if (h->d.transcription != MYR_TR_HERMITE_SIMPSON)
    return arg_fail(who, MYR_E_UNSUPPORTED, "HERMITE_SIMPSON only, the one transcription myr_vjp / myr_exgd build for the network system");
  if (int rc = check_node_weights(h, who, params)) return rc;
  if (int rc = check_row_stride(h, who, "grad_stride", grad_stride, ROW_SUM_BATCH, "instance")) return rc;
  if (int rc = check_mem(who, mem)) return rc;
  if (int rc = check_node_lds(h, who, NODE_LDS_EXGD_GRAD)) return rc;
  return run_exgd_grad(h, EXGD_GRAD_NODE, mem, B, B, z, lam, lb, ub, params, (size_t)h->dims.np, 0, eta_x, eta_v, nsteps, seed_z, seed_lam, grad, grad_stride,
                       dz0, dlam0);
}

// ... and under SHOOTING (node_shoot_exgd_grad.h): the arguments, null rules and outputs of myr_exgd_grad_node
extern "C" int myr_exgd_grad_node_shoot(myr_handle h, int32_t B, const double* z, const double* lam, const double* lb, const double* ub,
                                        const double* params, double eta_x, double eta_v, int32_t nsteps, const double* seed_z, const double* seed_lam,
                                        double* grad, int32_t grad_stride, double* dz0, double* dlam0, int32_t mem) {
  const char* who = "myr_exgd_grad_node_shoot";
  if (int rc = check_handle_and_arrays(who, h, z, lam, lb)) return rc;
  if (int rc = check_ub(who, ub)) return rc;
  if (int rc = check_batch(who, B)) return rc;
  if (int rc = check_steps_and_seed(who, nsteps, seed_z, grad)) return rc;
  if (int rc = check_is_node(h, who, "myr_exgd_grad_shoot")) return rc;
  if (h->d.transcription == MYR_TR_HERMITE_SIMPSON)
    return arg_fail(who, MYR_E_UNSUPPORTED, "this handle's transcription is HERMITE_SIMPSON, not SHOOTING; use myr_exgd_grad_node");
  if (int rc = check_node_not_trapezoidal(h, who, "SHOOTING")) return rc;
  if (int rc = check_node_weights(h, who, params)) return rc;
  if (int rc = check_row_stride(h, who, "grad_stride", grad_stride, ROW_SUM_BATCH, "instance")) return rc;
  if (int rc = check_mem(who, mem)) return rc;
  if (int rc = check_node_lds(h, who, NODE_LDS_EXGD_GRAD)) return rc;
  return run_exgd_grad(h, EXGD_GRAD_NODE_SHOOT, mem, B, B, z, lam, lb, ub, params, (size_t)h->dims.np, 0, eta_x, eta_v, nsteps, seed_z, seed_lam, grad,
                       grad_stride, dz0, dlam0);
}

// ... and for E weight sets of R instances each in one call, under either transcription of the network system: the two calls above are its E = 1,
// R = B case (run_exgd_grad with R = B).  Set e has the bits of the single-set call on that set alone
extern "C" int myr_exgd_grad_node_sets(myr_handle h, int32_t E, int32_t R, const double* z, const double* lam, const double* lb, const double* ub,
                                       const double* params, double eta_x, double eta_v, int32_t nsteps, const double* seed_z, const double* seed_lam,
                                       double* grad, int32_t grad_stride, double* dz0, double* dlam0, int32_t mem) {
  const char* who = "myr_exgd_grad_node_sets";
  if (int rc = check_handle_and_arrays(who, h, z, lam, lb)) return rc;
  if (int rc = check_ub(who, ub)) return rc;
  if (int rc = check_sets(who, E, R)) return rc;
  if (int rc = check_steps_and_seed(who, nsteps, seed_z, grad)) return rc;
  if (int rc = check_is_node(h, who, "myr_exgd_grad or myr_exgd_grad_shoot")) return rc;
  if (int rc = check_node_not_trapezoidal(h, who, "HERMITE_SIMPSON and SHOOTING")) return rc;
  if (int rc = check_weight_sets(who, params)) return rc;
  if (int rc = check_row_stride(h, who, "grad_stride", grad_stride, ROW_SUM_SETS, "instance")) return rc;
  if (int rc = check_mem(who, mem)) return rc;
  if (int rc = check_node_lds(h, who, NODE_LDS_EXGD_GRAD)) return rc;
  return run_exgd_grad(h, h->d.transcription == MYR_TR_SHOOTING ? EXGD_GRAD_NODE_SHOOT : EXGD_GRAD_NODE, mem, E * R, R, z, lam, lb, ub, params, (size_t)E * h->dims.np, 0, eta_x, eta_v, nsteps,
                       seed_z, seed_lam, grad, grad_stride, dz0, dlam0);
}

// the same derivative under SHOOTING (shoot_exgd_grad.h)
extern "C" int myr_exgd_grad_shoot(myr_handle h, int32_t B, const double* z, const double* lam, const double* lb, const double* ub, const double* params,
                                   int32_t params_stride, double eta_x, double eta_v, int32_t nsteps, const double* seed_z, const double* seed_lam,
                                   double* grad, int32_t grad_stride, double* dz0, double* dlam0, int32_t mem) {
  const char* who = "myr_exgd_grad_shoot";
  if (int rc = check_products_args(h, who, B, z, lam, lb, params, params_stride)) return rc;
  if (int rc = check_ub(who, ub)) return rc;
  if (int rc = check_steps_and_seed(who, nsteps, seed_z, grad)) return rc;
  if (int rc = check_row_stride(h, who, "grad_stride", grad_stride, ROW_SUM_BATCH, "instance")) return rc;
  if (h->d.system_id >= 100)
    return fail(MYR_E_UNSUPPORTED, "myr_exgd_grad_shoot: an elastic twin has no model of its own to differentiate; use the handle of its system");
  if (h->d.system_id == MYR_SYS_NODE_CARTPOLE)
    return fail(MYR_E_UNSUPPORTED, "myr_exgd_grad_shoot: the network system is not built (second derivatives in 4 804 weights); myr_exgd_grad_node has HERMITE_SIMPSON");
  if (h->d.transcription != MYR_TR_SHOOTING)
    return fail(MYR_E_UNSUPPORTED, "myr_exgd_grad_shoot: this handle's transcription is not SHOOTING; use myr_exgd_grad");
  if (int rc = check_mem(who, mem)) return rc;
  return run_exgd_grad(h, EXGD_GRAD_SHOOT, mem, B, B, z, lam, lb, ub, params, n_params(h, params, params_stride, B), params_stride, eta_x, eta_v, nsteps,
                       seed_z, seed_lam, grad, grad_stride, dz0, dlam0);
}

// device pointers throughout (a.hist, a.side, a.Pp and, for the sums, a.rows are set here); out_p: [B][np] rows (p_stride == np), per weight set of a.R
// instances the sum of its rows in fit_reduce_sets_kernel's fixed order, [B / R][np] (myr_hvp and myr_hvp_node have R = B: one row), or null
enum { HVP_CLOSED_FORM = 0, HVP_NODE = 1 };      // which kernel family runs the product (node_hvp.h for the network system)
static int dispatch_hvp(myr_handle h, HvpArgs a, double* out_p, int p_stride, int route) {
  const myr_dims& dm = h->dims;
  const bool shoot = h->d.transcription == MYR_TR_SHOOTING, node = route == HVP_NODE;
  const int kt = !node ? MYR_K_PROD : shoot ? MYR_K_HVP_NODE_SHOOT : MYR_K_HVP_NODE;
  DevStage st = scratch_stage(h, &h->sbuf, &h->sbuf_bytes);
  if (shoot && !node) {      // per (instance, interval) pair: the history of its steps and its side record (ShootHvp::hist_doubles, side_doubles), a column per lane
    const long I = h->d.intervals, cpi = h->d.controls_per_interval, M = h->d.integration_method == MYR_INT_RK4 ? 2 : 1;
    const long P = (long)a.B * I;
    if (P > (1L << 30)) return fail(MYR_E_CAPACITY, "myr_hvp: more than 2^30 (instance, interval) pairs in one call");
    a.Pp = (P + 63) / 64 * 64;
    if (((a.Pp / 64) & 1) == 0) a.Pp += 64;      // an odd number of wavefronts, as padded_lanes
    st.scratch(a.hist, (size_t)(cpi * 2 * dm.ns) * (size_t)a.Pp);
    st.scratch(a.side, (size_t)(dm.ns + (M * cpi + 1) * dm.nu + dm.np) * (size_t)a.Pp);
  }
  if (out_p && p_stride) a.rows = out_p;
  else if (out_p) st.scratch(a.rows, (size_t)a.B * dm.np);
  if (int rc = st.commit()) return rc;
  if (int rc = timed_begin(h, kt)) return rc;
  const int rc = node ? (shoot ? hvp_node_shoot_for_system<SysNODE_CARTPOLE>(h, a) : hvp_node_colloc_for_system<SysNODE_CARTPOLE>(h, a))
                 : shoot ? for_system(h->d.system_id, true, [&](auto t) { return hvp_shoot_for_system<SYS_OF(t)>(h, a); }, [] { return (int)MYR_OK; })
                         : for_system(h->d.system_id, true, [&](auto t) { return hvp_colloc_for_system<SYS_OF(t)>(h, a); }, [] { return (int)MYR_OK; });
  if (!rc && out_p && !p_stride)
    hipLaunchKernelGGL(fit_reduce_sets_kernel, dim3((unsigned)dm.np * (unsigned)(a.B / a.R)), dim3(256), 0, h->stream, a.R, (int)dm.np, (const double*)a.rows,
                       out_p);
  const int rc_end = timed_end(h, kt);          // on every path
  return rc ? rc : rc_end;
}

// what myr_hvp, myr_hvp_node and myr_hvp_node_sets share behind their own checks: the staging, the product of `route`, the copies back.  B instances;
// n_param_doubles: what `params` holds (a row per instance or one shared set; the network route: a weight set for every R instances, B / R sets)
static int run_hvp(myr_handle h, int route, int mem, int B, int R, const double* z, const double* lam, const double* v, const double* params,
                   size_t n_param_doubles, int pstride, int with_cost, double* out_z, double* out_p, int p_stride) {
  if (B == 0) return MYR_OK;                          // (nothing is written)
  HIPCHK(hipSetDevice(h->d.device));
  const myr_dims& dm = h->dims;
  const size_t nz = (size_t)B * dm.n;
  HvpArgs a{};
  a.B = B; a.R = R; a.pstride = pstride; a.with_cost = with_cost != 0;
  double* gp = nullptr;
  DevStage st = call_stage(h, mem);
  st.in(a.z, z, nz);
  st.in(a.lam, lam, (size_t)B * dm.m);
  st.in(a.v, v, nz);
  st.in(a.params, params, n_param_doubles);
  st.out(a.out_z, out_z, nz);
  st.out(gp, out_p, p_stride ? (size_t)B * dm.np : (size_t)(B / R) * dm.np);
  if (int rc = st.commit()) return rc;
  if (int rc = dispatch_hvp(h, a, gp, p_stride, route)) return rc;
  return st.finish();
}

extern "C" int myr_hvp(myr_handle h, int32_t B, const double* z, const double* lam, const double* v, const double* params, int32_t params_stride,
                       int32_t with_cost, double* out_z, double* out_p, int32_t p_stride, int32_t mem) {
  const char* who = "myr_hvp";
  if (!h || !z || !v) return fail(MYR_E_ARG, "myr_hvp: null handle, z or v");
  if (!out_z && !out_p) return fail(MYR_E_ARG, "myr_hvp: both outputs are null");
  if (h->d.system_id == MYR_SYS_INVASIVEPLANT) return no_such_path(h, who);
  if (h->d.system_id >= 100) return fail(MYR_E_UNSUPPORTED, "myr_hvp: an elastic twin has no model of its own to differentiate; use the handle of its system");
  if (h->d.system_id == MYR_SYS_NODE_CARTPOLE)
    return fail(MYR_E_UNSUPPORTED, "myr_hvp: the network system is not built (second derivatives in 4 804 weights)");
  if (int rc = check_batch(who, B)) return rc;
  if (int rc = check_row_stride(h, who, "p_stride", p_stride, ROW_SUM_BATCH, "instance")) return rc;
  if (int rc = check_stride(h, who, params, params_stride)) return rc;
  if (int rc = check_mem(who, mem)) return rc;
  return run_hvp(h, HVP_CLOSED_FORM, mem, B, B, z, lam, v, params, n_params(h, params, params_stride, B), params_stride, with_cost, out_z, out_p, p_stride);
}

// the product for the network system (node_hvp.h): one shared weight set (no params_stride), HERMITE_SIMPSON or SHOOTING

extern "C" int myr_hvp_node(myr_handle h, int32_t B, const double* z, const double* lam, const double* v, const double* params, int32_t with_cost,
                            double* out_z, double* out_p, int32_t p_stride, int32_t mem) {
  const char* who = "myr_hvp_node";
  if (!h || !z || !v) return fail(MYR_E_ARG, "myr_hvp_node: null handle, z or v");
  if (!out_z && !out_p) return fail(MYR_E_ARG, "myr_hvp_node: both outputs are null");
  if (int rc = check_is_node(h, who, "myr_hvp")) return rc;
  if (int rc = check_node_not_trapezoidal(h, who, "HERMITE_SIMPSON and SHOOTING")) return rc;
  if (int rc = check_node_weights(h, who, params)) return rc;
  if (int rc = check_batch(who, B)) return rc;
  if (int rc = check_row_stride(h, who, "p_stride", p_stride, ROW_SUM_BATCH, "instance")) return rc;
  if (int rc = check_mem(who, mem)) return rc;
  if (int rc = check_node_lds(h, who, NODE_LDS_HVP)) return rc;
  return run_hvp(h, HVP_NODE, mem, B, B, z, lam, v, params, (size_t)h->dims.np, 0, with_cost, out_z, out_p, p_stride);
}

// ... and for E weight sets of R instances each in one call: myr_hvp_node is its E = 1, R = B case.  Set e has the bits of myr_hvp_node on that set alone
extern "C" int myr_hvp_node_sets(myr_handle h, int32_t E, int32_t R, const double* z, const double* lam, const double* v, const double* params,
                                 int32_t with_cost, double* out_z, double* out_p, int32_t p_stride, int32_t mem) {
  const char* who = "myr_hvp_node_sets";
  if (!h || !z || !v) return fail(MYR_E_ARG, "myr_hvp_node_sets: null handle, z or v");
  if (!out_z && !out_p) return fail(MYR_E_ARG, "myr_hvp_node_sets: both outputs are null");
  if (int rc = check_is_node(h, who, "myr_hvp")) return rc;
  if (int rc = check_node_not_trapezoidal(h, who, "HERMITE_SIMPSON and SHOOTING")) return rc;
  if (int rc = check_weight_sets(who, params)) return rc;
  if (int rc = check_sets(who, E, R)) return rc;
  if (int rc = check_row_stride(h, who, "p_stride", p_stride, ROW_SUM_SETS, "instance")) return rc;
  if (int rc = check_mem(who, mem)) return rc;
  if (int rc = check_node_lds(h, who, NODE_LDS_HVP)) return rc;
  return run_hvp(h, HVP_NODE, mem, E * R, R, z, lam, v, params, (size_t)E * h->dims.np, 0, with_cost, out_z, out_p, p_stride);
}

extern "C" int myr_fbsm(myr_handle h, int32_t B, int32_t N, const double* x0, const double* adj_T, const double* params,
                        int32_t params_stride, const double* clip_lo, const double* clip_hi, double bang, double delta,
                        int32_t max_sweeps, double* xs, double* us, double* adjs, int32_t* sweeps, int32_t mem) {
  if (!h || !x0 || !xs || !us || !adjs || !clip_lo || !clip_hi) return fail(MYR_E_ARG, "myr_fbsm: null handle or array");
  if (h->dims.nu > 8) return fail(MYR_E_CAPACITY, "myr_fbsm: more than 8 controls");
  FbsmArgs a{};
  for (int c = 0; c < h->dims.nu; ++c) { a.lo.s[c] = clip_lo[c]; a.hi.s[c] = clip_hi[c]; }
  if (B < 0 || N < 1 || max_sweeps < 1) return fail(MYR_E_ARG, "myr_fbsm: bad sizes");
  if (mem != MYR_MEM_HOST) return fail(MYR_E_ARG, "myr_fbsm: host arrays only");
  if (int rc = check_stride(h, "myr_fbsm", params, params_stride)) return rc;
  if (B == 0) return MYR_OK;
  HIPCHK(hipSetDevice(h->d.device));
  const myr_dims& dm = h->dims;
  const long Bp = padded_lanes(B);
  const bool discrete = h->d.system_id == MYR_SYS_INVASIVEPLANT;      // u has one row per step, not per point
  if (discrete && !params) return fail(MYR_E_ARG, "myr_fbsm: a discrete system needs `params`");
  const size_t rows_x = (size_t)(N + 1) * dm.ns, rows_u = (size_t)(N + (discrete ? 0 : 1)) * dm.nu;
  a.B = B; a.Bp = Bp; a.N = N; a.pstride = params_stride; a.bang = bang; a.delta = delta; a.max_sweeps = max_sweeps;
  // the inputs; the batch-minor working arrays X | A | U; an instance-major array for the transposes back; the sweep counts
  double* back = nullptr;
  DevStage st = call_stage(h, mem);
  st.in(a.x0, x0, (size_t)B * dm.ns);
  st.in(a.params, params, n_params(h, params, params_stride, B));
  st.in(a.adjT, adj_T, (size_t)dm.ns);
  st.scratch(a.X, (2 * rows_x + rows_u) * (size_t)Bp);
  st.scratch(back, (size_t)B * (rows_x > rows_u ? rows_x : rows_u));
  st.scratch(a.sweeps, (size_t)B);
  if (int rc = st.commit()) return rc;
  a.A = a.X + rows_x * Bp;
  a.U = a.A + rows_x * Bp;
  int rc;
  if (discrete) {
    if (int rc_begin = timed_begin(h, MYR_K_FBSM)) return rc_begin;
    hipLaunchKernelGGL(fbsm_discrete_kernel<DiscINVASIVEPLANT>, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, B, Bp, N, a.x0,
                       a.adjT, a.params, params_stride, a.lo, a.hi, delta, max_sweeps, a.X, a.U, a.A, a.sweeps);
    rc = timed_end(h, MYR_K_FBSM);
  } else {
    rc = for_system(h->d.system_id, false, [&](auto t) { return launch_fbsm<SYS_OF(t)>(h, a); },
                    [] { return fail(MYR_E_UNSUPPORTED, "myr_fbsm: this system has no adjoint dynamics"); });
  }
  if (rc) return rc;
  // one result at a time through `back`: transpose, download, synchronise (no st.finish(): nothing is registered as an output)
  struct { double* src; double* dst; size_t cols; } outs[3] = {{a.X, xs, rows_x}, {a.U, us, rows_u}, {a.A, adjs, rows_x}};
  for (auto& o : outs) {
    dim3 grid((unsigned)((o.cols + 31) / 32), (unsigned)((B + 31) / 32));
    hipLaunchKernelGGL(transpose_back_kernel, grid, dim3(256), 0, h->stream, o.src, back, B, (int)o.cols, Bp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(o.dst, back, (size_t)B * o.cols * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  if (sweeps) HIPCHK(hipMemcpy(sweeps, a.sweeps, (size_t)B * 4, hipMemcpyDeviceToHost));
  return MYR_OK;
}
#endif  // !MYR_TU_SYSTEM
