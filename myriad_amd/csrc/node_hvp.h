// node_hvp.h -- Lagrangian Hessian-vector product of the network system (K16 in DESIGN.md; C-ABI myr_hvp_node), HERMITE_SIMPSON and SHOOTING.
// With L(z, lam, w) = with_cost f(z) + lam^T c(z, w) in the 4 804 weights w and a direction v, psi = <grad_z L, v>:
//   out_z = grad_z psi = grad^2_zz L v,      out_p = grad_w psi = (d^2 L / dw dz) v.
// Nothing of the algebra is new: the point pass and the pair pass of the unrolled-extragradient kernels (K12, K15) get an entry of their own.
//   Hermite-Simpson: grad^2_zz L is block-diagonal over the K = 2 N + 1 points.  Point j with mu_j = ExgdGradPoint::combine(lam), d_j = v at the
//     point and cost weight with_cost wq_j is item (c) of node_exgd_grad.h -- NodeExgdHost::second / NodeExgdWave::second: hd = (sum_r mu_r d2 f_r) d
//     and the weight gradient of mu^T J(w) d -- plus the TRUE system's wq d2g d (NodeExgdHost::cost_hd; the cost has no weights).
//   SHOOTING: per (instance, interval) pair NodeShootExgd<M>::interval<true> (node_shoot_exgd_grad.h) with scale = 0 over a zeroed a_lam column: the
//     reverse starts from ad = 0 and what is left of the seeded pass is ShootHvp::interval -- the forward tangent rollout and the second-order
//     reverse sweep through the stages, the network differentiated layer by layer; the running cost's dg enters every stage costate (and so
//     out_p), its d2g d every stage's second-order cotangent.  The pairs' node cotangents and control rows meet by ShootHvp::gather_z.
// node_hvp_colloc_host / node_hvp_shoot_host: one instance in plain loops (NodeExgdPoint::hess; NseHostNet) -- tests/hostsim/node_hvp_twin.cpp.
// node_hvp_colloc_kernel<WPI>: one workgroup of WPI wavefronts per instance, wavefront w takes the points w, w + WPI, ...; lane j = hidden unit j.
//   z, v and lam are read where they lie: the weight copy is the only LDS tenant, no horizon is refused.
// node_hvp_shoot_kernel<M>: one workgroup of 1, 2 or 4 wavefronts (from I alone) per instance, one wavefront per pair, k = w, w + WPI, ...
//   Dynamic LDS (doubles): weights NodeMfma64::L_N | lam [NS][I] | a_lam (zero) [NS][I] | step-start (x, xd) [2 NS cpi][I] |
//   side record (node | control rows) [NS + (M cpi + 1) NU][I] -- pair-minor; z and v are read from global memory (wave-uniform addresses).
// In both the weight gradient stays in NodeFit::Acc registers over the instance; at the end the wavefronts add theirs in the order 0, 1, ... into
// the idle weight copy (node_hvp_store_row), which goes out as the row -- or nothing does when out_p is null: out_z never reads the accumulators.
// Every loop has a wave-uniform trip count; no lane-0 block, no atomics.
#pragma once
#include "node_shoot_exgd_grad.h"

namespace myriad {

struct NodeHvp {
  using P = NodeExgdHost;
  using G = P::G;
  static constexpr int NS = P::NS, NU = P::NU, NW = P::NW, NP = P::NP;
  // entry r of point j in an instance's z: the K state rows, then the K control rows
  MYR_HD static inline long idx(int K, int j, int r) { return r < NS ? (long)j * NS + r : (long)K * NS + (long)j * NU + (r - NS); }
  // the point's multiplier combination (zero without lam) and cost weight.  (+ 0.0: a zero multiplier array combines to -0.0 at a midpoint; with
  // it a null lam and an array of zeros give the same bits)
  MYR_HD static inline void weights_of(const double* lam, int N, int K, int j, double h, int with_cost, double* mu, double& wq) {
    double e[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) mu[q] = 0.0;
    if (lam) G::combine(lam, N, j, h, mu, e);
#pragma unroll
    for (int q = 0; q < NS; ++q) mu[q] = mu[q] + 0.0;
    wq = with_cost ? G::wq(K, j, h) : 0.0;
  }
};

template <int M>
struct NodeHvpShoot {
  using A = NodeShootExgd<M>;
  using HV = typename A::HV;
  static constexpr int NS = A::NS;
  // doubles per instance beside the weight copy: lam and a_lam columns, the pairs' step-start records and side records
  MYR_HD static inline long work_doubles(int I, int cpi) { return (long)I * (2 * NS + A::pair_hist_doubles(cpi) + A::side_doubles(cpi)); }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin --------------------------------------------------------------------------------------------------------------------------------
// One Hermite-Simpson instance: the points in ascending order.  p: the NP shared weights; lam, oz, op may be null
inline void node_hvp_colloc_host(int N, double h, const double* z, const double* lam, const double* v, const double* p, int with_cost, double* oz,
                                 double* op) {
  using C = NodeHvp;
  constexpr int NS = C::NS, NW = C::NW, NP = C::NP;
  const int K = C::G::points(N);
  double gl[NP];
  double* gp = op ? op : gl;
  for (int e = 0; e < NP; ++e) gp[e] = 0.0;
  for (int j = 0; j < K; ++j) {
    double w[NW], d[NW], mu[NS], wq, hd[NW], wo[NS];
    for (int r = 0; r < NW; ++r) { w[r] = z[C::idx(K, j, r)]; d[r] = v[C::idx(K, j, r)]; }
    C::weights_of(lam, N, K, j, h, with_cost, mu, wq);
    NodeExgdPoint::hess(w, p, mu, wq, false, 0.0, d, hd, wo, gp);
    if (oz) for (int r = 0; r < NW; ++r) oz[C::idx(K, j, r)] = hd[r];
  }
}

// One SHOOTING instance: the pairs in ascending order.  work: NodeHvpShoot<M>::work_doubles(I, cpi) doubles (the carve of the kernel's LDS);
// lam, oz, op may be null
template <int M>
inline void node_hvp_shoot_host(int method, int I, int cpi, double T, const double* z, const double* lam, const double* v, const double* p,
                                int with_cost, double* work, double* oz, double* op) {
  using S = NodeHvpShoot<M>;
  using A = typename S::A;
  constexpr int NS = A::NS, NP = A::NP;
  const long n = A::nvars(I, cpi), m = (long)I * NS;
  const double h = T / ((double)I * cpi);
  const typename A::Rule R = A::P::rule(method);
  double* lc = work;                                          // [NS][I]: pair-minor, as on the device
  double* al = lc + m;
  double* phist = al + m;
  double* side = phist + A::pair_hist_doubles(cpi) * I;
  double gl[NP];
  double* gp = op ? op : gl;
  for (int e = 0; e < NP; ++e) gp[e] = 0.0;
  NseHostNet net{p, gp};
  for (int k = 0; k < I; ++k)
    for (int q = 0; q < NS; ++q) { lc[k + (long)q * I] = lam ? lam[(long)k * NS + q] : 0.0; al[k + (long)q * I] = 0.0; }
  for (int k = 0; k < I; ++k)
    A::template interval<true>(net, R, I, cpi, k, h, z, v, lc + k, p, with_cost ? 1.0 : 0.0, phist + k, side + k, I, al + k, 0.0);
  if (oz) for (long i = 0; i < n; ++i) oz[i] = S::HV::gather_z(I, cpi, i, side, I);
}

// the host twin over a batch: transcription 0 Hermite-Simpson (N = I intervals; cpi, method not read), 2 SHOOTING with method 0 Euler, 1 Heun,
// 2 midpoint, 3 RK4.  params [NP] shared; out_z [B][n] or null; out_p [B][NP] or null; lam [B][m] or null.  Returns 0, or -1 for anything else.
inline int node_hvp_host(int transcription, int method, int B, int I, int cpi, double T, const double* z, const double* lam, const double* v,
                         const double* params, int with_cost, double* out_z, double* out_p) {
  constexpr int NS = NodeHvp::NS, NW = NodeHvp::NW, NP = NodeHvp::NP;
  if (transcription == 0) {
    const long n = (long)NodeHvp::G::points(I) * NW, m = NodeHvp::G::rows(I);
    for (long b = 0; b < B; ++b)
      node_hvp_colloc_host(I, T / I, z + b * n, lam ? lam + b * m : nullptr, v + b * n, params, with_cost, out_z ? out_z + b * n : nullptr,
                           out_p ? out_p + b * NP : nullptr);
    return 0;
  }
  if (transcription != 2 || method < 0 || method > 3) return -1;
  const long m = (long)I * NS;
  const long n = method == 3 ? NodeShootExgd<2>::nvars(I, cpi) : NodeShootExgd<1>::nvars(I, cpi);
  const long wd = method == 3 ? NodeHvpShoot<2>::work_doubles(I, cpi) : NodeHvpShoot<1>::work_doubles(I, cpi);
  double* work = new double[wd];
  for (long b = 0; b < B; ++b) {
    const double* lb = lam ? lam + b * m : nullptr;
    double* oz = out_z ? out_z + b * n : nullptr;
    double* op = out_p ? out_p + b * NP : nullptr;
    if (method == 3) node_hvp_shoot_host<2>(method, I, cpi, T, z + b * n, lb, v + b * n, params, with_cost, work, oz, op);
    else node_hvp_shoot_host<1>(method, I, cpi, T, z + b * n, lb, v + b * n, params, with_cost, work, oz, op);
  }
  delete[] work;
  return 0;
}
#endif  // !__HIP_DEVICE_COMPILE__

#if defined(__HIPCC__)
// The weight rows of a workgroup's wavefronts, added in the order 0, 1, ... over the weight copy `gl` (idle: the caller has passed a barrier behind
// its last read) in the parameter order of node_system.h, then out as row[NP].  Every thread of the workgroup calls (barriers inside).
// (Forced inline: behind a call the accumulators would live in scratch.)
__device__ static __forceinline__ void node_hvp_store_row(const NodeFit::Acc& acc, double* gl, int tid, int NT, int lane, int wave, int WPI, double* row) {
  using S_ = SysNODE_CARTPOLE;
  constexpr int NS = S_::NS, NW = S_::NW, NP = S_::NP, H = NodeFit::H;
  static_assert(NP <= NodeMfma64::L_N, "the row fits the weight copy");
  for (int wv = 0; wv < WPI; ++wv) {
    if (wave == wv) {                                              // (wave-uniform)
      const bool first = wv == 0;
#pragma unroll
      for (int c = 0; c < NW; ++c) { double* q = gl + S_::O_W1 + c * H + lane; *q = first ? acc.w1[c] : *q + acc.w1[c]; }
      { double* q = gl + S_::O_B1 + lane; *q = first ? acc.b1 : *q + acc.b1; }
#pragma unroll
      for (int k = 0; k < H; ++k) { double* q = gl + S_::O_W2 + k * H + lane; *q = first ? acc.w2[k] : *q + acc.w2[k]; }
      { double* q = gl + S_::O_B2 + lane; *q = first ? acc.b2 : *q + acc.b2; }
#pragma unroll
      for (int r = 0; r < NS; ++r) { double* q = gl + S_::O_W3 + lane * NS + r; *q = first ? acc.w3[r] : *q + acc.w3[r]; }
#pragma unroll
      for (int r = 0; r < NS; ++r) {                               // (db3 is the same in every lane: lane r stores entry r)
        double* q = gl + S_::O_B3 + r;
        const double v = first ? acc.b3[r] : *q + acc.b3[r];
        if (lane == r) *q = v;
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < NP; i += NT) row[i] = gl[i];
}

inline size_t node_hvp_colloc_lds_bytes() { return (size_t)NodeMfma64::L_N * 8 + 16; }

// One workgroup of WPI wavefronts per instance (blockIdx.x).  params [E][NP], R instances to a set: instance b reads the row of set b / R (one
// shared set: R = B).  lam, out_z, rows may be null (kernel arguments: the tests on them are uniform over the workgroup).  An idle wavefront of the last round leaves the point loop by its wave-uniform bound; no barrier inside it.
template <int WPI>
__global__ __launch_bounds__(64 * WPI)
void node_hvp_colloc_kernel(int B, int N, double h, const double* __restrict__ z, const double* __restrict__ lam, const double* __restrict__ v,
                            const double* __restrict__ params, int with_cost, double* __restrict__ out_z, double* __restrict__ rows, int R) {
  using C = NodeHvp;
  using W = NodeExgdWave;
  constexpr int NS = C::NS, NW = C::NW, NP = C::NP, NT = 64 * WPI;
  extern __shared__ __attribute__((aligned(16))) char smem_node_hvp_colloc[];
  const long b = blockIdx.x;
  if (b >= B) return;                                             // (the whole workgroup)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = C::G::points(N), m = C::G::rows(N);
  const long n = (long)K * NW;
  double* wl = reinterpret_cast<double*>(smem_node_hvp_colloc);
  const double* zb = z + b * n;
  const double* vb = v + b * n;
  const double* lamb = lam ? lam + b * m : nullptr;
  params += (long)((int)blockIdx.x / R) * NP;                     // this instance's weight set
  NodeMfma64::load_weights(params, wl, tid, NT);
  __syncthreads();
  typename W::Acc acc;
  W::zero(acc);
  for (int j = wave; j < K; j += WPI) {                            // (wave-uniform bounds; every value of the point is wave-uniform)
    double w[NW], d[NW], mu[NS], wq, hd[NW], hc[NW], wo[NS], f[NS], h1, h2;
#pragma unroll
    for (int r = 0; r < NW; ++r) { w[r] = zb[C::idx(K, j, r)]; d[r] = vb[C::idx(K, j, r)]; }
    C::weights_of(lamb, N, K, j, h, with_cost, mu, wq);
    NodeFit::fwd(wl, lane, w, h1, h2, f);
    W::second(wl, lane, w, h1, h2, mu, d, acc, wo, hd);
    C::P::cost_hd(w, wq, d, hc);
    if (out_z) {
#pragma unroll
      for (int r = 0; r < NW; ++r) out_z[b * n + C::idx(K, j, r)] = hd[r] + hc[r];      // (every lane stores the same bits)
    }
  }
  __syncthreads();                                                 // the weight copy is idle from here
  if (rows) node_hvp_store_row(acc, wl, tid, NT, lane, wave, WPI, rows + b * NP);
}

struct NodeHvpArgs {
  int B, I, cpi, method, with_cost;
  int R;                                   // weight sets: R instances to a set, params [B / R][NP]
  double T;
  const double *z, *lam, *v, *params;      // lam may be null
  double *out_z, *rows;                    // either may be null
};

template <int M>
inline size_t node_hvp_shoot_lds_bytes(int I, int cpi) {
  return (size_t)(NodeMfma64::L_N + NodeHvpShoot<M>::work_doubles(I, cpi)) * 8 + 16;
}
// wavefronts per instance: from I alone, as K15
inline int node_hvp_shoot_wpi(int I) { return node_shoot_exgd_grad_wpi(I); }

// One workgroup of WPI = blockDim.x / 64 wavefronts per instance (blockIdx.x).  Wavefront w takes the intervals k = w, w + WPI, ... and writes only
// their columns (wave-uniform values: every lane stores); an idle wavefront of the last round leaves the loop by its wave-uniform bound.
template <int M>
__global__ __launch_bounds__(256)
void node_hvp_shoot_kernel(NodeHvpArgs a) {
  using S = NodeHvpShoot<M>;
  using A = typename S::A;
  constexpr int NS = A::NS, NP = A::NP;
  extern __shared__ __attribute__((aligned(16))) char smem_node_hvp_shoot[];
  const long b = blockIdx.x;
  if (b >= a.B) return;                                           // (the whole workgroup)
  const int tid = threadIdx.x, lane = tid & 63, NT = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int WPI = __builtin_amdgcn_readfirstlane(NT >> 6);
  const int I = a.I, cpi = a.cpi;
  const long n = A::nvars(I, cpi), m = (long)I * NS;
  const double h = a.T / ((double)I * cpi);
  double* wl = reinterpret_cast<double*>(smem_node_hvp_shoot);
  double* lc = wl + NodeMfma64::L_N;
  double* al = lc + m;
  double* phist = al + m;
  double* side = phist + A::pair_hist_doubles(cpi) * I;
  const double* zb = a.z + b * n;
  const double* vb = a.v + b * n;
  const double* params = a.params + (long)((int)blockIdx.x / a.R) * NP;      // this instance's weight set: every use below
  NodeMfma64::load_weights(params, wl, tid, NT);
  for (long i = tid; i < m; i += NT) {
    const long k = i / NS, q = i - k * NS;
    lc[k + q * I] = a.lam ? a.lam[b * m + i] : 0.0;
    al[k + q * I] = 0.0;
  }
  __syncthreads();
  const typename A::Rule R = A::P::rule(a.method);
  NodeFit::Acc acc;
  NodeExgdWave::zero(acc);
  NseWaveNet net{wl, lane, &acc};
  const double cw = a.with_cost ? 1.0 : 0.0;
  for (int k = wave; k < I; k += WPI)                              // (wave-uniform bounds; no barrier inside)
    A::template interval<true>(net, R, I, cpi, k, h, zb, vb, lc + k, params, cw, phist + k, side + k, I, al + k, 0.0);
  __syncthreads();                                                 // every side record is written; the weight copy is idle from here
  if (a.out_z)
    for (long i = tid; i < n; i += NT) a.out_z[b * n + i] = S::HV::gather_z(I, cpi, i, side, I);
  if (a.rows) node_hvp_store_row(acc, wl, tid, NT, lane, wave, WPI, a.rows + b * NP);
}
#endif  // __HIPCC__

}  // namespace myriad
