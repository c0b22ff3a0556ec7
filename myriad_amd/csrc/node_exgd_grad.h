// node_exgd_grad.h -- derivative of `nsteps` unrolled extragradient steps in the 4 804 weights of the network system (K12 in DESIGN.md).
// The sweep is K10's (exgd_grad.h: items 1-5, the masks, the buffer swap, the history); the transcription algebra is ExgdGradPoint's, used as it
// stands (combine, jd_rows, wq, inside, clip, hist_doubles do not depend on the system).  What is new is the point pass: no lane can hold the weight
// gradient, so the network is differentiated layer by layer.  At a point w = [x; u]:
//   a1 = W1^T w + b1, h1 = s(a1);  a2 = W2^T h1 + b2, h2 = s(a2);  f = W3^T h2 + b3;   s' = h (1 - h), s'' = h (1 - h)(1 - 2 h)
//  (a) first order, cotangent v[NS] on f:  jt[NW] = J^T v  and the weight gradient of v^T f           (item 1; without the gradient: the forward steps)
//  (b) value f                                                                                           (the multiplier update)
//  (c) second order, mu[NS] and a direction d[NW]:  w = J d,  hd = (sum_r mu_r d2 f_r) d  and the weight gradient of psi = mu^T J(w) d   (items 3, 5)
//      tangent:  da1 = W1^T d, dh1 = s1' da1;  da2 = W2^T dh1, dh2 = s2' da2;  df = W3^T dh2 (= w)
//      reverse of psi = mu . df:  g2 = W3 mu;  dW3[j][r] += dh2_j mu_r;  t2 = g2 s2' (cotangent of da2),  c2 = g2 da2 s2'' (of a2);
//        dW2[k][j] += dh1_k t2_j + h1_k c2_j;  db2 += c2;  gd1 = W2 t2,  g1 = W2 c2;  t1 = gd1 s1',  c1 = gd1 da1 s1'' + g1 s1';
//        dW1[c][i] += d_c t1_i + w_c c1_i;  db1 += c1;  hd = W1 c1.                         (b3 has no share)
// The running cost is the TRUE system's: it has no weights, adds wq dg to the gradient of the Lagrangian and wq d2g d to hd.
//
// NodeExgdHost: (a)-(c) as plain loops; NodeExgdPoint hands them to colloc_exgd_grad_host (exgd_grad.h), the one host sequence of K10 and K12
// (node_exgd_grad_host, tests/hostsim/node_exgd_grad_twin.cpp).
// NodeExgdWave: the same on one wavefront, lane j = hidden unit j of both layers, weights from the LDS copy of NodeMfma64::load_weights,
// activations broadcast by v_readlane (NodeFit::fwd / bcast / wsum, fit.h); the weight gradient in NodeFit::Acc.
// node_exgd_grad_kernel<WPI>: one workgroup of WPI wavefronts per instance.
// Weight sets (myr_exgd_grad_node_sets): params [E][NP], R instances to a set; a workgroup is one instance and takes the row of its set.
#pragma once
#include "exgd_grad.h"
#include "node_system.h"
#if defined(__HIPCC__)
#include "fit.h"
#endif

namespace myriad {

struct NodeExgdHost {
  using Sys = SysNODE_CARTPOLE;
  using True = SysCARTPOLE;
  using G = ExgdGradPoint<Sys, EXGD_GRAD_HS>;
  static constexpr int NS = Sys::NS, NU = Sys::NU, NW = Sys::NW, NP = Sys::NP, H = 64;

  // wq d2g d of the true system's running cost
  MYR_HD static inline void cost_hd(const double* w, double wq, const double* d, double* hd) {
    double tp[True::NPX], tf[NS], tA[NS * NS], tB[NS * NU], tg, tgw[NW], tD2[True::NNZ2], Wg[NW * NW], zero[NS];
    True::default_params(tp);
#pragma unroll
    for (int r = 0; r < NS; ++r) zero[r] = 0.0;
    True::lin_d2(w, w + NS, tp, tf, tA, tB, &tg, tgw, tD2);
    True::contract(tD2, zero, wq, Wg);
#pragma unroll
    for (int a = 0; a < NW; ++a) {
      double s = 0.0;
#pragma unroll
      for (int b = 0; b < NW; ++b) s += (a <= b ? Wg[a * NW + b] : Wg[b * NW + a]) * d[b];      // (contract fills the upper triangle)
      hd[a] = s;
    }
  }
  // grad_z L at the point from the network's J^T a (jt), the multiplier's direct share e and the cost
  MYR_HD static inline void assemble(const double* w, const double* p, const double* e, const double* jt, double wq, double* g) {
    double go, gw[NW];
    Sys::cost_grad(w, w + NS, p, &go, gw);
#pragma unroll
    for (int r = 0; r < NW; ++r) g[r] = (r < NS ? e[r] : 0.0) + jt[r] + wq * gw[r];
  }

  // (a): f, jt = J^T v, and gp += the weight gradient of v^T f where gp is not null
  static inline void first(const double* w, const double* p, const double* v, double* f, double* jt, double* gp) {
    double h1[H], h2[H], e2[H];
    Sys::fwd(w, w + NS, p, h1, h2, f);
    for (int j = 0; j < H; ++j) {
      double g2 = 0.0;
      for (int r = 0; r < NS; ++r) {
        g2 += p[Sys::O_W3 + j * NS + r] * v[r];
        if (gp) gp[Sys::O_W3 + j * NS + r] += h2[j] * v[r];
      }
      e2[j] = g2 * h2[j] * (1.0 - h2[j]);
      if (gp) gp[Sys::O_B2 + j] += e2[j];
    }
    if (gp) for (int r = 0; r < NS; ++r) gp[Sys::O_B3 + r] += v[r];
    for (int c = 0; c < NW; ++c) jt[c] = 0.0;
    for (int k = 0; k < H; ++k) {
      double g1 = 0.0;
      for (int j = 0; j < H; ++j) {
        g1 += p[Sys::O_W2 + k * H + j] * e2[j];
        if (gp) gp[Sys::O_W2 + k * H + j] += h1[k] * e2[j];
      }
      const double e1 = g1 * h1[k] * (1.0 - h1[k]);
      if (gp) gp[Sys::O_B1 + k] += e1;
      for (int c = 0; c < NW; ++c) {
        if (gp) gp[Sys::O_W1 + c * H + k] += w[c] * e1;
        jt[c] += p[Sys::O_W1 + c * H + k] * e1;
      }
    }
  }

  // (c): wo = J d, hd = (sum_r mu_r d2 f_r) d, gp += the weight gradient of mu^T J(w) d
  static inline void second(const double* w, const double* p, const double* mu, const double* d, double* wo, double* hd, double* gp) {
    double h1[H], h2[H], f[NS], da1[H], dh1[H], t2[H], c2[H];
    Sys::fwd(w, w + NS, p, h1, h2, f);
    for (int i = 0; i < H; ++i) {
      double a = 0.0;
      for (int c = 0; c < NW; ++c) a += d[c] * p[Sys::O_W1 + c * H + i];
      da1[i] = a;
      dh1[i] = h1[i] * (1.0 - h1[i]) * a;
    }
    for (int r = 0; r < NS; ++r) wo[r] = 0.0;
    for (int j = 0; j < H; ++j) {
      double a = 0.0;
      for (int k = 0; k < H; ++k) a += dh1[k] * p[Sys::O_W2 + k * H + j];
      const double sp = h2[j] * (1.0 - h2[j]);
      const double dh2 = sp * a;
      double g2 = 0.0;
      for (int r = 0; r < NS; ++r) {
        wo[r] += dh2 * p[Sys::O_W3 + j * NS + r];
        g2 += p[Sys::O_W3 + j * NS + r] * mu[r];
        gp[Sys::O_W3 + j * NS + r] += dh2 * mu[r];
      }
      t2[j] = g2 * sp;
      c2[j] = g2 * a * sp * (1.0 - 2.0 * h2[j]);
      gp[Sys::O_B2 + j] += c2[j];
    }
    for (int c = 0; c < NW; ++c) hd[c] = 0.0;
    for (int k = 0; k < H; ++k) {
      double gd1 = 0.0, g1 = 0.0;
      for (int j = 0; j < H; ++j) {
        const double wkj = p[Sys::O_W2 + k * H + j];
        gd1 += wkj * t2[j];
        g1 += wkj * c2[j];
        gp[Sys::O_W2 + k * H + j] += dh1[k] * t2[j] + h1[k] * c2[j];
      }
      const double sp = h1[k] * (1.0 - h1[k]);
      const double t1 = gd1 * sp, c1 = gd1 * da1[k] * sp * (1.0 - 2.0 * h1[k]) + g1 * sp;
      gp[Sys::O_B1 + k] += c1;
      for (int c = 0; c < NW; ++c) {
        gp[Sys::O_W1 + c * H + k] += d[c] * t1 + w[c] * c1;
        hd[c] += p[Sys::O_W1 + c * H + k] * c1;
      }
    }
  }
};

// The point policy of the network system for colloc_exgd_grad_host (exgd_grad.h): the point functions above at w = [x; u], the weight gradient
// accumulated into gp directly.  p: the NP shared weights (node_system.h's order)
struct NodeExgdPoint {
  using P = NodeExgdHost;
  using Sys = P::Sys;
  using G = P::G;
  static constexpr int NS = P::NS, NW = P::NW;
  static inline void grad(const double* w, const double* p, const double* a, const double* e, double wq, bool, double, double* g) {
    double f[NS], jt[NW];
    P::first(w, p, a, f, jt, nullptr);
    P::assemble(w, p, e, jt, wq, g);
  }
  // item 1: the cotangent eta_v a(a_lam) on f
  static inline void constraint(const double* w, const double* p, const double* a, const double*, double, double eta_v, double* jt, double* gp) {
    double v[NS], f[NS];
    for (int q = 0; q < NS; ++q) v[q] = eta_v * a[q];
    P::first(w, p, v, f, jt, gp);
  }
  static inline double step_ax(double ax, int r, double eta_v, const double* e, const double* jt) {
    return ax + ((r < NS ? eta_v * e[r] : 0.0) + jt[r]);
  }
  static inline void hess(const double* w, const double* p, const double* mu, double wq, bool, double, const double* d, double* hd, double* wo,
                          double* gp) {
    double hc[NW];
    P::second(w, p, mu, d, wo, hd, gp);
    P::cost_hd(w, wq, d, hc);
    for (int r = 0; r < NW; ++r) hd[r] = hd[r] + hc[r];
  }
};

template <class... A>
inline void node_exgd_grad_host(A... a) { colloc_exgd_grad_host<NodeExgdPoint>(a...); }

#if defined(__HIPCC__)
struct NodeExgdWave {
  using F = NodeFit;
  using NM = NodeMfma64;
  using Acc = NodeFit::Acc;
  static constexpr int NS = F::NS, NW = F::NW, H = F::H;

  __device__ static inline void zero(Acc& g) {
#pragma unroll
    for (int c = 0; c < NW; ++c) g.w1[c] = 0.0;
#pragma unroll
    for (int k = 0; k < H; ++k) g.w2[k] = 0.0;
#pragma unroll
    for (int r = 0; r < NS; ++r) { g.w3[r] = 0.0; g.b3[r] = 0.0; }
    g.b1 = 0.0; g.b2 = 0.0;
  }

  // (a) behind NodeFit::fwd: NodeFit::bwd with the control column; ACC false leaves the accumulators alone (the forward steps)
  template <bool ACC>
  __device__ static inline void first(const double* wl, int lane, const double* w, double h1, double h2, const double* v, Acc& g, double* jt) {
    double g2 = 0.0;
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      if (ACC) { g.w3[r] += h2 * v[r]; g.b3[r] += v[r]; }
      g2 += wl[NM::L_W3 + lane * NS + r] * v[r];
    }
    const double e2 = g2 * h2 * (1.0 - h2);
    if (ACC) g.b2 += e2;
    double g1 = 0.0;
#pragma unroll
    for (int k = 0; k < H; ++k) {
      if (ACC) g.w2[k] += F::bcast(h1, k) * e2;
      g1 += wl[NM::L_W2 + lane * NM::LD2 + k] * F::bcast(e2, k);
      if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);       // (as NodeFit::bwd: eight broadcasts in flight)
    }
    const double e1 = g1 * h1 * (1.0 - h1);
    if (ACC) {
      g.b1 += e1;
#pragma unroll
      for (int c = 0; c < NW; ++c) g.w1[c] += w[c] * e1;
    }
#pragma unroll
    for (int c = 0; c < NW; ++c) jt[c] = F::wsum(wl[NM::L_W1 + c * H + lane] * e1);
  }

  // (c) behind NodeFit::fwd.  The two W2 reverse products share one loop, and so do the two outer products into dW2
  __device__ static inline void second(const double* wl, int lane, const double* w, double h1, double h2, const double* mu, const double* d,
                                       Acc& g, double* wo, double* hd) {
    const double sp1 = h1 * (1.0 - h1), sp2 = h2 * (1.0 - h2);
    double da1 = 0.0;
#pragma unroll
    for (int c = 0; c < NW; ++c) da1 += d[c] * wl[NM::L_W1 + c * H + lane];
    const double dh1 = sp1 * da1;
    double da2 = 0.0;
#pragma unroll 8
    for (int k = 0; k < H; ++k) da2 += F::bcast(dh1, k) * wl[NM::L_W2 + k * NM::LD2 + lane];
    const double dh2 = sp2 * da2;
    double g2 = 0.0;
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      const double w3 = wl[NM::L_W3 + lane * NS + r];
      wo[r] = F::wsum(dh2 * w3);
      g2 += w3 * mu[r];
      g.w3[r] += dh2 * mu[r];
    }
    const double t2 = g2 * sp2, c2 = g2 * da2 * sp2 * (1.0 - 2.0 * h2);
    g.b2 += c2;
    double gd1 = 0.0, g1 = 0.0;
#pragma unroll
    for (int k = 0; k < H; ++k) {
      g.w2[k] += F::bcast(dh1, k) * t2 + F::bcast(h1, k) * c2;  // dW2[k][lane]
      const double wr = wl[NM::L_W2 + lane * NM::LD2 + k];       // row `lane` of W2
      gd1 += wr * F::bcast(t2, k);
      g1 += wr * F::bcast(c2, k);
      if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);       // four broadcasts a term: the same number in flight as in `first`
    }
    const double t1 = gd1 * sp1, c1 = gd1 * da1 * sp1 * (1.0 - 2.0 * h1) + g1 * sp1;
    g.b1 += c1;
#pragma unroll
    for (int c = 0; c < NW; ++c) {
      g.w1[c] += d[c] * t1 + w[c] * c1;
      hd[c] = F::wsum(wl[NM::L_W1 + c * H + lane] * c1);
    }
  }

};

inline size_t node_exgd_grad_lds_bytes(int N) {
  using G = NodeExgdHost::G;
  const int K = G::points(N), n = K * NodeExgdHost::NW, m = G::rows(N);
  return (size_t)(NodeMfma64::L_N + 3 * n + 2 * m + K * NodeExgdHost::NS) * 8 + 16;
}

// One workgroup of WPI wavefronts per instance (blockIdx.x: the instance within this launch's chunk; every batch pointer is the chunk's).  params is
// the CALL's [E][NP]: it does not advance with the chunk; the chunk's first instance is number inst0 of the call, and instance i reads the row of set
// i / R (a chunk may begin and end inside a set; one shared set: R = the call's batch, set 0 throughout).  Dynamic LDS:
// the weight copy, then colloc_exgd_grad_kernel's buffers.  In a point pass wavefront w takes the points j = w, w + WPI, ... one after the other and
// writes only their entries (wave-uniform values: every lane stores); an idle wavefront of the last round skips the point's work behind a
// wave-uniform test and reaches every barrier.  The interval passes and the copies run with all 64 WPI lanes.  The weight gradient stays in
// registers through the sweep; at the end the wavefronts add theirs in the order 0, 1, ... into the idle weight copy, which then goes out as the row.
template <int WPI>
__global__ __launch_bounds__(64 * WPI)
void node_exgd_grad_kernel(int B, int N, double h, const double* __restrict__ z, const double* __restrict__ lam, const double* __restrict__ lb,
                           const double* __restrict__ ub, const double* __restrict__ params, double eta_x, double eta_v, int nsteps,
                           const double* __restrict__ seed_z, const double* __restrict__ seed_lam, double* __restrict__ hist,
                           double* __restrict__ grad, double* __restrict__ dz0, double* __restrict__ dlam0, int inst0, int R) {
  using P = NodeExgdHost;
  using W = NodeExgdWave;
  using G = P::G;
  using S_ = P::Sys;
  constexpr int NS = P::NS, NU = P::NU, NW = P::NW, NP = P::NP, H = P::H, NT = 64 * WPI;
  extern __shared__ __attribute__((aligned(16))) char smem_node_exgd_grad[];
  const long b = blockIdx.x;
  if (b >= B) return;                                             // (the whole workgroup)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = G::points(N), n = K * NW, m = G::rows(N);
  const long hs = 2L * n + m;
  double* wl = reinterpret_cast<double*>(smem_node_exgd_grad);
  double* sx = wl + NodeMfma64::L_N;
  double* sax = sx + n;
  double* sd = sax + n;
  double* sl = sd + n;
  double* sal = sl + m;
  double* sdf = sal + m;
  const double* zb = z + b * n;
  const double* lamb = lam + b * m;
  const double* lo = lb + b * n;
  const double* hi = ub + b * n;
  double* hb = hist + b * G::hist_doubles(N, nsteps);
  params += (size_t)(((unsigned)inst0 + blockIdx.x) / (unsigned)R) * NP;      // this instance's weight set: every use of params below
  NodeMfma64::load_weights(params, wl, tid, NT);
  for (int i = tid; i < n; i += NT) sx[i] = zb[i];
  for (int i = tid; i < m; i += NT) sl[i] = lamb[i];
  __syncthreads();
  auto idx = [&](int j, int r) { return r < NS ? j * NS + r : K * NS + j * NU + (r - NS); };
  typename W::Acc acc;
  W::zero(acc);
  // ---- forward ----
  for (int s = 0; s < nsteps; ++s) {
    double* Hh = hb + s * hs;
    for (int i = tid; i < n; i += NT) Hh[i] = sx[i];
    for (int i = tid; i < m; i += NT) Hh[2 * n + i] = sl[i];
    for (int pass = 0; pass < 2; ++pass) {
      const double* src = pass == 0 ? sx : sax;
      double* dst = pass == 0 ? sax : sx;
      for (int j = wave; j < K; j += WPI) {                        // (wave-uniform bounds; no barrier inside)
        double w[NW], a[NS], e[NS], f[NS], jt[NW], g[NW], h1, h2;
#pragma unroll
        for (int r = 0; r < NW; ++r) w[r] = src[idx(j, r)];
        G::combine(sl, N, j, h, a, e);
        NodeFit::fwd(wl, lane, w, h1, h2, f);
        W::template first<false>(wl, lane, w, h1, h2, a, acc, jt);
        P::assemble(w, params, e, jt, G::wq(K, j, h), g);
#pragma unroll
        for (int r = 0; r < NW; ++r) { const int i = idx(j, r); dst[i] = G::clip(sx[i] - eta_x * g[r], lo[i], hi[i]); }
      }
      if (pass == 0) {
        __syncthreads();
        for (int i = tid; i < n; i += NT) Hh[n + i] = sax[i];
      }
    }
    for (int j = wave; j < K; j += WPI) {                          // f at x+ (this wavefront's own points)
      double w[NW], f[NS], h1, h2;
#pragma unroll
      for (int r = 0; r < NW; ++r) w[r] = sx[idx(j, r)];
      NodeFit::fwd(wl, lane, w, h1, h2, f);
#pragma unroll
      for (int q = 0; q < NS; ++q) sdf[j * NS + q] = f[q];
    }
    __syncthreads();
    for (int k0 = 0; k0 < N; k0 += NT) {
      const bool live = k0 + tid < N;
      const int k = live ? k0 + tid : N - 1;
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        double r0, r1;
        G::jd_rows(sx, sdf, k, q, h, r0, r1);
        if (live) {
          sl[k * NS + q] += eta_v * r0;
          sl[N * NS + k * NS + q] += eta_v * r1;
        }
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += NT) hb[nsteps * hs + i] = sx[i];
  // ---- reverse ----
  const double* sz = seed_z + b * n;
  for (int i = tid; i < n; i += NT) sax[i] = sz[i];
  for (int i = tid; i < m; i += NT) sal[i] = seed_lam ? seed_lam[b * m + i] : 0.0;
  __syncthreads();
  for (int s = nsteps - 1; s >= 0; --s) {
    const double* Hh = hb + s * hs;
    for (int i = tid; i < m; i += NT) sl[i] = Hh[2 * n + i];
    __syncthreads();
    for (int j = wave; j < K; j += WPI) {                          // items 1, 2: sx = x+
      double w[NW], a[NS], e[NS], v[NS], f[NS], jt[NW], h1, h2;
#pragma unroll
      for (int r = 0; r < NW; ++r) w[r] = sx[idx(j, r)];
      G::combine(sal, N, j, h, a, e);
#pragma unroll
      for (int q = 0; q < NS; ++q) v[q] = eta_v * a[q];
      NodeFit::fwd(wl, lane, w, h1, h2, f);
      W::template first<true>(wl, lane, w, h1, h2, v, acc, jt);
#pragma unroll
      for (int r = 0; r < NW; ++r) {
        const int i = idx(j, r);
        const double ax = sax[i] + ((r < NS ? eta_v * e[r] : 0.0) + jt[r]);
        const double m2 = G::inside(sx[i], lo[i], hi[i]) ? ax : 0.0;
        sax[i] = m2;
        sd[i] = -eta_x * m2;
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += NT) sx[i] = Hh[n + i];
    __syncthreads();
    for (int item = 3; item <= 5; item += 2) {                     // items 3, 4 (sx = x_bar, whose place the new direction takes), then 5 (sx = x)
      for (int j = wave; j < K; j += WPI) {
        double w[NW], mu[NS], e[NS], d[NW], hd[NW], hc[NW], wo[NS], f[NS], h1, h2;
#pragma unroll
        for (int r = 0; r < NW; ++r) { w[r] = sx[idx(j, r)]; d[r] = sd[idx(j, r)]; }
        G::combine(sl, N, j, h, mu, e);
        NodeFit::fwd(wl, lane, w, h1, h2, f);
        W::second(wl, lane, w, h1, h2, mu, d, acc, wo, hd);
        P::cost_hd(w, G::wq(K, j, h), d, hc);
#pragma unroll
        for (int q = 0; q < NS; ++q) sdf[j * NS + q] = wo[q];
#pragma unroll
        for (int r = 0; r < NW; ++r) {
          const int i = idx(j, r);
          const double v = hd[r] + hc[r];
          if (item == 3) {
            const double m1 = G::inside(sx[i], lo[i], hi[i]) ? v : 0.0;
            sax[i] += m1;
            sx[i] = -eta_x * m1;
          } else {
            sax[i] += v;
          }
        }
      }
      __syncthreads();
      for (int k0 = 0; k0 < N; k0 += NT) {
        const bool live = k0 + tid < N;
        const int k = live ? k0 + tid : N - 1;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          double r0, r1;
          G::jd_rows(sd, sdf, k, q, h, r0, r1);
          if (live) {
            sal[k * NS + q] += r0;
            sal[N * NS + k * NS + q] += r1;
          }
        }
      }
      __syncthreads();
      if (item == 3) {
        double* t = sd; sd = sx; sx = t;
        for (int i = tid; i < n; i += NT) sx[i] = Hh[i];
        __syncthreads();
      }
    }
  }
  if (dz0) for (int i = tid; i < n; i += NT) dz0[b * n + i] = sax[i];
  if (dlam0) for (int i = tid; i < m; i += NT) dlam0[b * m + i] = sal[i];
  // the weight gradient: wavefront 0 writes its share over the weight copy (idle behind the last barrier) in the parameter order of
  // node_system.h, wavefronts 1, 2, ... add theirs in turn; no atomics, the same bits on every call
  double* gl = wl;
  static_assert(NP <= NodeMfma64::L_N, "the row fits the weight copy");
  double b3v = acc.b3[0];                                          // (the same in every lane: lane r < NS stores entry r)
#pragma unroll
  for (int r = 1; r < NS; ++r) b3v = lane == r ? acc.b3[r] : b3v;
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
      {
        const bool own = lane < NS;
        double* q = gl + S_::O_B3 + (own ? lane : 0);
        const double v = first ? b3v : *q + b3v;
        if (own) *q = v;
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < NP; i += NT) grad[b * NP + i] = gl[i];
}
#endif  // __HIPCC__

}  // namespace myriad
