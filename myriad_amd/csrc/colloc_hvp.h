// colloc_hvp.h -- Lagrangian Hessian-vector product of the collocation transcriptions (K11 in DESIGN.md; C-ABI myr_hvp; shooting: shoot_hvp.h).
// grad^2_zz L is block-diagonal over the points: point j contributes W_j v_j with W_j = Sys::hessian(x_j, u_j, p, D2, mu = a_j(lam), w = with_cost wq_j)
// to out_z and SysDpw::vjp_p_dir(x_j, u_j, p, a_j(lam), with_cost wq_j, v_j) -- plus term_vjp_p_dir where the trapezoidal rule folds a terminal cost
// into its last point -- to out_p.  That is ExgdGradPoint::combine + ExgdGradPoint::back_grad (exgd_grad.h), used as they stand.
#pragma once
#include "exgd_grad.h"

namespace myriad {

template <class Sys, int SCHEME>
struct CollocHvp {
  using G = ExgdGradPoint<Sys, SCHEME>;
  static constexpr int NS = Sys::NS, NU = Sys::NU, NW = Sys::NW, NP = Sys::NP;
  // point j of one instance: hd[NW] = W_j v_j, gs[NP] = the point's share of out_p.  zb, vb: the instance's z and v; lam: its multipliers or null
  MYR_HD static inline void point(int N, int K, int j, double h, const double* zb, const double* lam, const double* vb, const double* p, int with_cost,
                                  double* hd, double* gs) {
    double x[NS], u[NU], d[NW], mu[NS], e[NS], w[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) { x[q] = zb[(long)j * NS + q]; d[q] = vb[(long)j * NS + q]; mu[q] = 0.0; }
#pragma unroll
    for (int c = 0; c < NU; ++c) { u[c] = zb[(long)K * NS + (long)j * NU + c]; d[NS + c] = vb[(long)K * NS + (long)j * NU + c]; }
    if (lam) G::combine(lam, N, j, h, mu, e);
    G::back_grad(x, u, p, mu, with_cost ? G::wq(K, j, h) : 0.0, with_cost && j == K - 1, G::time_of(j, h), d, hd, w, gs);
  }
};

// one instance on the host: the points in ascending order.  lam, oz, op may be null
template <class Sys, int SCHEME>
inline void colloc_hvp_host(int N, double h, const double* z, const double* lam, const double* v, const double* p, int with_cost, double* oz, double* op) {
  using C = CollocHvp<Sys, SCHEME>;
  constexpr int NS = Sys::NS, NU = Sys::NU, NW = Sys::NW, NP = Sys::NP;
  const int K = C::G::points(N);
  double gp[NP];
  for (int k = 0; k < NP; ++k) gp[k] = 0.0;
  for (int j = 0; j < K; ++j) {
    double hd[NW], gs[NP];
    C::point(N, K, j, h, z, lam, v, p, with_cost, hd, gs);
    for (int k = 0; k < NP; ++k) gp[k] += gs[k];
    if (oz) for (int r = 0; r < NW; ++r) oz[r < NS ? (long)j * NS + r : (long)K * NS + (long)j * NU + (r - NS)] = hd[r];
  }
  if (op) for (int k = 0; k < NP; ++k) op[k] = gp[k];
}

#if defined(__HIPCC__)
// One wavefront per instance, lanes over the points in rounds of 64 (a wave-uniform trip count, `live`-gated stores); the inputs are read where they
// lie (no LDS: every horizon fits).  The point's share of out_p lives in NP registers per lane and meets in one butterfly: every lane ends with the
// same bits and every lane stores them.  No lane-0 block, no atomics.
template <class Sys, int SCHEME>
__global__ __launch_bounds__(64)
void colloc_hvp_kernel(int B, int N, double h, const double* __restrict__ z, const double* __restrict__ lam, const double* __restrict__ v,
                       const double* __restrict__ params, int params_stride, int with_cost, double* __restrict__ out_z, double* __restrict__ rows) {
  using C = CollocHvp<Sys, SCHEME>;
  constexpr int NS = Sys::NS, NU = Sys::NU, NW = Sys::NW, NP = Sys::NP;
  const long b = blockIdx.x;
  if (b >= B) return;
  const int lane = threadIdx.x;
  const int K = C::G::points(N), m = C::G::rows(N);
  const long n = (long)K * NW;
  SysParams<Sys> pp;
  pp.load(params, b, params_stride);
  double gp[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) gp[k] = 0.0;
  for (int j0 = 0; j0 < K; j0 += 64) {
    const bool live = j0 + lane < K;
    const int j = live ? j0 + lane : K - 1;
    double hd[NW], gs[NP];
    C::point(N, K, j, h, z + b * n, lam ? lam + b * m : nullptr, v + b * n, pp.get(), with_cost, hd, gs);
#pragma unroll
    for (int k = 0; k < NP; ++k) gp[k] += live ? gs[k] : 0.0;
    if (out_z) {
#pragma unroll
      for (int r = 0; r < NW; ++r) {
        const long i = r < NS ? (long)j * NS + r : (long)K * NS + (long)j * NU + (r - NS);
        if (live) out_z[b * n + i] = hd[r];
      }
    }
  }
  if (rows) {
#pragma unroll
    for (int k = 0; k < NP; ++k) rows[b * NP + k] = wv_sum(gp[k]);      // (the same bits in every lane: every lane stores)
  }
}
#endif  // __HIPCC__

}  // namespace myriad
