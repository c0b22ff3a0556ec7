// exgd_jac.h -- forward-mode Jacobian of `nsteps` unrolled extragradient steps in the model parameters (K10j in DESIGN.md).
// Restates what the reference's experiments/e2e_sysid.py:148-177 (many_steps_grad) carries: the full dx/dp and dlam/dp, forward through the steps
//   x_bar = clip(x - eta_x g(x, lam, p)),  x+ = clip(x - eta_x g(x_bar, lam, p)),  lam+ = lam + eta_v c(x+, p)
// of exgd_grad.h (K10 gives seed^T of this Jacobian by one reverse sweep).  With Zx [np][n] = dx/dp, Zl [np][m] = dlam/dp, column k:
//   1. Zxb = m1 o (Zx - eta_x [H(x, lam) Zx      + J(x)^T Zl      + (dg/dp_k)(x, lam)])          m1 = [lb < x_bar < ub]
//   2. Zx+ = m2 o (Zx - eta_x [H(x_bar, lam) Zxb + J(x_bar)^T Zl  + (dg/dp_k)(x_bar, lam)])      m2 = [lb < x+ < ub]
//   3. Zl+ = Zl + eta_v [J(x+) Zx+ + (dc/dp_k)(x+)]
// H, J and the masks are K10's.  Per point, the columns share one evaluation: the Hessian block W (Sys::lin_d2 / Sys::hessian, as back_grad), the
// dynamics Jacobian A, B, and the mixed block M[k][r] = d g_r / d p_k from SysDpw::vjp_p_dir with the NW unit directions (plus term_vjp_p_dir where the
// trapezoidal rule folds the terminal cost into its last point).  Item 3: the constraints are affine in (x, f) (jd_rows(x, f) is c itself), so
// J Zx + dc/dp_k = jd_rows(Zx, A Zx + B Zu + df/dp_k); the rows of df/dp come from SysDp::vjp_p with the NS unit cotangents, as in fit_gn.h.
// No history: the memory does not depend on nsteps.
//
// ExgdJacPoint holds the point algebra as functions of values (host and device); the iterate's own steps are ExgdGradPoint's combine / grad_point /
// jd_rows in colloc_exgd_kernel's order, in loops of their own, so that zn / lamn carry the bits of myr_exgd.  colloc_exgd_jac_kernel runs one
// wavefront per (instance, group of columns); exgd_jac_host is the same sequence as plain loops (tests/hostsim/exgd_jac_twin.cpp).
#pragma once
#include "exgd_grad.h"

namespace myriad {

template <class Sys, int SCHEME>
struct ExgdJacPoint {
  using G = ExgdGradPoint<Sys, SCHEME>;
  static constexpr int NS = Sys::NS, NU = Sys::NU, NW = Sys::NW, NP = Sys::NP;
  // doubles of the iterate's record (x, x_bar, lam, f) and of one tangent column (Zx, Zxb, Zl, A Zx + B Zu + df/dp_k): the same number
  MYR_HD static inline long rec_doubles(int N) { return 2L * G::points(N) * NW + G::rows(N) + (long)G::points(N) * NS; }

  // what the columns share at a point of items 1, 2: W[NW][NW] the Hessian block with mu = a(lam), A, Bm, and M[NP][NW], row k = d g / d p_k
  MYR_HD static inline void grad_blocks(const double* x, const double* u, const double* p, const double* mu, double wj, bool last, double t, double* W,
                                        double* A, double* Bm, double* M) {
    double f[NS], g, gw[NW], D2[Sys::NNZ2];
    set_time<Sys>(p, t);
    Sys::lin_d2(x, u, p, f, A, Bm, &g, gw, D2);
    Sys::hessian(x, u, p, D2, mu, wj, W);
#pragma unroll
    for (int r = 0; r < NW; ++r) {
      double d[NW], gs[NP];
#pragma unroll
      for (int c = 0; c < NW; ++c) d[c] = c == r ? 1.0 : 0.0;
      SysDpw<Sys>::vjp_p_dir(x, u, p, mu, wj, d, gs);
      if constexpr (!G::HS && Sys::HAS_TERMINAL) {
        if (last) {
          double gt[NP];
          SysDpw<Sys>::term_vjp_p_dir(x, u, p, d, gt);
#pragma unroll
          for (int k = 0; k < NP; ++k) gs[k] += gt[k];
        }
      } else { (void)last; }
#pragma unroll
      for (int k = 0; k < NP; ++k) M[k * NW + r] = gs[k];
    }
  }

  // one column at that point: gd[NW] = W Z + (J^T Zl)_j + Mk, with (a, e) = combine(Zl) and Z[NW] the column's (Zx, Zu) of the point
  MYR_HD static inline void grad_col(const double* W, const double* A, const double* Bm, const double* Mk, const double* Z, const double* a,
                                     const double* e, double* gd) {
#pragma unroll
    for (int r = 0; r < NW; ++r) {
      double s = Mk[r];
#pragma unroll
      for (int c = 0; c < NW; ++c) s += W[r * NW + c] * Z[c];
      if (r < NS) {
        s += e[r];
#pragma unroll
        for (int q = 0; q < NS; ++q) s += A[q * NS + r] * a[q];
      } else {
#pragma unroll
        for (int q = 0; q < NS; ++q) s += Bm[q * NU + (r - NS)] * a[q];
      }
      gd[r] = s;
    }
  }

  // what the columns share at a point of item 3: A, Bm and Fp[NP][NS], row k = d f / d p_k
  MYR_HD static inline void dyn_blocks(const double* x, const double* u, const double* p, double t, double* A, double* Bm, double* Fp) {
    double f[NS], g, gw[NW];
    set_time<Sys>(p, t);
    Sys::lin(x, u, p, f, A, Bm, &g, gw);
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      double v[NS], gs[NP];
#pragma unroll
      for (int r = 0; r < NS; ++r) v[r] = r == q ? 1.0 : 0.0;
      SysDp<Sys>::vjp_p(x, u, p, v, gs);
#pragma unroll
      for (int k = 0; k < NP; ++k) Fp[k * NS + q] = gs[k];
    }
  }

  // one column at that point: w[NS] = A Zx + B Zu + Fk
  MYR_HD static inline void dyn_col(const double* A, const double* Bm, const double* Fk, const double* Z, double* w) {
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      double s = Fk[r];
#pragma unroll
      for (int q = 0; q < NS; ++q) s += A[r * NS + q] * Z[q];
#pragma unroll
      for (int c = 0; c < NU; ++c) s += Bm[r * NU + c] * Z[NS + c];
      w[r] = s;
    }
  }
};

// One instance on the host, the sequence of colloc_exgd_jac_kernel as plain loops, for the columns k0 <= k < k0 + nc.  p: SysParams::get();
// work: (1 + nc) rec_doubles(N) doubles; jz0, jlam0 ([NP][n], [NP][m]: the instance's), zn, lamn, jz, jlam may be null.
template <class Sys, int SCHEME>
inline void exgd_jac_host(int N, double h, const double* z, const double* lam, const double* lb, const double* ub, const double* p, double eta_x,
                          double eta_v, int nsteps, const double* jz0, const double* jlam0, int k0, int nc, double* work, double* zn, double* lamn,
                          double* jz, double* jlam) {
  using Q = ExgdJacPoint<Sys, SCHEME>;
  using G = typename Q::G;
  constexpr int NS = G::NS, NU = G::NU, NW = G::NW, NP = G::NP;
  const int K = G::points(N), n = K * NW, m = G::rows(N);
  const long rec = Q::rec_doubles(N);
  double* sx = work;
  double* sax = sx + n;
  double* sl = sax + n;
  double* sdf = sl + m;
  double* cols = work + rec;
  auto idx = [&](int j, int r) { return r < NS ? j * NS + r : K * NS + j * NU + (r - NS); };
  auto load_point = [&](const double* src, int j, double* w) { for (int r = 0; r < NW; ++r) w[r] = src[idx(j, r)]; };
  for (int i = 0; i < n; ++i) sx[i] = z[i];
  for (int i = 0; i < m; ++i) sl[i] = lam[i];
  for (int c = 0; c < nc; ++c) {
    double* zx = cols + c * rec;
    double* zl = zx + 2 * n;
    for (int i = 0; i < n; ++i) zx[i] = jz0 ? jz0[(long)(k0 + c) * n + i] : 0.0;
    for (int i = 0; i < m; ++i) zl[i] = jlam0 ? jlam0[(long)(k0 + c) * m + i] : 0.0;
  }
  for (int s = 0; s < nsteps; ++s) {
    for (int pass = 0; pass < 2; ++pass) {
      const double* src = pass == 0 ? sx : sax;
      double* dst = pass == 0 ? sax : sx;
      if (pass == 1) {                                           // item 1, before x gives way to x+
        for (int j = 0; j < K; ++j) {
          double w[NW], mu[NS], e[NS], W[NW * NW], A[NS * NS], Bm[NS * NU], M[NP * NW];
          load_point(sx, j, w);
          G::combine(sl, N, j, h, mu, e);
          Q::grad_blocks(w, w + NS, p, mu, G::wq(K, j, h), j == K - 1, G::time_of(j, h), W, A, Bm, M);
          for (int c = 0; c < nc; ++c) {
            double* zx = cols + c * rec;
            double* zxb = zx + n;
            double Z[NW], a2[NS], e2[NS], gd[NW];
            load_point(zx, j, Z);
            G::combine(zx + 2 * n, N, j, h, a2, e2);
            Q::grad_col(W, A, Bm, M + (k0 + c) * NW, Z, a2, e2, gd);
            for (int r = 0; r < NW; ++r) { const int i = idx(j, r); zxb[i] = G::inside(sax[i], lb[i], ub[i]) ? zx[i] - eta_x * gd[r] : 0.0; }
          }
        }
      }
      for (int j = 0; j < K; ++j) {
        double w[NW], a[NS], e[NS], g[NW];
        load_point(src, j, w);
        G::combine(sl, N, j, h, a, e);
        G::grad_point(w, w + NS, p, a, e, G::wq(K, j, h), j == K - 1, G::time_of(j, h), g, g + NS);
        for (int r = 0; r < NW; ++r) { const int i = idx(j, r); dst[i] = G::clip(sx[i] - eta_x * g[r], lb[i], ub[i]); }
      }
    }
    for (int j = 0; j < K; ++j) {                                // item 2 (sax = x_bar, sx = x+), and item 3's point part
      double w[NW], mu[NS], e[NS], W[NW * NW], A[NS * NS], Bm[NS * NU], M[NP * NW], Fp[NP * NS];
      load_point(sax, j, w);
      G::combine(sl, N, j, h, mu, e);
      Q::grad_blocks(w, w + NS, p, mu, G::wq(K, j, h), j == K - 1, G::time_of(j, h), W, A, Bm, M);
      for (int c = 0; c < nc; ++c) {
        double* zx = cols + c * rec;
        double* zxb = zx + n;
        double Z[NW], a2[NS], e2[NS], gd[NW];
        load_point(zxb, j, Z);
        G::combine(zx + 2 * n, N, j, h, a2, e2);
        Q::grad_col(W, A, Bm, M + (k0 + c) * NW, Z, a2, e2, gd);
        for (int r = 0; r < NW; ++r) { const int i = idx(j, r); zx[i] = G::inside(sx[i], lb[i], ub[i]) ? zx[i] - eta_x * gd[r] : 0.0; }
      }
      load_point(sx, j, w);
      Q::dyn_blocks(w, w + NS, p, G::time_of(j, h), A, Bm, Fp);
      for (int c = 0; c < nc; ++c) {
        double* zx = cols + c * rec;
        double* zw = zx + 2 * n + m;
        double Z[NW], wo[NS];
        load_point(zx, j, Z);
        Q::dyn_col(A, Bm, Fp + (k0 + c) * NS, Z, wo);
        for (int q = 0; q < NS; ++q) zw[j * NS + q] = wo[q];
      }
    }
    for (int j = 0; j < K; ++j) {
      double w[NW], f[NS];
      load_point(sx, j, w);
      Sys::f(w, w + NS, p, f);
      for (int q = 0; q < NS; ++q) sdf[j * NS + q] = f[q];
    }
    for (int k = 0; k < N; ++k)
      for (int q = 0; q < NS; ++q) {
        double r0, r1;
        G::jd_rows(sx, sdf, k, q, h, r0, r1);
        sl[k * NS + q] += eta_v * r0;
        if (G::HS) sl[N * NS + k * NS + q] += eta_v * r1;
        for (int c = 0; c < nc; ++c) {
          double* zx = cols + c * rec;
          double* zl = zx + 2 * n;
          G::jd_rows(zx, zl + m, k, q, h, r0, r1);
          zl[k * NS + q] += eta_v * r0;
          if (G::HS) zl[N * NS + k * NS + q] += eta_v * r1;
        }
      }
  }
  if (zn) for (int i = 0; i < n; ++i) zn[i] = sx[i];
  if (lamn) for (int i = 0; i < m; ++i) lamn[i] = sl[i];
  for (int c = 0; c < nc; ++c) {
    const double* zx = cols + c * rec;
    if (jz) for (int i = 0; i < n; ++i) jz[(long)(k0 + c) * n + i] = zx[i];
    if (jlam) for (int i = 0; i < m; ++i) jlam[(long)(k0 + c) * m + i] = zx[2 * n + i];
  }
}

#if defined(__HIPCC__)
// One wavefront per (instance, group of columns): blockIdx.x the instance, blockIdx.y the group, which carries the columns
// k0 = blockIdx.y gcols <= k < min(k0 + gcols, NP).  Dynamic LDS: (1 + gcols) rec_doubles(N) doubles -- the iterate's record (x, x_bar, lam, f) and one
// record of the same size per column (Zx, Zxb, Zl, A Zx + B Zu + df/dp_k).  Every group runs the iterate's steps itself (columns do not interact: a
// column has the same bits in every grouping); group 0 writes zn, lamn.  Passes with lanes over points, then over intervals; every loop has a
// wave-uniform trip count, stores are gated by `live`; the loop over the columns is unrolled over all NP, a column outside the group skipped by a
// wave-uniform test, so that M and Fp are indexed by constants.
template <class Sys, int SCHEME>
__global__ __launch_bounds__(64)
void colloc_exgd_jac_kernel(int B, int N, double h, const double* __restrict__ z, const double* __restrict__ lam, const double* __restrict__ lb,
                            const double* __restrict__ ub, const double* __restrict__ params, int params_stride, double eta_x, double eta_v,
                            int nsteps, const double* __restrict__ jz0, const double* __restrict__ jlam0, double* __restrict__ zn,
                            double* __restrict__ lamn, double* __restrict__ jz, double* __restrict__ jlam, int gcols) {
  using Q = ExgdJacPoint<Sys, SCHEME>;
  using G = typename Q::G;
  constexpr int NS = G::NS, NU = G::NU, NW = G::NW, NP = G::NP;
  extern __shared__ __attribute__((aligned(16))) char smem_exgd_jac[];
  const long b = blockIdx.x;
  if (b >= B) return;
  const int lane = threadIdx.x;
  const int k0 = (int)blockIdx.y * gcols;
  const int k1 = k0 + gcols < NP ? k0 + gcols : NP;
  const int K = G::points(N), n = K * NW, m = G::rows(N);
  const long rec = Q::rec_doubles(N);
  double* sx = reinterpret_cast<double*>(smem_exgd_jac);      // x, then x+
  double* sax = sx + n;                                        // x_bar
  double* sl = sax + n;                                        // lam
  double* sdf = sl + m;                                        // f at x+
  double* cols = sx + rec;                                     // column c = k - k0: Zx [n], Zxb [n], Zl [m], A Zx + B Zu + df/dp_k [K NS]
  const double* zb = z + b * n;
  const double* lamb = lam + b * m;
  const double* lo = lb + b * n;
  const double* hi = ub + b * n;
  SysParams<Sys> pp;
  pp.load(params, b, params_stride);
  const double* p = pp.get();
  for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) sx[i] = zb[i]; }
  for (int i0 = 0; i0 < m; i0 += 64) { const int i = i0 + lane; if (i < m) sl[i] = lamb[i]; }
  for (int k = k0; k < k1; ++k) {
    double* zx = cols + (k - k0) * rec;
    double* zl = zx + 2 * n;
    const long row = b * NP + k;
    for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) zx[i] = jz0 ? jz0[row * n + i] : 0.0; }
    for (int i0 = 0; i0 < m; i0 += 64) { const int i = i0 + lane; if (i < m) zl[i] = jlam0 ? jlam0[row * m + i] : 0.0; }
  }
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    for (int pass = 0; pass < 2; ++pass) {
      const double* src = pass == 0 ? sx : sax;
      double* dst = pass == 0 ? sax : sx;
      // the tangent of the half-step that ended at src's successor: pass 1 does item 1 (at x, masked by x_bar) before x gives way to x+
      if (pass == 1) {
        for (int j0 = 0; j0 < K; j0 += 64) {
          const bool live = j0 + lane < K;
          const int j = live ? j0 + lane : K - 1;
          double x[NS], u[NU], mu[NS], e[NS], W[NW * NW], A[NS * NS], Bm[NS * NU], M[NP * NW];
#pragma unroll
          for (int q = 0; q < NS; ++q) x[q] = sx[j * NS + q];
#pragma unroll
          for (int c = 0; c < NU; ++c) u[c] = sx[K * NS + j * NU + c];
          G::combine(sl, N, j, h, mu, e);
          Q::grad_blocks(x, u, p, mu, G::wq(K, j, h), j == K - 1, G::time_of(j, h), W, A, Bm, M);
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            if (k < k0 || k >= k1) continue;
            double* zx = cols + (k - k0) * rec;
            double* zxb = zx + n;
            double Z[NW], a2[NS], e2[NS], gd[NW];
#pragma unroll
            for (int r = 0; r < NW; ++r) Z[r] = zx[r < NS ? j * NS + r : K * NS + j * NU + (r - NS)];
            G::combine(zx + 2 * n, N, j, h, a2, e2);
            Q::grad_col(W, A, Bm, M + k * NW, Z, a2, e2, gd);
#pragma unroll
            for (int r = 0; r < NW; ++r) {
              const int i = r < NS ? j * NS + r : K * NS + j * NU + (r - NS);
              const double v = G::inside(sax[i], lo[i], hi[i]) ? zx[i] - eta_x * gd[r] : 0.0;
              if (live) zxb[i] = v;
            }
          }
        }
        __syncthreads();
      }
      // the iterate's half-step: colloc_exgd_kernel's arithmetic in its order
      for (int j0 = 0; j0 < K; j0 += 64) {
        const bool live = j0 + lane < K;
        const int j = live ? j0 + lane : K - 1;
        double x[NS], u[NU], a[NS], e[NS], gx[NS], gu[NU];
#pragma unroll
        for (int q = 0; q < NS; ++q) x[q] = src[j * NS + q];
#pragma unroll
        for (int c = 0; c < NU; ++c) u[c] = src[K * NS + j * NU + c];
        G::combine(sl, N, j, h, a, e);
        G::grad_point(x, u, p, a, e, G::wq(K, j, h), j == K - 1, G::time_of(j, h), gx, gu);
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          const int i = j * NS + q;
          const double v = G::clip(sx[i] - eta_x * gx[q], lo[i], hi[i]);
          if (live) dst[i] = v;
        }
#pragma unroll
        for (int c = 0; c < NU; ++c) {
          const int i = K * NS + j * NU + c;
          const double v = G::clip(sx[i] - eta_x * gu[c], lo[i], hi[i]);
          if (live) dst[i] = v;
        }
      }
      __syncthreads();
    }
    // item 2 (at x_bar, masked by x+), then the point part of item 3 at x+
    for (int j0 = 0; j0 < K; j0 += 64) {
      const bool live = j0 + lane < K;
      const int j = live ? j0 + lane : K - 1;
      {
        double x[NS], u[NU], mu[NS], e[NS], W[NW * NW], A[NS * NS], Bm[NS * NU], M[NP * NW];
#pragma unroll
        for (int q = 0; q < NS; ++q) x[q] = sax[j * NS + q];
#pragma unroll
        for (int c = 0; c < NU; ++c) u[c] = sax[K * NS + j * NU + c];
        G::combine(sl, N, j, h, mu, e);
        Q::grad_blocks(x, u, p, mu, G::wq(K, j, h), j == K - 1, G::time_of(j, h), W, A, Bm, M);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          if (k < k0 || k >= k1) continue;
          double* zx = cols + (k - k0) * rec;
          const double* zxb = zx + n;
          double Z[NW], a2[NS], e2[NS], gd[NW];
#pragma unroll
          for (int r = 0; r < NW; ++r) Z[r] = zxb[r < NS ? j * NS + r : K * NS + j * NU + (r - NS)];
          G::combine(zx + 2 * n, N, j, h, a2, e2);
          Q::grad_col(W, A, Bm, M + k * NW, Z, a2, e2, gd);
#pragma unroll
          for (int r = 0; r < NW; ++r) {
            const int i = r < NS ? j * NS + r : K * NS + j * NU + (r - NS);
            const double v = G::inside(sx[i], lo[i], hi[i]) ? zx[i] - eta_x * gd[r] : 0.0;
            if (live) zx[i] = v;
          }
        }
      }
      {
        double x[NS], u[NU], A[NS * NS], Bm[NS * NU], Fp[NP * NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) x[q] = sx[j * NS + q];
#pragma unroll
        for (int c = 0; c < NU; ++c) u[c] = sx[K * NS + j * NU + c];
        Q::dyn_blocks(x, u, p, G::time_of(j, h), A, Bm, Fp);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          if (k < k0 || k >= k1) continue;
          double* zx = cols + (k - k0) * rec;
          double* zw = zx + 2 * n + m;
          double Z[NW], w[NS];
#pragma unroll
          for (int r = 0; r < NW; ++r) Z[r] = zx[r < NS ? j * NS + r : K * NS + j * NU + (r - NS)];      // (this lane's own stores of item 2)
          Q::dyn_col(A, Bm, Fp + k * NS, Z, w);
#pragma unroll
          for (int q = 0; q < NS; ++q) if (live) zw[j * NS + q] = w[q];
        }
      }
    }
    // f at x+ and the multiplier update: colloc_exgd_kernel's
    for (int j0 = 0; j0 < K; j0 += 64) {
      const bool live = j0 + lane < K;
      const int j = live ? j0 + lane : K - 1;
      double x[NS], u[NU], f[NS];
#pragma unroll
      for (int q = 0; q < NS; ++q) x[q] = sx[j * NS + q];
#pragma unroll
      for (int c = 0; c < NU; ++c) u[c] = sx[K * NS + j * NU + c];
      Sys::f(x, u, p, f);
#pragma unroll
      for (int q = 0; q < NS; ++q) if (live) sdf[j * NS + q] = f[q];
    }
    __syncthreads();
    for (int k0i = 0; k0i < N; k0i += 64) {
      const bool live = k0i + lane < N;
      const int k = live ? k0i + lane : N - 1;
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        double r0, r1;
        G::jd_rows(sx, sdf, k, q, h, r0, r1);
        if (live) {
          sl[k * NS + q] += eta_v * r0;
          if (G::HS) sl[N * NS + k * NS + q] += eta_v * r1;
        }
      }
    }
    for (int kc = k0; kc < k1; ++kc) {                           // item 3, lanes over intervals
      double* zx = cols + (kc - k0) * rec;
      double* zl = zx + 2 * n;
      for (int k0i = 0; k0i < N; k0i += 64) {
        const bool live = k0i + lane < N;
        const int k = live ? k0i + lane : N - 1;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          double r0, r1;
          G::jd_rows(zx, zl + m, k, q, h, r0, r1);
          if (live) {
            zl[k * NS + q] += eta_v * r0;
            if (G::HS) zl[N * NS + k * NS + q] += eta_v * r1;
          }
        }
      }
    }
    __syncthreads();
  }
  if (blockIdx.y == 0) {
    if (zn) for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) zn[b * n + i] = sx[i]; }
    if (lamn) for (int i0 = 0; i0 < m; i0 += 64) { const int i = i0 + lane; if (i < m) lamn[b * m + i] = sl[i]; }
  }
  for (int k = k0; k < k1; ++k) {
    const double* zx = cols + (k - k0) * rec;
    const long row = b * NP + k;
    if (jz) for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) jz[row * n + i] = zx[i]; }
    if (jlam) for (int i0 = 0; i0 < m; i0 += 64) { const int i = i0 + lane; if (i < m) jlam[row * m + i] = zx[2 * n + i]; }
  }
}

// bytes of dynamic LDS for `gcols` columns to a group
template <class Sys, int SCHEME>
inline size_t colloc_exgd_jac_lds_bytes(int N, int gcols) {
  return (size_t)(1 + gcols) * (size_t)ExgdJacPoint<Sys, SCHEME>::rec_doubles(N) * 8 + 16;
}
#endif  // __HIPCC__

}  // namespace myriad
