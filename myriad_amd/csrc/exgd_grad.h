// exgd_grad.h -- derivative of `nsteps` unrolled extragradient steps in the model parameters (K10 in DESIGN.md).
// Restates what the reference's experiments/e2e_sysid.py:148-177, 209-218 (many_steps_grad, lookahead_update) differentiates: with
//   L(z, lam, p) = f(z, p) + lam^T c(z, p),  g = grad_z L,  and one step
//   x_bar = clip(x - eta_x g(x, lam, p)),  x+ = clip(x - eta_x g(x_bar, lam, p)),  lam+ = lam + eta_v c(x+, p)
// the reference carries dx/dp, dlam/dp forward from a starting point held fixed.  Here ONE reverse sweep gives, for a seed (w_z, w_lam),
//   grad = w_z^T dz_n/dp + w_lam^T dlam_n/dp   and the same cotangent in the starting point (dz0, dlam0),
// whatever the number of parameters.  From (a_x+, a_lam+) behind step s, with the stored x_s, x_bar_s, x_{s+1}, lam_s:
//   1. a_x+ += eta_v J(x+)^T a_lam+          gp += eta_v (dc/dp)(x+)^T a_lam+          a_lam = a_lam+
//   2. m2 = [lb < x+ < ub] o a_x+            a_x = m2          t = -eta_x m2
//   3. a_xbar = H(x_bar, lam) t              a_lam += J(x_bar) t                       gp += (dg/dp)(x_bar, lam)^T t
//   4. m1 = [lb < x_bar < ub] o a_xbar       a_x += m1         s = -eta_x m1
//   5. a_x += H(x, lam) s                    a_lam += J(x) s                           gp += (dg/dp)(x, lam)^T s
// H = grad^2_zz L is block-diagonal over the collocation points: Sys::hessian with mu = a_j(lam) (the `a` of CollocProducts::combine) and the
// quadrature weight of the point; (dc/dp)^T a_lam = sum_j SysDp::vjp_p(point j, a_j(a_lam)); (dg/dp)^T d at point j is SysDpw::vjp_p_dir
// (systems_dpw_gen.h), plus term_vjp_p_dir where the trapezoidal transcription folds the terminal cost into its last point.  A pinned variable
// (lb == ub) and a variable that sits on a bound have mask 0.
//
// ExgdGradPoint holds the point / interval algebra as functions of values (host and device; combine / grad_point restate CollocProducts' device-only
// combine / vjp_point, so that both phases of kernel and twin run one text); colloc_exgd_grad_kernel runs it with one
// wavefront per instance, colloc_exgd_grad_host<ExgdGradClosedPoint> (= exgd_grad_host) is the same sequence as plain loops
// (tests/hostsim/exgd_grad_twin.cpp).
#pragma once
#include "systems_gen.h"
#include "systems_dp_gen.h"
#include "systems_dpw_gen.h"
#if defined(__HIPCC__)
#include "wave_prims.h"
#endif

namespace myriad {

enum { EXGD_GRAD_HS = 0, EXGD_GRAD_TRAP = 1 };      // = PROD_HS, PROD_TRAP

template <class Sys, int SCHEME>
struct ExgdGradPoint {
  static constexpr int NS = Sys::NS, NU = Sys::NU, NW = Sys::NW, NP = Sys::NP;
  static constexpr bool HS = SCHEME == EXGD_GRAD_HS;
  MYR_HD static inline int points(int N) { return HS ? 2 * N + 1 : N + 1; }
  MYR_HD static inline int rows(int N) { return (HS ? 2 : 1) * N * NS; }
  MYR_HD static inline double wq(int K, int j, double h) {
    if (HS) return (j & 1) ? 4.0 * h / 6.0 : ((j == 0 || j == K - 1) ? h / 6.0 : 2.0 * h / 6.0);
    return (j == 0 || j == K - 1) ? 0.5 * h : h;
  }
  MYR_HD static inline double time_of(int j, double h) { return (HS ? 0.5 * h : h) * j; }
  // doubles of one instance's history: x_s, x_bar_s, lam_s of every step, then the final x
  MYR_HD static inline long hist_doubles(int N, int nsteps) {
    const long n = (long)points(N) * NW, m = rows(N);
    return (long)nsteps * (2 * n + m) + n;
  }
  MYR_HD static inline bool inside(double v, double lo, double hi) { return v > lo && v < hi; }
  MYR_HD static inline double clip(double v, double l, double u) { return v < l ? l : (v > u ? u : v); }

  // multiplier combination of point j (CollocProducts::combine, host and device)
  MYR_HD static inline void combine(const double* lam, int N, int j, double h, double* a, double* e) {
    if (HS) {
      const double h6 = h / 6.0, h8 = h / 8.0;
      const double* ld = lam;
      const double* li = lam + (long)N * NS;
      if (j & 1) {
        const int k = (j - 1) >> 1;
#pragma unroll
        for (int q = 0; q < NS; ++q) { a[q] = -4.0 * h6 * ld[k * NS + q]; e[q] = li[k * NS + q]; }
      } else {
        const int kL = (j >> 1) - 1, kR = j >> 1;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          const double dl = kL >= 0 ? ld[kL * NS + q] : 0.0, il = kL >= 0 ? li[kL * NS + q] : 0.0;
          const double dr = kR < N ? ld[kR * NS + q] : 0.0, ir = kR < N ? li[kR * NS + q] : 0.0;
          a[q] = -h6 * (dl + dr) + h8 * (il - ir);
          e[q] = dl - dr - 0.5 * (il + ir);
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        const double l0 = j >= 1 ? lam[(j - 1) * NS + q] : 0.0, l1 = j < N ? lam[j * NS + q] : 0.0;
        a[q] = 0.5 * h * (l0 + l1);
        e[q] = l1 - l0;
      }
    }
  }

  // grad_z L restricted to point j (CollocProducts::vjp_point with add_gradf, host and device)
  MYR_HD static inline void grad_point(const double* x, const double* u, const double* p, const double* a, const double* e, double wj, bool last,
                                       double t, double* gx, double* gu) {
    double f[NS], A[NS * NS], Bm[NS * NU], g, gw[NW];
    set_time<Sys>(p, t);
    Sys::lin(x, u, p, f, A, Bm, &g, gw);
    if (!HS && last) fold_terminal<Sys>(x, u, p, wj, g, gw);
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      double s = e[q] + wj * gw[q];
#pragma unroll
      for (int r = 0; r < NS; ++r) s += A[r * NS + q] * a[r];
      gx[q] = s;
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) {
      double s = wj * gw[NS + c];
#pragma unroll
      for (int r = 0; r < NS; ++r) s += Bm[r * NU + c] * a[r];
      gu[c] = s;
    }
  }

  // item 1 at a point of x+: jt[NW] = (J^T a_lam)_j from (a, e) = combine(a_lam); gs[NP] = (dc/dp)^T a_lam restricted to the point
  MYR_HD static inline void back_constraint(const double* x, const double* u, const double* p, const double* a, const double* e, double t,
                                            double* jt, double* gs) {
    double f[NS], A[NS * NS], Bm[NS * NU], g, gw[NW];
    set_time<Sys>(p, t);
    Sys::lin(x, u, p, f, A, Bm, &g, gw);
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      double s = e[q];
#pragma unroll
      for (int r = 0; r < NS; ++r) s += A[r * NS + q] * a[r];
      jt[q] = s;
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < NS; ++r) s += Bm[r * NU + c] * a[r];
      jt[NS + c] = s;
    }
    SysDp<Sys>::vjp_p(x, u, p, a, gs);
  }

  // items 3 and 5 at a point: direction d[NW] = (d_x, d_u) through the point's Hessian block (hd[NW]), through its dynamics Jacobian
  // (w[NS] = A d_x + B d_u, which the interval pass turns into J d) and through the mixed derivative (gs[NP] = (dg/dp)^T d).
  // The terminal cost the trapezoidal rule folds into its last point adds its p-derivative only: it is LINEAR in (x, u) -- tools/gen_systems.py
  // asserts that for every system, in gen_system() and in gen_system_dpw() -- so it has no share in the Hessian block
  MYR_HD static inline void back_grad(const double* x, const double* u, const double* p, const double* mu, double wj, bool last, double t,
                                      const double* d, double* hd, double* w, double* gs) {
    double f[NS], A[NS * NS], Bm[NS * NU], g, gw[NW], D2[Sys::NNZ2], W[NW * NW];
    set_time<Sys>(p, t);
    Sys::lin_d2(x, u, p, f, A, Bm, &g, gw, D2);
    Sys::hessian(x, u, p, D2, mu, wj, W);
#pragma unroll
    for (int r = 0; r < NW; ++r) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < NW; ++c) s += W[r * NW + c] * d[c];
      hd[r] = s;
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < NS; ++q) s += A[r * NS + q] * d[q];
#pragma unroll
      for (int c = 0; c < NU; ++c) s += Bm[r * NU + c] * d[NS + c];
      w[r] = s;
    }
    SysDpw<Sys>::vjp_p_dir(x, u, p, mu, wj, d, gs);
    if constexpr (!HS && Sys::HAS_TERMINAL) {
      if (last) {
        double gt[NP];
        SysDpw<Sys>::term_vjp_p_dir(x, u, p, d, gt);
#pragma unroll
        for (int k = 0; k < NP; ++k) gs[k] += gt[k];
      }
    } else { (void)last; }
  }

  // rows of J d of interval k, component q, from the direction's state part vx ([point][NS]) and w ([point][NS]): r0 the defect row (k NS + q),
  // (the constraints are affine in (x, f) with the same coefficients: jd_rows(x, f) is c itself, which the multiplier update uses)
  // r1 the Hermite-Simpson interpolation row (N NS + k NS + q; 0 for the trapezoidal rule)
  MYR_HD static inline void jd_rows(const double* vx, const double* w, int k, int q, double h, double& r0, double& r1) {
    if (HS) {
      const double h6 = h / 6.0, h8 = h / 8.0;
      const int js = 2 * k, jm = js + 1, je = js + 2;
      r0 = (vx[je * NS + q] - vx[js * NS + q]) - h6 * (w[js * NS + q] + 4.0 * w[jm * NS + q] + w[je * NS + q]);
      r1 = vx[jm * NS + q] - 0.5 * (vx[js * NS + q] + vx[je * NS + q]) - h8 * (w[js * NS + q] - w[je * NS + q]);
    } else {
      r0 = 0.5 * h * (w[k * NS + q] + w[(k + 1) * NS + q]) - (vx[(k + 1) * NS + q] - vx[k * NS + q]);
      r1 = 0.0;
    }
  }
};

// The point policy of the closed-form systems for colloc_exgd_grad_host: ExgdGradPoint's functions at w = [x; u], gp[k] += ... from the point's gs
template <class Sys_, int SCHEME>
struct ExgdGradClosedPoint {
  using Sys = Sys_;
  using G = ExgdGradPoint<Sys, SCHEME>;
  static constexpr int NS = G::NS, NP = G::NP;
  // grad_z L at the point (the forward steps)
  static inline void grad(const double* w, const double* p, const double* a, const double* e, double wq, bool last, double t, double* g) {
    G::grad_point(w, w + NS, p, a, e, wq, last, t, g, g + NS);
  }
  // item 1 from (a, e) = combine(a_lam): jt, the point's share of gp, and a_x+ of entry r
  static inline void constraint(const double* w, const double* p, const double* a, const double* e, double t, double eta_v, double* jt, double* gp) {
    double gs[NP];
    G::back_constraint(w, w + NS, p, a, e, t, jt, gs);
    for (int k = 0; k < NP; ++k) gp[k] += eta_v * gs[k];
  }
  static inline double step_ax(double ax, int r, double eta_v, const double* e, const double* jt) { (void)e; return ax + eta_v * jt[r]; }
  // items 3 and 5: hd = H d at the point, wo = A d_x + B d_u, the point's share of gp
  static inline void hess(const double* w, const double* p, const double* mu, double wq, bool last, double t, const double* d, double* hd, double* wo,
                          double* gp) {
    double gs[NP];
    G::back_grad(w, w + NS, p, mu, wq, last, t, d, hd, wo, gs);
    for (int k = 0; k < NP; ++k) gp[k] += gs[k];
  }
};

// One instance on the host, the sequence of colloc_exgd_grad_kernel (and of node_exgd_grad_kernel) as plain loops: the forward steps, items 1-5,
// the buffer swap and the history, once for both; every floating-point expression of a point is the policy's (ExgdGradClosedPoint above,
// NodeExgdPoint in node_exgd_grad.h).  p: the instance's parameter buffer (SysParams::get(); the shared weights); hist: hist_doubles(N, nsteps)
// doubles; work: 3 n + 2 m + K NS doubles; seed_lam, dz0, dlam0 may be null; gp[NP].
template <class Point>
inline void colloc_exgd_grad_host(int N, double h, const double* z, const double* lam, const double* lb, const double* ub, const double* p,
                                  double eta_x, double eta_v, int nsteps, const double* seed_z, const double* seed_lam, double* hist, double* work,
                                  double* gp, double* dz0, double* dlam0) {
  using G = typename Point::G;
  constexpr int NS = G::NS, NU = G::NU, NW = G::NW, NP = G::NP;
  const int K = G::points(N), n = K * NW, m = G::rows(N);
  const long hs = 2L * n + m;
  double* sx = work;
  double* sax = sx + n;
  double* sd = sax + n;
  double* sl = sd + n;
  double* sal = sl + m;
  double* sdf = sal + m;
  auto idx = [&](int j, int r) { return r < NS ? j * NS + r : K * NS + j * NU + (r - NS); };
  auto load_point = [&](const double* src, int j, double* w) { for (int r = 0; r < NW; ++r) w[r] = src[idx(j, r)]; };
  // forward: sx = z, sax = x_bar, sl = lam, sdf = f
  for (int i = 0; i < n; ++i) sx[i] = z[i];
  for (int i = 0; i < m; ++i) sl[i] = lam[i];
  for (int s = 0; s < nsteps; ++s) {
    double* H = hist + s * hs;
    for (int i = 0; i < n; ++i) H[i] = sx[i];
    for (int i = 0; i < m; ++i) H[2 * n + i] = sl[i];
    for (int pass = 0; pass < 2; ++pass) {
      const double* src = pass == 0 ? sx : sax;
      double* dst = pass == 0 ? sax : sx;
      for (int j = 0; j < K; ++j) {
        double w[NW], a[NS], e[NS], g[NW];
        load_point(src, j, w);
        G::combine(sl, N, j, h, a, e);
        Point::grad(w, p, a, e, G::wq(K, j, h), j == K - 1, G::time_of(j, h), g);
        for (int r = 0; r < NW; ++r) { const int i = idx(j, r); dst[i] = G::clip(sx[i] - eta_x * g[r], lb[i], ub[i]); }
      }
      if (pass == 0) for (int i = 0; i < n; ++i) H[n + i] = sax[i];
    }
    for (int j = 0; j < K; ++j) {
      double w[NW], f[NS];
      load_point(sx, j, w);
      Point::Sys::f(w, w + NS, p, f);
      for (int q = 0; q < NS; ++q) sdf[j * NS + q] = f[q];
    }
    for (int k = 0; k < N; ++k)
      for (int q = 0; q < NS; ++q) {
        double r0, r1;
        G::jd_rows(sx, sdf, k, q, h, r0, r1);      // c itself: the rows of J d with (x, f) in the place of (d_x, A d_x + B d_u)
        sl[k * NS + q] += eta_v * r0;
        if (G::HS) sl[N * NS + k * NS + q] += eta_v * r1;
      }
  }
  for (int i = 0; i < n; ++i) hist[nsteps * hs + i] = sx[i];
  // reverse
  for (int i = 0; i < n; ++i) sax[i] = seed_z[i];
  for (int i = 0; i < m; ++i) sal[i] = seed_lam ? seed_lam[i] : 0.0;
  for (int k = 0; k < NP; ++k) gp[k] = 0.0;
  for (int s = nsteps - 1; s >= 0; --s) {
    const double* H = hist + s * hs;
    for (int i = 0; i < m; ++i) sl[i] = H[2 * n + i];
    for (int j = 0; j < K; ++j) {                                // items 1, 2 (sx = x+)
      double w[NW], a[NS], e[NS], jt[NW];
      load_point(sx, j, w);
      G::combine(sal, N, j, h, a, e);
      Point::constraint(w, p, a, e, G::time_of(j, h), eta_v, jt, gp);
      for (int r = 0; r < NW; ++r) {
        const int i = idx(j, r);
        const double ax = Point::step_ax(sax[i], r, eta_v, e, jt);
        const double m2 = G::inside(sx[i], lb[i], ub[i]) ? ax : 0.0;
        sax[i] = m2;
        sd[i] = -eta_x * m2;
      }
    }
    for (int i = 0; i < n; ++i) sx[i] = H[n + i];
    for (int item = 3; item <= 5; item += 2) {                   // items 3, 4 (sx = x_bar, whose place the new direction takes), then 5 (sx = x)
      for (int j = 0; j < K; ++j) {
        double w[NW], mu[NS], e[NS], d[NW], hd[NW], wo[NS];
        load_point(sx, j, w);
        load_point(sd, j, d);
        G::combine(sl, N, j, h, mu, e);
        Point::hess(w, p, mu, G::wq(K, j, h), j == K - 1, G::time_of(j, h), d, hd, wo, gp);
        for (int q = 0; q < NS; ++q) sdf[j * NS + q] = wo[q];
        for (int r = 0; r < NW; ++r) {
          const int i = idx(j, r);
          if (item == 3) {
            const double m1 = G::inside(sx[i], lb[i], ub[i]) ? hd[r] : 0.0;
            sax[i] += m1;
            sx[i] = -eta_x * m1;
          } else {
            sax[i] += hd[r];
          }
        }
      }
      for (int k = 0; k < N; ++k)
        for (int q = 0; q < NS; ++q) {
          double r0, r1;
          G::jd_rows(sd, sdf, k, q, h, r0, r1);
          sal[k * NS + q] += r0;
          if (G::HS) sal[N * NS + k * NS + q] += r1;
        }
      if (item == 3) {
        double* t = sd; sd = sx; sx = t;
        for (int i = 0; i < n; ++i) sx[i] = H[i];
      }
    }
  }
  if (dz0) for (int i = 0; i < n; ++i) dz0[i] = sax[i];
  if (dlam0) for (int i = 0; i < m; ++i) dlam0[i] = sal[i];
}

template <class Sys, int SCHEME, class... A>
inline void exgd_grad_host(A... a) { colloc_exgd_grad_host<ExgdGradClosedPoint<Sys, SCHEME>>(a...); }

#if defined(__HIPCC__)
// One wavefront per instance (blockIdx.x: the instance within this launch's chunk; every pointer is the chunk's).  Dynamic LDS:
// (3 n + 2 m + K NS) doubles.  Forward phase: the steps of colloc_exgd_kernel (the same point arithmetic in the same order), x_s, x_bar_s, lam_s of
// every step and the final x written to `hist` (lane-contiguous).  Reverse phase: items 1-5 above, passes with lanes over points followed by lanes over
// intervals; gp in NP registers per lane, one butterfly sum at the end.  Every loop has a wave-uniform trip count; stores are gated by `live`.
template <class Sys, int SCHEME>
__global__ __launch_bounds__(64)
void colloc_exgd_grad_kernel(int B, int N, double h, const double* __restrict__ z, const double* __restrict__ lam,
                             const double* __restrict__ lb, const double* __restrict__ ub, const double* __restrict__ params, int params_stride,
                             double eta_x, double eta_v, int nsteps, const double* __restrict__ seed_z,
                             const double* __restrict__ seed_lam, double* __restrict__ hist, double* __restrict__ grad, double* __restrict__ dz0,
                             double* __restrict__ dlam0) {
  using G = ExgdGradPoint<Sys, SCHEME>;
  constexpr int NS = G::NS, NU = G::NU, NW = G::NW, NP = G::NP;
  extern __shared__ __attribute__((aligned(16))) char smem_exgd_grad[];
  const long b = blockIdx.x;
  if (b >= B) return;
  const int lane = threadIdx.x;
  const int K = G::points(N), n = K * NW, m = G::rows(N);
  const long hs = 2L * n + m;
  double* sx = reinterpret_cast<double*>(smem_exgd_grad);      // forward: z; reverse: the point the pass stands at (x+, x_bar, x)
  double* sax = sx + n;                                         // forward: x_bar; reverse: a_x
  double* sd = sax + n;                                         // reverse: the direction (t, then s)
  double* sl = sd + n;                                          // lam of the step
  double* sal = sl + m;                                         // reverse: a_lam
  double* sdf = sal + m;                                        // forward: f at x+; reverse: A d_x + B d_u of every point
  const double* zb = z + b * n;
  const double* lamb = lam + b * m;
  const double* lo = lb + b * n;
  const double* hi = ub + b * n;
  double* hb = hist + b * G::hist_doubles(N, nsteps);
  SysParams<Sys> pp;
  pp.load(params, b, params_stride);
  const double* p = pp.get();
  for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) sx[i] = zb[i]; }
  for (int i0 = 0; i0 < m; i0 += 64) { const int i = i0 + lane; if (i < m) sl[i] = lamb[i]; }
  __syncthreads();
  // ---- forward ----
  for (int s = 0; s < nsteps; ++s) {
    double* H = hb + s * hs;
    for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) H[i] = sx[i]; }
    for (int i0 = 0; i0 < m; i0 += 64) { const int i = i0 + lane; if (i < m) H[2 * n + i] = sl[i]; }
    for (int pass = 0; pass < 2; ++pass) {
      const double* src = pass == 0 ? sx : sax;
      double* dst = pass == 0 ? sax : sx;
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
      if (pass == 0) {
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) H[n + i] = sax[i]; }
      }
    }
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
    for (int k0 = 0; k0 < N; k0 += 64) {
      const bool live = k0 + lane < N;
      const int k = live ? k0 + lane : N - 1;
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        double r0, r1;
        G::jd_rows(sx, sdf, k, q, h, r0, r1);      // c itself: the rows of J d with (x, f) in the place of (d_x, A d_x + B d_u)
        if (live) {
          sl[k * NS + q] += eta_v * r0;
          if (G::HS) sl[N * NS + k * NS + q] += eta_v * r1;
        }
      }
    }
    __syncthreads();
  }
  for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) hb[nsteps * hs + i] = sx[i]; }
  // ---- reverse ----
  const double* sz = seed_z + b * n;
  for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) sax[i] = sz[i]; }
  for (int i0 = 0; i0 < m; i0 += 64) { const int i = i0 + lane; if (i < m) sal[i] = seed_lam ? seed_lam[b * m + i] : 0.0; }
  double gp[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) gp[k] = 0.0;
  __syncthreads();
  for (int s = nsteps - 1; s >= 0; --s) {
    const double* H = hb + s * hs;
    for (int i0 = 0; i0 < m; i0 += 64) { const int i = i0 + lane; if (i < m) sl[i] = H[2 * n + i]; }
    __syncthreads();
    // items 1, 2: sx = x+
    for (int j0 = 0; j0 < K; j0 += 64) {
      const bool live = j0 + lane < K;
      const int j = live ? j0 + lane : K - 1;
      double x[NS], u[NU], a[NS], e[NS], jt[NW], gs[NP];
#pragma unroll
      for (int q = 0; q < NS; ++q) x[q] = sx[j * NS + q];
#pragma unroll
      for (int c = 0; c < NU; ++c) u[c] = sx[K * NS + j * NU + c];
      G::combine(sal, N, j, h, a, e);
      G::back_constraint(x, u, p, a, e, G::time_of(j, h), jt, gs);
#pragma unroll
      for (int k = 0; k < NP; ++k) gp[k] += live ? eta_v * gs[k] : 0.0;
#pragma unroll
      for (int r = 0; r < NW; ++r) {
        const int i = r < NS ? j * NS + r : K * NS + j * NU + (r - NS);
        const double ax = sax[i] + eta_v * jt[r];
        const double m2 = G::inside(sx[i], lo[i], hi[i]) ? ax : 0.0;
        if (live) { sax[i] = m2; sd[i] = -eta_x * m2; }
      }
    }
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) sx[i] = H[n + i]; }
    __syncthreads();
    // items 3, 4 (sx = x_bar, whose place the new direction s takes), then item 5 (sx = x)
    for (int item = 3; item <= 5; item += 2) {
      for (int j0 = 0; j0 < K; j0 += 64) {
        const bool live = j0 + lane < K;
        const int j = live ? j0 + lane : K - 1;
        double x[NS], u[NU], mu[NS], e[NS], d[NW], hd[NW], w[NS], gs[NP];
#pragma unroll
        for (int q = 0; q < NS; ++q) { x[q] = sx[j * NS + q]; d[q] = sd[j * NS + q]; }
#pragma unroll
        for (int c = 0; c < NU; ++c) { u[c] = sx[K * NS + j * NU + c]; d[NS + c] = sd[K * NS + j * NU + c]; }
        G::combine(sl, N, j, h, mu, e);
        G::back_grad(x, u, p, mu, G::wq(K, j, h), j == K - 1, G::time_of(j, h), d, hd, w, gs);
#pragma unroll
        for (int k = 0; k < NP; ++k) gp[k] += live ? gs[k] : 0.0;
#pragma unroll
        for (int q = 0; q < NS; ++q) if (live) sdf[j * NS + q] = w[q];
#pragma unroll
        for (int r = 0; r < NW; ++r) {
          const int i = r < NS ? j * NS + r : K * NS + j * NU + (r - NS);
          if (item == 3) {
            const double m1 = G::inside(sx[i], lo[i], hi[i]) ? hd[r] : 0.0;
            if (live) { sax[i] += m1; sx[i] = -eta_x * m1; }
          } else {
            if (live) sax[i] += hd[r];
          }
        }
      }
      __syncthreads();
      for (int k0 = 0; k0 < N; k0 += 64) {
        const bool live = k0 + lane < N;
        const int k = live ? k0 + lane : N - 1;
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          double r0, r1;
          G::jd_rows(sd, sdf, k, q, h, r0, r1);
          if (live) {
            sal[k * NS + q] += r0;
            if (G::HS) sal[N * NS + k * NS + q] += r1;
          }
        }
      }
      __syncthreads();
      if (item == 3) {
        double* t = sd; sd = sx; sx = t;
        for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) sx[i] = H[i]; }
        __syncthreads();
      }
    }
  }
  if (dz0) for (int i0 = 0; i0 < n; i0 += 64) { const int i = i0 + lane; if (i < n) dz0[b * n + i] = sax[i]; }
  if (dlam0) for (int i0 = 0; i0 < m; i0 += 64) { const int i = i0 + lane; if (i < m) dlam0[b * m + i] = sal[i]; }
#pragma unroll
  for (int k = 0; k < NP; ++k) grad[b * NP + k] = wv_sum(gp[k]);      // (the same bits in every lane: every lane stores)
}

template <class Sys, int SCHEME>
inline size_t colloc_exgd_grad_lds_bytes(int N) {
  using G = ExgdGradPoint<Sys, SCHEME>;
  const int K = G::points(N), n = K * Sys::NW, m = G::rows(N);
  return (size_t)(3 * n + 2 * m + K * Sys::NS) * 8 + 16;
}
#endif  // __HIPCC__

}  // namespace myriad
