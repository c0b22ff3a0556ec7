// shoot_exgd_grad.h -- derivative of `nsteps` unrolled extragradient steps in the model parameters under the SHOOTING transcription (K13 in DESIGN.md;
// C-ABI myr_exgd_grad_shoot).  The five items of exgd_grad.h (K10) over the shooting Lagrangian L = f + lam^T c, c_k = x_end(x_k, u) - x_{k+1}:
//   1. a_x += eta_v J(x+)^T a_lam            gp += eta_v (dc/dp)(x+)^T a_lam
//   2. m2 = inside(x+) o a_x                 a_x = m2          t = -eta_x m2
//   3. r = H(x_bar, lam) t                   a_lam += J(x_bar) t                       gp += (dg/dp)(x_bar, lam)^T t
//   4. m1 = inside(x_bar) o r                a_x += m1         d = -eta_x m1
//   5. a_x += H(x, lam) d                    a_lam += J(x) d                           gp += (dg/dp)(x, lam)^T d
// H v is ShootHvp's second-order reverse per (instance, interval) pair.  That reverse is linear in the costate's tangent, so ONE pair pass over
// (z, lam, v, alpha) -- ShootHvp::interval<true>: the reverse started from ad = alpha_k instead of 0 -- returns
//   in z   H v + J^T alpha      (the linear term -alpha_{k-1}^T x_k of the constraints joins in the gather: out_z)
//   in p   (dg/dp)^T v + (dc/dp)^T alpha
// and its forward half has pair k's rows of J v, xd_end - v_{x_{k+1}}, which it adds to a_lam,k.  Item 5 of step s and item 1 of step s - 1 stand at
// the same point x_s: after the forward half the lane holds the completed a_lam,k and seeds alpha_k = eta_v a_lam,k in the same pass.  A call is
// 2 nsteps + 1 pair passes:
//   at x_n            v = 0, alpha = eta_v seed_lam                          then MASK_STEP  (items 1, 2 of step n - 1)
//   at x_bar_s        v = t, alpha = 0                                       then MASK_BAR   (items 3, 4)
//   at x_s            v = d, alpha = eta_v a_lam (0 at s = 0)                then MASK_STEP  (items 5, 1, 2), MASK_LAST at s = 0 (item 5)
// each followed by one elementwise pass over [n] that gathers out_z, applies the mask, writes the next direction and adds the pass's I partial
// parameter rows to the instance's running row in ascending k.  a_lam lives in a column per pair ([NS][Pp], like ShootHvp's side records): the idle
// lanes of the last wavefront update columns of their own.  No atomics.  ShootExgdGrad is host/device shared: the kernels below and
// tests/hostsim/shoot_exgd_grad_twin.cpp run the same text.
//
// History of a chunk of nb instances (doubles): per step s the blocks x_s [nb][n], x_bar_s [nb][n], lam_s [nb][m]; behind the last step x_n [nb][n].
#pragma once
#include "shoot_hvp.h"
#include "os_solver.h"

namespace myriad {

enum { SHOOT_MASK_STEP = 0, SHOOT_MASK_BAR = 1, SHOOT_MASK_LAST = 2 };

template <class Sys, int M>
struct ShootExgdGrad {
  using H = ShootHvp<Sys, M>;
  static constexpr int NS = Sys::NS, NU = Sys::NU, NP = Sys::NP;
  MYR_HD static inline long nvars(int I, int cpi) { return (long)(I + 1) * NS + ((long)M * I * cpi + 1) * NU; }
  MYR_HD static inline long step_doubles(int I, int cpi) { return 2 * nvars(I, cpi) + (long)I * NS; }      // of one instance: x_s, x_bar_s, lam_s
  MYR_HD static inline long hist_doubles(int I, int cpi, int nsteps) { return (long)nsteps * step_doubles(I, cpi) + nvars(I, cpi); }
  MYR_HD static inline bool inside(double v, double lo, double hi) { return v > lo && v < hi; }

  // entry i of an instance's out_z of a seeded pass: ShootHvp::gather_z plus the linear term's share -alpha_{k-1} on node k.  al0: the a_lam column
  // of the instance's first pair (as the pass left it), scale: alpha = scale a_lam
  MYR_HD static inline double out_z(int I, int cpi, long i, const double* side0, const double* al0, double scale, long stride) {
    double v = H::gather_z(I, cpi, i, side0, stride);
    if (scale != 0.0 && i >= NS && i < (long)(I + 1) * NS) {
      const long k = i / NS;
      v -= scale * al0[k - 1 + (i - k * NS) * stride];
    }
    return v;
  }

  // the mask behind a pass (items 2 and 4; MASK_LAST: the end of item 5 at s = 0).  oz: the pass's out_z entry, pt: the point it stood at
  MYR_HD static inline void mask(int mode, double oz, double pt, double lo, double hi, double eta_x, double& ax, double& dir) {
    if (mode == SHOOT_MASK_LAST) { ax += oz; dir = 0.0; return; }
    const double c = mode == SHOOT_MASK_BAR ? oz : ax + oz;
    const double mk = inside(pt, lo, hi) ? c : 0.0;
    ax = mode == SHOOT_MASK_BAR ? ax + mk : mk;
    dir = -eta_x * mk;
  }

  // entry e of the instance's running parameter row behind a pass: the I partial rows in ascending order
  MYR_HD static inline double add_rows(int I, int cpi, int e, const double* side0, long stride, double row) {
    for (int k = 0; k < I; ++k) row += side0[k + (NS + H::ctrl_doubles(cpi) + e) * stride];
    return row;
  }

  // The schedule of the reverse sweep, for the kernels, the launcher and the host twins of K13 and K15 alike.  A pass stands at x_s (x_n for
  // s = nsteps) or, with at_bar, at x_bar_s; `alone` marks items 1, 2 as a pass of their own: on the zero direction and without multipliers
  // (alpha = scale a_lam is all that drives it); every other pass takes lam_s and the direction the mask before it wrote.
  struct Pass { int s, at_bar, alone, mode; double scale; };
  // the fused order: pass 0 at x_n, then per step s = nsteps - 1 ... 0 one pass at x_bar_s and one at x_s (item 5 of step s with item 1 of s - 1)
  MYR_HD static inline int passes(int nsteps) { return nsteps > 0 ? 2 * nsteps + 1 : 0; }
  MYR_HD static inline Pass pass_of(int ps, int nsteps, double eta_v) {
    Pass q;
    q.alone = ps == 0;
    if (ps == 0) { q.s = nsteps; q.at_bar = 0; q.mode = SHOOT_MASK_STEP; q.scale = eta_v; return q; }
    q.s = nsteps - 1 - (ps - 1) / 2;
    q.at_bar = (ps & 1);
    if (q.at_bar) { q.mode = SHOOT_MASK_BAR; q.scale = 0.0; }
    else { q.mode = q.s > 0 ? SHOOT_MASK_STEP : SHOOT_MASK_LAST; q.scale = q.s > 0 ? eta_v : 0.0; }
    return q;
  }
  // the unfused order of exgd_grad.h, three passes a step: items 1, 2 alone at x_{s+1}, then x_bar_s, then x_s (the host twins' test of the fusion)
  MYR_HD static inline int passes_unfused(int nsteps) { return 3 * nsteps; }
  MYR_HD static inline Pass pass_of_unfused(int ps, int nsteps, double eta_v) {
    const int s = nsteps - 1 - ps / 3, r = ps % 3;
    Pass q;
    q.alone = r == 0;
    q.s = r == 0 ? s + 1 : s;
    q.at_bar = r == 1;
    q.mode = r == 0 ? SHOOT_MASK_STEP : (r == 1 ? SHOOT_MASK_BAR : SHOOT_MASK_LAST);
    q.scale = r == 0 ? eta_v : 0.0;
    return q;
  }
};

// ---- one instance on the host: the forward steps (the arithmetic of shoot_eval_kernel + exgd_update_kernel + axpy_kernel) and the passes as loops ----
// g[n] = grad_z (f + lam^T c), c[I NS] (either may be null); xs: (cpi + 1) NS doubles
template <class Sys, int M>
inline void shoot_lagrangian_host(int method, int I, int cpi, double T, const double* zb, const double* lam, const double* p, double* xs, double* g,
                                  double* c) {
  using SC = ShootCore<Sys, M>;
  constexpr int NS = Sys::NS, NU = Sys::NU, NY = SC::NY;
  const int S = I * cpi;
  const long n = ShootExgdGrad<Sys, M>::nvars(I, cpi);
  const double h = T / S;
  const double* ub = zb + (long)(I + 1) * NS;
  if (g) for (long i = 0; i < n; ++i) g[i] = 0.0;
  for (int k = 0; k < I; ++k) {
    double x[NS];
    for (int q = 0; q < NS; ++q) x[q] = zb[(long)k * NS + q];
    for (int j = 0; j < cpi; ++j) {
      const int i = k * cpi + j;
      double xn[NS], dc;
      for (int q = 0; q < NS; ++q) xs[(long)j * NS + q] = x[q];
      SC::sval(method, h, x, ub + (long)M * i * NU, p, xn, dc, h * i, i == S - 1);
      for (int q = 0; q < NS; ++q) x[q] = xn[q];
    }
    if (c) for (int q = 0; q < NS; ++q) c[(long)k * NS + q] = x[q] - zb[(long)(k + 1) * NS + q];
    if (!g) continue;
    double a[NS];
    for (int q = 0; q < NS; ++q) { a[q] = lam[(long)k * NS + q]; g[(long)(k + 1) * NS + q] -= a[q]; }
    const double zero[NS] = {0};
    for (int j = cpi - 1; j >= 0; --j) {
      const int i = k * cpi + j;
      double xi[NS], Fy[NS * NY], gy[NY], Hs[NY * NY], na[NS];
      for (int q = 0; q < NS; ++q) xi[q] = xs[(long)j * NS + q];
      SC::slin(method, h, xi, ub + (long)M * i * NU, p, zero, Fy, gy, Hs, h * i, i == S - 1);
      for (int col = NS; col < NY; ++col) {
        double s = gy[col];
        for (int t = 0; t < NS; ++t) s += a[t] * Fy[t * NY + col];
        g[(long)(I + 1) * NS + (long)M * i * NU + (col - NS)] += s;
      }
      for (int q = 0; q < NS; ++q) {
        double s = gy[q];
        for (int t = 0; t < NS; ++t) s += a[t] * Fy[t * NY + q];
        na[q] = s;
      }
      for (int q = 0; q < NS; ++q) a[q] = na[q];
    }
    for (int q = 0; q < NS; ++q) g[(long)k * NS + q] += a[q];
  }
}

// p: the instance's parameter buffer (SysParams::get()); hist: hist_doubles(I, cpi, nsteps) doubles; work: 5 n + 2 m + (cpi + 1) NS + I (NS +
// ShootHvp::hist_doubles + side_doubles) doubles; seed_lam, dz0, dlam0 may be null; gp[NP].  fused == false runs items 1 .. 5 as THREE passes a step
// (item 1 as a pass of its own at x+ with v = 0: ShootExgdGrad::pass_of_unfused), the order of exgd_grad.h, for the test of the fusion.
template <class Sys, int M>
inline void shoot_exgd_grad_host(int method, int I, int cpi, double T, const double* z, const double* lam, const double* lb, const double* ub,
                                 const double* p, double eta_x, double eta_v, int nsteps, const double* seed_z, const double* seed_lam, double* hist,
                                 double* work, double* gp, double* dz0, double* dlam0, bool fused = true) {
  using G = ShootExgdGrad<Sys, M>;
  using H = ShootHvp<Sys, M>;
  constexpr int NS = Sys::NS, NP = Sys::NP;
  const long n = G::nvars(I, cpi), m = (long)I * NS, hs = G::step_doubles(I, cpi);
  double* zx = work;             // the iterate, then the zero direction of the first pass
  double* zbar = zx + n;
  double* g = zbar + n;
  double* ax = g + n;
  double* dir = ax + n;
  double* lm = dir + n;          // the multipliers of the forward steps
  double* c = lm + m;
  double* xs = c + m;
  double* al = xs + (long)(cpi + 1) * NS;                      // [NS][I]: pair-minor, as on the device
  double* phist = al + (long)NS * I;                           // [hist_doubles][I]
  double* side = phist + H::hist_doubles(cpi) * I;             // [side_doubles][I]
  auto clip = [](double v, double l, double u) { return v < l ? l : (v > u ? u : v); };
  // ---- forward ----
  for (long i = 0; i < n; ++i) zx[i] = z[i];
  for (long i = 0; i < m; ++i) lm[i] = lam[i];
  for (int s = 0; s < nsteps; ++s) {
    double* Hh = hist + s * hs;
    for (long i = 0; i < n; ++i) Hh[i] = zx[i];
    for (long i = 0; i < m; ++i) Hh[2 * n + i] = lm[i];
    shoot_lagrangian_host<Sys, M>(method, I, cpi, T, zx, lm, p, xs, g, nullptr);
    for (long i = 0; i < n; ++i) { zbar[i] = clip(zx[i] - eta_x * g[i], lb[i], ub[i]); Hh[n + i] = zbar[i]; }
    shoot_lagrangian_host<Sys, M>(method, I, cpi, T, zbar, lm, p, xs, g, nullptr);
    for (long i = 0; i < n; ++i) zx[i] = clip(zx[i] - eta_x * g[i], lb[i], ub[i]);
    shoot_lagrangian_host<Sys, M>(method, I, cpi, T, zx, nullptr, p, xs, nullptr, c);
    for (long i = 0; i < m; ++i) lm[i] += eta_v * c[i];
  }
  for (long i = 0; i < n; ++i) hist[nsteps * hs + i] = zx[i];
  // ---- reverse ----
  for (long i = 0; i < n; ++i) ax[i] = seed_z[i];
  for (int k = 0; k < I; ++k)
    for (int q = 0; q < NS; ++q) al[k + (long)q * I] = seed_lam ? seed_lam[(long)k * NS + q] : 0.0;
  for (int e = 0; e < NP; ++e) gp[e] = 0.0;
  auto pass = [&](const double* pt, const double* lk, const double* v, double scale, int mode) {
    for (int k = 0; k < I; ++k)
      H::template interval<true>(method, I, cpi, k, T, pt, v, lk ? lk + (long)k * NS : nullptr, p, 1, phist + k, side + k, I, al + k, scale);
    for (long i = 0; i < n; ++i) G::mask(mode, G::out_z(I, cpi, i, side, al, scale, I), pt[i], lb[i], ub[i], eta_x, ax[i], dir[i]);
    for (int e = 0; e < NP; ++e) gp[e] = G::add_rows(I, cpi, e, side, I, gp[e]);
  };
  for (long i = 0; i < n; ++i) zx[i] = 0.0;
  for (int ps = 0; ps < (fused ? G::passes(nsteps) : G::passes_unfused(nsteps)); ++ps) {
    const typename G::Pass q = fused ? G::pass_of(ps, nsteps, eta_v) : G::pass_of_unfused(ps, nsteps, eta_v);
    const double* Hh = hist + q.s * hs;
    pass(q.at_bar ? Hh + n : Hh, q.alone ? nullptr : Hh + 2 * n, q.alone ? zx : dir, q.scale, q.mode);
  }
  if (dz0) for (long i = 0; i < n; ++i) dz0[i] = ax[i];
  if (dlam0)
    for (int k = 0; k < I; ++k)
      for (int q = 0; q < NS; ++q) dlam0[(long)k * NS + q] = al[k + (long)q * I];
}

#if defined(__HIPCC__)
// The seeded pair pass: one (instance, interval) pair per lane, pair q = b I + k, exactly as shoot_hvp_kernel (a column of hist, side and al per lane:
// the idle lanes of the last wavefront redo the last pair into columns nobody reads, no store is masked; wave-uniform trip counts; no lane-0 block).
// al [NS][Pp]: a_lam of the pair, in/out; alpha = scale a_lam seeds the reverse.
template <class Sys, int M>
__global__ __launch_bounds__(64)
void shoot_exgd_grad_pair_kernel(int B, long Pp, int I, int cpi, int method, double T, const double* __restrict__ z, const double* __restrict__ lam,
                                 const double* __restrict__ v, const double* __restrict__ params, int params_stride, double scale,
                                 double* __restrict__ al, double* __restrict__ hist, double* __restrict__ side) {
  using G = ShootExgdGrad<Sys, M>;
  const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;      // < Pp
  const long P = (long)B * I;
  const long q = lane < P ? lane : P - 1;
  const long b = q / I;
  const int k = (int)(q - b * I);
  const long n = G::nvars(I, cpi);
  SysParams<Sys> pp;
  pp.load(params, b, params_stride);
  ShootHvp<Sys, M>::template interval<true>(method, I, cpi, k, T, z + b * n, v + b * n, lam ? lam + b * (long)I * Sys::NS + (long)k * Sys::NS : nullptr,
                                            pp.get(), 1, hist + lane, side + lane, Pp, al + lane, scale);
}

// behind a pass: a_x, the next direction [B][n] and the running parameter rows [B][NP]; one thread per entry, grid-stride
template <class Sys, int M>
__global__ __launch_bounds__(256)
void shoot_exgd_grad_mask_kernel(int B, long Pp, int I, int cpi, int mode, double scale, double eta_x, const double* __restrict__ side,
                                 const double* __restrict__ al, const double* __restrict__ pt, const double* __restrict__ lb,
                                 const double* __restrict__ ub, double* __restrict__ ax, double* __restrict__ dir, double* __restrict__ rows) {
  using G = ShootExgdGrad<Sys, M>;
  const long n = G::nvars(I, cpi);
  const long nz = (long)B * n, np = (long)B * Sys::NP;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < nz + np; t += (long)gridDim.x * blockDim.x) {
    if (t < nz) {
      const long b = t / n;
      double a = ax[t], d;
      G::mask(mode, G::out_z(I, cpi, t - b * n, side + b * I, al + b * I, scale, Pp), pt[t], lb[t], ub[t], eta_x, a, d);
      ax[t] = a; dir[t] = d;
    } else {
      const long u = t - nz, b = u / Sys::NP;
      rows[u] = G::add_rows(I, cpi, (int)(u - b * Sys::NP), side + b * I, Pp, rows[u]);
    }
  }
}

// a_lam between the caller's [B][I NS] layout and the pair columns [NS][Pp].  to_cols: every one of the Pp columns is written (seed_lam, or 0 where it
// is null and in the columns behind the last pair), the direction [B][n] and the rows [B][np] are cleared; otherwise dlam0 is read from the columns
static __global__ __launch_bounds__(256)
void shoot_exgd_grad_lam_kernel(int to_cols, int B, long Pp, int I, int ns, long n, int np, const double* __restrict__ seed_lam, double* al,
                                double* __restrict__ dir, double* __restrict__ rows, double* __restrict__ dlam0) {
  const long P = (long)B * I, nl = to_cols ? Pp * ns : P * ns, nd = to_cols ? (long)B * n : 0, nr = to_cols ? (long)B * np : 0;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < nl + nd + nr; t += (long)gridDim.x * blockDim.x) {
    if (t < nl) {
      const long cols = to_cols ? Pp : P;
      const long q = t / cols, pr = t - q * cols;
      if (to_cols) al[q * Pp + pr] = (seed_lam && pr < P) ? seed_lam[pr * ns + q] : 0.0;
      else dlam0[pr * ns + q] = al[q * Pp + pr];
    } else if (t < nl + nd) dir[t - nl] = 0.0;
    else rows[t - nl - nd] = 0.0;
  }
}
#endif  // __HIPCC__

}  // namespace myriad
