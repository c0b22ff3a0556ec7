// shoot_hvp.h -- Lagrangian Hessian-vector product of the shooting transcription (K11 in DESIGN.md; C-ABI myr_hvp).
// With L(z, lam, p) = f(z, p) + lam^T c(z, p) and a direction v, psi = <grad_z L, v>:
//   out_z = grad_z psi = grad^2_zz L v,      out_p = grad_p psi = (d^2 L / dp dz) v.
// The intervals of a multiple-shooting problem are independent given z: interval k rolls out from its own node x_k under its own control rows, and
// -lam_k^T x_{k+1} is linear.  One (instance, interval) pair is one unit of work (one lane on the device).  Per pair, forward over reverse:
//   forward  the steps of ShootCore::step_val / rk4_val (os_solver.h) with the tangent (xd, ud) of v rolled along; x_j, xd_j kept at the step boundaries;
//   reverse  from a = lam_k (+ the gradient of the terminal cost behind the last interval: the cost is linear in (x, u), the integrated end state is not
//            linear in z), ad = 0.  Per step the stage points and their tangents are recomputed and the cotangent pair goes through the stages.  For a
//            stage k_s = f(X, U, p) with tangent (Xd, Ud), cotangent kap on k_s, its tangent kapd and cost weight om (with_cost x the rule's weight x h):
//              first order    Xbar  = A^T kap + om g_x
//              second order   (Xdbar, Udbar) = (A^T kapd, B^T kapd) + Sys::hessian(X, U, p, D2, mu = kap, w = om) (Xd, Ud)
//              parameters     gp += SysDp::vjp_p(X, U, p, kapd) + SysDpw::vjp_p_dir(X, U, p, kap, om, (Xd, Ud))
//            and the rule's linear combinations carry (Xbar, Xdbar) to the stage before and to (a, ad).  At the interval's start out_z[x_k] = ad; the
//            step's control rows receive Udbar.
// Every rule is X_0 = x, X_{s+1} = x + a_{s+1} h k_s, x+ = x + h sum_s b_s k_s, cost h sum_s b_s g(X_s, U_s, t0 + c_s h):
//   Euler     1 stage,  b = {1}
//   Heun      2 stages, a = {0, 1}, b = {1/2, 1/2}, c = {0, 1},   controls u_i, u_{i+1}
//   midpoint  2 stages, a = {0, 1}, b = {0, 1},     c = {0, 1/2}, controls u_i, (u_i + u_{i+1}) / 2     (the reference's rule: a full Euler predictor)
//   RK4       4 stages, a = {0, 1/2, 1/2, 1}, b = {1/6, 1/3, 1/3, 1/6}, c = a, controls u_{2i}, u_{2i+1}, u_{2i+1}, u_{2i+2}
// A control row two steps share gets its two contributions in a fixed order (the later step's, carried in registers, is added to the earlier step's);
// a row two INTERVALS share and the I partial parameter rows of an instance meet in a second pass (gather_z / gather_p), again in a fixed order.
// No atomics anywhere.  ShootHvp is host/device shared: shoot_hvp_kernel and tests/hostsim/hvp_twin.cpp run the same text.
#pragma once
#include "systems_gen.h"
#include "systems_dp_gen.h"
#include "systems_dpw_gen.h"

namespace myriad {

template <class Sys, int M>      // M control rows per step (2: RK4, 1: the other rules), as in shoot_eval_kernel
struct ShootHvp {
  static constexpr int NS = Sys::NS, NU = Sys::NU, NW = Sys::NW, NP = Sys::NP;
  static constexpr int NR = M + 1;                      // control rows a step reads
  static constexpr int MAXST = M == 2 ? 4 : 2;

  MYR_HD static inline int nstages(int method) { return M == 2 ? 4 : (method == 0 ? 1 : 2); }
  MYR_HD static inline double ca(int, int s) { return M == 2 ? (s == 0 ? 0.0 : (s == 3 ? 1.0 : 0.5)) : (s == 0 ? 0.0 : 1.0); }
  MYR_HD static inline double cb(int method, int s) {
    if (M == 2) return (s == 0 || s == 3) ? 1.0 / 6.0 : 2.0 / 6.0;
    return method == 0 ? 1.0 : (method == 2 ? (s == 0 ? 0.0 : 1.0) : 0.5);
  }
  MYR_HD static inline double cc(int method, int s) { return (M == 1 && method == 2 && s == 1) ? 0.5 : ca(method, s); }
  // weight of control row r of the step in the control of stage s
  MYR_HD static inline double cu(int method, int s, int r) {
    if (M == 2) return r == (s == 0 ? 0 : (s == 3 ? 2 : 1)) ? 1.0 : 0.0;
    if (s == 0) return r == 0 ? 1.0 : 0.0;
    return method == 2 ? 0.5 : (r == 1 ? 1.0 : 0.0);
  }
  // doubles per pair of: the history (x_j, xd_j at the start of every step), the control side buffer, the whole side record (node | controls | parameters)
  MYR_HD static inline long hist_doubles(int cpi) { return (long)cpi * 2 * NS; }
  MYR_HD static inline long ctrl_doubles(int cpi) { return (long)(M * cpi + 1) * NU; }
  MYR_HD static inline long side_doubles(int cpi) { return NS + ctrl_doubles(cpi) + NP; }

  // stage point s of a step and its tangent: X = x + a_s h k, U = sum_r cu(s, r) uc[r]; d[NW] = (Xd, Ud)
  MYR_HD static inline void stage_point(int method, int s, double h, const double* x, const double* xd, const double* k, const double* kd,
                                        const double* uc, const double* ud, double* X, double* U, double* d) {
    const double ah = ca(method, s) * h;
#pragma unroll
    for (int q = 0; q < NS; ++q) { X[q] = x[q] + ah * k[q]; d[q] = xd[q] + ah * kd[q]; }
#pragma unroll
    for (int c = 0; c < NU; ++c) {
      double su = 0.0, sd = 0.0;
#pragma unroll
      for (int r = 0; r < NR; ++r) { const double w = cu(method, s, r); su += w * uc[r * NU + c]; sd += w * ud[r * NU + c]; }
      U[c] = su; d[NS + c] = sd;
    }
  }

  // k = f(X, U, p) and its tangent kd = A Xd + B Ud
  MYR_HD static inline void stage_tangent(const double* X, const double* U, const double* p, const double* d, double* k, double* kd) {
    double A[NS * NS], Bm[NS * NU], g, gw[NW];
    Sys::lin(X, U, p, k, A, Bm, &g, gw);
#pragma unroll
    for (int r = 0; r < NS; ++r) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < NS; ++q) s += A[r * NS + q] * d[q];
#pragma unroll
      for (int c = 0; c < NU; ++c) s += Bm[r * NU + c] * d[NS + c];
      kd[r] = s;
    }
  }

  // THE STAGE RULE: cotangent kap[NS] on k_s = f(X, U, p), its tangent kapd[NS], cost weight om, tangent d[NW] of the stage point, time t.
  // xbar[NS] = A^T kap + om g_x;  dbar[NW] = [A B]^T kapd + hessian(mu = kap, w = om) d;  gp[NP] += vjp_p(kapd) + vjp_p_dir(kap, om, d)
  MYR_HD static inline void stage_rule(const double* X, const double* U, const double* p, double t, const double* d, const double* kap,
                                       const double* kapd, double om, double* xbar, double* dbar, double* gp) {
    double f[NS], A[NS * NS], Bm[NS * NU], g, gw[NW], D2[Sys::NNZ2], W[NW * NW], g1[NP], g2[NP];
    set_time<Sys>(p, t);
    Sys::lin_d2(X, U, p, f, A, Bm, &g, gw, D2);
    Sys::hessian(X, U, p, D2, kap, om, W);
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      double s = om * gw[q];
#pragma unroll
      for (int r = 0; r < NS; ++r) s += A[r * NS + q] * kap[r];
      xbar[q] = s;
    }
#pragma unroll
    for (int c = 0; c < NW; ++c) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < NS; ++r) s += (c < NS ? A[r * NS + c] : Bm[r * NU + (c - NS)]) * kapd[r];
#pragma unroll
      for (int e = 0; e < NW; ++e) s += W[c * NW + e] * d[e];
      dbar[c] = s;
    }
    SysDp<Sys>::vjp_p(X, U, p, kapd, g1);
    SysDpw<Sys>::vjp_p_dir(X, U, p, kap, om, d, g2);
#pragma unroll
    for (int k = 0; k < NP; ++k) gp[k] += g1[k] + g2[k];
  }

  // one step forward with its tangent: (x, xd) <- (x+, xd+).  uc, ud: the step's NR control rows and their tangents
  MYR_HD static inline void step_fwd(int method, double h, const double* uc, const double* ud, const double* p, double* x, double* xd) {
    const int nst = nstages(method);
    double k[NS], kd[NS], acc[NS], accd[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) { k[q] = 0.0; kd[q] = 0.0; acc[q] = 0.0; accd[q] = 0.0; }
#pragma unroll
    for (int s = 0; s < MAXST; ++s) {
      if (s < nst) {
        double X[NS], U[NU], d[NW];
        stage_point(method, s, h, x, xd, k, kd, uc, ud, X, U, d);
        stage_tangent(X, U, p, d, k, kd);
        const double b = cb(method, s);
#pragma unroll
        for (int q = 0; q < NS; ++q) { acc[q] += b * k[q]; accd[q] += b * kd[q]; }
      }
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) { x[q] += h * acc[q]; xd[q] += h * accd[q]; }
  }

  // one step backwards.  (x, xd): the state and tangent at the START of the step, t0 its time; (a, ad): cotangent of x+ and its tangent, replaced by
  // those of x; ub[NR NU] += the second-order cotangent of the step's control rows; gp[NP] += the step's share of out_p; cw: with_cost as 1.0 / 0.0
  MYR_HD static inline void step_back(int method, double h, double t0, const double* x, const double* xd, const double* uc, const double* ud,
                                      const double* p, double cw, double* a, double* ad, double* ub, double* gp) {
    const int nst = nstages(method);
    double X[MAXST][NS], U[MAXST][NU], D[MAXST][NW];
    {
      double k[NS], kd[NS];
#pragma unroll
      for (int q = 0; q < NS; ++q) { k[q] = 0.0; kd[q] = 0.0; }
#pragma unroll
      for (int s = 0; s < MAXST; ++s) {
        if (s < nst) {
          stage_point(method, s, h, x, xd, k, kd, uc, ud, X[s], U[s], D[s]);
          if (s + 1 < nst) stage_tangent(X[s], U[s], p, D[s], k, kd);
        }
      }
    }
    double xb[NS], db[NW], sa[NS], sad[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) { xb[q] = 0.0; sa[q] = a[q]; sad[q] = ad[q]; }
#pragma unroll
    for (int c = 0; c < NW; ++c) db[c] = 0.0;
#pragma unroll
    for (int s = MAXST - 1; s >= 0; --s) {
      if (s < nst) {
        const double hb = h * cb(method, s);
        const double hn = s + 1 < nst ? h * ca(method, s + 1) : 0.0;      // what stage s + 1 hands back: X_{s+1} = x + a_{s+1} h k_s
        double kap[NS], kapd[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) { kap[q] = hb * a[q] + hn * xb[q]; kapd[q] = hb * ad[q] + hn * db[q]; }
        stage_rule(X[s], U[s], p, t0 + cc(method, s) * h, D[s], kap, kapd, cw * hb, xb, db, gp);
#pragma unroll
        for (int q = 0; q < NS; ++q) { sa[q] += xb[q]; sad[q] += db[q]; }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const double w = cu(method, s, r);
#pragma unroll
          for (int c = 0; c < NU; ++c) ub[r * NU + c] += w * db[NS + c];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) { a[q] = sa[q]; ad[q] = sad[q]; }
  }

  // One (instance, interval) pair.  zb, vb: the instance's z and v ([I+1][NS] nodes, then [M S + 1][NU] control rows); lk: lam_k [NS] or null;
  // hist: hist_doubles(cpi) doubles and side: side_doubles(cpi) doubles of this pair, consecutive doubles `stride` apart (1 on the host, the padded
  // number of pairs on the device: batch-minor).  side = ad at the node [NS] | second-order cotangent of the interval's M cpi + 1 control rows | gp [NP]
  // SEEDED (shoot_exgd_grad.h; myr_hvp runs SEEDED = false, where al and scale are not read): al [NS], `stride` apart, gets the pair's rows of J v,
  // xd_end - v_{x_{k+1}}, added, and the reverse starts from ad = alpha = scale al instead of 0: it is linear in ad, so side then holds
  // H v + (d x_end / d (x_k, u))^T alpha and gp gains (dc_k/dp)^T alpha
  template <bool SEEDED = false>
  MYR_HD static inline void interval(int method, int I, int cpi, int k, double T, const double* zb, const double* vb, const double* lk,
                                     const double* p, int with_cost, double* hist, double* side, long stride, double* al = nullptr,
                                     double scale = 0.0) {
    const int S = I * cpi;
    const double h = T / S, cw = with_cost ? 1.0 : 0.0;
    const double* zu = zb + (long)(I + 1) * NS;
    const double* vu = vb + (long)(I + 1) * NS;
    double x[NS], xd[NS], gp[NP];
#pragma unroll
    for (int q = 0; q < NS; ++q) { x[q] = zb[(long)k * NS + q]; xd[q] = vb[(long)k * NS + q]; }
#pragma unroll
    for (int e = 0; e < NP; ++e) gp[e] = 0.0;
    for (int j = 0; j < cpi; ++j) {
      const long i = (long)k * cpi + j;
#pragma unroll
      for (int q = 0; q < NS; ++q) { hist[((long)j * 2 * NS + q) * stride] = x[q]; hist[((long)j * 2 * NS + NS + q) * stride] = xd[q]; }
      step_fwd(method, h, zu + M * i * NU, vu + M * i * NU, p, x, xd);
    }
    double a[NS], ad[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) { a[q] = lk ? lk[q] : 0.0; ad[q] = 0.0; }
    if constexpr (SEEDED) {
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        const double al_q = al[(long)q * stride] + (xd[q] - vb[(long)(k + 1) * NS + q]);
        al[(long)q * stride] = al_q;
        ad[q] = scale * al_q;
      }
    }
    if constexpr (Sys::HAS_TERMINAL) {
      // the terminal cost sits on the INTEGRATED end state of the last interval and the last control row: its (constant) gradient joins the costate,
      // and its p-derivative along the end state's tangent goes to out_p
      if (with_cost && k == I - 1) {
        const double* ul = zu + (long)M * S * NU;
        double tg[NW], d[NW], gt[NP];
        Sys::term_grad(x, ul, p, tg);
#pragma unroll
        for (int q = 0; q < NS; ++q) { a[q] += tg[q]; d[q] = xd[q]; }
#pragma unroll
        for (int c = 0; c < NU; ++c) d[NS + c] = vu[(long)M * S * NU + c];
        SysDpw<Sys>::term_vjp_p_dir(x, ul, p, d, gt);
#pragma unroll
        for (int e = 0; e < NP; ++e) gp[e] += gt[e];
      }
    }
    double* su = side + (long)NS * stride;
    double carry[NU];      // what the step behind has for the row it shares with this one
#pragma unroll
    for (int c = 0; c < NU; ++c) carry[c] = 0.0;
    for (int j = cpi - 1; j >= 0; --j) {
      const long i = (long)k * cpi + j;
      double ub[NR * NU];
#pragma unroll
      for (int q = 0; q < NS; ++q) { x[q] = hist[((long)j * 2 * NS + q) * stride]; xd[q] = hist[((long)j * 2 * NS + NS + q) * stride]; }
#pragma unroll
      for (int c = 0; c < NR * NU; ++c) ub[c] = 0.0;
      step_back(method, h, h * i, x, xd, zu + M * i * NU, vu + M * i * NU, p, cw, a, ad, ub, gp);
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        su[((long)(M * j + M) * NU + c) * stride] = ub[M * NU + c] + carry[c];
        if (M == 2) su[((long)(M * j + 1) * NU + c) * stride] = ub[NU + c];
        carry[c] = ub[c];
      }
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) su[(long)c * stride] = carry[c];
#pragma unroll
    for (int q = 0; q < NS; ++q) side[(long)q * stride] = ad[q];
    double* sp = su + ctrl_doubles(cpi) * stride;
#pragma unroll
    for (int e = 0; e < NP; ++e) sp[(long)e * stride] = gp[e];
  }

  // entry i of an instance's out_z from the side records of its I pairs (side0: the record of the instance's first pair): a node entry is its own
  // interval's (zero for the last node: -lam^T x_{k+1} is linear); a control row two intervals share is (the earlier interval's) + (the later one's)
  MYR_HD static inline double gather_z(int I, int cpi, long i, const double* side0, long stride) {
    const long nx = (long)(I + 1) * NS;
    if (i < nx) {
      const long k = i / NS;
      return k < I ? side0[k + (i - k * NS) * stride] : 0.0;
    }
    const long r = (i - nx) / NU, c = (i - nx) - r * NU, W = (long)M * cpi;
    long k = r / W;
    if (k > I - 1) k = I - 1;
    const long l = r - k * W;
    const double own = side0[k + (NS + l * NU + c) * stride];
    if (l == 0 && k > 0) return side0[k - 1 + (NS + W * NU + c) * stride] + own;
    return own;
  }
  // entry e of an instance's out_p row: the I partial rows in ascending order
  MYR_HD static inline double gather_p(int I, int cpi, int e, const double* side0, long stride) {
    double s = 0.0;
    for (int k = 0; k < I; ++k) s += side0[k + (NS + ctrl_doubles(cpi) + e) * stride];
    return s;
  }
};

// One instance on the host, the sequence of the two kernels as plain loops.  p: the instance's parameter buffer (SysParams::get()); work:
// I (hist_doubles + side_doubles) doubles; lam, oz, op may be null
template <class Sys, int M>
inline void shoot_hvp_host(int method, int I, int cpi, double T, const double* z, const double* lam, const double* v, const double* p, int with_cost,
                           double* work, double* oz, double* op) {
  using H = ShootHvp<Sys, M>;
  const long n = (long)(I + 1) * Sys::NS + ((long)M * I * cpi + 1) * Sys::NU;
  double* hist = work;                                   // [hist_doubles][I]
  double* side = work + H::hist_doubles(cpi) * I;        // [side_doubles][I]: pair-minor, as on the device
  for (int k = 0; k < I; ++k) H::interval(method, I, cpi, k, T, z, v, lam ? lam + (long)k * Sys::NS : nullptr, p, with_cost, hist + k, side + k, I);
  if (oz) for (long i = 0; i < n; ++i) oz[i] = H::gather_z(I, cpi, i, side, I);
  if (op) for (int e = 0; e < Sys::NP; ++e) op[e] = H::gather_p(I, cpi, e, side, I);
}

#if defined(__HIPCC__)
// One (instance, interval) pair per lane: pair q = b I + k.  hist [hist_doubles][Pp], side [side_doubles][Pp], Pp >= the lanes of the grid: every lane
// has a column of its own, so the idle lanes of the last wavefront redo the last pair into columns nobody reads and no store needs a mask.  Every loop
// has a wave-uniform trip count (cpi, the stages of the method); no lane-0 block, no atomics.
template <class Sys, int M>
__global__ __launch_bounds__(64)
void shoot_hvp_kernel(int B, long Pp, int I, int cpi, int method, double T, const double* __restrict__ z, const double* __restrict__ lam,
                      const double* __restrict__ v, const double* __restrict__ params, int params_stride, int with_cost,
                      double* __restrict__ hist, double* __restrict__ side) {
  using H = ShootHvp<Sys, M>;
  const long lane = (long)blockIdx.x * blockDim.x + threadIdx.x;      // < Pp
  const long P = (long)B * I;
  const long q = lane < P ? lane : P - 1;
  const long b = q / I;
  const int k = (int)(q - b * I);
  const long n = (long)(I + 1) * Sys::NS + ((long)M * I * cpi + 1) * Sys::NU;
  SysParams<Sys> pp;
  pp.load(params, b, params_stride);
  H::interval(method, I, cpi, k, T, z + b * n, v + b * n, lam ? lam + b * (long)I * Sys::NS + (long)k * Sys::NS : nullptr, pp.get(), with_cost,
              hist + lane, side + lane, Pp);
}

// second pass: out_z [B][n] and the parameter rows [B][NP] from the side records (either may be null); one thread per entry, grid-stride
template <class Sys, int M>
__global__ __launch_bounds__(256)
void shoot_hvp_gather_kernel(int B, long Pp, int I, int cpi, const double* __restrict__ side, double* __restrict__ out_z, double* __restrict__ rows) {
  using H = ShootHvp<Sys, M>;
  const long n = (long)(I + 1) * Sys::NS + ((long)M * I * cpi + 1) * Sys::NU;
  const long nz = out_z ? (long)B * n : 0, np = rows ? (long)B * Sys::NP : 0;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < nz + np; t += (long)gridDim.x * blockDim.x) {
    if (t < nz) {
      const long b = t / n;
      out_z[t] = H::gather_z(I, cpi, t - b * n, side + b * I, Pp);
    } else {
      const long u = t - nz, b = u / Sys::NP;
      rows[u] = H::gather_p(I, cpi, (int)(u - b * Sys::NP), side + b * I, Pp);
    }
  }
}
#endif  // __HIPCC__

}  // namespace myriad
