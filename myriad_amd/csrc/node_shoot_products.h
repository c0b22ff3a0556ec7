// node_shoot_products.h -- Lagrangian products and extragradient steps of the SHOOTING transcription with the network as the dynamics
// (K14 in DESIGN.md): myr_vjp, myr_jvp and myr_exgd for MYR_SYS_NODE_CARTPOLE.
//
// Replaces, for a NodeSystem under the reference's default transcription (config.py:66), jax.grad of the Lagrangian in x, jax.jvp of the
// constraints and the extragradient iteration (nlp_solvers/extra_gradient.py:21-33, experiments/node_e2e_sysid.py:106-131) over
// shooting.py:144-167 (parametrized_objective) and :212-228 (parametrized_constraints).
//
// Unit of work: one (instance, interval) PAIR -- the intervals of a multiple-shooting problem are independent given z.  lane = pair: the 64 lanes
// of the one wavefront of a workgroup hold up to 64 pairs of DIFFERENT instances, four tiles of v_mfma_f64_16x16x4_f64 per network pass
// (node_mfma.h, unchanged: pass<0> for values, pass<1> with use_rec for F, A, B into the lane's LDS record).  Per step and stage every lane writes
// its stage point into the point list, the wavefront makes ONE pass, every lane reads its record and applies the rule's combination.  The passes
// are the wavefront's: lanes without a pair call them too and discard the result.
//
// Ownership: a workgroup owns whole instances (G of them: as many as fit in 64 lanes and in LDS when I <= 64; one, in chunks of 64 pairs, when
// I > 64), so the control rows two intervals share meet inside the workgroup and an extragradient step never leaves it.  G depends on I, cpi and
// params_stride only -- never on the batch size -- and a tile's columns are independent: an instance's bits do not depend on its neighbours.
// One weight copy per workgroup (40 KB of LDS); params_stride == np: one instance per workgroup, that instance's weights.
//
// myr_vjp: forward rollout of every pair with pass<1>; the step-start states and the stages' F, A, B go to global scratch, pair-minor (the 64
//          lanes store 64 consecutive doubles); then shoot_eval_kernel's reverse sweep per lane (ShootCore::slin read through RecEval), seeded
//          with lam_k, with no further network work.  A pair writes the rows it owns; the contribution to the control row it shares with the
//          NEXT pair goes to an LDS slot and is added by that pair's owner after a barrier: fixed order, no atomics.
// myr_jvp: the same rollout with the tangent carried through each stage's A, B as it is produced; nothing is stored.
// myr_exgd: ONE launch; the workgroup loops nsteps times over gradient at x -> x_bar -> gradient at x_bar -> x -> value rollout (pass<0>) -> lam,
//          the sequence and the rounding of shoot_exgd_steps.  z, x_bar, g, lam of the group's instances live in LDS where they fit, in the
//          handle's global scratch where not even one instance does.
// Capacity: the LDS holds I doubles of shared-row slots for an instance wider than 64 pairs; an instance of more than ~12 000 intervals is refused.
//
// The pair algebra (NodeShootProd) is host/device shared: the device evaluates the network through NspDevNet (the passes), the host twin
// (tests/hostsim/node_shoot_products_twin.cpp) through NspHostNet (SysNODE::lin / f in plain loops), and both run the same text.
#pragma once
#include "os_solver.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "node_mfma.h"
#endif

namespace myriad {

template <class Sys, int M>
struct NodeShootProd {
  using SC = ShootCore<Sys, M>;
  static constexpr int NS = Sys::NS, NU = Sys::NU, NW = Sys::NW, NY = SC::NY;
  static constexpr int NST = (M == 2) ? 4 : 2;                                     // stage points per step at most
  static constexpr int R_F = 0, R_A = NS, R_B = NS + NS * NS, REC = R_B + NS * NU;   // a stage's record: F | A | B
  static constexpr int REC_LD = REC | 1;                                           // the lane's LDS record: an odd stride
  MYR_HD static inline long nvars(int I, int cpi) { return (long)(I + 1) * NS + ((long)M * I * cpi + 1) * NU; }
  MYR_HD static inline long pair_doubles(int cpi) { return (long)cpi * (NS + NST * REC); }     // global scratch of one pair

  // The integration rules as tableaux (utils.py:31-54): X_j = x + c_j h k_{j-1}, U_j = sum_s cu[j][s] u_row(s), x_next = x + h sum_j b_j k_j.
  // Same values as ShootCore::step_val / rk4_val (a factor 1/2 moves through a product exactly).
  struct Rule { int nst; double c[NST], b[NST], cu[NST][M + 1]; };
  MYR_HD static inline Rule rule(int method) {
    Rule R;
#pragma unroll
    for (int j = 0; j < NST; ++j) {
      R.c[j] = 0.0; R.b[j] = 0.0;
#pragma unroll
      for (int s = 0; s <= M; ++s) R.cu[j][s] = 0.0;
    }
    if constexpr (M == 2) {                               // RK4 on rows u[2i], u[2i+1], u[2i+2]
      R.nst = 4;
      R.c[1] = 0.5; R.c[2] = 0.5; R.c[3] = 1.0;
      R.b[0] = 1.0 / 6.0; R.b[1] = 2.0 / 6.0; R.b[2] = 2.0 / 6.0; R.b[3] = 1.0 / 6.0;
      R.cu[0][0] = 1.0; R.cu[1][1] = 1.0; R.cu[2][1] = 1.0; R.cu[3][2] = 1.0;
    } else if (method == 0) {                             // Euler
      R.nst = 1; R.b[0] = 1.0; R.cu[0][0] = 1.0;
    } else if (method == 2) {                             // the reference's midpoint: full Euler predictor, averaged control
      R.nst = 2; R.c[1] = 1.0; R.b[1] = 1.0; R.cu[0][0] = 1.0; R.cu[1][0] = 0.5; R.cu[1][1] = 0.5;
    } else {                                              // Heun
      R.nst = 2; R.c[1] = 1.0; R.b[0] = 0.5; R.b[1] = 0.5; R.cu[0][0] = 1.0; R.cu[1][1] = 1.0;
    }
    return R;
  }

  // a pair's global scratch, pair-minor: field e of pair `col` at base[e * Pp + col]
  struct Scr {
    double* base; long Pp, col; int cpi;
    MYR_HD inline double& xs(int s, int c) const { return base[((long)s * NS + c) * Pp + col]; }
    MYR_HD inline double& rec(int s, int j, int q) const { return base[((long)cpi * NS + ((long)s * NST + j) * REC + q) * Pp + col]; }
  };
  // what the step algebra reads instead of calling the system (os_solver.h: SysEval): stage j of step s from the records of the rollout
  struct RecEval {
    Scr sc; int s;
    MYR_HD inline void lin(int j, HsPoint<Sys>& P, const double* p) const {
#pragma unroll
      for (int c = 0; c < NS; ++c) P.f[c] = sc.rec(s, j, R_F + c);
#pragma unroll
      for (int q = 0; q < NS * NS; ++q) P.A[q] = sc.rec(s, j, R_A + q);
#pragma unroll
      for (int q = 0; q < NS * NU; ++q) P.B[q] = sc.rec(s, j, R_B + q);
      Sys::cost_grad(P.x, P.u, p, &P.g, P.gw);
    }
    MYR_HD inline void hess(int, const HsPoint<Sys>&, const double*, const double*, double, double* W) const {
#pragma unroll
      for (int q = 0; q < NW * NW; ++q) W[q] = 0.0;
    }
  };

  MYR_HD static inline void stage_point(const Rule& R, double h, int j, const double* x, const double* kp, const double* uc, double* X, double* U) {
#pragma unroll
    for (int c = 0; c < NS; ++c) X[c] = x[c] + R.c[j] * h * kp[c];
#pragma unroll
    for (int a = 0; a < NU; ++a) {
      double u = 0.0;
#pragma unroll
      for (int s = 0; s <= M; ++s) u += R.cu[j][s] * uc[s * NU + a];
      U[a] = u;
    }
  }

  // Forward rollout of one pair from node state xk over its control rows uk, linearised: the step-start states and every stage's F, A, B -> sc.
  // Net::lin / Net::val evaluate the network at this lane's point; on the device they are the wavefront's pass, so EVERY lane calls them the
  // same number of times (`on`: this lane has a pair; the others roll a valid pair along and store nothing).
  template <class Net>
  MYR_HD static inline void pair_lin_rollout(Net& net, bool on, const Rule& R, double h, int cpi, const double* xk, const double* uk, const Scr& sc) {
    double x[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) x[c] = xk[c];
    for (int s = 0; s < cpi; ++s) {
      const double* uc = uk + (long)M * s * NU;
      double kp[NS], acc[NS];
#pragma unroll
      for (int c = 0; c < NS; ++c) { kp[c] = 0.0; acc[c] = 0.0; }
      if (on) {
#pragma unroll
        for (int c = 0; c < NS; ++c) sc.xs(s, c) = x[c];
      }
      for (int j = 0; j < R.nst; ++j) {
        double X[NS], U[NU], F[NS], A[NS * NS], Bm[NS * NU];
        stage_point(R, h, j, x, kp, uc, X, U);
        net.lin(X, U, F, A, Bm);
        if (on) {
#pragma unroll
          for (int c = 0; c < NS; ++c) sc.rec(s, j, R_F + c) = F[c];
#pragma unroll
          for (int q = 0; q < NS * NS; ++q) sc.rec(s, j, R_A + q) = A[q];
#pragma unroll
          for (int q = 0; q < NS * NU; ++q) sc.rec(s, j, R_B + q) = Bm[q];
        }
#pragma unroll
        for (int c = 0; c < NS; ++c) { kp[c] = F[c]; acc[c] += R.b[j] * F[c]; }
      }
#pragma unroll
      for (int c = 0; c < NS; ++c) x[c] = x[c] + h * acc[c];
    }
  }

  // shoot_eval_kernel's reverse sweep for pair k of one instance (z, lam, gradient g; cw = 1: with the objective), from the records of the
  // rollout.  The pair owns node row k (a_k - lam_{k-1}) and its control rows but the last, which the next pair owns: that contribution goes to
  // edge[k] (pair_join adds it).  Pair I - 1 also owns node row I (-lam_{I-1}) and the last control row.
  MYR_HD static inline void pair_reverse(int method, double h, int I, int cpi, int k, const double* z, const double* lam, const double* p, double cw,
                                         const Scr& sc, double* g, double* edge) {
    const int S = I * cpi, W = M * cpi + 1;
    const double* ub = z + (long)(I + 1) * NS;
    double* gu = g + (long)(I + 1) * NS + (long)M * k * cpi * NU;      // the pair's first control row
    for (int r = 0; r < (W - 1) * NU; ++r) gu[r] = 0.0;
    double a[NS], last[NU];
#pragma unroll
    for (int c = 0; c < NS; ++c) a[c] = lam[(long)k * NS + c];
#pragma unroll
    for (int u = 0; u < NU; ++u) last[u] = 0.0;
    double zero[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) zero[c] = 0.0;
    for (int j = cpi - 1; j >= 0; --j) {
      const int i = k * cpi + j;
      double xi[NS], Fy[NS * NY], gy[NY], Hs[NY * NY];
#pragma unroll
      for (int c = 0; c < NS; ++c) xi[c] = sc.xs(j, c);
      const RecEval ev{sc, j};
      SC::slin(method, h, xi, ub + (long)M * i * NU, p, zero, Fy, gy, Hs, h * i, i == S - 1, ev);
#pragma unroll
      for (int sl = 0; sl <= M; ++sl)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const int col = NS + sl * NU + u;
          double gsum = cw * gy[col];
#pragma unroll
          for (int t = 0; t < NS; ++t) gsum += a[t] * Fy[t * NY + col];
          const int r = M * j + sl;
          if (r == W - 1) last[u] += gsum; else gu[r * NU + u] += gsum;
        }
      double na[NS];
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        double sg = cw * gy[c];
#pragma unroll
        for (int t = 0; t < NS; ++t) sg += a[t] * Fy[t * NY + c];
        na[c] = sg;
      }
#pragma unroll
      for (int c = 0; c < NS; ++c) a[c] = na[c];
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) g[(long)k * NS + c] = k > 0 ? a[c] - lam[(long)(k - 1) * NS + c] : a[c];
    if (k == I - 1) {
#pragma unroll
      for (int c = 0; c < NS; ++c) g[(long)I * NS + c] = -lam[(long)k * NS + c];
#pragma unroll
      for (int u = 0; u < NU; ++u) gu[(W - 1) * NU + u] = last[u];
    } else {
#pragma unroll
      for (int u = 0; u < NU; ++u) edge[(long)k * NU + u] = last[u];
    }
  }
  // ... and the shared row of pairs k - 1 and k (k >= 1), after every pair of the instance has run: the earlier interval's part first
  MYR_HD static inline void pair_join(int I, int cpi, int k, double* g, const double* edge) {
    double* gu = g + (long)(I + 1) * NS + (long)M * k * cpi * NU;
#pragma unroll
    for (int u = 0; u < NU; ++u) gu[u] = edge[(long)(k - 1) * NU + u] + gu[u];
  }

  // J v of one pair: the rollout with the tangent (vxk of the node state, vuk of the control rows) carried through each stage's A, B -> the
  // tangent of the end state
  template <class Net>
  MYR_HD static inline void pair_jvp(Net& net, const Rule& R, double h, int cpi, const double* xk, const double* uk, const double* vxk, const double* vuk,
                                     double* dxe) {
    double x[NS], dx[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) { x[c] = xk[c]; dx[c] = vxk[c]; }
    for (int s = 0; s < cpi; ++s) {
      const double* uc = uk + (long)M * s * NU;
      const double* vc = vuk + (long)M * s * NU;
      double kp[NS], acc[NS], dkp[NS], dacc[NS];
#pragma unroll
      for (int c = 0; c < NS; ++c) { kp[c] = 0.0; acc[c] = 0.0; dkp[c] = 0.0; dacc[c] = 0.0; }
      for (int j = 0; j < R.nst; ++j) {
        double X[NS], U[NU], dX[NS], dU[NU], F[NS], A[NS * NS], Bm[NS * NU];
        stage_point(R, h, j, x, kp, uc, X, U);
        stage_point(R, h, j, dx, dkp, vc, dX, dU);
        net.lin(X, U, F, A, Bm);
#pragma unroll
        for (int r = 0; r < NS; ++r) {
          double d = 0.0;
#pragma unroll
          for (int c = 0; c < NS; ++c) d += A[r * NS + c] * dX[c];
#pragma unroll
          for (int q = 0; q < NU; ++q) d += Bm[r * NU + q] * dU[q];
          dkp[r] = d; dacc[r] += R.b[j] * d;
          kp[r] = F[r]; acc[r] += R.b[j] * F[r];
        }
      }
#pragma unroll
      for (int c = 0; c < NS; ++c) { x[c] = x[c] + h * acc[c]; dx[c] = dx[c] + h * dacc[c]; }
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) dxe[c] = dx[c];
  }

  // the end state of one pair (values only)
  template <class Net>
  MYR_HD static inline void pair_values(Net& net, const Rule& R, double h, int cpi, const double* xk, const double* uk, double* xe) {
    double x[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) x[c] = xk[c];
    for (int s = 0; s < cpi; ++s) {
      const double* uc = uk + (long)M * s * NU;
      double kp[NS], acc[NS];
#pragma unroll
      for (int c = 0; c < NS; ++c) { kp[c] = 0.0; acc[c] = 0.0; }
      for (int j = 0; j < R.nst; ++j) {
        double X[NS], U[NU], F[NS];
        stage_point(R, h, j, x, kp, uc, X, U);
        net.val(X, U, F);
#pragma unroll
        for (int c = 0; c < NS; ++c) { kp[c] = F[c]; acc[c] += R.b[j] * F[c]; }
      }
#pragma unroll
      for (int c = 0; c < NS; ++c) x[c] = x[c] + h * acc[c];
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) xe[c] = x[c];
  }

  // the projected step of exgd_update_kernel and the multiplier step of axpy_kernel (shoot_eval.h), one variable
  MYR_HD static inline double clip_step(double zref, double g, double eta, double lb, double ub) {
    const double v = zref - eta * g;
    return v < lb ? lb : (v > ub ? ub : v);
  }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: the pairs of one instance one after the other, the network by SysNODE::lin / f ---------------------------------------------
template <class Sys>
struct NspHostNet {
  const double* p;
  inline void lin(const double* X, const double* U, double* F, double* A, double* Bm) const {
    double g, gw[Sys::NW];
    Sys::lin(X, U, p, F, A, Bm, &g, gw);
  }
  inline void val(const double* X, const double* U, double* F) const { Sys::f(X, U, p, F); }
};

// g = (cw grad f) + J^T lam of one instance; scratch: pair_doubles(cpi), edge: I * NU
template <class Sys, int M>
inline void node_shoot_grad_host(int method, int I, int cpi, double T, const double* z, const double* lam, const double* p, double cw, double* scratch,
                                 double* edge, double* g) {
  using P = NodeShootProd<Sys, M>;
  const typename P::Rule R = P::rule(method);
  const double h = T / ((double)I * cpi);
  NspHostNet<Sys> net{p};
  const typename P::Scr sc{scratch, 1, 0, cpi};
  const double* ub = z + (long)(I + 1) * P::NS;
  for (int k = 0; k < I; ++k) {
    P::pair_lin_rollout(net, true, R, h, cpi, z + (long)k * P::NS, ub + (long)M * k * cpi * P::NU, sc);
    P::pair_reverse(method, h, I, cpi, k, z, lam, p, cw, sc, g, edge);
  }
  for (int k = 1; k < I; ++k) P::pair_join(I, cpi, k, g, edge);
}
template <class Sys, int M>
inline void node_shoot_jvp_host(int method, int I, int cpi, double T, const double* z, const double* v, const double* p, double* out) {
  using P = NodeShootProd<Sys, M>;
  const typename P::Rule R = P::rule(method);
  const double h = T / ((double)I * cpi);
  NspHostNet<Sys> net{p};
  const long uo = (long)(I + 1) * P::NS;
  for (int k = 0; k < I; ++k) {
    double dxe[P::NS];
    P::pair_jvp(net, R, h, cpi, z + (long)k * P::NS, z + uo + (long)M * k * cpi * P::NU, v + (long)k * P::NS, v + uo + (long)M * k * cpi * P::NU, dxe);
    for (int c = 0; c < P::NS; ++c) out[(long)k * P::NS + c] = dxe[c] - v[(long)(k + 1) * P::NS + c];
  }
}
// nsteps extragradient steps of one instance in place; work: 2 n + pair_doubles(cpi) + I * NU
template <class Sys, int M>
inline void node_shoot_exgd_host(int method, int I, int cpi, double T, double* z, double* lam, const double* lb, const double* ub, const double* p,
                                 double eta_x, double eta_v, int nsteps, double* work) {
  using P = NodeShootProd<Sys, M>;
  const typename P::Rule R = P::rule(method);
  const long n = P::nvars(I, cpi);
  const double h = T / ((double)I * cpi);
  double* zb = work; double* g = zb + n; double* scratch = g + n; double* edge = scratch + P::pair_doubles(cpi);
  NspHostNet<Sys> net{p};
  const long uo = (long)(I + 1) * P::NS;
  for (int s = 0; s < nsteps; ++s) {
    node_shoot_grad_host<Sys, M>(method, I, cpi, T, z, lam, p, 1.0, scratch, edge, g);
    for (long i = 0; i < n; ++i) zb[i] = P::clip_step(z[i], g[i], eta_x, lb[i], ub[i]);
    node_shoot_grad_host<Sys, M>(method, I, cpi, T, zb, lam, p, 1.0, scratch, edge, g);
    for (long i = 0; i < n; ++i) z[i] = P::clip_step(z[i], g[i], eta_x, lb[i], ub[i]);
    for (int k = 0; k < I; ++k) {
      double xe[P::NS];
      P::pair_values(net, R, h, cpi, z + (long)k * P::NS, z + uo + (long)M * k * cpi * P::NU, xe);
      for (int c = 0; c < P::NS; ++c) lam[(long)k * P::NS + c] += eta_v * (xe[c] - z[(long)(k + 1) * P::NS + c]);
    }
  }
}
#endif  // !__HIP_DEVICE_COMPILE__

#if defined(__HIPCC__)
enum { NSP_VJP = 0, NSP_JVP = 1, NSP_EXGD = 2 };
struct NspArgs {
  int op, B, I, cpi, method, G;          // G: instances per workgroup
  double T;
  const double *z, *w, *params; int pstride;      // vjp / jvp: the point, lam or v
  double* out; int add_gradf;
  double *zio, *lamio; const double *lb, *ub; double eta_x, eta_v; int nsteps;      // exgd
  double* scr; long Pp;                  // pair scratch: pair_doubles(cpi) fields of Pp columns
  double* iter;                          // exgd: the iterate arrays of every workgroup in global memory, or null (LDS)
  long lds_doubles;                      // the launch's dynamic LDS (MYRIAD_POISON fills it)
  unsigned long long poison;
};

// workgroup LDS: weights | point list | the lanes' records | values of a pass<0> | shared-row slots | exgd: z, x_bar, g, lam of G instances
template <class Sys, int M>
struct NspLds {
  using P = NodeShootProd<Sys, M>;
  __host__ __device__ static long edge_doubles(int I) { return (long)(I > 64 ? I : 64) * P::NU; }
  __host__ __device__ static long fixed_doubles(int I) {
    return (long)NodeMfma64::L_N + P::NW * 64 + 64 * P::REC_LD + P::NS * 64 + edge_doubles(I);
  }
  __host__ __device__ static long iter_doubles(int I, int cpi) { return 3 * P::nvars(I, cpi) + (long)I * P::NS; }      // per instance
};

// the network at the lanes' points by ONE pass of the wavefront (all 64 lanes call; K = lanes with a pair, the first K)
template <class Sys, int M>
struct NspDevNet {
  using P = NodeShootProd<Sys, M>;
  static constexpr int NS = P::NS, NU = P::NU;
  const nd_lds* wl; nd_lds* pts; nd_lds* rec; nd_lds* sF;
  int K, lane; bool on;
  __device__ inline NodeMfma64::ArgsT<nd_lds> args() const {
    NodeMfma64::ArgsT<nd_lds> a;
    a.z = (const nd_lds*)pts; a.dz = (const nd_lds*)pts; a.lam = nullptr; a.pt = nullptr; a.sF = sF;
    a.alpha = 0.0; a.h6 = 0.0; a.h8 = 0.0; a.K = K; a.N = 0; a.pf_f = 0; a.pf_a = 0; a.pf_b = 0; a.pf_d2 = 0;
    a.t0 = 0; a.ts = 1; a.hb = nullptr; a.mb = nullptr; a.h_valid = 0;
    return a;
  }
  __device__ inline void put(const double* X, const double* U) const {
    if (on) {
#pragma unroll
      for (int c = 0; c < NS; ++c) pts[lane * NS + c] = X[c];
      pts[K * NS + lane] = U[0];
    }
    __syncthreads();
  }
  __device__ inline void lin(const double* X, const double* U, double* F, double* A, double* Bm) const {
    put(X, U);
    NodeMfma64::ArgsT<nd_lds> a = args();
    a.rec = rec; a.use_rec = 1; a.rec_stride = P::REC_LD; a.rec_f = P::R_F; a.rec_a = P::R_A; a.rec_b = P::R_B;
    NodeMfma64::pass<1, nd_lds>(wl, a, lane);
    __syncthreads();
    const nd_lds* r = rec + (on ? lane : 0) * P::REC_LD;
#pragma unroll
    for (int c = 0; c < NS; ++c) F[c] = r[P::R_F + c];
#pragma unroll
    for (int q = 0; q < NS * NS; ++q) A[q] = r[P::R_A + q];
#pragma unroll
    for (int q = 0; q < NS * NU; ++q) Bm[q] = r[P::R_B + q];
  }
  __device__ inline void val(const double* X, const double* U, double* F) const {
    put(X, U);
    NodeMfma64::pass<0, nd_lds>(wl, args(), lane);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NS; ++c) F[c] = sF[(on ? lane : 0) * NS + c];
  }
};

template <class Sys, int M>
struct NspDev {
  using P = NodeShootProd<Sys, M>;
  static constexpr int NS = P::NS, NU = P::NU;
  // which pair this lane holds in chunk `ch` of the workgroup's instances: local instance gl, interval k; lanes without one mirror the chunk's first pair
  struct Slot { bool on; int gl, k, K; };
  __device__ static inline Slot slot(int I, int gact, int ch, int lane) {
    Slot s;
    if (I <= 64) { s.K = gact * I; s.on = lane < s.K; s.gl = s.on ? lane / I : 0; s.k = s.on ? lane - s.gl * I : 0; }
    else { const int kb = ch * 64; s.K = I - kb < 64 ? I - kb : 64; s.on = lane < s.K; s.gl = 0; s.k = s.on ? kb + lane : kb; }
    return s;
  }
  __device__ static inline int chunks(int I) { return I <= 64 ? 1 : (I + 63) / 64; }

  // g = (cw grad f) + J^T lam for the workgroup's instances: z, lam, g of local instance gl at zb + gl n, lb + gl m, gb + gl n
  __device__ static void grad_all(const NspArgs& a, NspDevNet<Sys, M>& net, const typename P::Rule& R, long b0, int gact, const double* zb, const double* lb,
                                  double* gb, double* edge, const double* p, double cw) {
    const int I = a.I, cpi = a.cpi, lane = threadIdx.x;
    const long n = P::nvars(I, cpi), m = (long)I * NS;
    const double h = a.T / ((double)I * cpi);
    for (int ch = 0; ch < chunks(I); ++ch) {
      const Slot s = slot(I, gact, ch, lane);
      net.K = s.K; net.on = s.on;
      const double* zi = zb + s.gl * n;
      const typename P::Scr sc{a.scr, a.Pp, (b0 + s.gl) * I + s.k, cpi};
      P::pair_lin_rollout(net, s.on, R, h, cpi, zi + (long)s.k * NS, zi + (long)(I + 1) * NS + (long)M * s.k * cpi * NU, sc);
      if (s.on) P::pair_reverse(a.method, h, I, cpi, s.k, zi, lb + s.gl * m, p, cw, sc, gb + s.gl * n, edge + (long)s.gl * I * NU);
    }
    __syncthreads();
    for (int q = lane; q < gact * I; q += 64) {
      const int gl = q / I, k = q - gl * I;
      if (k > 0) P::pair_join(I, cpi, k, gb + gl * n, edge + (long)gl * I * NU);
    }
    __syncthreads();
  }
};

// grid: ceil(B / G) workgroups of ONE wavefront; dynamic LDS: NspLds
template <class Sys, int M>
__global__ __launch_bounds__(64)
void node_shoot_products_kernel(NspArgs a) {
  using P = NodeShootProd<Sys, M>;
  using L = NspLds<Sys, M>;
  using D = NspDev<Sys, M>;
  constexpr int NS = P::NS, NU = P::NU;
  extern __shared__ __attribute__((aligned(16))) char smem_nsp[];
  double* l0 = reinterpret_cast<double*>(smem_nsp);
  const int lane = threadIdx.x, I = a.I, cpi = a.cpi;
  const long n = P::nvars(I, cpi), m = (long)I * NS;
  const long b0 = (long)blockIdx.x * a.G;
  const int gact = (a.B - b0) < a.G ? (int)(a.B - b0) : a.G;
  const double h = a.T / ((double)I * cpi);
  if (a.poison) {      // MYRIAD_POISON (tests): everything the workgroup inherits -- its LDS and its pairs' scratch columns
    for (long i = lane; i < a.lds_doubles; i += 64) l0[i] = poison_value(a.poison, (unsigned long long)i, (unsigned long long)blockIdx.x * 1315423911ULL);
    for (int ch = 0; ch < D::chunks(I); ++ch) {
      const typename D::Slot s = D::slot(I, gact, ch, lane);
      if (s.on) {
        const long col = (b0 + s.gl) * I + s.k;
        for (long e = 0; e < P::pair_doubles(cpi); ++e) a.scr[e * a.Pp + col] = poison_value(a.poison, (unsigned long long)e + (1ULL << 32), (unsigned long long)col);
      }
    }
    __syncthreads();
  }
  double* wl = l0;
  double* pts = wl + NodeMfma64::L_N;
  double* rec = pts + P::NW * 64;
  double* sF = rec + 64 * P::REC_LD;
  double* edge = sF + NS * 64;
  double* it = a.iter ? a.iter + (long)blockIdx.x * a.G * L::iter_doubles(I, cpi) : edge + L::edge_doubles(I);
  const double* p = a.params + (a.pstride ? b0 * (long)a.pstride : 0L);      // (params_stride == np: G = 1)
  NodeMfma64::load_weights(p, wl, lane, 64);
  __syncthreads();
  NspDevNet<Sys, M> net;
  net.wl = (const nd_lds*)wl; net.pts = (nd_lds*)pts; net.rec = (nd_lds*)rec; net.sF = (nd_lds*)sF; net.lane = lane; net.K = 1; net.on = false;
  const typename P::Rule R = P::rule(a.method);

  if (a.op == NSP_VJP) {
    D::grad_all(a, net, R, b0, gact, a.z + b0 * n, a.w + b0 * m, a.out + b0 * n, edge, p, a.add_gradf ? 1.0 : 0.0);
  } else if (a.op == NSP_JVP) {
    for (int ch = 0; ch < D::chunks(I); ++ch) {
      const typename D::Slot s = D::slot(I, gact, ch, lane);
      net.K = s.K; net.on = s.on;
      const double* zi = a.z + (b0 + s.gl) * n; const double* vi = a.w + (b0 + s.gl) * n;
      const long uo = (long)(I + 1) * NS + (long)M * s.k * cpi * NU;
      double dxe[NS];
      P::pair_jvp(net, R, h, cpi, zi + (long)s.k * NS, zi + uo, vi + (long)s.k * NS, vi + uo, dxe);
      if (s.on) {
#pragma unroll
        for (int c = 0; c < NS; ++c) a.out[(b0 + s.gl) * m + (long)s.k * NS + c] = dxe[c] - vi[(long)(s.k + 1) * NS + c];
      }
    }
  } else {
    double* zw = it; double* zbar = zw + a.G * n; double* gw = zbar + a.G * n; double* lw = gw + a.G * n;
    for (long q = lane; q < gact * n; q += 64) zw[q] = a.zio[b0 * n + q];
    for (long q = lane; q < gact * m; q += 64) lw[q] = a.lamio[b0 * m + q];
    __syncthreads();
    for (int st = 0; st < a.nsteps; ++st) {
      D::grad_all(a, net, R, b0, gact, zw, lw, gw, edge, p, 1.0);
      for (long q = lane; q < gact * n; q += 64) zbar[q] = P::clip_step(zw[q], gw[q], a.eta_x, a.lb[b0 * n + q], a.ub[b0 * n + q]);
      __syncthreads();
      D::grad_all(a, net, R, b0, gact, zbar, lw, gw, edge, p, 1.0);
      for (long q = lane; q < gact * n; q += 64) zw[q] = P::clip_step(zw[q], gw[q], a.eta_x, a.lb[b0 * n + q], a.ub[b0 * n + q]);
      __syncthreads();
      for (int ch = 0; ch < D::chunks(I); ++ch) {
        const typename D::Slot s = D::slot(I, gact, ch, lane);
        net.K = s.K; net.on = s.on;
        const double* zi = zw + s.gl * n;
        double xe[NS];
        P::pair_values(net, R, h, cpi, zi + (long)s.k * NS, zi + (long)(I + 1) * NS + (long)M * s.k * cpi * NU, xe);
        if (s.on) {
#pragma unroll
          for (int c = 0; c < NS; ++c) lw[s.gl * m + (long)s.k * NS + c] += a.eta_v * (xe[c] - zi[(long)(s.k + 1) * NS + c]);
        }
      }
      __syncthreads();
    }
    for (long q = lane; q < gact * n; q += 64) a.zio[b0 * n + q] = zw[q];
    for (long q = lane; q < gact * m; q += 64) a.lamio[b0 * m + q] = lw[q];
  }
}
#endif  // __HIPCC__

}  // namespace myriad
