// hostsim.cpp -- TEST-ONLY host build of the solver core (myriad_amd/csrc/hs_solver.h) so the per-trajectory
// SQP algebra can be exercised by the CPU test-suite (`-m "not gpu"`) in a container without a GPU.
// It is never loaded by the myriad_amd package and is not a fallback: the product path is the HIP kernel
// that calls the very same HsSolver<Sys>::solve, one trajectory per lane.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../myriad_amd/csrc/hs_solver.h"
#include "../../myriad_amd/csrc/rollout.h"
#include "../../myriad_amd/csrc/os_solver.h"

using namespace myriad;

// test/dev knobs: every solver option can be overridden from the environment
static void apply_env(HsSolveOpts& o) {
  if (getenv("RHO")) o.rho_term = atof(getenv("RHO"));
  if (getenv("REGF")) o.reg_floor = atof(getenv("REGF"));
  if (getenv("NONM")) o.nonmono = atoi(getenv("NONM"));
  if (getenv("DUALF")) o.dual_follow = atoi(getenv("DUALF"));
  if (getenv("LM")) o.lm_init = atof(getenv("LM"));
  if (getenv("TAU")) o.tau_min = atof(getenv("TAU"));
  if (getenv("LMABS")) o.lm_abs = atoi(getenv("LMABS"));
  if (getenv("DWARM")) o.delta_warm = atoi(getenv("DWARM"));
  if (getenv("DWMIN")) o.delta_warm_min = atof(getenv("DWMIN"));
  if (getenv("KSIG")) o.kappa_sigma = atof(getenv("KSIG"));
  if (getenv("KMU")) o.kappa_mu = atof(getenv("KMU"));
  if (getenv("TMU")) o.theta_mu = atof(getenv("TMU"));
  if (getenv("KEPS")) o.kappa_eps = atof(getenv("KEPS"));
  if (getenv("RECN")) o.recenter = atoi(getenv("RECN"));
  if (getenv("RECA")) o.recenter_alpha = atof(getenv("RECA"));
}

template <class Sys>
static void solve_batch(int N, double T, int B, double* z, const double* lb, const double* ub, const double* params,
                        int pstride, int max_iter, double tol_feas, double tol_stat, double tol_compl, double mu_init,
                        double* lam, double* cost, int32_t* status, int32_t* iters, double* kkt) {
  using S = HsSolver<Sys>;
  const int K = 2 * N + 1, n = K * Sys::NW, m = 2 * N * Sys::NS;
  HsSolveOpts o{N, T / N, max_iter, tol_feas, tol_stat, tol_compl, mu_init};
  apply_env(o);

#pragma omp parallel for schedule(dynamic)
  for (int b = 0; b < B; ++b) {
    std::vector<double> zL(n), zU(n), dz(n), lbv(lb + (size_t)b * n, lb + (size_t)(b + 1) * n),
        ubv(ub + (size_t)b * n, ub + (size_t)(b + 1) * n), st(HsSol<Sys>::stage_doubles(N));
    if (getenv("POISON")) {   // the device scratch is not zero-initialised: NaN here exposes a read-before-write
      for (auto* v : {&zL, &zU, &dz, &st}) for (auto& x : *v) x = NAN;
      for (int i = 0; i < m; ++i) lam[(size_t)b * m + i] = NAN;
    }
    SysParams<Sys> pp;
    pp.load(params, b, pstride);
    const double* p = pp.get();
    HsWork w{{z + (size_t)b * n, 1}, {lbv.data(), 1}, {ubv.data(), 1}, {zL.data(), 1}, {zU.data(), 1},
             {lam + (size_t)b * m, 1}, {dz.data(), 1}, {st.data(), 1}};
    HsSolveResult r;
    S::solve(w, o, p, r);
    cost[b] = r.cost; status[b] = r.status; iters[b] = r.iters;
    if (kkt) { kkt[3 * b] = r.feas; kkt[3 * b + 1] = r.stat; kkt[3 * b + 2] = getenv("SWEEPS") ? (double)r.sweeps : r.compl_; }
  }
}

// One Newton/SQP step at a given (interior) iterate: for checking the Riccati recursion against a dense KKT solve.
template <class Sys>
static void one_step(int N, double T, double* z, const double* lb, const double* ub, double* zL, double* zU,
                     const double* nuT, double mu, double* lam, double* dz, double* nu_out, double* info) {
  using S = HsSolver<Sys>;
  const int K = 2 * N + 1, n = K * Sys::NW;
  HsSolveOpts o{N, T / N, 1, 1e-8, 1e-6, 1e-7, mu};
  if (getenv("RHO")) o.rho_term = atof(getenv("RHO"));
  if (getenv("REGF")) o.reg_floor = atof(getenv("REGF"));
  std::vector<double> st(HsSol<Sys>::stage_doubles(N)), lbv(lb, lb + n), ubv(ub, ub + n);
  double p[Sys::NPX];
  Sys::default_params(p);
  HsWork w{{z, 1}, {lbv.data(), 1}, {ubv.data(), 1}, {zL, 1}, {zU, 1}, {lam, 1}, {dz, 1}, {st.data(), 1}};
  typename S::SweepOut so;
  so.abort_on_reg = false;
  S::backward(w, o, p, nuT, 0.0, so);
  S::solve_nu(so, mu, nu_out);
  typename S::FwdOut fo;
  S::forward(w, o, p, mu, nu_out, so.term_pinned, fo);
  info[0] = so.f; info[1] = so.c1; info[2] = so.cinf; info[3] = so.stat; info[4] = so.compl_max;
  info[5] = fo.alpha_p; info[6] = fo.alpha_d; info[7] = fo.gphi; info[8] = so.nreg;
}

extern "C" int hostsim_solve(int system_id, int N, double T, int B, double* z, const double* lb, const double* ub,
                             const double* params, int pstride, int max_iter, double tol_feas, double tol_stat,
                             double tol_compl, double mu_init, double* lam, double* cost, int32_t* status,
                             int32_t* iters, double* kkt) {
#define GO(S) solve_batch<S>(N, T, B, z, lb, ub, params, pstride, max_iter, tol_feas, tol_stat, tol_compl, mu_init, lam, cost, status, iters, kkt)
  switch (system_id) {
    case 0: GO(SysCARTPOLE); return 0;
    case 1: GO(SysVANDERPOL); return 0;
    case 2: GO(SysCANCERTREATMENT); return 0;
    case 3: GO(SysSIMPLECASE); return 0;
    case 13: GO(SysPENDULUM); return 0;     // dev: solver traces of the later systems
    case 10: GO(SysEPIDEMICSEIRN); return 0;
  }
  return -1;
}

extern "C" int hostsim_step(int system_id, int N, double T, double* z, const double* lb, const double* ub, double* zL,
                            double* zU, const double* nuT, double mu, double* lam, double* dz, double* nu_out, double* info) {
#define ST(S) one_step<S>(N, T, z, lb, ub, zL, zU, nuT, mu, lam, dz, nu_out, info)
  switch (system_id) {
    case 0: ST(SysCARTPOLE); return 0;
    case 1: ST(SysVANDERPOL); return 0;
    case 2: ST(SysCANCERTREATMENT); return 0;
    case 3: ST(SysSIMPLECASE); return 0;
  }
  return -1;
}

extern "C" double hostsim_rollout(int system_id, int method, int num_steps, double h, int u_rows, const double* x0,
                                  const double* us, const double* params, double* xs) {
#define RL(S) { double p[S::NPX]; S::default_params(p); if (params) for (int i = 0; i < S::NP; ++i) p[i] = params[i]; \
                return Rollout<S>::run(method, num_steps, h, u_rows, x0, us, p, xs); }
  switch (system_id) {
    case 0: RL(SysCARTPOLE)
    case 1: RL(SysVANDERPOL)
    case 2: RL(SysCANCERTREATMENT)
    case 3: RL(SysSIMPLECASE)
  }
  return NAN;
}

// generic batch driver for the one-step cores (trapezoid / shooting)
template <class Core, class Sys>
static void os_batch(const HsSolveOpts& o0, int n, int m, long nst, int B, double* z, const double* lb, const double* ub,
                     const double* params, int pstride, double* lam, double* cost, int32_t* status, int32_t* iters, double* kkt) {
#pragma omp parallel for schedule(dynamic)
  for (int b = 0; b < B; ++b) {
    std::vector<double> zL(n), zU(n), dz(n), lbv(lb + (size_t)b * n, lb + (size_t)(b + 1) * n),
        ubv(ub + (size_t)b * n, ub + (size_t)(b + 1) * n), st(nst);
    SysParams<Sys> pp;
    pp.load(params, b, pstride);
    const double* p = pp.get();
    HsWork w{{z + (size_t)b * n, 1}, {lbv.data(), 1}, {ubv.data(), 1}, {zL.data(), 1}, {zU.data(), 1},
             {lam + (size_t)b * m, 1}, {dz.data(), 1}, {st.data(), 1}};
    HsSolveResult r;
    HsSolveOpts o = o0;
    if (getenv("TAU")) o.tau_min = atof(getenv("TAU"));
    if (getenv("LMABS")) o.lm_abs = atoi(getenv("LMABS"));
    if (getenv("KSIG")) o.kappa_sigma = atof(getenv("KSIG"));
    if (getenv("MU0")) o.mu_init = atof(getenv("MU0"));
    if (getenv("LM")) o.lm_init = atof(getenv("LM"));
    Core::solve(w, o, p, r);
    cost[b] = r.cost; status[b] = r.status; iters[b] = r.iters;
    if (kkt) { kkt[3 * b] = r.feas; kkt[3 * b + 1] = r.stat; kkt[3 * b + 2] = r.compl_; }
  }
}

extern "C" int hostsim_solve_trap(int system_id, int N, double T, int B, double* z, const double* lb, const double* ub,
                                  const double* params, int pstride, int max_iter, double* lam, double* cost,
                                  int32_t* status, int32_t* iters, double* kkt) {
  HsSolveOpts o{N, T / N, max_iter, 1e-8, 1e-6, 1e-7, 0.1};
  apply_env(o);
#define TR(S) os_batch<TrapCore<S>, S>(o, (N + 1) * S::NW, N * S::NS, TrapCore<S>::stage_doubles(N), B, z, lb, ub, params, pstride, lam, cost, status, iters, kkt)
  switch (system_id) {
    case 0: TR(SysCARTPOLE); return 0;
    case 1: TR(SysVANDERPOL); return 0;
    case 2: TR(SysCANCERTREATMENT); return 0;
    case 3: TR(SysSIMPLECASE); return 0;
  }
  return -1;
}

extern "C" int hostsim_solve_shoot(int system_id, int I, int cpi, int method, double T, int B, double* z, const double* lb,
                                   const double* ub, const double* params, int pstride, int max_iter, double* lam,
                                   double* cost, int32_t* status, int32_t* iters, double* kkt) {
  HsSolveOpts o{I, T / I, max_iter, 1e-8, 1e-6, 1e-7, 0.1};
  o.cpi = cpi; o.method = method;
  apply_env(o);
#define SH(S) { if (method == 3) os_batch<ShootCore<S, 2>, S>(o, (I + 1) * S::NS + (2 * I * cpi + 1) * S::NU, I * S::NS, ShootCore<S, 2>::stage_doubles(I, cpi), B, z, lb, ub, params, pstride, lam, cost, status, iters, kkt); \
                else os_batch<ShootCore<S>, S>(o, (I + 1) * S::NS + (I * cpi + 1) * S::NU, I * S::NS, ShootCore<S>::stage_doubles(I, cpi), B, z, lb, ub, params, pstride, lam, cost, status, iters, kkt); }
  switch (system_id) {
    case 0: SH(SysCARTPOLE); return 0;
    case 1: SH(SysVANDERPOL); return 0;
    case 2: SH(SysCANCERTREATMENT); return 0;
    case 3: SH(SysSIMPLECASE); return 0;
  }
  return -1;
}

// ---- the interior-point policy (myriad_amd/csrc/ip_policy.h) on given scalars: tests/test_hostsim.py restates the rules ----
static HsSolveOpts policy_opts(double tol_stat, double tol_compl, double mu_init) { return HsSolveOpts{1, 1.0, 1, 1e-8, tol_stat, tol_compl, mu_init}; }

// out[0] = the first rung, out[i] = rung i of the ladder, out[rungs] = delta_last as the ladder closed at rung `rungs - 1` leaves it
extern "C" void hostsim_policy_ladder(double lm, double delta_last, int delta_warm, double delta_warm_min, int rungs, double* out) {
  HsSolveOpts o = policy_opts(1e-6, 1e-7, 0.1);
  o.delta_warm = delta_warm; o.delta_warm_min = delta_warm_min;
  IpState<4> s;
  s.start(o);
  s.lm = lm; s.delta_last = delta_last;
  out[0] = s.first_delta(o);
  for (int i = 1; i < rungs; ++i) out[i] = s.next_delta(out[i - 1]);
  s.close_ladder(out[rungs - 1]);
  out[rungs] = s.delta_last;
}

// one barrier update at the given KKT figures; returns the new mu, *mu_min the floor the state derived from the tolerances
extern "C" double hostsim_policy_barrier(double mu, double tol_stat, double tol_compl, double kappa_mu, double theta_mu, double kappa_eps,
                                         double sd, double stat, double cinf, double compl_min, double compl_max, double* mu_min) {
  HsSolveOpts o = policy_opts(tol_stat, tol_compl, mu);
  o.kappa_mu = kappa_mu; o.theta_mu = theta_mu; o.kappa_eps = kappa_eps;
  IpState<4> s;
  s.start(o);
  IpKkt k{sd, stat, 0.0, true, false};
  s.barrier_update(o, k, cinf, compl_min, compl_max);
  *mu_min = s.mu_min;
  return s.mu;
}

// the penalty rule over `iters` iterations; out[3 i ..] = penalty, pen_over, pen_cuts after iteration i; slope[i] = the returned merit slope
extern "C" void hostsim_policy_penalty(int iters, const double* gphi, const double* c1, const double* floor_, double* out, double* slope) {
  HsSolveOpts o = policy_opts(1e-6, 1e-7, 0.1);
  IpState<4> s;
  s.start(o);
  for (int i = 0; i < iters; ++i) {
    slope[i] = floor_ ? s.penalty_update(gphi[i], c1[i], floor_[i]) : s.penalty_update(gphi[i], c1[i]);
    out[3 * i] = s.pen; out[3 * i + 1] = s.pen_over; out[3 * i + 2] = s.pen_cuts;
  }
}

// park record of a state with NS = 4: the fields in `in` (12 scalars, 5 of the step, 4 nuT, 8 hist; assigned by NAME here) are saved
// to sv, loaded into a fresh state and read back, by name again, to `back`.  Returns the record's length.
extern "C" int hostsim_policy_record(const double* in, double* sv, double* back) {
  struct Step { bool on; double ap, ad, mu, ksig; };
  HsSolveOpts o = policy_opts(1e-6, 1e-7, 0.1);
  IpState<4> s, r;
  double hist[NMMAX], rhist[NMMAX];
  s.start(o); r.start(o);
  s.mu = in[0]; s.pen = in[1]; s.pen_over = (int)in[2]; s.pen_cuts = (int)in[3]; s.stall = (int)in[4]; s.small_steps = (int)in[5];
  s.delta_last = in[6]; s.lm = in[7]; s.nhist = (int)in[8]; s.hpos = (int)in[9]; s.hist_mu = in[10]; s.hist_pen = in[11];
  Step p{in[12] != 0.0, in[13], in[14], in[15], in[16]}, q{false, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < 4; ++i) s.nuT[i] = in[17 + i];
  for (int i = 0; i < NMMAX; ++i) { hist[i] = in[21 + i]; rhist[i] = 0.0; }
  s.save(sv, hist, p);
  r.load(sv, rhist, q);
  back[0] = r.mu; back[1] = r.pen; back[2] = r.pen_over; back[3] = r.pen_cuts; back[4] = r.stall; back[5] = r.small_steps;
  back[6] = r.delta_last; back[7] = r.lm; back[8] = r.nhist; back[9] = r.hpos; back[10] = r.hist_mu; back[11] = r.hist_pen;
  back[12] = q.on ? 1.0 : 0.0; back[13] = q.ap; back[14] = q.ad; back[15] = q.mu; back[16] = q.ksig;
  for (int i = 0; i < 4; ++i) back[17 + i] = r.nuT[i];
  for (int i = 0; i < NMMAX; ++i) back[21 + i] = rhist[i];
  return IpState<4>::RECORD;
}

// ---- the bound rules (myriad_amd/csrc/bound_rules.h) on plain arrays of cases: tests/test_hostsim.py restates each rule ----
// out[3 i ..] = z, zL, zU of the starting point of case i
extern "C" void hostsim_bound_start(int n, const double* v0, const double* l, const double* u, double* out) {
  for (int i = 0; i < n; ++i) {
    const BoundStart b = bound_start(v0[i], l[i], u[i]);
    out[3 * i] = b.z; out[3 * i + 1] = b.zL; out[3 * i + 2] = b.zU;
  }
}

// the accepted step of case i with zn = zv + ap d formed here, as HsSolver::update forms it; rcp selects bound_accept<true>;
// out[3 i ..] = zn, zL, zU
extern "C" void hostsim_bound_accept(int n, int rcp, const double* l, const double* u, const double* zv, const double* d, const double* zl,
                                     const double* zu, const double* ap, const double* ad, const double* mu, const double* ksig, double* out) {
  for (int i = 0; i < n; ++i) {
    const BoundKind k = bound_kind(l[i], u[i]);
    const double zn = k.fr ? zv[i] + ap[i] * d[i] : zv[i], iks = 1.0 / ksig[i];
    const BoundMult m = rcp ? bound_accept<true>(k, l[i], u[i], zv[i], zn, d[i], zl[i], zu[i], ad[i], mu[i], ksig[i], iks)
                            : bound_accept<false>(k, l[i], u[i], zv[i], zn, d[i], zl[i], zu[i], ad[i], mu[i], ksig[i], iks);
    out[3 * i] = zn; out[3 * i + 1] = m.zL; out[3 * i + 2] = m.zU;
  }
}

// out[6 i ..] = sigma, g1, zlu, pinned, and the complementarity extremes as case i leaves them when they arrive as cmax[i], cmin[i]
extern "C" void hostsim_bound_terms(int n, const double* zv, const double* l, const double* u, const double* zl, const double* zu,
                                    const double* cmax, const double* cmin, double* out) {
  for (int i = 0; i < n; ++i) {
    double cx = cmax[i], cn = cmin[i];
    const BoundTerms b = bound_terms(zv[i], l[i], u[i], zl[i], zu[i], cx, cn);
    out[6 * i] = b.sigma; out[6 * i + 1] = b.g1; out[6 * i + 2] = b.zlu; out[6 * i + 3] = b.pinned ? 1.0 : 0.0; out[6 * i + 4] = cx; out[6 * i + 5] = cn;
  }
}

// out[3 i ..] = alpha_p, alpha_d, gphi of case i alone (from 1, 1, 0)
extern "C" void hostsim_step_limits(int n, const double* zv, const double* l, const double* u, const double* zl, const double* zu, const double* d,
                                    const double* mu, const double* wg, const double* tau, double* out) {
  struct { double alpha_p, alpha_d, gphi; } fo;
  for (int i = 0; i < n; ++i) {
    fo.alpha_p = 1.0; fo.alpha_d = 1.0; fo.gphi = 0.0;
    step_limits(zv[i], l[i], u[i], zl[i], zu[i], d[i], mu[i], wg[i], tau[i], fo);
    out[3 * i] = fo.alpha_p; out[3 * i + 1] = fo.alpha_d; out[3 * i + 2] = fo.gphi;
  }
}

// n points of k variables each: out[4 p ..] = value(), slk, sexp, bad of point p; pairs[p k + i] = slack_pair of its variable i
extern "C" void hostsim_slack_log(int n, int k, const double* v, const double* l, const double* u, double* out, double* pairs) {
  for (int p = 0; p < n; ++p) {
    SlackLog s;
    int bad = 0;
    for (int i = p * k; i < (p + 1) * k; ++i) {
      const BoundKind kd = bound_kind(l[i], u[i]);
      s.add(kd, v[i], l[i], u[i]);
      pairs[i] = slack_pair(kd, v[i], l[i], u[i], bad);
    }
    out[4 * p] = s.value(); out[4 * p + 1] = s.slk; out[4 * p + 2] = s.sexp; out[4 * p + 3] = s.bad == bad ? s.bad : -1;
  }
}
