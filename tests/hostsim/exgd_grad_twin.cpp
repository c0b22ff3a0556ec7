// exgd_grad_twin.cpp -- TEST-ONLY host build of the derivative of the unrolled extragradient steps (myriad_amd/csrc/exgd_grad.h): the point
// algebra the device kernel runs (ExgdGradPoint<Sys, SCHEME>) in the sequence of exgd_grad_host, looped over a batch.  Compiled by
// tests/exgd_grad_cases.py with g++ -O2 -std=c++17 (and, with a main of its own, by exgd_grad_check.cpp); never loaded by the package.
#include <vector>
#include "../../myriad_amd/csrc/exgd_grad.h"

using namespace myriad;

#define EXGD_GRAD_TWIN_SYSTEMS(X)                                                                            \
  X(CARTPOLE) X(VANDERPOL) X(CANCERTREATMENT) X(SIMPLECASE) X(BIOREACTOR) X(GLUCOSE) X(MOULDFUNGICIDE)       \
  X(SIMPLECASEWITHBOUNDS) X(HIVTREATMENT) X(EPIDEMICSEIRN) X(SEIR) X(BEARPOPULATIONS) X(PENDULUM)            \
  X(MOUNTAINCAR) X(ROCKETLANDING) X(BACTERIA) X(TUMOUR) X(HARVEST) X(TIMBERHARVEST) X(PREDATORPREY)

template <class Sys, int SCHEME>
static int run(int B, int N, double T, const double* z, const double* lam, const double* lb, const double* ub, const double* params, int pstride,
               double eta_x, double eta_v, int nsteps, const double* seed_z, const double* seed_lam, double* grad, double* dz0, double* dlam0) {
  static_assert(SysDpw<Sys>::SUPPORTED, "no mixed derivatives for this system");
  using G = ExgdGradPoint<Sys, SCHEME>;
  const int K = G::points(N), n = K * Sys::NW, m = G::rows(N);
  std::vector<double> hist((size_t)G::hist_doubles(N, nsteps)), work((size_t)3 * n + 2 * m + (size_t)K * Sys::NS);
  for (long b = 0; b < B; ++b) {
    SysParams<Sys> pp;
    pp.load(params, b, pstride);
    exgd_grad_host<Sys, SCHEME>(N, T / N, z + b * n, lam + b * m, lb + b * n, ub + b * n, pp.get(), eta_x, eta_v, nsteps, seed_z + b * n,
                                seed_lam ? seed_lam + b * m : nullptr, hist.data(), work.data(), grad + b * Sys::NP, dz0 ? dz0 + b * n : nullptr,
                                dlam0 ? dlam0 + b * m : nullptr);
  }
  return 0;
}

// scheme: 0 Hermite-Simpson, 1 trapezoidal.  grad [B][np]; params [np] (params_stride 0) or [B][np]; seed_lam, dz0, dlam0 may be null.
// Returns 0, or -1 for a system id without a specialisation or another scheme.
extern "C" int exgd_grad_twin(int system_id, int scheme, int B, int N, double T, const double* z, const double* lam, const double* lb,
                              const double* ub, const double* params, int params_stride, double eta_x, double eta_v, int nsteps,
                              const double* seed_z, const double* seed_lam, double* grad, double* dz0, double* dlam0) {
  if (scheme != 0 && scheme != 1) return -1;
  switch (system_id) {
#define X(S)                                                                                                                                      \
  case Sys##S::ID:                                                                                                                                \
    return scheme == 0 ? run<Sys##S, EXGD_GRAD_HS>(B, N, T, z, lam, lb, ub, params, params_stride, eta_x, eta_v, nsteps, seed_z, seed_lam, grad, dz0, dlam0) \
                       : run<Sys##S, EXGD_GRAD_TRAP>(B, N, T, z, lam, lb, ub, params, params_stride, eta_x, eta_v, nsteps, seed_z, seed_lam, grad, dz0, dlam0);
    EXGD_GRAD_TWIN_SYSTEMS(X)
#undef X
  }
  return -1;
}

// One evaluation of the generated mixed derivatives (systems_dpw_gen.h) at a point: which = 0 vjp_p_dir (gp[np]), which = 1 term_vjp_p_dir
// (systems with a terminal cost; others return -1).  params [np]; t: the point's time; unit variable scales.
template <class Sys>
static int dpw_one(int which, const double* x, const double* u, const double* params, double t, const double* mu, double wg, const double* d,
                   double* gp) {
  SysParams<Sys> pp;
  pp.load(params, 0, 0);
  set_time<Sys>(pp.get(), t);
  if (which == 0) { SysDpw<Sys>::vjp_p_dir(x, u, pp.get(), mu, wg, d, gp); return 0; }
  if constexpr (Sys::HAS_TERMINAL) { SysDpw<Sys>::term_vjp_p_dir(x, u, pp.get(), d, gp); return 0; }
  return -1;
}

extern "C" int dpw_point(int system_id, int which, const double* x, const double* u, const double* params, double t, const double* mu, double wg,
                         const double* d, double* gp) {
  switch (system_id) {
#define X(S) case Sys##S::ID: return dpw_one<Sys##S>(which, x, u, params, t, mu, wg, d, gp);
    EXGD_GRAD_TWIN_SYSTEMS(X)
#undef X
  }
  return -1;
}
