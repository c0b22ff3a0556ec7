// shoot_exgd_grad_twin.cpp -- TEST-ONLY host build of the derivative of the unrolled extragradient steps under SHOOTING
// (myriad_amd/csrc/shoot_exgd_grad.h): the pair algebra the device kernels run (ShootHvp<Sys, M>::interval<true>, ShootExgdGrad<Sys, M>) in the
// sequence of shoot_exgd_grad_host, looped over a batch.  Compiled by tests/shoot_exgd_grad_cases.py with g++ -O2 -std=c++17; never loaded by the
// package.
#include <vector>
#include "../../myriad_amd/csrc/shoot_exgd_grad.h"

using namespace myriad;

#define SHOOT_EXGD_GRAD_TWIN_SYSTEMS(X)                                                                      \
  X(CARTPOLE) X(VANDERPOL) X(CANCERTREATMENT) X(SIMPLECASE) X(BIOREACTOR) X(GLUCOSE) X(MOULDFUNGICIDE)       \
  X(SIMPLECASEWITHBOUNDS) X(HIVTREATMENT) X(EPIDEMICSEIRN) X(SEIR) X(BEARPOPULATIONS) X(PENDULUM)            \
  X(MOUNTAINCAR) X(ROCKETLANDING) X(BACTERIA) X(TUMOUR) X(HARVEST) X(TIMBERHARVEST) X(PREDATORPREY)

template <class Sys, int M>
static int run(int method, int B, int I, int cpi, double T, const double* z, const double* lam, const double* lb, const double* ub,
               const double* params, int pstride, double eta_x, double eta_v, int nsteps, const double* seed_z, const double* seed_lam, int fused,
               double* grad, double* dz0, double* dlam0) {
  static_assert(SysDpw<Sys>::SUPPORTED, "no mixed derivatives for this system");
  using G = ShootExgdGrad<Sys, M>;
  using H = ShootHvp<Sys, M>;
  const long n = G::nvars(I, cpi), m = (long)I * Sys::NS;
  std::vector<double> hist((size_t)G::hist_doubles(I, cpi, nsteps));
  std::vector<double> work((size_t)(5 * n + 2 * m + (long)(cpi + 1) * Sys::NS + (long)I * (Sys::NS + H::hist_doubles(cpi) + H::side_doubles(cpi))));
  for (long b = 0; b < B; ++b) {
    SysParams<Sys> pp;
    pp.load(params, b, pstride);
    shoot_exgd_grad_host<Sys, M>(method, I, cpi, T, z + b * n, lam + b * m, lb + b * n, ub + b * n, pp.get(), eta_x, eta_v, nsteps, seed_z + b * n,
                                 seed_lam ? seed_lam + b * m : nullptr, hist.data(), work.data(), grad + b * Sys::NP, dz0 ? dz0 + b * n : nullptr,
                                 dlam0 ? dlam0 + b * m : nullptr, fused != 0);
  }
  return 0;
}

// method: 0 Euler, 1 Heun, 2 midpoint, 3 RK4.  grad [B][np]; params [np] (params_stride 0) or [B][np]; seed_lam, dz0, dlam0 may be null.
// fused: 1 the schedule of the device (2 nsteps + 1 passes), 0 items 1 .. 5 as three passes a step.  Returns 0, or -1 for a system id without a
// specialisation or another method.
extern "C" int shoot_exgd_grad_twin(int system_id, int method, int B, int I, int cpi, double T, const double* z, const double* lam, const double* lb,
                                    const double* ub, const double* params, int params_stride, double eta_x, double eta_v, int nsteps,
                                    const double* seed_z, const double* seed_lam, int fused, double* grad, double* dz0, double* dlam0) {
  if (method < 0 || method > 3) return -1;
  switch (system_id) {
#define X(S)                                                                                                                                          \
  case Sys##S::ID:                                                                                                                                    \
    return method == 3 ? run<Sys##S, 2>(method, B, I, cpi, T, z, lam, lb, ub, params, params_stride, eta_x, eta_v, nsteps, seed_z, seed_lam, fused,   \
                                        grad, dz0, dlam0)                                                                                             \
                       : run<Sys##S, 1>(method, B, I, cpi, T, z, lam, lb, ub, params, params_stride, eta_x, eta_v, nsteps, seed_z, seed_lam, fused,   \
                                        grad, dz0, dlam0);
    SHOOT_EXGD_GRAD_TWIN_SYSTEMS(X)
#undef X
  }
  return -1;
}
