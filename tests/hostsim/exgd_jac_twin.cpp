// exgd_jac_twin.cpp -- TEST-ONLY host build of the forward-mode Jacobian of the unrolled extragradient steps (myriad_amd/csrc/exgd_jac.h): the point
// algebra the device kernel runs (ExgdJacPoint<Sys, SCHEME> beside ExgdGradPoint) in the sequence of exgd_jac_host, looped over a batch and over the
// groups of columns.  Compiled by tests/exgd_jac_cases.py with g++ -O2 -std=c++17 (and, with a main of its own, by exgd_jac_check.cpp); never loaded
// by the package.
#include <vector>
#include "../../myriad_amd/csrc/exgd_jac.h"

using namespace myriad;

#define EXGD_JAC_TWIN_SYSTEMS(X)                                                                             \
  X(CARTPOLE) X(VANDERPOL) X(CANCERTREATMENT) X(SIMPLECASE) X(BIOREACTOR) X(GLUCOSE) X(MOULDFUNGICIDE)       \
  X(SIMPLECASEWITHBOUNDS) X(HIVTREATMENT) X(EPIDEMICSEIRN) X(SEIR) X(BEARPOPULATIONS) X(PENDULUM)            \
  X(MOUNTAINCAR) X(ROCKETLANDING) X(BACTERIA) X(TUMOUR) X(HARVEST) X(TIMBERHARVEST) X(PREDATORPREY)

template <class Sys, int SCHEME>
static int run(int B, int N, double T, const double* z, const double* lam, const double* lb, const double* ub, const double* params, int pstride,
               double eta_x, double eta_v, int nsteps, const double* jz0, const double* jlam0, int gcols, double* zn, double* lamn, double* jz,
               double* jlam) {
  static_assert(SysDpw<Sys>::SUPPORTED, "no mixed derivatives for this system");
  using Q = ExgdJacPoint<Sys, SCHEME>;
  using G = typename Q::G;
  constexpr int NP = Sys::NP;
  const int K = G::points(N), n = K * Sys::NW, m = G::rows(N);
  if (gcols < 1 || gcols > NP) gcols = NP;
  std::vector<double> work((size_t)(1 + gcols) * (size_t)Q::rec_doubles(N));
  for (long b = 0; b < B; ++b) {
    SysParams<Sys> pp;
    pp.load(params, b, pstride);
    for (int k0 = 0; k0 < NP; k0 += gcols)
      exgd_jac_host<Sys, SCHEME>(N, T / N, z + b * n, lam + b * m, lb + b * n, ub + b * n, pp.get(), eta_x, eta_v, nsteps,
                                 jz0 ? jz0 + b * NP * n : nullptr, jlam0 ? jlam0 + b * NP * m : nullptr, k0, k0 + gcols < NP ? gcols : NP - k0,
                                 work.data(), zn && k0 == 0 ? zn + b * n : nullptr, lamn && k0 == 0 ? lamn + b * m : nullptr,
                                 jz ? jz + b * NP * n : nullptr, jlam ? jlam + b * NP * m : nullptr);
  }
  return 0;
}

// scheme: 0 Hermite-Simpson, 1 trapezoidal.  jz [B][np][n], jlam [B][np][m]; params [np] (params_stride 0) or [B][np]; gcols: columns to a group
// (0: all at once).  jz0, jlam0, zn, lamn, jz, jlam may be null.  Returns 0, or -1 for a system id without a specialisation or another scheme.
extern "C" int exgd_jac_twin(int system_id, int scheme, int B, int N, double T, const double* z, const double* lam, const double* lb,
                             const double* ub, const double* params, int params_stride, double eta_x, double eta_v, int nsteps, const double* jz0,
                             const double* jlam0, int gcols, double* zn, double* lamn, double* jz, double* jlam) {
  if (scheme != 0 && scheme != 1) return -1;
  switch (system_id) {
#define X(S)                                                                                                                                       \
  case Sys##S::ID:                                                                                                                                 \
    return scheme == 0 ? run<Sys##S, EXGD_GRAD_HS>(B, N, T, z, lam, lb, ub, params, params_stride, eta_x, eta_v, nsteps, jz0, jlam0, gcols, zn,   \
                                                   lamn, jz, jlam)                                                                                 \
                       : run<Sys##S, EXGD_GRAD_TRAP>(B, N, T, z, lam, lb, ub, params, params_stride, eta_x, eta_v, nsteps, jz0, jlam0, gcols, zn, \
                                                     lamn, jz, jlam);
    EXGD_JAC_TWIN_SYSTEMS(X)
#undef X
  }
  return -1;
}
