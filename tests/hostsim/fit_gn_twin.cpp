// fit_gn_twin.cpp -- TEST-ONLY host build of the Gauss-Newton fit (myriad_amd/csrc/fit_gn.h): the very FitGnLane<Sys> the device kernel runs,
// looped over a batch, and the rollout that makes noise-free data for it.  Compiled by tests/fit_gn_cases.py with g++ -O2 -std=c++17; never
// loaded by the package.
#include "../../myriad_amd/csrc/fit_gn.h"
#include "../../myriad_amd/csrc/rollout.h"

using namespace myriad;

#define FIT_GN_TWIN_SYSTEMS(X)                                                                               \
  X(CARTPOLE) X(VANDERPOL) X(CANCERTREATMENT) X(SIMPLECASE) X(BIOREACTOR) X(GLUCOSE) X(MOULDFUNGICIDE)       \
  X(SIMPLECASEWITHBOUNDS) X(HIVTREATMENT) X(EPIDEMICSEIRN) X(SEIR) X(BEARPOPULATIONS) X(PENDULUM)            \
  X(MOUNTAINCAR) X(ROCKETLANDING) X(BACTERIA) X(TUMOUR) X(HARVEST) X(TIMBERHARVEST) X(PREDATORPREY)

template <class Sys>
static int run(int method, int B, int S, double T, int u_rows, const double* xs_obs, const double* us, const double* wt,
               const double* params, int pstride, double* loss, double* grad, double* gn) {
  static_assert(SysDp<Sys>::SUPPORTED, "no parameter derivatives for this system");
  using L = FitGnLane<Sys>;
  for (long b = 0; b < B; ++b) {
    SysParams<Sys> pp;
    pp.load(params, b, pstride);
    double gp[L::NP], gu[L::NT];
    const double l = L::run(method, S, T / S, u_rows, xs_obs + b * (long)(S + 1) * Sys::NS, us + b * (long)u_rows * Sys::NU, wt, pp.get(), gp, gu,
                            grad != nullptr);
    if (loss) loss[b] = l;
    if (grad)
      for (int k = 0; k < L::NP; ++k) grad[b * L::NP + k] = gp[k];
    L::mirror(gu, gn + b * (long)L::NP * L::NP);
  }
  return 0;
}

template <class Sys>
static int roll(int method, int B, int S, double T, int u_rows, const double* x0, const double* us, const double* params, int pstride, double* xs) {
  for (long b = 0; b < B; ++b) {
    SysParams<Sys> pp;
    pp.load(params, b, pstride);
    Rollout<Sys>::run(method, S, T / S, u_rows, x0 + b * Sys::NS, us + b * (long)u_rows * Sys::NU, pp.get(), xs + b * (long)(S + 1) * Sys::NS);
  }
  return 0;
}

// loss [B] (or null), grad [B][np] (or null), gn [B][np][np]; params [np] (params_stride 0), [B][np] or null (the defaults); returns 0, or -1 for a
// system id without a specialisation
extern "C" int fit_gn_twin(int system_id, int method, int B, int num_steps, double T, int u_rows, const double* xs_obs, const double* us,
                           const double* wt, const double* params, int params_stride, double* loss, double* grad, double* gn) {
  switch (system_id) {
#define X(N) case Sys##N::ID: return run<Sys##N>(method, B, num_steps, T, u_rows, xs_obs, us, wt, params, params_stride, loss, grad, gn);
    FIT_GN_TWIN_SYSTEMS(X)
#undef X
  }
  return -1;
}

// xs [B][num_steps+1][ns]: Rollout<Sys>::run from x0 [B][ns] -- the states FitGnLane advances through, to the bit
extern "C" int fit_gn_twin_rollout(int system_id, int method, int B, int num_steps, double T, int u_rows, const double* x0, const double* us,
                                   const double* params, int params_stride, double* xs) {
  switch (system_id) {
#define X(N) case Sys##N::ID: return roll<Sys##N>(method, B, num_steps, T, u_rows, x0, us, params, params_stride, xs);
    FIT_GN_TWIN_SYSTEMS(X)
#undef X
  }
  return -1;
}
