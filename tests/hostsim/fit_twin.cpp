// fit_twin.cpp -- TEST-ONLY host build of the trajectory-matching loss and gradient (myriad_amd/csrc/fit.h): the very FitLane<Sys> the
// device kernel runs, looped over a batch.  Compiled by tests/test_fit_host_twin.py with g++ -O2 -std=c++17; never loaded by the package.
#include <vector>
#include "../../myriad_amd/csrc/fit.h"

using namespace myriad;

#define FIT_TWIN_SYSTEMS(X)                                                                                  \
  X(CARTPOLE) X(VANDERPOL) X(CANCERTREATMENT) X(SIMPLECASE) X(BIOREACTOR) X(GLUCOSE) X(MOULDFUNGICIDE)       \
  X(SIMPLECASEWITHBOUNDS) X(HIVTREATMENT) X(EPIDEMICSEIRN) X(SEIR) X(BEARPOPULATIONS) X(PENDULUM)            \
  X(MOUNTAINCAR) X(ROCKETLANDING) X(BACTERIA) X(TUMOUR) X(HARVEST) X(TIMBERHARVEST) X(PREDATORPREY)

template <class Sys>
static int run(int method, int B, int S, double T, int u_rows, const double* xs_obs, const double* us, const double* wt,
               const double* params, int pstride, double* loss, double* grad) {
  static_assert(SysDp<Sys>::SUPPORTED, "no parameter derivatives for this system");
  std::vector<double> xh((size_t)(S + 1) * Sys::NS);
  for (long b = 0; b < B; ++b) {
    SysParams<Sys> pp;
    pp.load(params, b, pstride);
    const double l = FitLane<Sys>::run(method, S, T / S, u_rows, xs_obs + b * (long)(S + 1) * Sys::NS, us + b * (long)u_rows * Sys::NU, wt,
                                       pp.get(), xh.data(), 1, grad + b * Sys::NP);
    if (loss) loss[b] = l;
  }
  return 0;
}

// loss [B], grad [B][np]; params [np] (params_stride 0) or [B][np]; returns 0, or -1 for a system id without a specialisation
extern "C" int fit_twin(int system_id, int method, int B, int num_steps, double T, int u_rows, const double* xs_obs, const double* us,
                        const double* wt, const double* params, int params_stride, double* loss, double* grad) {
  switch (system_id) {
#define X(N) case Sys##N::ID: return run<Sys##N>(method, B, num_steps, T, u_rows, xs_obs, us, wt, params, params_stride, loss, grad);
    FIT_TWIN_SYSTEMS(X)
#undef X
  }
  return -1;
}
