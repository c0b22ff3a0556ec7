// hvp_twin.cpp -- TEST-ONLY host build of the Lagrangian Hessian-vector product (myriad_amd/csrc/shoot_hvp.h, colloc_hvp.h): the algebra the device
// kernels run (ShootHvp<Sys, M>, CollocHvp<Sys, SCHEME>) in the sequence of shoot_hvp_host / colloc_hvp_host, looped over a batch.  Compiled by
// tests/hvp_cases.py with g++ -O2 -std=c++17 (and, with a main of its own, by hvp_check.cpp); never loaded by the package.
#include <vector>
#include "../../myriad_amd/csrc/colloc_hvp.h"
#include "../../myriad_amd/csrc/shoot_hvp.h"
#include "../../myriad_amd/csrc/os_solver.h"

using namespace myriad;

#define HVP_TWIN_SYSTEMS(X)                                                                                  \
  X(CARTPOLE) X(VANDERPOL) X(CANCERTREATMENT) X(SIMPLECASE) X(BIOREACTOR) X(GLUCOSE) X(MOULDFUNGICIDE)       \
  X(SIMPLECASEWITHBOUNDS) X(HIVTREATMENT) X(EPIDEMICSEIRN) X(SEIR) X(BEARPOPULATIONS) X(PENDULUM)            \
  X(MOUNTAINCAR) X(ROCKETLANDING) X(BACTERIA) X(TUMOUR) X(HARVEST) X(TIMBERHARVEST) X(PREDATORPREY)

template <class Sys, int SCHEME>
static int run_colloc(int B, int N, double T, const double* z, const double* lam, const double* v, const double* params, int pstride, int with_cost,
                      double* oz, double* op) {
  using G = ExgdGradPoint<Sys, SCHEME>;
  const long n = (long)G::points(N) * Sys::NW, m = G::rows(N);
  for (long b = 0; b < B; ++b) {
    SysParams<Sys> pp;
    pp.load(params, b, pstride);
    colloc_hvp_host<Sys, SCHEME>(N, T / N, z + b * n, lam ? lam + b * m : nullptr, v + b * n, pp.get(), with_cost, oz ? oz + b * n : nullptr,
                                 op ? op + b * Sys::NP : nullptr);
  }
  return 0;
}

template <class Sys, int M>
static int run_shoot(int method, int B, int I, int cpi, double T, const double* z, const double* lam, const double* v, const double* params,
                     int pstride, int with_cost, double* oz, double* op) {
  using H = ShootHvp<Sys, M>;
  const long n = (long)(I + 1) * Sys::NS + ((long)M * I * cpi + 1) * Sys::NU, m = (long)I * Sys::NS;
  std::vector<double> work((size_t)I * (size_t)(H::hist_doubles(cpi) + H::side_doubles(cpi)));
  for (long b = 0; b < B; ++b) {
    SysParams<Sys> pp;
    pp.load(params, b, pstride);
    shoot_hvp_host<Sys, M>(method, I, cpi, T, z + b * n, lam ? lam + b * m : nullptr, v + b * n, pp.get(), with_cost, work.data(),
                           oz ? oz + b * n : nullptr, op ? op + b * Sys::NP : nullptr);
  }
  return 0;
}

template <class Sys>
static int run(int tr, int method, int B, int N, int cpi, double T, const double* z, const double* lam, const double* v, const double* params,
               int pstride, int with_cost, double* oz, double* op) {
  static_assert(SysDpw<Sys>::SUPPORTED, "no mixed derivatives for this system");
  if (tr == 0) return run_colloc<Sys, EXGD_GRAD_HS>(B, N, T, z, lam, v, params, pstride, with_cost, oz, op);
  if (tr == 1) return run_colloc<Sys, EXGD_GRAD_TRAP>(B, N, T, z, lam, v, params, pstride, with_cost, oz, op);
  if (tr != 2 || method < 0 || method > 3) return -1;
  return method == 3 ? run_shoot<Sys, 2>(method, B, N, cpi, T, z, lam, v, params, pstride, with_cost, oz, op)
                     : run_shoot<Sys, 1>(method, B, N, cpi, T, z, lam, v, params, pstride, with_cost, oz, op);
}

// transcription: 0 Hermite-Simpson, 1 trapezoidal, 2 shooting (N = intervals; method 0 Euler, 1 Heun, 2 midpoint, 3 RK4).  out_z [B][n], out_p [B][np]
// (either may be null); lam may be null; params [np] (params_stride 0) or [B][np].  Returns 0, or -1 for an id or a transcription it does not have.
extern "C" int hvp_twin(int system_id, int transcription, int method, int B, int N, int cpi, double T, const double* z, const double* lam,
                        const double* v, const double* params, int params_stride, int with_cost, double* out_z, double* out_p) {
  switch (system_id) {
#define X(S) case Sys##S::ID: return run<Sys##S>(transcription, method, B, N, cpi, T, z, lam, v, params, params_stride, with_cost, out_z, out_p);
    HVP_TWIN_SYSTEMS(X)
#undef X
  }
  return -1;
}

// One step two ways.  y = (x, the step's M + 1 control rows), yd its tangent, a the costate of x+:
//   hs[NY]   = Hs yd, Hs the solver's own step Hessian d2 (dc + a^T x+) / dy2 (ShootCore::slin with pin = a);
//   rule[NY] = what ShootHvp::step_back hands back as second-order cotangent for ad = 0 (the state part, then the control rows).
template <class Sys, int M>
static int step_two_ways(int method, double h, double t0, const double* y, const double* yd, const double* params, const double* a, double* hs,
                         double* rule) {
  using SC = ShootCore<Sys, M>;
  using H = ShootHvp<Sys, M>;
  constexpr int NS = Sys::NS, NU = Sys::NU, NY = SC::NY;
  static_assert(NY == NS + (M + 1) * NU, "y = (x, M + 1 control rows)");
  SysParams<Sys> pp;
  pp.load(params, 0, 0);
  double Fy[NS * NY], gy[NY], Hs[NY * NY];
  SC::slin(method, h, y, y + NS, pp.get(), a, Fy, gy, Hs, t0, false);
  for (int r = 0; r < NY; ++r) {
    double s = 0.0;
    for (int c = 0; c < NY; ++c) s += Hs[r * NY + c] * yd[c];
    hs[r] = s;
  }
  double aa[NS], ad[NS], ub[(M + 1) * NU], gp[Sys::NP];
  for (int q = 0; q < NS; ++q) { aa[q] = a[q]; ad[q] = 0.0; }
  for (int c = 0; c < (M + 1) * NU; ++c) ub[c] = 0.0;
  for (int k = 0; k < Sys::NP; ++k) gp[k] = 0.0;
  H::step_back(method, h, t0, y, yd, y + NS, yd + NS, pp.get(), 1.0, aa, ad, ub, gp);
  for (int q = 0; q < NS; ++q) rule[q] = ad[q];
  for (int c = 0; c < (M + 1) * NU; ++c) rule[NS + c] = ub[c];
  return NY;
}

// returns NY (the length of y), or -1
extern "C" int hvp_step_two_ways(int system_id, int method, double h, double t0, const double* y, const double* yd, const double* params,
                                 const double* a, double* hs, double* rule) {
  if (method < 0 || method > 3) return -1;
  switch (system_id) {
#define X(S)                                                                                                            \
  case Sys##S::ID:                                                                                                      \
    return method == 3 ? step_two_ways<Sys##S, 2>(method, h, t0, y, yd, params, a, hs, rule)                            \
                       : step_two_ways<Sys##S, 1>(method, h, t0, y, yd, params, a, hs, rule);
    HVP_TWIN_SYSTEMS(X)
#undef X
  }
  return -1;
}
