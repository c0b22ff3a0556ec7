// node_shoot_exgd_grad_twin.cpp -- TEST-ONLY host build of the derivative of the unrolled extragradient steps in the network weights under SHOOTING
// (myriad_amd/csrc/node_shoot_exgd_grad.h): the pair and step algebra the device kernel runs (NodeShootExgd<M>) with the network in plain loops
// (NseHostNet: NodeExgdHost::first / second, SysNODE::f / lin), in the sequence of node_shoot_exgd_grad_host, looped over a batch.  Compiled by
// tests/node_shoot_exgd_grad_cases.py with g++ -O2 -std=c++17; never loaded by the package.
#include <vector>
#include "../../myriad_amd/csrc/node_shoot_exgd_grad.h"

using namespace myriad;

template <int M>
static int run(int method, int B, int I, int cpi, double T, const double* z, const double* lam, const double* lb, const double* ub,
               const double* params, double eta_x, double eta_v, int nsteps, const double* seed_z, const double* seed_lam, int fused, double* grad,
               double* dz0, double* dlam0) {
  using A = NodeShootExgd<M>;
  const long n = A::nvars(I, cpi), m = (long)I * A::NS;
  std::vector<double> hist((size_t)A::hist_doubles(I, cpi, nsteps));
  std::vector<double> work((size_t)(A::work_doubles(I, cpi) + n));
  for (long b = 0; b < B; ++b)
    node_shoot_exgd_grad_host<M>(method, I, cpi, T, z + b * n, lam + b * m, lb + b * n, ub + b * n, params, eta_x, eta_v, nsteps, seed_z + b * n,
                                 seed_lam ? seed_lam + b * m : nullptr, hist.data(), work.data(), grad + b * A::NP, dz0 ? dz0 + b * n : nullptr,
                                 dlam0 ? dlam0 + b * m : nullptr, fused != 0);
  return A::NP;
}

// method: 0 Euler, 1 Heun, 2 midpoint, 3 RK4.  params [4804] shared; grad [B][4804]; seed_lam, dz0, dlam0 may be null.  fused: 1 the schedule of
// the device (2 nsteps + 1 passes), 0 items 1 .. 5 as three passes a step.  Returns the number of weights, or -1 for another method.
extern "C" int node_shoot_exgd_grad_twin(int method, int B, int I, int cpi, double T, const double* z, const double* lam, const double* lb,
                                         const double* ub, const double* params, double eta_x, double eta_v, int nsteps, const double* seed_z,
                                         const double* seed_lam, int fused, double* grad, double* dz0, double* dlam0) {
  if (method < 0 || method > 3) return -1;
  return method == 3 ? run<2>(method, B, I, cpi, T, z, lam, lb, ub, params, eta_x, eta_v, nsteps, seed_z, seed_lam, fused, grad, dz0, dlam0)
                     : run<1>(method, B, I, cpi, T, z, lam, lb, ub, params, eta_x, eta_v, nsteps, seed_z, seed_lam, fused, grad, dz0, dlam0);
}
