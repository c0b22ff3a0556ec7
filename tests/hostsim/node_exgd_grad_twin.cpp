// node_exgd_grad_twin.cpp -- TEST-ONLY host build of the derivative of the unrolled extragradient steps in the network weights
// (myriad_amd/csrc/node_exgd_grad.h): NodeExgdHost's plain loops in the sequence of node_exgd_grad_host, looped over a batch.  Compiled by
// tests/node_exgd_grad_cases.py with g++ -O2 -std=c++17; never loaded by the package.
#include <vector>
#include "../../myriad_amd/csrc/node_exgd_grad.h"

using namespace myriad;

// Hermite-Simpson; params: the NP shared weights; grad [B][NP]; seed_lam, dz0, dlam0 may be null.  Returns NP.
extern "C" int node_exgd_grad_twin(int B, int N, double T, const double* z, const double* lam, const double* lb, const double* ub,
                                   const double* params, double eta_x, double eta_v, int nsteps, const double* seed_z, const double* seed_lam,
                                   double* grad, double* dz0, double* dlam0) {
  using G = NodeExgdHost::G;
  const int K = G::points(N), n = K * NodeExgdHost::NW, m = G::rows(N);
  std::vector<double> hist((size_t)G::hist_doubles(N, nsteps)), work((size_t)3 * n + 2 * m + (size_t)K * NodeExgdHost::NS);
  for (long b = 0; b < B; ++b)
    node_exgd_grad_host(N, T / N, z + b * n, lam + b * m, lb + b * n, ub + b * n, params, eta_x, eta_v, nsteps, seed_z + b * n,
                        seed_lam ? seed_lam + b * m : nullptr, hist.data(), work.data(), grad + b * NodeExgdHost::NP, dz0 ? dz0 + b * n : nullptr,
                        dlam0 ? dlam0 + b * m : nullptr);
  return NodeExgdHost::NP;
}
