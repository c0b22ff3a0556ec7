// node_shoot_products_twin.cpp -- TEST-ONLY host build of the Lagrangian products and extragradient steps of the SHOOTING transcription with the
// network as the dynamics (myriad_amd/csrc/node_shoot_products.h): the pair algebra the device kernel runs (NodeShootProd<Sys, M>), with the
// network evaluated by SysNODE::lin / f in plain loops, looped over a batch.  Compiled by tests/node_shoot_products_cases.py with g++ -O2
// -std=c++17; never loaded by the package.
#include <vector>
#include "../../myriad_amd/csrc/node_shoot_products.h"
#include "../../myriad_amd/csrc/node_system.h"

using namespace myriad;
using Sys = SysNODE_CARTPOLE;

template <int M>
static int run(int op, int method, int B, int I, int cpi, double T, const double* z, const double* w, const double* params, int pstride, int add_gradf,
               double* out, double* zio, double* lamio, const double* lb, const double* ub, double eta_x, double eta_v, int nsteps) {
  using P = NodeShootProd<Sys, M>;
  const long n = P::nvars(I, cpi), m = (long)I * Sys::NS;
  std::vector<double> work((size_t)(2 * n + P::pair_doubles(cpi) + (long)I * Sys::NU));
  double* scratch = work.data() + 2 * n; double* edge = scratch + P::pair_doubles(cpi);
  for (long b = 0; b < B; ++b) {
    const double* p = params + b * (long)pstride;
    if (op == 0) node_shoot_grad_host<Sys, M>(method, I, cpi, T, z + b * n, w + b * m, p, add_gradf ? 1.0 : 0.0, scratch, edge, out + b * n);
    else if (op == 1) node_shoot_jvp_host<Sys, M>(method, I, cpi, T, z + b * n, w + b * n, p, out + b * m);
    else node_shoot_exgd_host<Sys, M>(method, I, cpi, T, zio + b * n, lamio + b * m, lb + b * n, ub + b * n, p, eta_x, eta_v, nsteps, work.data());
  }
  return 0;
}

// method: 0 Euler, 1 Heun, 2 midpoint, 3 RK4.  params [np] (params_stride 0) or [B][np].  Returns 0, or -1 for another method.
extern "C" int node_shoot_vjp_twin(int method, int B, int I, int cpi, double T, const double* z, const double* lam, const double* params, int params_stride,
                                   int add_gradf, double* out) {
  if (method < 0 || method > 3) return -1;
  return method == 3 ? run<2>(0, method, B, I, cpi, T, z, lam, params, params_stride, add_gradf, out, nullptr, nullptr, nullptr, nullptr, 0, 0, 0)
                     : run<1>(0, method, B, I, cpi, T, z, lam, params, params_stride, add_gradf, out, nullptr, nullptr, nullptr, nullptr, 0, 0, 0);
}
extern "C" int node_shoot_jvp_twin(int method, int B, int I, int cpi, double T, const double* z, const double* v, const double* params, int params_stride,
                                   double* out) {
  if (method < 0 || method > 3) return -1;
  return method == 3 ? run<2>(1, method, B, I, cpi, T, z, v, params, params_stride, 0, out, nullptr, nullptr, nullptr, nullptr, 0, 0, 0)
                     : run<1>(1, method, B, I, cpi, T, z, v, params, params_stride, 0, out, nullptr, nullptr, nullptr, nullptr, 0, 0, 0);
}
extern "C" int node_shoot_exgd_twin(int method, int B, int I, int cpi, double T, double* z, double* lam, const double* lb, const double* ub,
                                    const double* params, int params_stride, double eta_x, double eta_v, int nsteps) {
  if (method < 0 || method > 3 || nsteps < 0) return -1;
  return method == 3 ? run<2>(2, method, B, I, cpi, T, nullptr, nullptr, params, params_stride, 0, nullptr, z, lam, lb, ub, eta_x, eta_v, nsteps)
                     : run<1>(2, method, B, I, cpi, T, nullptr, nullptr, params, params_stride, 0, nullptr, z, lam, lb, ub, eta_x, eta_v, nsteps);
}
