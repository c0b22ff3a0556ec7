// node_shoot_products_check.cpp -- TEST-ONLY stand-alone program (its own main) over the host build of myriad_amd/csrc/node_shoot_products.h, for
// AddressSanitizer / UBSan: compiled with -fsanitize=address,undefined and run directly by tests/test_node_shoot_products_host_twin.py.  Every
// buffer is allocated at exactly the size the header documents, so that an index past a row, a pair's scratch or the shared-row slots is caught.
// Two small shapes, weights from a fixed generator; checked: <J v, lam> == <v, J^T lam>, two extragradient steps == one + one, finite results.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../myriad_amd/csrc/node_shoot_products.h"
#include "../../myriad_amd/csrc/node_system.h"

using namespace myriad;
using Sys = SysNODE_CARTPOLE;

static unsigned long long g_state = 0x9e3779b97f4a7c15ULL;
static double rnd() {      // uniform in (-1, 1)
  g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(g_state >> 11) / 4503599627370496.0 - 1.0;
}

template <int M>
static int check(const char* name, int method, int I, int cpi) {
  using P = NodeShootProd<Sys, M>;
  const long n = P::nvars(I, cpi), m = (long)I * Sys::NS;
  const double T = 1.0;
  std::vector<double> p(Sys::NP), z(n), lam(m), v(n), g(n), jv(m), scratch(P::pair_doubles(cpi)), edge((size_t)I * Sys::NU);
  for (double& w : p) w = 0.3 * rnd();
  for (double& w : z) w = 0.5 * rnd();
  for (double& w : lam) w = rnd();
  for (double& w : v) w = rnd();
  node_shoot_grad_host<Sys, M>(method, I, cpi, T, z.data(), lam.data(), p.data(), 0.0, scratch.data(), edge.data(), g.data());
  node_shoot_jvp_host<Sys, M>(method, I, cpi, T, z.data(), v.data(), p.data(), jv.data());
  double lhs = 0.0, rhs = 0.0;
  for (long i = 0; i < m; ++i) lhs += jv[i] * lam[i];
  for (long i = 0; i < n; ++i) rhs += v[i] * g[i];
  bool ok = std::isfinite(lhs) && std::fabs(lhs - rhs) <= 1e-10 * std::fabs(lhs);
  // two steps == one + one, with a box that clips
  std::vector<double> lb(n), ub(n), z2(z), l2(lam), z11(z), l11(lam), work((size_t)(2 * n + P::pair_doubles(cpi) + (long)I * Sys::NU));
  for (long i = 0; i < n; ++i) { lb[i] = z[i] - 1e-3; ub[i] = z[i] + 1e-3; }
  node_shoot_exgd_host<Sys, M>(method, I, cpi, T, z2.data(), l2.data(), lb.data(), ub.data(), p.data(), 1e-2, 1e-3, 2, work.data());
  for (int s = 0; s < 2; ++s)
    node_shoot_exgd_host<Sys, M>(method, I, cpi, T, z11.data(), l11.data(), lb.data(), ub.data(), p.data(), 1e-2, 1e-3, 1, work.data());
  long clipped = 0;
  for (long i = 0; i < n; ++i) { ok = ok && std::isfinite(z2[i]) && z2[i] == z11[i]; clipped += (z2[i] == lb[i] || z2[i] == ub[i]); }
  for (long i = 0; i < m; ++i) ok = ok && std::isfinite(l2[i]) && l2[i] == l11[i];
  ok = ok && clipped > 0;
  std::printf("%s I=%d cpi=%d: <Jv,lam> %.17g <v,JTlam> %.17g clipped %ld: %s\n", name, I, cpi, lhs, rhs, clipped, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  bad += check<1>("HEUN", 1, 3, 2);
  bad += check<2>("RK4", 3, 2, 3);
  return bad;
}
