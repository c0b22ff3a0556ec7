// hvp_check.cpp -- TEST-ONLY stand-alone program: the host twin of the Lagrangian Hessian-vector product (hvp_twin.cpp, which runs
// myriad_amd/csrc/colloc_hvp.h and shoot_hvp.h) under the host sanitizers.  tests/test_hvp_host_twin.py compiles it with
// -fsanitize=address,undefined and runs it directly.  Two systems per transcription, B = 2: CARTPOLE and BACTERIA under Hermite-Simpson (N = 33 / 3),
// the trapezoidal rule (N = 65 / 5, terminal cost) and shooting (7 x 3 RK4 / 3 x 2 Heun, terminal cost; CARTPOLE also 1 x 1 Euler, every row shared).
// Exits 0 when every result is finite, v = 0 gives exact zeros and a null lam equals a zero lam bit for bit.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "hvp_twin.cpp"

static double unit(unsigned long long& s) {      // splitmix64 -> [0, 1)
  s += 0x9e3779b97f4a7c15ULL;
  unsigned long long z = s;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  z ^= z >> 31;
  return (double)(z >> 11) / 9007199254740992.0;
}

static int one(const char* what, int system_id, int tr, int method, int ns, int nu, int np, int N, int cpi, double T, double x0) {
  const int B = 2, M = method == 3 ? 2 : 1;
  const int xr = tr == 2 ? N + 1 : (tr == 0 ? 2 * N + 1 : N + 1), ur = tr == 2 ? M * N * cpi + 1 : xr;
  const int n = xr * ns + ur * nu, m = tr == 2 ? N * ns : (tr == 0 ? 2 : 1) * N * ns;
  unsigned long long s = 4321 + 1000 * system_id + 10 * N + tr;
  std::vector<double> z((size_t)B * n), v((size_t)B * n), zero((size_t)B * n, 0.0), lam((size_t)B * m), lam0((size_t)B * m, 0.0);
  std::vector<double> oz((size_t)B * n), op((size_t)B * np), oz2((size_t)B * n), op2((size_t)B * np);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < n; ++i) {
      z[(size_t)b * n + i] = (i < xr * ns ? x0 : 0.3) + 0.1 * (unit(s) - 0.5);
      v[(size_t)b * n + i] = unit(s) - 0.5;
    }
  for (double& l : lam) l = 0.2 * (unit(s) - 0.5);
  int bad = 0;
  for (int wc = 0; wc < 2; ++wc) {
    if (hvp_twin(system_id, tr, method, B, N, cpi, T, z.data(), lam.data(), v.data(), nullptr, 0, wc, oz.data(), op.data())) {
      printf("%s: no specialisation\n", what);
      return 1;
    }
    for (double x : oz) bad += !isfinite(x);
    for (double x : op) bad += !isfinite(x);
    hvp_twin(system_id, tr, method, B, N, cpi, T, z.data(), lam.data(), zero.data(), nullptr, 0, wc, oz.data(), op.data());
    for (double x : oz) bad += x != 0.0;
    for (double x : op) bad += x != 0.0;
    hvp_twin(system_id, tr, method, B, N, cpi, T, z.data(), nullptr, v.data(), nullptr, 0, wc, oz.data(), op.data());
    hvp_twin(system_id, tr, method, B, N, cpi, T, z.data(), lam0.data(), v.data(), nullptr, 0, wc, oz2.data(), op2.data());
    bad += memcmp(oz.data(), oz2.data(), oz.size() * 8) != 0 || memcmp(op.data(), op2.data(), op.size() * 8) != 0;
    hvp_twin(system_id, tr, method, B, N, cpi, T, z.data(), lam.data(), v.data(), nullptr, 0, wc, nullptr, op2.data());      // one output alone
    hvp_twin(system_id, tr, method, B, N, cpi, T, z.data(), lam.data(), v.data(), nullptr, 0, wc, oz2.data(), nullptr);
  }
  printf("%s: %s\n", what, bad ? "FAILED" : "ok");
  return bad != 0;
}

int main() {
  using C = SysCARTPOLE;
  using K = SysBACTERIA;
  int rc = 0;
  rc |= one("CARTPOLE Hermite-Simpson N=33", C::ID, 0, 1, C::NS, C::NU, C::NP, 33, 1, 1.65, 0.2);
  rc |= one("BACTERIA Hermite-Simpson N=3", K::ID, 0, 1, K::NS, K::NU, K::NP, 3, 1, 0.15, 1.0);
  rc |= one("CARTPOLE trapezoidal N=65", C::ID, 1, 1, C::NS, C::NU, C::NP, 65, 1, 2.0, 0.2);
  rc |= one("BACTERIA trapezoidal N=5", K::ID, 1, 1, K::NS, K::NU, K::NP, 5, 1, 0.25, 1.0);
  rc |= one("CARTPOLE shooting 7x3 RK4", C::ID, 2, 3, C::NS, C::NU, C::NP, 7, 3, 1.05, 0.2);
  rc |= one("CARTPOLE shooting 1x1 Euler", C::ID, 2, 0, C::NS, C::NU, C::NP, 1, 1, 0.05, 0.2);
  rc |= one("BACTERIA shooting 3x2 Heun", K::ID, 2, 1, K::NS, K::NU, K::NP, 3, 2, 0.3, 1.0);
  return rc;
}
