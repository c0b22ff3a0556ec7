// exgd_grad_check.cpp -- TEST-ONLY stand-alone program: the host twin of the unrolled-extragradient derivative (exgd_grad_twin.cpp, which runs
// myriad_amd/csrc/exgd_grad.h) under the host sanitizers.  tests/test_exgd_grad_host_twin.py compiles it with -fsanitize=address,undefined and runs
// it directly.  Cases: CARTPOLE Hermite-Simpson N = 3 and N = 33, BACTERIA trapezoidal N = 5 (terminal cost); B = 2, three steps, bounds that clip.
// Exits 0 when every result is finite and dz0 / dlam0 of a zero-step call return the seeds.
#include <math.h>
#include <stdio.h>
#include <vector>
#include "exgd_grad_twin.cpp"

static double unit(unsigned long long& s) {      // splitmix64 -> [0, 1)
  s += 0x9e3779b97f4a7c15ULL;
  unsigned long long z = s;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  z ^= z >> 31;
  return (double)(z >> 11) / 9007199254740992.0;
}

static int one(const char* what, int system_id, int scheme, int ns, int nu, int np, int N, double T, double x0) {
  const int B = 2, K = scheme == 0 ? 2 * N + 1 : N + 1, n = K * (ns + nu), m = (scheme == 0 ? 2 : 1) * N * ns;
  unsigned long long s = 12345 + 1000 * system_id + N;
  std::vector<double> z((size_t)B * n), lam((size_t)B * m), lb((size_t)B * n), ub((size_t)B * n), sz((size_t)B * n), sl((size_t)B * m);
  std::vector<double> grad((size_t)B * np), dz0((size_t)B * n), dlam0((size_t)B * m);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < n; ++i) {
      const size_t k = (size_t)b * n + i;
      z[k] = (i < K * ns ? x0 : 0.3) + 0.1 * (unit(s) - 0.5);
      const double r = unit(s);
      lb[k] = r < 0.3 ? z[k] - 1e-3 : -INFINITY;      // a third of the variables in a box a step leaves, the first point pinned
      ub[k] = r < 0.3 ? z[k] + 1e-3 : INFINITY;
      if (i < ns) lb[k] = ub[k] = z[k];
      sz[k] = unit(s) - 0.5;
    }
  for (size_t k = 0; k < lam.size(); ++k) { lam[k] = 0.2 * (unit(s) - 0.5); sl[k] = unit(s) - 0.5; }
  int bad = 0;
  for (int nsteps = 0; nsteps <= 3; nsteps += 3) {
    if (exgd_grad_twin(system_id, scheme, B, N, T, z.data(), lam.data(), lb.data(), ub.data(), nullptr, 0, 0.05, 0.05, nsteps, sz.data(),
                       nsteps ? sl.data() : nullptr, grad.data(), dz0.data(), nsteps ? dlam0.data() : nullptr)) {
      printf("%s: no specialisation\n", what);
      return 1;
    }
    for (double v : grad) bad += !isfinite(v) || (nsteps == 0 && v != 0.0);
    for (size_t k = 0; k < dz0.size(); ++k) bad += !isfinite(dz0[k]) || (nsteps == 0 && dz0[k] != sz[k]);
    if (nsteps) for (double v : dlam0) bad += !isfinite(v);
  }
  printf("%s: %s\n", what, bad ? "FAILED" : "ok");
  return bad != 0;
}

int main() {
  int rc = 0;
  rc |= one("CARTPOLE Hermite-Simpson N=3", SysCARTPOLE::ID, 0, SysCARTPOLE::NS, SysCARTPOLE::NU, SysCARTPOLE::NP, 3, 0.3, 0.2);
  rc |= one("CARTPOLE Hermite-Simpson N=33", SysCARTPOLE::ID, 0, SysCARTPOLE::NS, SysCARTPOLE::NU, SysCARTPOLE::NP, 33, 2.0, 0.2);
  rc |= one("BACTERIA trapezoidal N=5", SysBACTERIA::ID, 1, SysBACTERIA::NS, SysBACTERIA::NU, SysBACTERIA::NP, 5, 0.5, 1.0);
  return rc;
}
