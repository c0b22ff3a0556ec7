// exgd_jac_check.cpp -- TEST-ONLY stand-alone program: the host twin of the forward-mode Jacobian of the unrolled extragradient steps
// (exgd_jac_twin.cpp, which runs myriad_amd/csrc/exgd_jac.h) under the host sanitizers.  tests/test_exgd_jac_host_twin.py compiles it with
// -fsanitize=address,undefined and runs it directly.  Cases: CARTPOLE Hermite-Simpson N = 3 and N = 33, BACTERIA trapezoidal N = 5 (terminal cost),
// HIVTREATMENT Hermite-Simpson N = 4 (nine columns, in groups of four); B = 2, bounds that clip.  Exits 0 when every result is finite, a zero-step
// call returns its inputs, 2 + 1 chained steps have the bits of 3, and the grouped run has the bits of the ungrouped one.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "exgd_jac_twin.cpp"

static double unit(unsigned long long& s) {      // splitmix64 -> [0, 1)
  s += 0x9e3779b97f4a7c15ULL;
  unsigned long long z = s;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  z ^= z >> 31;
  return (double)(z >> 11) / 9007199254740992.0;
}

static bool same(const std::vector<double>& a, const std::vector<double>& b) { return memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

static int one(const char* what, int system_id, int scheme, int ns, int nu, int np, int N, double T, double x0, int gcols) {
  const int B = 2, K = scheme == 0 ? 2 * N + 1 : N + 1, n = K * (ns + nu), m = (scheme == 0 ? 2 : 1) * N * ns;
  unsigned long long s = 54321 + 1000 * system_id + N;
  std::vector<double> z((size_t)B * n), lam((size_t)B * m), lb((size_t)B * n), ub((size_t)B * n);
  const size_t nz = (size_t)B * np * n, nl = (size_t)B * np * m;
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < n; ++i) {
      const size_t k = (size_t)b * n + i;
      z[k] = (i < K * ns ? x0 : 0.3) + 0.1 * (unit(s) - 0.5);
      const double r = unit(s);
      lb[k] = r < 0.3 ? z[k] - 1e-3 : -INFINITY;      // a third of the variables in a box a step leaves, the first point pinned
      ub[k] = r < 0.3 ? z[k] + 1e-3 : INFINITY;
      if (i < ns) lb[k] = ub[k] = z[k];
    }
  for (size_t k = 0; k < lam.size(); ++k) lam[k] = 0.2 * (unit(s) - 0.5);
  auto call = [&](int nsteps, const std::vector<double>& zi, const std::vector<double>& li, const double* jz0, const double* jlam0, int g,
                  std::vector<double>& zn, std::vector<double>& ln, std::vector<double>& jz, std::vector<double>& jl) {
    zn.assign(zi.size(), NAN); ln.assign(li.size(), NAN); jz.assign(nz, NAN); jl.assign(nl, NAN);
    return exgd_jac_twin(system_id, scheme, B, N, T, zi.data(), li.data(), lb.data(), ub.data(), nullptr, 0, 0.05, 0.05, nsteps, jz0, jlam0, g, zn.data(),
                         ln.data(), jz.data(), jl.data());
  };
  std::vector<double> zn, ln, jz, jl, z2, l2, jz2, jl2, z3, l3, jz3, jl3;
  if (call(3, z, lam, nullptr, nullptr, 0, zn, ln, jz, jl)) { printf("%s: no specialisation\n", what); return 1; }
  int bad = 0;
  for (double v : zn) bad += !isfinite(v);
  for (double v : ln) bad += !isfinite(v);
  for (double v : jz) bad += !isfinite(v);
  for (double v : jl) bad += !isfinite(v);
  for (int b = 0; b < B; ++b)                           // the pinned first point has zero rows
    for (int k = 0; k < np; ++k)
      for (int i = 0; i < ns; ++i) bad += jz[((size_t)b * np + k) * n + i] != 0.0;
  call(0, z, lam, jz.data(), jl.data(), 0, z2, l2, jz2, jl2);      // zero steps: the inputs come back
  bad += !same(z2, z) + !same(l2, lam) + !same(jz2, jz) + !same(jl2, jl);
  call(2, z, lam, nullptr, nullptr, 0, z2, l2, jz2, jl2);          // 2 + 1 = 3
  call(1, z2, l2, jz2.data(), jl2.data(), 0, z3, l3, jz3, jl3);
  bad += !same(z3, zn) + !same(l3, ln) + !same(jz3, jz) + !same(jl3, jl);
  call(3, z, lam, nullptr, nullptr, gcols, z3, l3, jz3, jl3);      // groups of columns
  bad += !same(z3, zn) + !same(l3, ln) + !same(jz3, jz) + !same(jl3, jl);
  printf("%s: %s\n", what, bad ? "FAILED" : "ok");
  return bad != 0;
}

int main() {
  int rc = 0;
  rc |= one("CARTPOLE Hermite-Simpson N=3", SysCARTPOLE::ID, 0, SysCARTPOLE::NS, SysCARTPOLE::NU, SysCARTPOLE::NP, 3, 0.3, 0.2, 1);
  rc |= one("CARTPOLE Hermite-Simpson N=33", SysCARTPOLE::ID, 0, SysCARTPOLE::NS, SysCARTPOLE::NU, SysCARTPOLE::NP, 33, 2.0, 0.2, 3);
  rc |= one("BACTERIA trapezoidal N=5", SysBACTERIA::ID, 1, SysBACTERIA::NS, SysBACTERIA::NU, SysBACTERIA::NP, 5, 0.5, 1.0, 2);
  rc |= one("HIVTREATMENT Hermite-Simpson N=4", SysHIVTREATMENT::ID, 0, SysHIVTREATMENT::NS, SysHIVTREATMENT::NU, SysHIVTREATMENT::NP, 4, 0.4, 1.0, 4);
  return rc;
}
