// node_hvp_check.cpp -- TEST-ONLY stand-alone program (its own main) over the host build of myriad_amd/csrc/node_hvp.h, for AddressSanitizer /
// UBSan: compiled with -fsanitize=address,undefined and run directly by tests/test_node_hvp_host_twin.py.  Every buffer is allocated at exactly
// the size the header documents, so that an index past a pair's column or the side record is caught.
// Shapes: Hermite-Simpson N = 3; SHOOTING 3 x 2 RK4 and 1 x 4 HEUN; weights from a fixed generator; with_cost 1 and 0.
// Checked: out_z against (g(z + e v) - g(z - e v)) / 2 e and out_p . dp against (<g(z; p + e dp), v> - <g(z; p - e dp), v>) / 2 e, where g is
// the FIRST-ORDER pass of the same header family (NodeExgdPoint::grad; NodeShootExgd::interval<false> + ShootExgdGrad::out_z) -- nothing of the
// second-order code takes part in the differences; out_z with and without out_p; finite, non-zero results.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../myriad_amd/csrc/node_hvp.h"

using namespace myriad;

static unsigned long long g_state = 0x9e3779b97f4a7c15ULL;
static double rnd() {      // uniform in (-1, 1)
  g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(g_state >> 11) / 4503599627370496.0 - 1.0;
}

using Vec = std::vector<double>;

// grad_z (with_cost f + lam^T c) of one instance, first order only
static void grad_hs(int N, double T, const Vec& z, const Vec& lam, const Vec& p, int with_cost, Vec& g) {
  using C = NodeHvp;
  const int K = C::G::points(N);
  const double h = T / N;
  for (int j = 0; j < K; ++j) {
    double w[C::NW], a[C::NS], e[C::NS], gj[C::NW];
    for (int r = 0; r < C::NW; ++r) w[r] = z[C::idx(K, j, r)];
    C::G::combine(lam.data(), N, j, h, a, e);
    NodeExgdPoint::grad(w, p.data(), a, e, with_cost ? C::G::wq(K, j, h) : 0.0, false, 0.0, gj);
    for (int r = 0; r < C::NW; ++r) g[C::idx(K, j, r)] = gj[r];
  }
}

template <int M>
static void grad_shoot(int method, int I, int cpi, double T, const Vec& z, const Vec& lam, const Vec& p, int with_cost, Vec& g) {
  using A = NodeShootExgd<M>;
  const long n = A::nvars(I, cpi), m = (long)I * A::NS;
  Vec lc(m), phist((size_t)A::pair_hist_doubles(cpi) * I), side((size_t)A::side_doubles(cpi) * I);
  Vec none(A::NP);
  NseHostNet net{p.data(), none.data()};
  const typename A::Rule R = A::P::rule(method);
  for (int k = 0; k < I; ++k)
    for (int q = 0; q < A::NS; ++q) lc[k + (long)q * I] = lam[(long)k * A::NS + q];
  for (int k = 0; k < I; ++k)
    A::template interval<false>(net, R, I, cpi, k, T / ((double)I * cpi), z.data(), nullptr, lc.data() + k, p.data(), with_cost ? 1.0 : 0.0,
                                phist.data() + k, side.data() + k, I, nullptr, 0.0);
  for (long i = 0; i < n; ++i) g[i] = A::G::out_z(I, cpi, i, side.data(), lc.data(), 1.0, I);
}

static Vec shifted(const Vec& a, const Vec& d, double e) {
  Vec r(a);
  for (size_t i = 0; i < r.size(); ++i) r[i] += e * d[i];
  return r;
}

// transcription 0 / 2 as node_hvp_host
static int check(const char* name, int transcription, int method, int I, int cpi, int with_cost) {
  constexpr int NS = NodeHvp::NS, NW = NodeHvp::NW, NP = NodeHvp::NP;
  const bool hs = transcription == 0;
  const int M = method == 3 ? 2 : 1;
  const long nx = hs ? (long)(2 * I + 1) * NS : (long)(I + 1) * NS;
  const long n = hs ? (long)(2 * I + 1) * NW : nx + ((long)M * I * cpi + 1);
  const long m = hs ? 2L * I * NS : (long)I * NS;
  const double T = 0.1 * I * (hs ? 1 : cpi);
  Vec p(NP), z(n), lam(m), v(n), dp(NP), oz(n), oz2(n), op(NP);
  for (double& w : p) w = 0.3 * rnd();
  for (long i = 0; i < n; ++i) z[i] = i < nx ? 0.5 * rnd() : 3.0 * rnd();
  for (double& w : lam) w = 0.1 * rnd();
  for (double& w : v) w = rnd();
  for (int e = 0; e < NP; ++e) dp[e] = std::fabs(p[e]) * rnd();
  auto grad = [&](const Vec& zz, const Vec& pp, Vec& g) {
    if (hs) grad_hs(I, T, zz, lam, pp, with_cost, g);
    else if (M == 2) grad_shoot<2>(method, I, cpi, T, zz, lam, pp, with_cost, g);
    else grad_shoot<1>(method, I, cpi, T, zz, lam, pp, with_cost, g);
  };
  int rc = node_hvp_host(transcription, method, 1, I, cpi, T, z.data(), lam.data(), v.data(), p.data(), with_cost, oz.data(), op.data());
  rc |= node_hvp_host(transcription, method, 1, I, cpi, T, z.data(), lam.data(), v.data(), p.data(), with_cost, oz2.data(), nullptr);
  const double e = 1e-6;
  Vec gp(n), gm(n);
  grad(shifted(z, v, e), p, gp);
  grad(shifted(z, v, -e), p, gm);
  double ez = 0.0, zmax = 0.0, same = 0.0, gmax = 0.0;
  for (long i = 0; i < n; ++i) {
    gmax = std::fmax(gmax, std::fabs(gp[i]));
    ez = std::fmax(ez, std::fabs(oz[i] - (gp[i] - gm[i]) / (2 * e)));
    zmax = std::fmax(zmax, std::fabs(oz[i]));
    same = std::fmax(same, std::fabs(oz[i] - oz2[i]));
  }
  grad(z, shifted(p, dp, e), gp);
  grad(z, shifted(p, dp, -e), gm);
  double fd_p = 0.0, an_p = 0.0;
  for (long i = 0; i < n; ++i) fd_p += (gp[i] - gm[i]) / (2 * e) * v[i];
  for (int k = 0; k < NP; ++k) an_p += op[k] * dp[k];
  // (a central difference of g with step e rounds at about 2^-52 |g| / e = 2.2e-10 |g|, whatever the size of the product itself)
  const bool okz = std::isfinite(ez) && zmax > 0.0 && ez <= 1e-6 * zmax + 1e-9 * gmax;
  const bool okp = std::isfinite(an_p) && an_p != 0.0 && std::fabs(an_p - fd_p) <= 1e-5 * std::fmax(std::fabs(an_p), std::fabs(fd_p));
  const bool ok = rc == 0 && okz && okp && same == 0.0;
  std::printf("%s I=%d cpi=%d with_cost=%d: out_z err %.2e of %.3g | out_p.dp %.12g fd %.12g | with/without out_p %.1e: %s\n", name, I, cpi, with_cost,
              ez, zmax, an_p, fd_p, same, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  for (int wc = 1; wc >= 0; --wc) {
    bad += check("HERMITE_SIMPSON", 0, 0, 3, 1, wc);
    bad += check("SHOOTING RK4", 2, 3, 3, 2, wc);
    bad += check("SHOOTING HEUN", 2, 1, 1, 4, wc);
  }
  return bad;
}
