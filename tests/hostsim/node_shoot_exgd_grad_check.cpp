// node_shoot_exgd_grad_check.cpp -- TEST-ONLY stand-alone program (its own main) over the host build of myriad_amd/csrc/node_shoot_exgd_grad.h, for
// AddressSanitizer / UBSan: compiled with -fsanitize=address,undefined and run directly by tests/test_node_shoot_exgd_grad_host_twin.py.  Every
// buffer is allocated at exactly the size the header documents, so that an index past a pair's column, the history or the side record is caught.
// Two small shapes (3 x 2 RK4, 1 x 4 Heun), two steps, weights from a fixed generator, a third of the variables in a box the steps leave.
// Checked: grad . delta, dz0 . dz and dlam0 . dl against central differences of the twin's OWN forward steps (the history of a run of one step
// more holds x_n and lam_n), the fused against the unfused order, finite results.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../myriad_amd/csrc/node_shoot_exgd_grad.h"

using namespace myriad;

static unsigned long long g_state = 0x9e3779b97f4a7c15ULL;
static double rnd() {      // uniform in (-1, 1)
  g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(g_state >> 11) / 4503599627370496.0 - 1.0;
}

template <int M>
static int check(const char* name, int method, int I, int cpi) {
  using A = NodeShootExgd<M>;
  constexpr int NP = A::NP;
  const int nsteps = 2;
  const long n = A::nvars(I, cpi), m = (long)I * A::NS, hs = 2 * n + m;
  const double T = 0.1 * I * cpi, eta_x = 0.05, eta_v = 0.5;
  std::vector<double> p(NP), z(n), lam(m), lb(n), ub(n), sz(n), sl(m), dp(NP), dz(n), dl(m);
  for (double& w : p) w = 0.3 * rnd();
  for (long i = 0; i < n; ++i) z[i] = i < (long)(I + 1) * A::NS ? 0.5 * rnd() : 3.0 * rnd();
  for (double& w : lam) w = 0.1 * rnd();
  for (double& w : sz) w = rnd();
  for (double& w : sl) w = rnd();
  for (int e = 0; e < NP; ++e) dp[e] = std::fabs(p[e]) * rnd();
  long boxed = 0;
  for (long i = 0; i < n; ++i) {
    const bool box = rnd() < -1.0 / 3.0;
    lb[i] = box ? z[i] - 1e-3 : -INFINITY; ub[i] = box ? z[i] + 1e-3 : INFINITY;
    if (i < A::NS) { lb[i] = z[i]; ub[i] = z[i]; }      // the first node is pinned
    boxed += box;
    dz[i] = rnd();
  }
  for (double& w : dl) w = rnd();
  std::vector<double> hist((size_t)A::hist_doubles(I, cpi, nsteps + 1)), work((size_t)(A::work_doubles(I, cpi) + n));
  std::vector<double> g(NP), g2(NP), dz0(n), dlam0(m), dz02(n), dlam02(m), none(NP), zero(n, 0.0);
  node_shoot_exgd_grad_host<M>(method, I, cpi, T, z.data(), lam.data(), lb.data(), ub.data(), p.data(), eta_x, eta_v, nsteps, sz.data(), sl.data(),
                               hist.data(), work.data(), g.data(), dz0.data(), dlam0.data(), true);
  node_shoot_exgd_grad_host<M>(method, I, cpi, T, z.data(), lam.data(), lb.data(), ub.data(), p.data(), eta_x, eta_v, nsteps, sz.data(), sl.data(),
                               hist.data(), work.data(), g2.data(), dz02.data(), dlam02.data(), false);
  // out(p, z, lam) = seed_z . x_n + seed_lam . lam_n from the forward steps alone: one step more, read at the start of step `nsteps`
  auto out = [&](const std::vector<double>& pp, const std::vector<double>& zz, const std::vector<double>& ll) {
    node_shoot_exgd_grad_host<M>(method, I, cpi, T, zz.data(), ll.data(), lb.data(), ub.data(), pp.data(), eta_x, eta_v, nsteps + 1, zero.data(), nullptr,
                                 hist.data(), work.data(), none.data(), nullptr, nullptr, true);
    const double* H = hist.data() + nsteps * hs;
    double s = 0.0;
    for (long i = 0; i < n; ++i) s += sz[i] * H[i];
    for (long i = 0; i < m; ++i) s += sl[i] * H[2 * n + i];
    return s;
  };
  auto shifted = [](const std::vector<double>& a, const std::vector<double>& d, double e) {
    std::vector<double> r(a);
    for (size_t i = 0; i < r.size(); ++i) r[i] += e * d[i];
    return r;
  };
  const double e = 1e-6;
  const double fd_p = (out(shifted(p, dp, e), z, lam) - out(shifted(p, dp, -e), z, lam)) / (2 * e);
  // the pinned node moves with z: its derivative is the clamp's, zero -- keep it where it is
  for (int i = 0; i < A::NS; ++i) dz[i] = 0.0;
  const double fd_z = (out(p, shifted(z, dz, e * 1e-2), lam) - out(p, shifted(z, dz, -e * 1e-2), lam)) / (2 * e * 1e-2);
  const double fd_l = (out(p, z, shifted(lam, dl, e)) - out(p, z, shifted(lam, dl, -e))) / (2 * e);
  double an_p = 0.0, an_z = 0.0, an_l = 0.0, dfu = 0.0, gmax = 0.0;
  for (int k = 0; k < NP; ++k) { an_p += g[k] * dp[k]; dfu = std::fmax(dfu, std::fabs(g[k] - g2[k])); gmax = std::fmax(gmax, std::fabs(g[k])); }
  for (long i = 0; i < n; ++i) { an_z += dz0[i] * dz[i]; dfu = std::fmax(dfu, std::fabs(dz0[i] - dz02[i])); }
  for (long i = 0; i < m; ++i) { an_l += dlam0[i] * dl[i]; dfu = std::fmax(dfu, std::fabs(dlam0[i] - dlam02[i])); }
  auto close = [](double a, double b) { return std::isfinite(a) && std::fabs(a - b) <= 1e-5 * std::fmax(std::fabs(a), std::fabs(b)); };
  // (z moves inside boxes of 1e-3 by 1e-8 |dz|: no clamp changes side)
  const bool ok = close(an_p, fd_p) && close(an_z, fd_z) && close(an_l, fd_l) && dfu <= 1e-12 * std::fmax(1.0, gmax) && gmax > 0.0 && boxed > 0;
  std::printf("%s I=%d cpi=%d: grad.dp %.12g fd %.12g | dz0.dz %.12g fd %.12g | dlam0.dl %.12g fd %.12g | fused-unfused %.2e boxed %ld: %s\n", name, I,
              cpi, an_p, fd_p, an_z, fd_z, an_l, fd_l, dfu, boxed, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  bad += check<2>("RK4", 3, 3, 2);
  bad += check<1>("HEUN", 1, 1, 4);
  return bad;
}
