// hostsim_scaled.cpp -- TEST-ONLY (see hostsim.cpp): the lane cores under a variable scale (myr_set_var_scale), for
// tests/test_var_scale_host_twin.py.  A translation unit of its own, linked into libhostsim.so: its 52 solver instantiations stay out of
// hostsim.cpp, which tests/test_hostsim_sanitized.py compiles a second time under the sanitizers.
#include <stdint.h>
#include <vector>
#include "../../myriad_amd/csrc/hs_solver.h"
#include "../../myriad_amd/csrc/os_solver.h"

using namespace myriad;

// One trajectory, the scales placed where lane_solve_kernel places them (SysParams::set_scale after load), the options as make_opts
// sets them (delta_warm for the collocation cores only).  z, lb, ub arrive in the SCALED variables and z, lam leave in them: the change
// of variables on the way in and out (scale_in_kernel / scale_out_kernel on the device) is the caller's, restated in tests/var_scale_cases.py.
template <class Core, class Sys>
static void scaled_one(HsSolveOpts o, long n, long nst, double* z, const double* lb, const double* ub, const double* scale,
                       double* lam, double* out) {
  std::vector<double> zL(n), zU(n), dz(n), lbv(lb, lb + n), ubv(ub, ub + n), st(nst);
  SysParams<Sys> pp;
  pp.load(nullptr, 0, 0);
  pp.set_scale(scale);
  const double* p = pp.get();
  HsWork w{{z, 1}, {lbv.data(), 1}, {ubv.data(), 1}, {zL.data(), 1}, {zU.data(), 1}, {lam, 1}, {dz.data(), 1}, {st.data(), 1}};
  HsSolveResult r;
  Core::solve(w, o, p, r);
  out[0] = r.cost; out[1] = r.status; out[2] = r.iters; out[3] = r.feas; out[4] = r.stat; out[5] = r.compl_;
}

template <class Sys, bool SHOOT>
static int scaled_for_system(int tr, int N, int cpi, int method, double T, int max_iter, double* z, const double* lb, const double* ub,
                             const double* scale, double* lam, double* out) {
  HsSolveOpts o{N, T / N, max_iter, 1e-8, 1e-6, 1e-7, 0.1};
  o.delta_warm = tr == 2 ? 0 : 1;
  if (tr == 0) { scaled_one<HsSolver<Sys>, Sys>(o, (2 * N + 1) * Sys::NW, HsSol<Sys>::stage_doubles(N), z, lb, ub, scale, lam, out); return 0; }
  if (tr == 1) { scaled_one<TrapCore<Sys>, Sys>(o, (N + 1) * Sys::NW, TrapCore<Sys>::stage_doubles(N), z, lb, ub, scale, lam, out); return 0; }
  if constexpr (SHOOT) {
    if (tr != 2) return -1;
    o.cpi = cpi; o.method = method;
    if (method == 3) scaled_one<ShootCore<Sys, 2>, Sys>(o, (N + 1) * Sys::NS + (2 * N * cpi + 1) * Sys::NU, ShootCore<Sys, 2>::stage_doubles(N, cpi), z, lb, ub, scale, lam, out);
    else scaled_one<ShootCore<Sys>, Sys>(o, (N + 1) * Sys::NS + (N * cpi + 1) * Sys::NU, ShootCore<Sys>::stage_doubles(N, cpi), z, lb, ub, scale, lam, out);
    return 0;
  }
  return -1;      // (the twins have no shooting solver on the device either)
}

// tr: 0 Hermite-Simpson, 1 trapezoidal, 2 shooting (N intervals of cpi controls, method 1 Heun / 3 RK4); scale[16] (states, then controls);
// out[6] = cost, status, iterations, and the solver's own feasibility, stationarity, complementarity
extern "C" int hostsim_solve_scaled(int system_id, int tr, int N, int cpi, int method, double T, int max_iter, double* z, const double* lb,
                                    const double* ub, const double* scale, double* lam, double* out) {
#define SC(S, SHOOT) return scaled_for_system<S, SHOOT>(tr, N, cpi, method, T, max_iter, z, lb, ub, scale, lam, out)
  switch (system_id) {
    case 0: SC(SysCARTPOLE, true);
    case 1: SC(SysVANDERPOL, true);
    case 2: SC(SysCANCERTREATMENT, true);
    case 3: SC(SysSIMPLECASE, true);
    case 5: SC(SysBIOREACTOR, true);
    case 6: SC(SysGLUCOSE, true);
    case 7: SC(SysMOULDFUNGICIDE, true);
    case 8: SC(SysSIMPLECASEWITHBOUNDS, true);
    case 14: SC(SysMOUNTAINCAR, true);
    case 16: SC(SysBACTERIA, true);
    case 18: SC(SysHARVEST, true);
    case 19: SC(SysTIMBERHARVEST, true);
    case 100: SC(SysCARTPOLE_ELASTIC, false);
    case 101: SC(SysVANDERPOL_ELASTIC, false);
  }
  return -1;
}
