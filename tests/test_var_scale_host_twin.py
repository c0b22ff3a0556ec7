"""CPU tests of the variable scaling on the lane cores (hs_solver.h: HsSolver, os_solver.h: TrapCore, ShootCore<.,1|2>: the source of the
GPU lane kernels) through their TEST-ONLY host build: SysParams::set_scale placed as lane_solve_kernel places it, the change of variables
of scale_in_kernel / scale_out_kernel restated in tests/var_scale_cases.py, and every solve -- unit scale, powers of two, and a vector that
is neither -- held to the KKT conditions of the oracle's UNSCALED transcription.  A wrong scale slot of a generated system or a wrong row
rule for lam fails here without a GPU; the device forms are in tests/test_gpu_var_scale.py, on the same cases with the same checker."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import var_scale_cases as V

HERE = os.path.dirname(os.path.abspath(__file__))
SID = {"CARTPOLE": 0, "VANDERPOL": 1, "CANCERTREATMENT": 2, "SIMPLECASE": 3, "BIOREACTOR": 5, "GLUCOSE": 6, "MOULDFUNGICIDE": 7,
       "SIMPLECASEWITHBOUNDS": 8, "MOUNTAINCAR": 14, "BACTERIA": 16, "HARVEST": 18, "TIMBERHARVEST": 19,
       "CARTPOLE_ELASTIC": 100, "VANDERPOL_ELASTIC": 101}
TR = {"HERMITE_SIMPSON": 0, "TRAPEZOIDAL": 1, "SHOOTING": 2}
METHOD = {"HEUN": 1, "RK4": 3}
A = lambda a: a.ctypes.data


@pytest.fixture(scope="module")
def sim():
  subprocess.run(["bash", os.path.join(HERE, "hostsim", "build.sh")], check=True)
  lib = C.CDLL(os.path.join(HERE, "hostsim", "libhostsim.so"))
  dp = C.c_void_p
  lib.hostsim_solve_scaled.argtypes = [C.c_int] * 5 + [C.c_double, C.c_int] + [dp] * 6
  lib.hostsim_solve_scaled.restype = C.c_int
  return lib


def solve_scaled(sim, name, tr, rule, N, cpi, method, T, scale):
  """one solve in the scaled variables; (z, lam) come back in the ORIGINAL ones"""
  nw = tr.ns + tr.nu
  s = np.ones(nw) if scale is None else np.asarray(scale, dtype=np.float64)
  z0, lb, ub = V.scaled_inputs(tr, s)
  z = np.ascontiguousarray(z0); lb = np.ascontiguousarray(lb); ub = np.ascontiguousarray(ub)
  s16 = np.ones(16); s16[:nw] = s
  m = (2 * N if rule == "HERMITE_SIMPSON" else N) * tr.ns
  lam = np.zeros(m); out = np.zeros(6)
  assert sim.hostsim_solve_scaled(SID[name], TR[rule], N, cpi, METHOD[method], float(T), V.MAX_ITER, A(z), A(lb), A(ub), A(s16), A(lam), A(out)) == 0
  z, lam = V.unscaled_outputs(tr, s, z, lam)
  return dict(z=z, lam=lam, cost=out[0], status=int(out[1]), iters=int(out[2]), kkt=out[3:6].copy())


@pytest.mark.parametrize("sysname,shape", V.CASES, ids=[f"{s}-{k}" for s, k in V.CASES])
def test_lane_cores_solve_the_original_problem_under_a_scale(sim, sysname, shape):
  rule, N, cpi, method = V.SHAPES[shape]
  s, tr, cb = V.problem(sysname, shape)
  unit = None
  for tag, mk in V.SCALES:
    scale = None if mk is None else mk(tr.ns + tr.nu)
    r = solve_scaled(sim, sysname, tr, rule, N, cpi, method, s.T, scale)
    print(sysname, shape, tag, "status", r["status"], "iters", r["iters"], "cost %.12g" % r["cost"], "kkt", r["kkt"])
    fig = V.check_original_kkt(tr, cb, scale, r["z"], r["lam"], r["cost"], r["status"])
    print("   feas %.2e (bound %.2e)  stat %.2e (bound %.2e)  cost err %.1e" % (fig["feas"], fig["feas_bound"], fig["stat"], fig["stat_bound"], fig["cost_err"]))
    if unit is None:
      unit = r["cost"]
    elif V.cost_agreement_applies(sysname, shape):
      print("   cost against the unit solve %.2e" % V.check_cost_agreement(r["cost"], unit))


@pytest.mark.parametrize("base,shape", V.TWIN_CASES, ids=[f"{b}-{k}" for b, k in V.TWIN_CASES])
def test_twin_cores_solve_the_weighted_penalty_problem_under_a_scale(sim, base, shape):
  """The elastic twins under a scale solve the problem whose penalty is rho/2 sum (s_i / sc_i)^2 (include/myriad_hip.h), not the unweighted one:
  the checker runs against oracle.Elastic(base, 1, slack_scale = the slacks' scale entries), and the returned cost is NOT the unweighted twin's."""
  rule, N = V.TWIN_SHAPES[shape]
  b, tr0, cb0 = V.twin_problem(base, shape)
  for tag, scale in V.twin_scales(b.base.ns, b.base.nu):
    s, tr, cb = V.twin_problem(base, shape, tuple(scale[b.base.ns + b.base.nu:]))
    r = solve_scaled(sim, base + "_ELASTIC", tr, rule, N, 1, "HEUN", s.T, scale)
    print(base, shape, tag, "status", r["status"], "iters", r["iters"], "cost %.12g" % r["cost"], "kkt", r["kkt"])
    fig = V.check_original_kkt(tr, cb, scale, r["z"], r["lam"], r["cost"], r["status"])
    print("   feas %.2e  stat %.2e (bound %.2e)  cost err %.1e" % (fig["feas"], fig["stat"], fig["stat_bound"], fig["cost_err"]))
    assert abs(r["cost"] - cb0.fun(r["z"])) > 1e-3            # the weighting is not a no-op: the unweighted twin's cost at z is another number
