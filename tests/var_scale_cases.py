"""What the CPU and the GPU test of the variable scaling (include/myriad_hip.h: myr_set_var_scale) share: the cases, the two scale
vectors, the change of variables as the library makes it (csrc/myriad_hip.hip: scale_in_kernel / scale_out_kernel), and ONE checker
that holds a returned (z, lam, cost) to the KKT conditions of the UNSCALED transcription of the oracle.

The header's promise is "the same optimisation problem in better-conditioned variables; inputs and outputs of myr_solve stay in the
ORIGINAL variables".  With z = s o z_s the scaled problem has c_s = c / s_state (row by row), grad_s f = s o grad f, J_s = S_c^-1 J S,
so a KKT point (z_s, lam_s) of it is the KKT point (s o z_s, lam_s / s_state) of the original one, and the solver's tolerances travel:
  feasibility   |c_s| <= 1e-8                        ->  |c| <= 1e-8 max state scale
  stationarity  |grad_s f + J_s^T lam_s| <= 1e-4 ..  ->  |grad f + J^T lam| <= 1e-4 .. / min scale
(1e-4 sd max(1, |grad f|) is the figure tests/test_gpu_systems.py holds the unscaled solves to.)"""
import dataclasses
import functools

import numpy as np

from oracle import myriad_oracle as O

_P2_EXP = (-2, 3, 1, -1, 2, -3, 2)
_ODD = (3.0, 0.7, 5.0, 1.3, 0.4, 2.2)


def P2(nw):
  """powers of two: the change of variables is exact in floating point"""
  return np.array([2.0 ** _P2_EXP[i % 7] for i in range(nw)])


def ODD(nw):
  """no powers of two: every scaling rounds"""
  return np.array([_ODD[i % 6] for i in range(nw)])


SCALES = (("unit", None), ("P2", P2), ("ODD", ODD))

SYSTEM_NAMES = ("CARTPOLE", "VANDERPOL", "CANCERTREATMENT", "SIMPLECASE", "SIMPLECASEWITHBOUNDS", "BACTERIA", "HARVEST", "TIMBERHARVEST",
                "MOUNTAINCAR", "BIOREACTOR", "GLUCOSE", "MOULDFUNGICIDE")
# shape -> (transcription of the C-ABI, intervals, controls per interval, integration method)
SHAPES = {"hs8": ("HERMITE_SIMPSON", 8, 1, "HEUN"), "trap9": ("TRAPEZOIDAL", 9, 1, "HEUN"),
          "shoot3x4_heun": ("SHOOTING", 3, 4, "HEUN"), "shoot3x4_rk4": ("SHOOTING", 3, 4, "RK4")}
# CANCERTREATMENT shooting 3 x 4 HEUN ends at the iteration limit at UNIT scale on the host twin: not a case
CASES = tuple((s, k) for s in SYSTEM_NAMES for k in SHAPES if (s, k) != ("CANCERTREATMENT", "shoot3x4_heun"))
assert len(CASES) == 47
MAX_ITER = 500


def cost_agreement_applies(sysname, shape):
  """"The same answer as the unscaled solve" is no property of a local method: BIOREACTOR ends at another KKT point of its flat optimum
  (-1.38725 against -1.38630) and VANDERPOL's Heun shooting in another local optimum under ODD (3.07 against 16.93), on the host twin."""
  return sysname != "BIOREACTOR" and (sysname, shape) != ("VANDERPOL", "shoot3x4_heun")


@functools.lru_cache(maxsize=None)
def problem(sysname, shape):
  """(oracle system, its transcription, the callbacks): built once per case, never modified"""
  rule, N, cpi, method = SHAPES[shape]
  s = O.SYSTEMS[sysname]()
  tr = O.make_transcription(s, "SHOOTING" if rule == "SHOOTING" else "COLLOCATION", N, cpi, rule, method)
  return s, tr, O.Callbacks(tr)


def variable_scales(tr, scale):
  """scale [ns + nu] (states, then controls) per variable of z: the state rows (x_rows x ns), then the control rows"""
  scale = np.asarray(scale, dtype=np.float64)
  assert scale.shape == (tr.ns + tr.nu,)
  return np.concatenate([np.tile(scale[:tr.ns], tr.x_rows), np.tile(scale[tr.ns:], tr.u_rows)])


def scaled_inputs(tr, scale):
  """z0 / s, lb / s, ub / s: what the solver cores see"""
  sv = variable_scales(tr, scale)
  return tr.guess / sv, tr.bounds[:, 0] / sv, tr.bounds[:, 1] / sv


def unscaled_outputs(tr, scale, z_s, lam_s):
  """z = s o z_s; lam = lam_s / s_state: every constraint row is a state-component row (row % ns)"""
  scale = np.asarray(scale, dtype=np.float64)
  return z_s * variable_scales(tr, scale), lam_s / scale[np.arange(lam_s.size) % tr.ns]


def check_original_kkt(tr, cb, scale, z, lam, cost, status):
  """(z, lam, cost) in the ORIGINAL variables against the oracle's UNSCALED transcription.  Returns the measured figures."""
  scale = np.ones(tr.ns + tr.nu) if scale is None else np.asarray(scale, dtype=np.float64)
  z, lam = np.asarray(z, dtype=np.float64), np.asarray(lam, dtype=np.float64)
  assert int(status) == 0, ("status", int(status))
  assert np.isfinite(z).all() and np.isfinite(lam).all() and np.isfinite(cost)
  lb, ub = tr.bounds[:, 0], tr.bounds[:, 1]
  tol_l = 1e-12 * np.maximum(1.0, np.abs(np.where(np.isfinite(lb), lb, 0.0)))
  tol_u = 1e-12 * np.maximum(1.0, np.abs(np.where(np.isfinite(ub), ub, 0.0)))
  assert (z >= lb - tol_l).all() and (z <= ub + tol_u).all(), ("bounds", float((lb - z).max()), float((z - ub).max()))
  feas = float(np.abs(cb.cons(z)).max())
  feas_bound = 1e-8 * max(1.0, scale[:tr.ns].max()) + 1e-12 * max(1.0, float(np.abs(z).max()))
  f = cb.fun(z)
  cost_err = abs(cost - f) / abs(f) if f != 0.0 else abs(cost)
  g = cb.grad(z)
  rr = g + cb.jac(z).T @ lam
  width = np.where(np.isfinite(ub - lb), ub - lb, 1.0)
  inact = (lb < ub) & (z - lb > 1e-3 * width) & (ub - z > 1e-3 * width)
  assert inact.any(), "no inactive variable: the stationarity check would be vacuous"
  assert np.abs(lam).max() > 0.0, "lam is zero: the multiplier rule would be unchecked"
  sd = max(1.0, float(np.abs(lam).mean()) / 100.0)                # the solver's multiplier scaling of the KKT error
  stat = float(np.abs(rr[inact]).max())
  stat_bound = 1e-4 * sd * max(1.0, float(np.abs(g).max())) * max(1.0, 1.0 / scale.min())
  fig = dict(feas=feas, feas_bound=feas_bound, cost_err=cost_err, stat=stat, stat_bound=stat_bound, stat_ratio=stat / stat_bound)
  assert feas <= feas_bound, ("feasibility", fig)
  assert cost_err <= 1e-11, ("cost", float(cost), f, fig)
  assert stat <= stat_bound, ("stationarity", fig)
  return fig


def check_cost_agreement(cost_scaled, cost_unit):
  """two solves of one problem, same solver form: the project's figure for that is 1e-6 (the host twin's worst is 5e-8)"""
  d = abs(cost_scaled - cost_unit) / max(1.0, abs(cost_unit))
  assert d <= 1e-6, ("cost against the unit-scale solve", float(cost_scaled), float(cost_unit), d)
  return d


# ---- the elastic twins --------------------------------------------------------------------------------------------------------
# Under a scale a twin does NOT solve the same problem: its penalty is rho/2 sum (s_i / sc_i)^2 with sc_i the slack's own scale entry
# (tools/gen_systems.py), which oracle.Elastic restates with slack_scale.  Both rules from the FIRST problem of the elastic phase
# (tests/test_gpu_elastic.py: the base system's guess and bounds widened by free slacks s = 0, rho = 1).
TWIN_BASES = ("CARTPOLE", "VANDERPOL")
TWIN_SHAPES = {"hs8": ("HERMITE_SIMPSON", 8), "trap9": ("TRAPEZOIDAL", 9)}
TWIN_CASES = tuple((b, k) for b in TWIN_BASES for k in TWIN_SHAPES)


def twin_scales(base_ns, base_nu):
  """[ns + nu + ns]: tied ODD (slack i takes state i's scale, as the library's own elastic phase sets it), and base 1 with slacks 4"""
  odd = ODD(base_ns + base_nu)
  return (("tiedODD", np.concatenate([odd, odd[:base_ns]])), ("slacks4", np.concatenate([np.ones(base_ns + base_nu), np.full(base_ns, 4.0)])))


@functools.lru_cache(maxsize=None)
def _twin_first_problem(base, shape):
  rule, N = TWIN_SHAPES[shape]
  b = O.SYSTEMS[base]()
  mk = O.hermite_simpson if rule == "HERMITE_SIMPSON" else O.trapezoidal
  trb, trt = mk(b, N), mk(O.Elastic(b, 1.0), N)
  nx, u_rows = trb.x_rows * b.ns, trb.u_rows
  def widen(v, fill):
    return np.concatenate([v[:nx], np.hstack([v[nx:].reshape(u_rows, b.nu), np.full((u_rows, b.ns), fill)]).ravel()])
  z0, lb, ub = widen(trb.guess, 0.0), widen(trb.bounds[:, 0], -np.inf), widen(trb.bounds[:, 1], np.inf)
  assert z0.size == trt.guess.size
  return b, z0, np.stack([lb, ub], axis=1)


def twin_problem(base, shape, slack_scale=None):
  """(twin system, transcription carrying the phase's first guess and bounds, callbacks) for the penalty rho/2 sum (s_i / slack_scale_i)^2"""
  rule, N = TWIN_SHAPES[shape]
  b, z0, bounds = _twin_first_problem(base, shape)
  s = O.Elastic(b, 1.0, slack_scale=slack_scale)
  tr = (O.hermite_simpson if rule == "HERMITE_SIMPSON" else O.trapezoidal)(s, N)
  tr = dataclasses.replace(tr, guess=z0, bounds=bounds)
  return s, tr, O.Callbacks(tr)
