"""GPU tests of the variable scaling of the solve path (include/myriad_hip.h: myr_set_var_scale): every solver form -- the lane kernels, round 2's
wavefront kernel, the fused kernel with one and two wavefronts, the shooting wavefront kernel -- under unit scales, powers of two and a vector that
is neither (tests/var_scale_cases.py), each returned (z, lam, cost) held to the KKT conditions of the oracle's UNSCALED transcription by the checker
the host twin's test uses (tests/test_var_scale_host_twin.py); the elastic twins against their weighted penalty; and the entry points and the
scheduling (batches of start states, two-phase launch, myr_solve_x0, handle state, restoration, error returns) under a scale."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import var_scale_cases as V
from myriad_amd import _lib

COLLOC_FORMS = {"lane": {"MYRIAD_SOLVE_MODE": "lane"}, "wave1": {"MYRIAD_SOLVE_MODE": "wave1"}, "fused1": {"MYRIAD_FUSED_WAVES": "1"},
                "fused2": {"MYRIAD_FUSED_WAVES": "2"}}      # the forms of tests/test_gpu_solve.py::_BOUND_FORMS
SHOOT_FORMS = {"wave": {"MYRIAD_SOLVE_MODE": "wave"}, "lane": {"MYRIAD_SOLVE_MODE": "lane"}}
TWIN_FORMS = {"default": {}, "lane": {"MYRIAD_SOLVE_MODE": "lane"}}
_ENV = ("MYRIAD_FUSED_WAVES", "MYRIAD_SOLVE_MODE", "MYRIAD_POISON", "MYRIAD_PARK_ITER", "MYRIAD_VAR_SCALE", "MYRIAD_ELASTIC", "MYRIAD_SECOND_STARTS",
        "MYRIAD_DELTA_WARM", "MYRIAD_MU_INIT")
# (case, form) pairs that do not converge on the device at UNIT scale (one attempt, 500 iterations) are no cases of that form: none was found
# (profiles/r19_var_scale/README.md).  A pair that fails only under a scale is never listed here: that failure is the finding.
LEFT_OUT = frozenset()
BITS = ("z", "lam", "cost", "status", "iters")


def forms_of(shape):
  return SHOOT_FORMS if V.SHAPES[shape][0] == "SHOOTING" else COLLOC_FORMS


def set_form(monkeypatch, env):
  for k in _ENV:
    monkeypatch.delenv(k, raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)


def one_attempt(eng, max_iter=V.MAX_ITER):
  o = eng.default_opts(); o.restoration = 0; o.restarts = 0; o.max_iter = max_iter
  return o


def bits(r, keys=BITS):
  return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in keys)


def solve_rows(eng, tr, scale, params=None, B=2):
  """B identical rows of the transcription's own guess and bounds, in the ORIGINAL variables, under `scale` (None: unscaled)"""
  eng.set_var_scale(scale)
  return eng.solve(np.tile(tr.guess, (B, 1)), np.tile(tr.bounds[:, 0], (B, 1)), np.tile(tr.bounds[:, 1], (B, 1)), params=params, opts=one_attempt(eng))


def check_rows(tag, tr, cb, scale, r):
  """both rows carry the same bits; row 0 is a KKT point of the unscaled problem; kkt[][0] (measured in scaled states) times the largest state
  scale bounds the oracle's max |c| (c = s o c_s row by row), up to the rounding of c at z: 1e-12 max(1, |z|), the term of the checker's own bound"""
  print(tag, "status", r["status"], "iters", r["iters"], "cost %.12g" % r["cost"][0], "kkt", r["kkt"][0])
  for k in BITS + ("kkt",):
    assert np.array_equal(r[k][0], r[k][1], equal_nan=True), (tag, "the two rows differ in", k)
  fig = V.check_original_kkt(tr, cb, scale, r["z"][0], r["lam"][0], r["cost"][0], r["status"][0])
  print("   feas %.2e (bound %.2e)  stat %.2e (bound %.2e, ratio %.2e)  cost err %.1e" % (fig["feas"], fig["feas_bound"], fig["stat"], fig["stat_bound"],
                                                                                          fig["stat_ratio"], fig["cost_err"]))
  smax = 1.0 if scale is None else float(np.max(scale[:tr.ns]))
  assert fig["feas"] <= r["kkt"][0, 0] * smax + 1e-12 * max(1.0, float(np.abs(r["z"][0]).max())), (tag, "kkt[0] does not bound max|c|", fig["feas"], r["kkt"][0, 0], smax)
  return fig


@pytest.mark.parametrize("sysname,shape", V.CASES, ids=[f"{s}-{k}" for s, k in V.CASES])
def test_every_solver_form_solves_the_original_problem_under_a_scale(monkeypatch, sysname, shape):
  rule, N, cpi, method = V.SHAPES[shape]
  s, tr, cb = V.problem(sysname, shape)
  for form, env in forms_of(shape).items():
    if (sysname, shape, form) in LEFT_OUT:
      continue
    set_form(monkeypatch, env)
    eng = _lib.Engine(sysname, rule, N, s.T, controls_per_interval=cpi, integration_method=method)
    unit = None
    for tag, mk in V.SCALES:
      scale = None if mk is None else mk(tr.ns + tr.nu)
      r = solve_rows(eng, tr, scale)
      check_rows(f"{sysname} {shape} {form} {tag}", tr, cb, scale, r)
      if unit is None:
        unit = r["cost"][0]
      elif V.cost_agreement_applies(sysname, shape):
        print("   cost against the unit solve %.2e" % V.check_cost_agreement(r["cost"][0], unit))
    eng.close()


@pytest.mark.parametrize("base,shape", V.TWIN_CASES, ids=[f"{b}-{k}" for b, k in V.TWIN_CASES])
def test_twin_handles_solve_the_weighted_penalty_problem_under_a_scale(monkeypatch, base, shape):
  """A twin handle under a scale solves the problem with the penalty rho/2 sum (s_i / sc_i)^2 (include/myriad_hip.h), from the first problem of the
  elastic phase: tied scales (slack i takes state i's, what the phase itself sets) and slack scales alone; the wavefront form the library picks
  (CARTPOLE's twin: the wide-stage block sweep, 9 variables per point) and the lane kernel.  The cost returned is NOT the unweighted twin's."""
  rule, N = V.TWIN_SHAPES[shape]
  b, tr0, cb0 = V.twin_problem(base, shape)
  nw = b.base.ns + b.base.nu
  for form, env in TWIN_FORMS.items():
    set_form(monkeypatch, env)
    eng = _lib.Engine(base + "_ELASTIC", rule, N, b.T)
    for tag, scale in V.twin_scales(b.base.ns, b.base.nu):
      s, tr, cb = V.twin_problem(base, shape, tuple(scale[nw:]))
      r = solve_rows(eng, tr, scale, params=s.params())
      check_rows(f"{base}_ELASTIC {shape} {form} {tag}", tr, cb, scale, r)
      assert abs(r["cost"][0] - cb0.fun(r["z"][0])) > 1e-3
    eng.close()


# ---- entry points and scheduling under a scale: CARTPOLE, Hermite-Simpson, N = 8, the ODD scale ----
N8, B70 = 8, 70


def _cartpole(monkeypatch, env=None, scale="ODD"):
  set_form(monkeypatch, env or {})
  s, tr, cb = V.problem("CARTPOLE", "hs8")
  eng = _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", N8, s.T)
  if scale == "ODD":
    eng.set_var_scale(V.ODD(5))
  return s, tr, cb, eng


def _batch():
  from bench import build_workload
  return build_workload(B70, N8, 2019)      # x0, z0, lb, ub, T


def test_batch_of_start_states_under_a_scale(monkeypatch):
  """70 x 85 variables: the scaling kernels run several blocks, the last one partial.  Every row converges, its cost is myr_eval's f at the returned z,
  and rows of the first, a middle and the partial last block are KKT points of their own unscaled problems."""
  s, tr, cb, eng = _cartpole(monkeypatch)
  x0, z0, lb, ub, T = _batch()
  r = eng.solve(z0, lb, ub, opts=one_attempt(eng))
  print("status", np.bincount(r["status"]), "iters", r["iters"].min(), r["iters"].max())
  assert (r["status"] == 0).all(), (r["status"], r["iters"])
  f = eng.eval(r["z"], want=("f",))["f"]
  np.testing.assert_allclose(r["cost"], f, rtol=1e-11, atol=0.0)
  for b in (0, 33, 69):
    trb = dataclasses.replace(tr, bounds=np.stack([lb[b], ub[b]], axis=1), guess=z0[b])
    fig = V.check_original_kkt(trb, cb, V.ODD(5), r["z"][b], r["lam"][b], r["cost"][b], r["status"][b])
    print("row", b, fig)


def test_two_phase_launch_gives_the_same_bits_under_a_scale(monkeypatch):
  """park_iter = 3 against whole solves (-1) on the scaled handle: "the same, bit for bit" (include/myriad_hip.h: park_iter)"""
  s, tr, cb, eng = _cartpole(monkeypatch, {"MYRIAD_FUSED_WAVES": "1"})
  x0, z0, lb, ub, T = _batch()
  out = {}
  for k in (-1, 3):
    o = one_attempt(eng); o.park_iter = k
    r = eng.solve(z0, lb, ub, opts=o)
    assert (r["status"] == 0).all()
    out[k] = bits(r)
  assert out[3] == out[-1]


def test_solve_x0_gives_the_bits_of_solve_under_a_scale(monkeypatch):
  s, tr, cb, eng = _cartpole(monkeypatch)
  x0, z0, lb, ub, T = _batch()
  K = 2 * N8 + 1
  lin = np.linspace(0.0, 1.0, K)
  g0 = np.zeros(tr.guess.size); g1 = np.zeros(tr.guess.size)
  g0[:K * 4] = (s.x_T[None, :] * lin[:, None]).ravel(); g1[:K * 4] = np.repeat(1 - lin, 4)
  ref = eng.solve(z0, lb, ub, opts=one_attempt(eng))
  got = eng.solve_x0(x0, g0, g1, lb[0], ub[0], opts=one_attempt(eng))
  assert (ref["status"] == 0).all()
  for k in BITS + ("kkt",):
    assert np.array_equal(ref[k], got[k]), k


def test_the_scale_is_state_of_the_handle(monkeypatch):
  """set_var_scale(None) after a scaled solve: the bits of a fresh unscaled handle; all ones: the bits of None; set twice: the second holds"""
  s, tr, cb, eng = _cartpole(monkeypatch)
  x0, z0, lb, ub, T = _batch()
  z0, lb, ub = z0[:5], lb[:5], ub[:5]
  run = lambda e: e.solve(z0, lb, ub, opts=one_attempt(e))
  odd = run(eng)
  eng.set_var_scale(None)
  back = run(eng)
  eng.set_var_scale(np.ones(5))
  ones = run(eng)
  eng.set_var_scale(V.P2(5)); eng.set_var_scale(V.ODD(5))
  twice = run(eng)
  _, _, _, fresh = _cartpole(monkeypatch, scale=None)
  ref = run(fresh)
  assert (ref["status"] == 0).all() and (odd["status"] == 0).all()
  assert bits(back) == bits(ref) and bits(ones) == bits(ref)
  assert bits(twice) == bits(odd) and bits(odd) != bits(ref)


def test_restoration_under_a_scale(monkeypatch):
  """PENDULUM from the reference's guess needs the elastic phase (tests/test_gpu_elastic.py); here with state scales (4, 0.5) and control scale 2, which
  the phase hands on to the twin.  Whatever the outcome it is reported consistently, z stays finite and inside its bounds, and a converged row is a KKT
  point of PENDULUM's own unscaled transcription.  (Whether the scaled run is restored is printed, not asserted: profiles/r19_var_scale/README.md.)"""
  from oracle import myriad_oracle as O
  set_form(monkeypatch, {})
  p = O.SYSTEMS["PENDULUM"]()
  tr = O.hermite_simpson(p, 20)
  cb = O.Callbacks(tr)
  scale = np.array([4.0, 0.5, 2.0])
  eng = _lib.Engine("PENDULUM", "HERMITE_SIMPSON", 20, p.T)
  lb, ub = tr.bounds[:, 0], tr.bounds[:, 1]
  for tag, sc in (("unit", None), ("scaled", scale)):
    eng.set_var_scale(sc)
    r = eng.solve(tr.guess[None], lb[None], ub[None])
    print("PENDULUM", tag, "status", r["status"], "iters", r["iters"], "restored", r["restored"], "attempts", r["attempts"], "start", r["start"], "cost", r["cost"])
    z = r["z"][0]
    assert np.isfinite(z).all()
    assert (z >= lb - 1e-12 * np.maximum(1.0, np.abs(lb))).all() and (z <= ub + 1e-12 * np.maximum(1.0, np.abs(ub))).all()
    if r["restored"][0]:
      assert r["attempts"][0] >= 4
    if r["status"][0] == 0:
      print("   ", V.check_original_kkt(tr, cb, sc, z, r["lam"][0], r["cost"][0], r["status"][0]))


def test_error_returns_of_set_var_scale(monkeypatch):
  """through the raw ABI: a refused vector leaves the previous scale in force (the next solve gives the bits of the one before), NODE handles take no scale"""
  s, tr, cb, eng = _cartpole(monkeypatch)
  x0, z0, lb, ub, T = _batch()
  z0, lb, ub = z0[:3], lb[:3], ub[:3]
  before = bits(eng.solve(z0, lb, ub, opts=one_attempt(eng)))
  lib = eng.lib
  for i, bad in ((0, 0.0), (1, -1.0), (2, float("nan")), (3, 1e300), (4, float("inf")), (4, 0.0)):
    v = V.P2(5); v[i] = bad
    assert lib.myr_set_var_scale(eng._h, v.ctypes.data) == -1, (i, bad)                      # MYR_E_ARG
    assert b"scales must be positive and finite" in lib.myr_last_error()
    assert bits(eng.solve(z0, lb, ub, opts=one_attempt(eng))) == before, (i, bad)
  assert lib.myr_set_var_scale(None, None) == -1 and lib.myr_set_var_scale(None, V.P2(5).ctypes.data) == -1      # null handle: MYR_E_ARG
  node = _lib.Engine("NODE_CARTPOLE", "HERMITE_SIMPSON", 3, 2.0)
  assert lib.myr_set_var_scale(node._h, V.P2(5).ctypes.data) == -2                           # MYR_E_UNSUPPORTED
  assert lib.myr_set_var_scale(node._h, None) == 0
  with pytest.raises(ValueError):
    eng.set_var_scale(np.ones(4))                                                            # the binding checks the length
