"""The host side of the Gauss-Newton product family, without a device: the conjugate-gradient / Levenberg-Marquardt routines of
neural_ode/node_training.py on a dense random symmetric positive definite operator against numpy.linalg.solve, and the Engine.fit_gnvp* methods
against a recording fake of the library (tests/test_lib_binding.py's, restated): argument order, strides, null outputs."""
import re
import os
import types

import numpy as np
import pytest

from myriad_amd import _lib
from myriad_amd.experiments import mle_sysid
from myriad_amd.neural_ode import node_training as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spd(n, seed, cond=1e3):
  rng = np.random.default_rng(seed)
  Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
  return (Q * np.geomspace(1.0, cond, n)) @ Q.T, rng.standard_normal(n)


# ---- conjugate gradients -----------------------------------------------------------------------------------------------------------------
def test_cg_converges_to_the_dense_solve():
  A, b = _spd(30, 0)
  calls = []
  op = lambda v: (calls.append(1), A @ v)[1]
  d, products, residual = nt.conjugate_gradient(op, b, iters=200, tol=1e-12)
  assert products == len(calls) <= 60
  np.testing.assert_allclose(d, np.linalg.solve(A, b), rtol=1e-9, atol=1e-12)
  assert residual <= 1e-12
  assert abs(np.linalg.norm(b - A @ d) / np.linalg.norm(b) - residual) <= 1e-10      # the recurrence's residual is the true one


def test_cg_is_truncated_by_iterations_and_by_the_tolerance():
  A, b = _spd(30, 1)
  errs = []
  exact = np.linalg.solve(A, b)
  for iters in (1, 3, 7):
    d, products, residual = nt.conjugate_gradient(lambda v: A @ v, b, iters=iters, tol=0.0)
    assert products == iters
    np.testing.assert_allclose(np.linalg.norm(b - A @ d) / np.linalg.norm(b), residual, rtol=1e-9)
    errs.append(float((d - exact) @ A @ (d - exact)))      # the A-norm of the error falls with every product
  assert errs[0] > errs[1] > errs[2] > 0.0
  d1 = nt.conjugate_gradient(lambda v: A @ v, b, iters=1, tol=0.0)[0]
  np.testing.assert_allclose(d1, (b @ b) / (b @ A @ b) * b, rtol=1e-14)      # one product: the steepest-descent step
  d, products, residual = nt.conjugate_gradient(lambda v: A @ v, b, iters=200, tol=1e-2)
  assert residual <= 1e-2 and products < 30
  full = nt.ConjugateGradient(b, 200, 1e-2)
  while not full.done:
    before = full.residual
    full.feed(A @ full.p)
  assert before > 1e-2 >= full.residual                    # it stopped at the first iterate that passes
  # nothing to solve: no product is asked for
  assert nt.conjugate_gradient(lambda v: 1 / 0, np.zeros(5), 10, 1e-2)[:2][1] == 0
  assert nt.conjugate_gradient(lambda v: 1 / 0, b, 0, 1e-2)[1] == 0
  # a direction without positive curvature ends the solve at the iterate it has
  d, products, _ = nt.conjugate_gradient(lambda v: -v, b, 10, 1e-2)
  assert products == 1 and (d == 0.0).all()


# ---- Levenberg-Marquardt on it -------------------------------------------------------------------------------------------------------------
class _Quadratic:
  """loss(p) = c + g0 . p + p . G p / 2 with G positive definite: its Gauss-Newton matrix is G itself"""
  def __init__(self, n, seed):
    self.G, self.g0 = _spd(n, seed)
    self.star = np.linalg.solve(self.G, -self.g0)
    self.c = 1.0 - (self.g0 @ self.star + self.star @ self.G @ self.star / 2)      # so that the minimum is 1 > 0
  def value_grad(self, p):
    return float(self.c + self.g0 @ p + p @ self.G @ p / 2), self.g0 + self.G @ p


class _LowRankQuadratic:
  """the same in the 4 804 weights of the network, G = diag(d) + U U^T kept as its factors"""
  def __init__(self, seed, rank, top):
    rng = np.random.default_rng(seed)
    self.d, self.U, self.g0 = np.geomspace(1.0, top, 4804), rng.standard_normal((4804, rank)), rng.standard_normal(4804)
  def mul(self, v):
    return self.d * v + self.U @ (self.U.T @ v)
  def value_grad(self, p):
    Gp = self.mul(p)
    return float(1e4 + self.g0 @ p + p @ Gp / 2), self.g0 + Gp


def _run(lm, q, products=None):
  lm.begin(*q.value_grad(lm.params))
  trials = []
  while not lm.done:
    while lm.solving:
      if products is not None:
        products.append(1)
      lm.feed(q.G @ lm.direction())
    lm.end(*q.value_grad(lm.trial()))
    trials.append(lm.last)
  return trials


def test_lm_cg_steps_are_the_damped_dense_solves():
  q = _Quadratic(20, 2)
  lm = nt.LevenbergMarquardtCG(np.zeros(20), lam=1e-3, cg_iters=200, cg_tol=1e-13, max_iter=6)
  products = []
  trials = _run(lm, q, products)
  assert len(trials) <= 6 and sum(t["cg_products"] for t in trials) == len(products)
  lam, p = 1e-3, np.zeros(20)
  for t in trials:                                    # every accepted step: (G + lam I) d = -g, lam a third of the one before
    assert t["accepted"] and t["lam"] == lam
    np.testing.assert_allclose(t["d"], np.linalg.solve(q.G + lam * np.eye(20), -q.value_grad(p)[1]), rtol=1e-8, atol=1e-12)
    assert t["trial_loss"] < t["loss"]
    p, lam = p + t["d"], mle_sysid.lm_next_lambda(lam, True)
  np.testing.assert_allclose(lm.params, q.star, rtol=1e-6, atol=1e-9)
  assert lm.lam == lam


def test_lm_cg_truncated_steps_still_descend():
  q = _Quadratic(40, 3)
  lm = nt.LevenbergMarquardtCG(np.zeros(40), cg_iters=3, cg_tol=1e-2, max_iter=10)
  trials = _run(lm, q)
  assert len(trials) == 10 and all(t["cg_products"] <= 3 for t in trials) and any(t["cg_products"] == 3 for t in trials)
  assert all(t["accepted"] for t in trials)           # on a quadratic with its own matrix every conjugate-gradient iterate lowers the loss
  assert trials[-1]["trial_loss"] < trials[0]["loss"]


def test_lm_cg_rejects_then_raises_lambda():
  """a loss whose matrix overstates nothing but whose values are made worse on purpose at the first two trial points"""
  q = _Quadratic(10, 4)
  lm = nt.LevenbergMarquardtCG(np.zeros(10), lam=1e-3, cg_iters=50, cg_tol=1e-10, max_iter=5)
  value0, grad0 = q.value_grad(lm.params)
  lm.begin(value0, grad0)
  seen = []
  for k in range(5):
    while lm.solving:
      lm.feed(q.G @ lm.direction())
    trial = lm.trial()
    value, grad = q.value_grad(trial)
    accepted = lm.end(value0 + 1.0 if k < 2 else value, grad)
    seen.append((accepted, lm.last["lam"], lm.last["params"].copy(), lm.last["d"].copy()))
  assert [s[0] for s in seen] == [False, False, True, True, True]
  assert [s[1] for s in seen[:4]] == [1e-3, 4e-3, 16e-3, 16e-3 / 3.0]      # times four on rejection, a third on acceptance: mle_sysid's rule
  for s in seen[:3]:                                  # a rejected point is left where it was and solved again with the larger lam
    assert (s[2] == 0.0).all()
    np.testing.assert_allclose(s[3], np.linalg.solve(q.G + s[1] * np.eye(10), -grad0), rtol=1e-7, atol=1e-12)
  assert np.linalg.norm(seen[1][3]) < np.linalg.norm(seen[0][3])
  assert lm.done and lm.iterations == 5
  # the rule is the one LevenbergMarquardt applies
  ref = mle_sysid.LevenbergMarquardt({"a": 1.0}, lam=1e-3)
  ref.begin(2.0, {"a": 1.0}, [[1.0]])
  ref.trial()
  assert ref.end(3.0, {"a": 1.0}, [[1.0]]) is False and ref.lam == mle_sysid.lm_next_lambda(1e-3, False) == 4e-3
  ref.trial()
  assert ref.end(1.0, {"a": 1.0}, [[1.0]]) is True and ref.lam == 4e-3 / 3.0
  assert mle_sysid.lm_accepts(1.0, 1.0) is False


def test_lockstep_models_equal_their_own_runs():
  """_gn_lockstep with two models of different length of solve: each gets the arithmetic of its run alone; the finished solve rides along with 0"""
  hp = types.SimpleNamespace(loss_recording_frequency=1, early_stop_check_frequency=1, early_stop_threshold=30)
  qs = [_LowRankQuadratic(5, 3, 50.0), _LowRankQuadratic(6, 0, 1.0)]      # (the second: the identity, solved by one product)
  rode = []

  def drive(sets_of):
    lms = [nt.LevenbergMarquardtCG(np.zeros(4804), cg_iters=4, cg_tol=1e-1, max_iter=3) for _ in sets_of]
    hist = [[] for _ in sets_of]
    def products(sets, P, V):
      rode.extend(not V[i].any() for i in range(len(sets)))
      return [qs[sets_of[e]].mul(V[i]) for i, e in enumerate(sets)]
    def value_grads(sets, P):
      vg = [qs[sets_of[e]].value_grad(P[i]) for i, e in enumerate(sets)]
      return [v for v, _ in vg], [g for _, g in vg]
    out = nt._gn_lockstep(hp, lms, value_grads, products, lambda sets, P: [qs[sets_of[e]].value_grad(P[i])[0] for i, e in enumerate(sets)], False, hist)
    return out, hist

  both, hist = drive([0, 1])
  assert any(rode)
  for e in range(2):
    alone, h1 = drive([e])
    assert alone[0][1:] == both[e][1:] and alone[0][1] == 3 and [r[0] for r in alone[0][2]] == [0, 1, 2, 3]
    for k in ("linear", "linear_1", "linear_2"):
      assert alone[0][0][k]["w"].tobytes() == both[e][0][k]["w"].tobytes()
    assert [t["d"].tobytes() for t in h1[0]] == [t["d"].tobytes() for t in hist[e]]
  assert [t["cg_products"] for t in hist[0]] != [t["cg_products"] for t in hist[1]]


# ---- the binding, against a recording fake ---------------------------------------------------------------------------------------------------
NS, NU, NP = 4, 1, 4804
B, E, R, S, U = 3, 2, 2, 4, 6
HOST, DEVICE = _lib.MEM_HOST, _lib.MEM_DEVICE
ORDER = {
  "myr_fit_gnvp": ("B", "num_steps", "u_rows", "xs_obs", "us", "wt", "params", "v", "jv", "out", "out_stride", "mem"),
  "myr_fit_gnvp_sets": ("E", "R", "num_steps", "u_rows", "xs_obs", "us", "data_shared", "wt", "params", "v", "jv", "out", "out_stride", "mem"),
}


class FakeLib:
  """every attribute is a C function that records its call and returns MYR_OK"""
  def __init__(self):
    self.calls = []

  def __getattr__(self, name):
    def fn(*args):
      self.calls.append((name, args))
      return 0
    return fn


@pytest.fixture
def engine(monkeypatch):
  monkeypatch.setattr(_lib, "_addr", lambda a: a)      # the arrays themselves reach the fake
  eng = object.__new__(_lib.Engine)
  eng.lib, eng._h = FakeLib(), types.SimpleNamespace(value=0)
  eng.ns, eng.nu, eng.np = NS, NU, NP
  return eng


def _last(eng, fn):
  assert len(eng.lib.calls) == 1, eng.lib.calls
  name, args = eng.lib.calls.pop()
  assert name == fn and args[0] is eng._h and len(args) == 1 + len(ORDER[fn])
  return dict(zip(ORDER[fn], args[1:]))


def _shape(a):
  return None if a is None else a.shape


def test_fit_gnvp_host_forms(engine):
  eng, rng = engine, np.random.default_rng(0)
  xs_obs, us, p, v = rng.standard_normal((B, S + 1, NS)), rng.standard_normal((B, U, NU)), rng.standard_normal(NP), rng.standard_normal(NP)
  for reduce in (False, True):
    for want_jv in (False, True):
      for want_out in (True, False):
        for wt in (None, np.ones(S + 1)):
          out = eng.fit_gnvp(xs_obs, us, p, v, wt=wt, reduce=reduce, want_jv=want_jv, want_out=want_out)
          a = _last(eng, "myr_fit_gnvp")
          assert (a["B"], a["num_steps"], a["u_rows"], a["out_stride"], a["mem"]) == (B, S, U, 0 if reduce else NP, HOST)
          assert all(isinstance(a[k], int) for k in ("B", "num_steps", "u_rows", "out_stride"))
          assert a["xs_obs"].shape == (B, S + 1, NS) and a["us"].shape == (B, U, NU) and a["params"].shape == (NP,) and a["v"].shape == (NP,)
          assert (a["params"] == p).all() and (a["v"] == v).all() and _shape(a["wt"]) == (None if wt is None else (S + 1,))
          assert _shape(a["jv"]) == ((B, S + 1, NS) if want_jv else None)
          assert _shape(a["out"]) == ((((NP,) if reduce else (B, NP))) if want_out else None)
          assert set(out) == ({"out"} if want_out else set()) | ({"jv"} if want_jv else set())
          assert all(out[k] is a[k] for k in out)
  out = eng.fit_gnvp(xs_obs[0], us[0], p, v)           # one trajectory without its batch axis
  assert _last(eng, "myr_fit_gnvp")["B"] == 1 and out["out"].shape == (1, NP)
  for bad in (lambda: eng.fit_gnvp(xs_obs, us[:2], p, v), lambda: eng.fit_gnvp(xs_obs, us, p[:-1], v), lambda: eng.fit_gnvp(xs_obs, us, p, v[None]),
              lambda: eng.fit_gnvp(xs_obs, us, p, v, wt=np.ones(S)), lambda: eng.fit_gnvp(xs_obs[:, :1], us, p, v)):
    with pytest.raises(ValueError):
      bad()
  assert not eng.lib.calls


def test_fit_gnvp_sets_host_forms(engine):
  eng, rng = engine, np.random.default_rng(1)
  P, V = rng.standard_normal((E, NP)), rng.standard_normal((E, NP))
  for shared in (False, True):
    lead = () if shared else (E,)
    xs_obs, us = rng.standard_normal(lead + (R, S + 1, NS)), rng.standard_normal(lead + (R, U, NU))
    for reduce in (False, True):
      for want_jv in (False, True):
        for want_out in (True, False):
          out = eng.fit_gnvp_sets(xs_obs, us, P, V, wt=np.ones(S + 1), reduce=reduce, want_jv=want_jv, want_out=want_out)
          a = _last(eng, "myr_fit_gnvp_sets")
          assert (a["E"], a["R"], a["num_steps"], a["u_rows"], a["data_shared"], a["out_stride"], a["mem"]) == (E, R, S, U, int(shared), 0 if reduce else NP, HOST)
          assert isinstance(a["data_shared"], int)
          assert a["xs_obs"].shape == lead + (R, S + 1, NS) and a["us"].shape == lead + (R, U, NU) and a["wt"].shape == (S + 1,)
          assert (a["params"] == P).all() and (a["v"] == V).all()
          assert _shape(a["jv"]) == ((E, R, S + 1, NS) if want_jv else None)
          assert _shape(a["out"]) == (((E, NP) if reduce else (E, R, NP)) if want_out else None)
          assert set(out) == ({"out"} if want_out else set()) | ({"jv"} if want_jv else set())
          assert all(out[k] is a[k] for k in out)
  for bad in (lambda: eng.fit_gnvp_sets(xs_obs, us, P, V[:1]), lambda: eng.fit_gnvp_sets(xs_obs, us, P[0], V[0]),
              lambda: eng.fit_gnvp_sets(xs_obs[None], us, P, V)):
    with pytest.raises(ValueError):
      bad()
  assert not eng.lib.calls


def test_fit_gnvp_device_forms(engine):
  eng = engine
  t = {k: object() for k in ("xs_obs", "us", "params", "v", "jv", "out", "wt")}
  eng.fit_gnvp_device(B, S, U, t["xs_obs"], t["us"], t["params"], t["v"], jv=t["jv"], out=t["out"], out_stride=NP, wt=t["wt"])
  a = _last(eng, "myr_fit_gnvp")
  assert all(a[k] is t[k] for k in t) and (a["B"], a["num_steps"], a["u_rows"], a["out_stride"], a["mem"]) == (B, S, U, NP, DEVICE)
  eng.fit_gnvp_device(B, S, U, t["xs_obs"], t["us"], t["params"], t["v"], out=t["out"])
  a = _last(eng, "myr_fit_gnvp")
  assert a["jv"] is None and a["wt"] is None and a["out"] is t["out"] and a["out_stride"] == 0
  eng.fit_gnvp_sets_device(E, R, S, U, t["xs_obs"], t["us"], t["params"], t["v"], jv=t["jv"], data_shared=True)
  a = _last(eng, "myr_fit_gnvp_sets")
  assert (a["E"], a["R"], a["data_shared"], a["out_stride"], a["mem"]) == (E, R, 1, 0, DEVICE) and a["out"] is None and a["jv"] is t["jv"]
  assert a["params"] is t["params"] and a["v"] is t["v"]


def test_the_signature_table_covers_the_new_exports():
  """every exported function has its signature in the table load() reads, the two new ones with the argument count of the header's prototypes"""
  table = _lib._SIGNATURES
  assert set(table) == set(_lib.EXPORTS) and list(table) == _lib.EXPORTS
  header = open(os.path.join(ROOT, "include", "myriad_hip.h")).read()
  for fn, names in ORDER.items():
    assert len(table[fn][0]) == 1 + len(names), fn
    proto = re.search(r"\nint %s\((.*?)\);" % fn, header, re.S).group(1)
    assert len(proto.split(",")) == 1 + len(names), fn
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")][1:] == list(names), fn      # ... and their names, in order
  declared = set(re.findall(r"\n(?:int|int32_t|void|const char\*) (myr_\w+)\(", header))
  assert declared == set(table), declared ^ set(table)


def test_gn_product_passes_the_loss_weights(monkeypatch):
  """NodeFitLoss.gn_product / gn_products: the 1 / (n (S+1) ns) weights of value_and_grad, the reduced product"""
  seen = {}
  class Eng:
    def fit_gnvp(self, xs, us, p, v, wt, reduce):
      seen.update(single=(xs.shape, us.shape, p.shape, v.shape, wt.copy(), reduce))
      return {"out": np.ones(NP)}
    def fit_gnvp_sets(self, xs, us, P, V, wt, reduce):
      seen.update(sets=(xs.shape, us.shape, P.shape, V.shape, wt.copy(), reduce))
      return {"out": np.ones((P.shape[0], NP))}
  fit = nt.NodeFitLoss(types.SimpleNamespace(state_size=NS), 1.0, engine=Eng())
  mb = np.zeros((3, S + 1, NS + NU))
  assert fit.gn_product(np.zeros(NP), np.zeros(NP), mb).shape == (NP,)
  assert seen["single"][:4] == ((3, S + 1, NS), (3, S + 1, NU), (NP,), (NP,)) and seen["single"][5] is True
  assert (seen["single"][4] == 1.0 / (3 * (S + 1) * NS)).all() and seen["single"][4].shape == (S + 1,)
  assert fit.gn_products(np.zeros((2, NP)), np.zeros((2, NP)), np.zeros((2, 3, S + 1, NS + NU))).shape == (2, NP)
  assert seen["sets"][:4] == ((2, 3, S + 1, NS), (2, 3, S + 1, NU), (2, NP), (2, NP)) and (seen["sets"][4] == 1.0 / (3 * (S + 1) * NS)).all()
