"""The references of test_gpu_eval_matrix.py checked on themselves, without a device (tests/eval_cases.py): every case of the matrix exists, is
finite and answers one ulp of its inputs with less than a tenth of the ceiling; the oracle's dense J goes through the device's block layout and back
unchanged, so that nothing of it lies outside the pattern the blocks can express; J and grad f agree with central differences; single shooting is
the rollout; the rollout's control-row rules are the clamp and `us[-1]`; and the capacity edge is where hs_eval_lds_bytes puts it."""
import numpy as np
import pytest
import torch

import eval_cases as EC
from eval_cases import O
from myriad_amd.trajectory_optimizers import hs_dense_from_blocks, shoot_dense_from_blocks, trap_dense_from_blocks

EPS = 2.0 ** -52
# central differences with step FD_STEP max(1, |z_i|): truncation FD_STEP^2 |d3| / 6 and rounding eps |value| / FD_STEP, 2e-10 of the value --
# held to FD_TOL of the largest of 1, the value and the derivative
FD_STEP, FD_TOL = 1e-6, 1e-6

PARITY = EC.parity_cases()
ROLLOUT_PARITY = EC.rollout_parity_cases()
ROWS = EC.rows_cases()


def _conditioned(c, ident):
  listed = EC.ILL_CONDITIONED if "z" in c else EC.ROLLOUT_ILL_CONDITIONED
  if ident in listed:
    assert max(c["response"].values()) > EC.MAX_RESPONSE, (ident, "is listed as ill-conditioned and is not", c["response"])
  else:
    assert max(c["response"].values()) <= EC.MAX_RESPONSE, (ident, c["response"])


def _blocks_and_back(c, J):
  """the oracle's dense J -> the device's blocks -> dense"""
  N, ns, nu = c["N"], c["ns"], c["nu"]
  if c["tr"] == "HERMITE_SIMPSON":
    return hs_dense_from_blocks(O.hs_blocks_from_dense(J, N, ns, nu), N, ns, nu)
  blk = []
  for k in range(N):
    r = slice(k * ns, (k + 1) * ns)
    if c["tr"] == "TRAPEZOIDAL":
      u0 = (N + 1) * ns + k * nu
      parts = [J[r, k * ns:(k + 1) * ns], J[r, (k + 1) * ns:(k + 2) * ns], J[r, u0:u0 + nu], J[r, u0 + nu:u0 + 2 * nu]]
    else:
      W = EC.mc(c) * c["cpi"]
      u0 = (N + 1) * ns + k * W * nu
      parts = [J[r, k * ns:(k + 1) * ns], J[r, u0:u0 + (W + 1) * nu]]
    blk.append(np.concatenate([p.ravel() for p in parts]))
  blk = np.stack(blk)
  return trap_dense_from_blocks(blk, N, ns, nu) if c["tr"] == "TRAPEZOIDAL" else shoot_dense_from_blocks(blk, N, EC.mc(c) * c["cpi"], ns, nu)


def _central(fun, z):
  cols = []
  for i in range(z.size):
    d = FD_STEP * max(1.0, abs(z[i]))
    zp, zm = z.copy(), z.copy()
    zp[i] += d
    zm[i] -= d
    cols.append((fun(zp) - fun(zm)) / (zp[i] - zm[i]))
  return np.stack(cols, axis=-1)


@pytest.mark.parametrize("ident,thunk", PARITY, ids=[i for i, _ in PARITY])
def test_eval_parity_case(ident, thunk):
  c = thunk()
  ref = EC.eval_reference(c)
  B = c["z"].shape[0]
  assert B == EC.B and c["rows"] == tuple(range(B))
  assert ref["f"].shape == (B, 1) and ref["gradf"].shape == (B, c["n"]) and ref["c"].shape == (B, c["m"]) and ref["J"].shape == (B, c["m"] * c["n"])
  for k, a in ref.items():
    assert np.isfinite(a).all(), k
    assert not a.flags.writeable
  _conditioned(c, ident)
  if c["kind"] != "node":
    assert c["params"].shape[0] == B and (c["params"][0] != c["params"][1]).any()      # a parameter row per instance
  for b in range(B):
    J = ref["J"][b].reshape(c["m"], c["n"])
    assert np.array_equal(_blocks_and_back(c, J), J), b      # nothing outside the block pattern, the implied identities exact
  # an independent check of J and grad f: central differences, on the first instance
  cb = O.Callbacks(EC.transcription(c, 0))
  z = c["z"][0].copy()
  J, cv = ref["J"][0].reshape(c["m"], c["n"]), ref["c"][0]
  assert np.abs(_central(cb.cons, z) - J).max() <= FD_TOL * max(1.0, np.abs(J).max(), np.abs(cv).max())
  g = _central(lambda x: np.array(cb.fun(x)), z)
  assert np.abs(g - ref["gradf"][0]).max() <= FD_TOL * max(1.0, np.abs(ref["gradf"][0]).max(), abs(ref["f"][0, 0]))


def test_the_matrices_are_the_ones_the_issue_names():
  import test_gpu_hvp
  assert EC.SHOOT_EXTRA_SYSTEMS == test_gpu_hvp.PARITY and len(EC.SYSTEMS) == 20
  ids = [i for i, _ in PARITY]
  assert len(ids) == len(set(ids)) == 20 * 5 + 8 * 2 + 5 + 5 * 4 + 5
  ids = [i for i, _ in ROLLOUT_PARITY]
  assert len(ids) == len(set(ids)) == 20 * 4 * 2 + 4 + 5 * 4 + 4
  assert len(ROWS) == 3 * 4 * 4
  assert set(EC.ILL_CONDITIONED) <= {i for i, _ in PARITY} and set(EC.ROLLOUT_ILL_CONDITIONED) <= set(ids)


@pytest.mark.parametrize("tr,N,cpi,method", [("HERMITE_SIMPSON", EC.HS_N, 1, "HEUN"), ("TRAPEZOIDAL", EC.TRAP_N, 1, "HEUN"), ("SHOOTING", 3, 2, "RK4")])
def test_timberharvest_case_discounts(tr, N, cpi, method):
  plain = EC.eval_case("closed", "TIMBERHARVEST", tr, N, cpi, method)
  disc = EC.eval_case("closed", "TIMBERHARVEST", tr, N, cpi, method, discounted=True)
  r = O.SYSTEMS["TIMBERHARVEST"].param_names.index("r")
  assert (disc["params"][:, r] == EC.DISCOUNT_R).all() and (np.abs(plain["params"][:, r]) == 0.0).all()
  assert (disc["z"] == plain["z"]).all()
  a, b = EC.eval_reference(plain), EC.eval_reference(disc)
  assert (np.abs(a["f"] - b["f"])[:, 0] > 1e-3 * np.abs(a["f"])[:, 0]).all()
  assert (np.abs(a["gradf"] - b["gradf"]).max(axis=1) > 1e-3 * np.abs(a["gradf"]).max(axis=1)).all()
  assert np.array_equal(a["c"], b["c"]) and np.array_equal(a["J"], b["J"])      # r stands in the cost alone


@pytest.mark.parametrize("name,tr,N", EC.FORM_CASES, ids=[f"{a}-{b}-{n}" for a, b, n in EC.FORM_CASES])
def test_form_case(name, tr, N):
  c = EC.form_case(name, tr, N)
  ref = EC.eval_reference(c)
  assert c["rows"] == (0, EC.B - 1) and all(np.isfinite(a).all() for a in ref.values())
  assert max(c["response"].values()) <= EC.MAX_RESPONSE
  rows = EC.jrows(c)
  assert (rows is None) == (N <= EC.DENSE_N)
  assert ref["J"].shape[1] == (c["m"] if rows is None else len(rows)) * c["n"]
  if rows is not None:      # the kept rows are those of the first and the last interval, each with its identity entries
    ns = c["ns"]
    J = ref["J"][0].reshape(len(rows), c["n"])
    assert (np.abs(J[:ns, :ns]).max(axis=1) > 0.4).all() and (np.abs(J[ns:2 * ns, (N - 1) * (2 if tr == "HERMITE_SIMPSON" else 1) * ns:]).max(axis=1) > 0.4).all()


def test_batch_and_capacity_cases():
  for c, rows in ([(EC.shoot_batch_case(*a), (0, 62, 64, 256)) for a in EC.SHOOT_BATCH_CASES] +
                  [(EC.colloc_batch_case(tr), (0, 36, 256)) for tr in ("HERMITE_SIMPSON", "TRAPEZOIDAL")] + [(EC.capacity_case(), (1,))]):
    assert c["rows"] == rows and max(c["response"].values()) <= EC.MAX_RESPONSE, EC.what(c)
    assert all(np.isfinite(a).all() for a in EC.eval_reference(c).values())
    assert len({a.tobytes() for a in c["z"]}) == c["z"].shape[0]
  for a in (("CARTPOLE", "RK4", 7), ("HARVEST", "HEUN", 40)):
    c = EC.rollout_batch_case(*a)
    assert c["rows"] == (0, 62, 64, 256) and max(c["response"].values()) <= EC.MAX_RESPONSE
    assert all(np.isfinite(x).all() for x in EC.rollout_reference(c).values())


def test_capacity_arithmetic():
  """hs_eval_lds_bytes (myriad_amd/csrc/hs_eval.h) for CARTPOLE Hermite-Simpson: records of REC = 29 doubles (x | f | A | B = 4 + 4 + 16 + 4, padded to
  an odd count) for K = 2 N + 1 points, rounded up to an even count; 100 stencil entries of 24 bytes; one partial sum per wavefront; 16 bytes"""
  def lds(N, wpt):
    K = 2 * N + 1
    return ((K * 29 + 1) & ~1) * 8 + 100 * 24 + wpt * 8 + 16
  c = EC.capacity_case()
  ns, nu = c["ns"], c["nu"]
  assert (2 * ns + ns * ns + ns * nu) | 1 == 29 and 5 * ns * ns + 5 * ns * nu == 100
  N = EC.CAPACITY_N
  assert N == 347 and lds(N, 8) == 163728 <= 160 * 1024
  assert all(lds(N + 1, w) > 160 * 1024 for w in (8, 4, 1)) and lds(N + 1, 8) == 164192
  assert c["N"] == N and c["z"].shape == (2, (2 * N + 1) * (ns + nu))


@pytest.mark.parametrize("name,N,lands", EC.STEP_DOWN)
def test_step_down_arithmetic(name, N, lands):
  """the same formula for any system: the horizon fits with `lands` wavefronts and with no more"""
  c = EC.form_case(name, "HERMITE_SIMPSON", N)
  ns, nu = c["ns"], c["nu"]
  rec, jpi = (2 * ns + ns * ns + ns * nu) | 1, 5 * ns * ns + 5 * ns * nu
  lds = lambda w: (((2 * N + 1) * rec + 1) & ~1) * 8 + jpi * 24 + w * 8 + 16
  assert [w for w in (8, 4, 1) if lds(w) <= 160 * 1024][0] == lands and lds(8) > 160 * 1024
  assert max(c["response"].values()) <= EC.MAX_RESPONSE and all(np.isfinite(a).all() for a in EC.eval_reference(c).values())


@pytest.mark.parametrize("method", EC.METHODS)
def test_timberharvest_rollout_discounts(method):
  plain, disc = (EC.rollout_case("closed", "TIMBERHARVEST", method, 40, discounted=d) for d in (False, True))
  a, b = EC.rollout_reference(plain), EC.rollout_reference(disc)
  assert np.array_equal(plain["us"], disc["us"]) and np.array_equal(a["xs"], b["xs"])
  assert (np.abs(a["cost"] - b["cost"]) > 1e-3 * np.abs(a["cost"])).all()


# ---- rollouts -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ident,thunk", ROLLOUT_PARITY + ROWS, ids=[i for i, _ in ROLLOUT_PARITY + ROWS])
def test_rollout_case(ident, thunk):
  c = thunk()
  ref = EC.rollout_reference(c)
  B, S = c["x0"].shape[0], c["S"]
  assert ref["xs"].shape == (B, S + 1, c["ns"]) and ref["cost"].shape == (B, 1) and np.array_equal(ref["xs"][:, 0], c["x0"])
  assert all(np.isfinite(a).all() and not a.flags.writeable for a in ref.values())
  _conditioned(c, ident)
  assert S * 0.05 >= c["T"] or c["name"] in ("BACTERIA", "HIVTREATMENT", "SEIR")      # fit_cases.horizon
  if c["kind"] != "node":
    assert (c["params"][0] != c["params"][1]).any()
  # the states through the oracle's other integrator (no time argument: no system's dynamics take one)
  s = EC.rollout_system(c, B - 1)
  with torch.no_grad():
    xs = O.integrate_time_independent(s.dynamics, torch.tensor(c["x0"][B - 1]), torch.tensor(c["us"][B - 1]), c["T"] / S, S, c["method"])[1].numpy()
  assert np.array_equal(xs, ref["xs"][B - 1])


@pytest.mark.parametrize("ident,thunk", ROWS, ids=[i for i, _ in ROWS])
def test_control_row_rules_of_the_oracle(ident, thunk):
  """a short array is the array with its last row repeated (the clamp); rows beyond the consumed ones do not reach the states, and reach the
  cost only as the second argument of the terminal cost"""
  c = thunk()
  ref = EC.rollout_reference(c)
  R, need = c["us"].shape[1], EC.consumed_rows(c["method"], c["S"])
  for b in range(c["x0"].shape[0]):
    us = c["us"][b]
    if R < need:
      other = EC.oracle_rollout(c, b, us=np.concatenate([us, np.repeat(us[-1:], need - R, axis=0)]))
      assert np.array_equal(other["xs"], ref["xs"][b]) and np.array_equal(other["cost"], ref["cost"][b])
    else:
      other = EC.oracle_rollout(c, b, us=us[:need])
      s = EC.rollout_system(c, b)
      assert np.array_equal(other["xs"], ref["xs"][b])
      if not s.terminal_cost:
        assert np.array_equal(other["cost"], ref["cost"][b])
      else:
        xe = torch.tensor(ref["xs"][b, -1])
        d = float(s.terminal_cost_fn(xe, torch.tensor(us[-1]))) - float(s.terminal_cost_fn(xe, torch.tensor(us[need - 1])))
        assert abs((ref["cost"][b, 0] - other["cost"][0]) - d) <= 4 * EPS * max(1.0, abs(ref["cost"][b, 0]))


class _TerminalInU:
  """a system with 0.3 |u_T|^2 added to its terminal cost: the stock terminal costs ignore their control argument"""
  def __init__(self, base):
    self.__dict__.update(base.__dict__)
    self._base = base
    self.terminal_cost = True
  def __getattr__(self, k):
    return getattr(self._base, k)
  def terminal_cost_fn(self, x_T, u_T, T=None):
    own = self._base.terminal_cost_fn(x_T, u_T) if self._base.terminal_cost else 0.0
    return own + 0.3 * (u_T ** 2).sum()


@pytest.mark.parametrize("method", EC.METHODS)
@pytest.mark.parametrize("name", EC.ROWS_SYSTEMS)
def test_single_shooting_is_the_rollout_on_the_oracle(name, method):
  """I = 1, cpi = S: the shooting objective at z = [x0, x1, us] is the rollout cost of (x0, us, S), and c = xs[S] - x1 -- CARTPOLE, BACTERIA
  (terminal cost) and HARVEST (time in the cost).  Where the two rules differ: shooting takes the terminal term on the integrated end state with the
  last of ITS control rows, the rollout with the last row of the array it is given; with a longer array and a terminal cost that sees u, the
  difference is that of the two terminal terms."""
  S = EC.ROWS_S
  need = EC.consumed_rows(method, S)
  c = EC.rollout_case("closed", name, method, S, 2 * S + 5)
  for b in range(c["x0"].shape[0]):
    for wrap in (False, True):
      s = EC.rollout_system(c, b)
      s = _TerminalInU(s) if wrap else s
      us = c["us"][b]
      tr = O.shooting(s, 1, S, method)
      with torch.no_grad():
        xs, cost = O.get_state_trajectory_and_cost(s, S, method, c["x0"][b], us[:need])
        xs_long, cost_long = O.get_state_trajectory_and_cost(s, S, method, c["x0"][b], us)
      x1 = xs[S] + 0.25
      z = O._t(np.concatenate([c["x0"][b], x1, us[:need].ravel()]))
      f, cv = float(tr.objective(z)), tr.constraints(z).numpy()
      tol = 4 * EPS * max(1.0, abs(cost))
      assert abs(f - cost) <= tol
      assert np.abs(cv - (xs[S] - x1)).max() <= 4 * EPS * max(1.0, np.abs(xs[S]).max())
      assert np.array_equal(xs_long, xs)
      d = 0.3 * float((us[-1] ** 2).sum() - (us[need - 1] ** 2).sum()) if wrap else 0.0
      assert abs((cost_long - f) - d) <= tol + 4 * EPS * abs(d)
      assert not wrap or abs(d) > 1e-3
