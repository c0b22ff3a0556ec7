"""The phase-1 fill of the two-phase launch (hs_solver_fused.h: ParkArgs).  A slot of launch 1 that finds no fresh ticket keeps
iterating the trajectory it holds and parks it at the first iteration top at which every trajectory of the batch has had its k1 iterations, instead
of parking it at k1 and leaving its SIMD idle until the slowest slot is done.  A scheduling matter only: every trajectory returns the bits of a whole
solve, whatever the number of slots, the batch, k1, and whatever it inherits (MYRIAD_POISON).

How the tests see the schedule: MYRIAD_PARK_DUMP writes the loop scalars of every record as parked, [B][NSCAL] doubles, and then four doubles --
NSCAL, the index of the parking iteration inside a record (HsFused::PK_IT: the iteration a parked trajectory stopped at, -1 for one that finished in
launch 1), the number of parked trajectories, and the device counter `reached` as launch 1 left it (read in the regular build, not a variant)."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("MYRIAD_FUSED_WAVES", "MYRIAD_SOLVE_MODE", "MYRIAD_POISON", "MYRIAD_PARK_ITER", "MYRIAD_PARK_FILL", "MYRIAD_PARK_SHIFT", "MYRIAD_PARK_DUMP", "MYRIAD_SOLVE_SLOTS",
         "MYRIAD_REG_FILL", "MYRIAD_STACK_FILL")
N = 12
_KEYS = ("xs_and_us", "lambda", "cost", "kkt", "status", "iters")      # z, lam, cost, kkt, status, iters
_whole = {}       # whole solves (MYRIAD_PARK_ITER=0), computed once per problem and never modified


def _solve(monkeypatch, env, system, rule, B, max_iter=300, same_x0=False, guess=None):
  """One batch on a fresh handle: restoration, second starts and the elastic phase off, one wavefront per trajectory."""
  from myriad_amd.config import Config, HParams, NLPSolverType, OptimizerType, QuadratureRule
  from myriad_amd.systems import SystemType
  from myriad_amd.trajectory_optimizers import get_optimizer
  for k in KNOBS:
    monkeypatch.delenv(k, raising=False)
  monkeypatch.setenv("MYRIAD_SECOND_STARTS", "0"); monkeypatch.setenv("MYRIAD_ELASTIC", "0"); monkeypatch.setenv("MYRIAD_FUSED_WAVES", "1")
  for k, v in env.items():
    monkeypatch.setenv(k, str(v))
  hp = HParams(system=SystemType[system], optimizer=OptimizerType.COLLOCATION, quadrature_rule=QuadratureRule[rule], intervals=N, nlpsolver=NLPSolverType.SQP)
  opt = get_optimizer(hp, Config(verbose=False, plot=False), hp.system())
  x0 = np.tile(opt.system.x_0, (B, 1)) * (1.0 if same_x0 else (1.0 + 0.01 * np.arange(B)[:, None]))
  o = opt.solve_batch(x0s=x0, max_iter=max_iter, guess=guess, second_starts=False)
  out = {k: np.array(o[k]) for k in _KEYS}
  out["bits"] = hashlib.sha1(b"".join(np.ascontiguousarray(out[k]).tobytes() for k in _KEYS)).hexdigest()
  opt.engine.close()
  return out


def _whole_solves(monkeypatch, system, rule, B, **kw):
  key = (system, rule, B) + tuple((k, v.tobytes() if k == "guess" else v) for k, v in sorted(kw.items()))
  if key not in _whole:
    _whole[key] = _solve(monkeypatch, {"MYRIAD_PARK_ITER": 0}, system, rule, B, **kw)
  return _whole[key]


def _dump(path, B):
  """(parking iteration per trajectory, trajectories parked, `reached`) of the launch that wrote `path`"""
  d = np.fromfile(path, dtype=np.float64)
  nscal, pk_it = int(d[-4]), int(d[-3])
  assert d.size == B * nscal + 4, (d.size, B, nscal)
  return d[:-4].reshape(B, nscal)[:, pk_it].astype(int), int(d[-2]), int(d[-1])


def _same(r, ref, tag):
  for k in _KEYS:
    assert np.array_equal(r[k], ref[k], equal_nan=True), (tag, k, r["status"], ref["status"], r["iters"], ref["iters"])
  assert r["bits"] == ref["bits"], tag


def _two_phase(monkeypatch, tmp_path, system, rule, slots, B, k1, fill, poison=None, **kw):
  path = tmp_path / "park.bin"
  env = {"MYRIAD_SOLVE_SLOTS": slots, "MYRIAD_PARK_ITER": k1, "MYRIAD_PARK_FILL": int(fill), "MYRIAD_PARK_DUMP": path}
  if poison: env["MYRIAD_POISON"] = poison
  r = _solve(monkeypatch, env, system, rule, B, **kw)
  it, parked, reached = _dump(path, B)
  path.unlink()
  return r, it, parked, reached


@pytest.mark.parametrize("system,rule", [("CARTPOLE", "HERMITE_SIMPSON"), ("CARTPOLE", "TRAPEZOIDAL"), ("BEARPOPULATIONS", "HERMITE_SIMPSON")])
def test_schedule_matrix_returns_the_bits_of_whole_solves_and_counts_every_trajectory(monkeypatch, tmp_path, system, rule):
  """slots x batch x k1, fill on and off, clean and under poison: z, lam, cost, status, iters and kkt are those of whole solves, bit for bit (and so
  the fill's are those of the launch without it); `reached` ends at B; every record was parked at k1 or later, without the fill at k1."""
  for slots in (1, 4):
    for B in (slots, slots + 1, 3 * slots + 1):
      ref = _whole_solves(monkeypatch, system, rule, B)
      for k1 in (1, 3):
        for fill in (True, False):
          for poison in (None, "nan"):
            tag = (system, rule, "slots", slots, "B", B, "k1", k1, "fill", fill, "poison", poison)
            r, it, parked, reached = _two_phase(monkeypatch, tmp_path, system, rule, slots, B, k1, fill, poison)
            _same(r, ref, tag)
            assert reached == B, (tag, reached)
            assert parked == (it >= 0).sum(), (tag, parked, it)
            assert ((it == -1) | (it >= k1)).all(), (tag, it)
            if not fill:
              assert ((it == -1) | (it == k1)).all() and ((it == -1) == (ref["iters"] < k1)).all(), (tag, it, ref["iters"])


def test_the_fill_runs_and_the_knob_switches_it_off(monkeypatch, tmp_path):
  """Four slots, five trajectories, k1 = 3: the slot that parks first takes the fifth trajectory; the other three find no ticket, and the fifth is
  three iterations from k1: they iterate on and park above k1.  With MYRIAD_PARK_FILL=0 every record is parked at k1."""
  ref = _whole_solves(monkeypatch, "CARTPOLE", "HERMITE_SIMPSON", 5)
  assert (ref["iters"] > 8).all(), ref["iters"]          # (nothing ends inside the window this test looks at)
  r, it, parked, reached = _two_phase(monkeypatch, tmp_path, "CARTPOLE", "HERMITE_SIMPSON", 4, 5, 3, True)
  _same(r, ref, "fill on")
  assert parked == 5 and reached == 5 and (it >= 3).all() and (it > 3).any(), (it, parked, reached)
  r, it, parked, reached = _two_phase(monkeypatch, tmp_path, "CARTPOLE", "HERMITE_SIMPSON", 4, 5, 3, False)
  _same(r, ref, "fill off")
  assert parked == 5 and reached == 5 and (it == 3).all(), (it, parked, reached)


def test_max_iter_one_past_k1_ends_the_fill(monkeypatch, tmp_path):
  """max_iter = k1 + 1: a filling slot runs into the iteration limit like any solve; the call returns, with the bits of whole solves."""
  k1 = 3
  ref = _whole_solves(monkeypatch, "CARTPOLE", "HERMITE_SIMPSON", 5, max_iter=k1 + 1)
  assert (ref["status"] == 1).all() and (ref["iters"] == k1 + 1).all(), (ref["status"], ref["iters"])
  for slots in (1, 4):
    r, it, parked, reached = _two_phase(monkeypatch, tmp_path, "CARTPOLE", "HERMITE_SIMPSON", slots, 5, k1, True, max_iter=k1 + 1)
    _same(r, ref, ("max_iter", slots))
    assert reached == 5 and ((it == -1) | ((it >= k1) & (it <= k1 + 1))).all(), (slots, it, reached)


def test_a_batch_that_converges_before_k1_parks_nothing(monkeypatch, tmp_path):
  """Every trajectory starts at a solved point and converges before k1: each counts itself when it leaves its solve, nothing is parked, launch 2 is empty."""
  B = 5
  cold = _whole_solves(monkeypatch, "CARTPOLE", "HERMITE_SIMPSON", B, same_x0=True)
  assert (cold["status"] == 0).all()
  guess = cold["xs_and_us"][0]
  ref = _whole_solves(monkeypatch, "CARTPOLE", "HERMITE_SIMPSON", B, same_x0=True, guess=guess)
  assert (ref["status"] == 0).all() and ref["iters"].max() < cold["iters"].min(), (ref["status"], ref["iters"], cold["iters"])
  k1 = int(ref["iters"].max()) + 2
  for slots in (1, 4):
    r, it, parked, reached = _two_phase(monkeypatch, tmp_path, "CARTPOLE", "HERMITE_SIMPSON", slots, B, k1, True, same_x0=True, guess=guess)
    _same(r, ref, ("solved start", slots))
    assert parked == 0 and reached == B and (it == -1).all(), (slots, it, parked, reached)


def test_a_batch_of_one(monkeypatch, tmp_path):
  """B = 1: the only trajectory is the last to arrive at k1, finds `reached` at B and parks there; launch 2 resumes it."""
  ref = _whole_solves(monkeypatch, "CARTPOLE", "HERMITE_SIMPSON", 1)
  for k1 in (1, 3):
    for poison in (None, "nan"):
      r, it, parked, reached = _two_phase(monkeypatch, tmp_path, "CARTPOLE", "HERMITE_SIMPSON", 4, 1, k1, True, poison)
      _same(r, ref, ("B = 1", k1, poison))
      assert reached == 1 and parked == 1 and it[0] >= k1, (k1, it, parked, reached)
