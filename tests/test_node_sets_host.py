"""The host side of the weight-set calls of the network system (myr_exgd_grad_node_sets, myr_hvp_node_sets, experiments/node_e2e_sysid.
run_node_endtoend_sets) that needs no device: the exports and their null-handle refusals, run_node_endtoend_sets = E separate run_node_endtoend
runs on a stub optimizer and engine -- records, weights and saved epochs, to the bit, a learning rate per set included --, and the host twins of the
two kernel families handed a different weight vector for every instance, against the oracle under those weights at the twins' own tolerances."""
import numpy as np
import pytest

import node_exgd_grad_cases as X
import node_hvp_cases as H
import node_sets_cases as NS_
from myriad_amd import _lib
from myriad_amd.config import Config, HParams, OptimizerType, QuadratureRule
from myriad_amd.experiments import node_e2e_sysid as D
from myriad_amd.systems import SystemType
from myriad_amd.systems.neural_ode import flat_from_mapping

EXGD_TWIN_TOL = 100.0 * 5.0e-15      # test_node_exgd_grad_host_twin.TWIN_TOL
HVP_TWIN_TOL = 100.0 * 3.1e-15       # test_node_hvp_host_twin.ORACLE_TOL


def test_exports_and_null_handles():
  lib = _lib.load()
  for name in ("myr_exgd_grad_node_sets", "myr_hvp_node_sets"):
    assert name in _lib.EXPORTS and hasattr(lib, name)
  a = np.zeros(8)
  p = a.ctypes.data
  rc = lib.myr_exgd_grad_node_sets(None, 1, 1, p, p, p, p, p, 0.1, 0.1, 1, p, None, p, 0, None, None, _lib.MEM_HOST)
  assert rc == -1 and b"myr_exgd_grad_node_sets" in lib.myr_last_error()
  rc = lib.myr_hvp_node_sets(None, 1, 1, p, None, p, p, 1, p, None, 0, _lib.MEM_HOST)
  assert rc == -1 and b"myr_hvp_node_sets" in lib.myr_last_error()
  assert lib.myr_version().decode() == "myriad_hip 0.10 (gfx950)"      # the capability is detected by the export, not by the version


# ---- the driver over a stub ------------------------------------------------------------------------------------------------------------------
ROWS, NS, NU, M = 3, 4, 1, 8
N = ROWS * (NS + NU)


class StubEngine:
  """The engine calls the drivers make, without a device: an instance's result is a fixed function of its own inputs and its own weight row,
  evaluated one instance at a time, so that a batch, a set and a call on one instance give the same bits."""
  m = M

  def __init__(self):
    self.calls = []

  @staticmethod
  def _centre(p):
    return np.tanh(p[:N]) + 0.1 * p[N:2 * N]

  def _step(self, z, lam, lb, ub, eta_x, eta_v, nsteps, p):
    for _ in range(nsteps):
      z = np.clip(z - eta_x * (z - self._centre(p)) + 1e-3 * lam.sum(), lb, ub)
      lam = lam + eta_v * (z[:M] - p[100:100 + M])
    return z, lam

  def _row(self, z, lam, nsteps, seed, p):
    g = np.zeros(p.size)
    g[:N] = nsteps * seed * (1.0 - np.tanh(p[:N]) ** 2) + 1e-3 * z
    g[N:2 * N] = 0.1 * seed * lam.sum()
    g[100:100 + M] = lam * p[100:100 + M]
    return g

  @staticmethod
  def _sum(rows):
    s = rows[0].copy()
    for r in rows[1:]:
      s = s + r
    return s

  def exgd(self, z, lam, lb, ub, eta_x, eta_v, nsteps, params=None):
    z, lam = np.atleast_2d(np.asarray(z, dtype=np.float64)), np.atleast_2d(np.asarray(lam, dtype=np.float64))
    B = z.shape[0]
    lb, ub, p = np.broadcast_to(lb, z.shape), np.broadcast_to(ub, z.shape), np.asarray(params)
    self.calls.append(("exgd", B, p.ndim))
    out = [self._step(z[b], lam[b], lb[b], ub[b], eta_x, eta_v, nsteps, p if p.ndim == 1 else p[b]) for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

  def exgd_grad_node(self, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, params, seed_lam=None, reduce=False, want_start=True):
    z, lam = np.atleast_2d(np.asarray(z, dtype=np.float64)), np.atleast_2d(np.asarray(lam, dtype=np.float64))
    seed = np.broadcast_to(seed_z, z.shape)
    self.calls.append(("grad", z.shape[0]))
    rows = [self._row(z[b], lam[b], nsteps, seed[b], np.asarray(params)) for b in range(z.shape[0])]
    return {"grad": self._sum(rows) if reduce else np.stack(rows)}

  exgd_grad_node_shoot = exgd_grad_node

  def exgd_grad_node_sets(self, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, params, seed_lam=None, reduce=False, want_start=True):
    E, R = z.shape[:2]
    seed = np.broadcast_to(seed_z, z.shape)
    self.calls.append(("grad_sets", E, R))
    rows = [[self._row(z[e, r], lam[e, r], nsteps, seed[e, r], params[e]) for r in range(R)] for e in range(E)]
    return {"grad": np.stack([self._sum(rs) for rs in rows]) if reduce else np.array(rows)}

  def exgd_grad_node_probe(self): pass
  def exgd_grad_node_shoot_probe(self): pass
  def exgd_grad_node_sets_probe(self): pass


class StubOptimizer:
  def __init__(self, transcription, engine):
    self.transcription, self.engine = transcription, engine
    rng = np.random.default_rng(1)
    self.guess = rng.standard_normal(N)
    self.bounds = np.stack([np.full(N, -0.9), np.full(N, 1.1)], axis=1)
    self._true_u = rng.standard_normal((ROWS, NU))

  def unravel(self, z):
    z = np.asarray(z)
    return z[..., :ROWS * NS].reshape(z.shape[:-1] + (ROWS, NS)), z[..., ROWS * NS:].reshape(z.shape[:-1] + (ROWS, NU))

  def step_sizes(self):
    return 0.3, 0.2

  def solve(self):
    return {"u": self._true_u}

  def solve_batch(self, x0s=None):
    return {"u": np.stack([self._true_u + 0.1 * x[0] for x in x0s])}

  def batch_inputs(self, x0s, params=None):
    B = x0s.shape[0]
    z0 = np.tile(self.guess, (B, 1)); z0[:, :NS] = x0s
    lb, ub = np.tile(self.bounds[:, 0], (B, 1)), np.tile(self.bounds[:, 1], (B, 1))
    lb[:, :NS] = x0s; ub[:, :NS] = x0s
    return z0, lb, ub


def _hp():
  return HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.COLLOCATION, quadrature_rule=QuadratureRule.HERMITE_SIMPSON, intervals=1,
                 num_unrolled=2)


@pytest.mark.parametrize("batched", [False, True], ids=["single", "start_states"])
@pytest.mark.parametrize("transcription", ["HERMITE_SIMPSON", "SHOOTING"])
def test_driver_equals_a_run_per_network_on_a_stub(monkeypatch, transcription, batched):
  engines = []

  def stub_optimizer(hp, cfg, system):
    if system.name == "NODE_CARTPOLE":
      engines.append(StubEngine())
      return StubOptimizer(transcription, engines[-1])
    return StubOptimizer(transcription, None)

  monkeypatch.setattr(D, "get_optimizer", stub_optimizer)
  hp, cfg = _hp(), Config(verbose=False, plot=False)
  shooting = transcription == "SHOOTING"
  x0s = np.array([[0.1, 0.0, -0.2, 0.3], [0.0, 0.2, 0.1, -0.1], [0.3, 0.3, 0.0, 0.0]]) if batched else None
  seeds, lrs = (3, 4, 5), (1e-4, 3e-3, 2e-2)
  kw = dict(num_epochs=25, start_states=x0s, save_and_reset_time=11, shooting=shooting)
  for rates in (None, lrs):
    runs = D.run_node_endtoend_sets(hp, cfg, [D.initial_node(s) for s in seeds], lrs=rates, **kw)
    sets_engine = engines[-1]
    assert len(runs) == 3
    for e, s in enumerate(seeds):
      monkeypatch.setattr(D, "ADAM_LR", 1e-4 if rates is None else rates[e])
      one = D.run_node_endtoend(hp, cfg, node=D.initial_node(s), **kw)
      monkeypatch.undo(); monkeypatch.setattr(D, "get_optimizer", stub_optimizer)
      got = runs[e]
      assert set(got) == set(one)
      assert got["ts"] == one["ts"] == list(range(11)) + [11, 20, 22]      # every epoch up to 10, then the resets and every tenth
      assert got["imitation_losses"] == one["imitation_losses"]      # equal floats, not close ones
      for k in ("primal_guesses", "dual_guesses"):
        assert len(got[k]) == len(one[k]) and all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got[k], one[k])), (e, k)
      assert sorted(got["saved_params"]) == sorted(one["saved_params"]) == [0, 11, 22, 25]
      for ep in one["saved_params"]:
        assert flat_from_mapping(got["saved_params"][ep]).tobytes() == flat_from_mapping(one["saved_params"][ep]).tobytes(), (e, ep)
      assert flat_from_mapping(got["params"]).tobytes() == flat_from_mapping(one["params"]).tobytes()
      assert np.asarray(got["true_opt_us"]).tobytes() == np.asarray(one["true_opt_us"]).tobytes()
    # every epoch of the sets run: one advance of all iterates with a weight row per instance, one gradient call with all sets
    R = 3 if batched else 1
    assert sets_engine.calls == [("exgd", 3 * R, 2), ("grad_sets", 3, R)] * 25
    if rates is None:
      default_run = runs
    else:      # the rates took part: set 0 keeps the default rate and its weights, the others moved further
      assert flat_from_mapping(runs[0]["params"]).tobytes() == flat_from_mapping(default_run[0]["params"]).tobytes()
      assert flat_from_mapping(runs[2]["params"]).tobytes() != flat_from_mapping(default_run[2]["params"]).tobytes()
  assert D.run_node_endtoend_sets(hp, cfg, [], **kw) == []


def test_adam_sets_takes_a_rate_per_row():
  from myriad_amd.experiments.mle_sysid import Adam
  from myriad_amd.neural_ode.node_training import AdamSets
  rng = np.random.default_rng(2)
  P, lrs = rng.standard_normal((3, 9)), (1e-4, 3e-3, 2e-2)
  opt, singles, ref = AdamSets(P.shape, np.array(lrs)), [Adam(lr) for lr in lrs], P.copy()
  for rows in ([0, 1, 2], [2, 0], [0, 1, 2]):
    g = rng.standard_normal((len(rows), 9))
    P[rows] = opt.update(rows, P[rows], g)
    for i, r in enumerate(rows):
      ref[r] = singles[r].update({"p": ref[r]}, {"p": g[i]})["p"]
  assert P.tobytes() == ref.tobytes()


# ---- the host twins under a weight vector per instance ---------------------------------------------------------------------------------------
def test_exgd_grad_twin_with_a_weight_vector_per_instance(tmp_path):
  """node_exgd_grad_host one instance at a time, instance b under the weights of set b + 1: the host sequence takes whatever set it is handed"""
  lib = X.build_twin(tmp_path)
  P = NS_.weight_sets(3)
  for b, e in ((0, 1), (1, 2)):
    case, *ref = NS_.hs_reference(P[e], 3, 3, 2)
    s = slice(b, b + 1)
    out = X.twin_grad(lib, case["N"], case["T"], case["z"][s], case["lam"][s], case["lb"][s], case["ub"][s], P[e], case["eta_x"], case["eta_v"],
                      case["nsteps"], case["seed_z"][s], case["seed_lam"][s])
    errs = tuple(X.rel_error(o[0], r[b]) for o, r in zip(out, ref))
    print("instance", b, "set", e, errs)
    assert max(errs) <= EXGD_TWIN_TOL, errs
    other = X.twin_grad(lib, case["N"], case["T"], case["z"][s], case["lam"][s], case["lb"][s], case["ub"][s], P[0], case["eta_x"], case["eta_v"],
                        case["nsteps"], case["seed_z"][s], case["seed_lam"][s])
    assert X.rel_error(other[0][0], ref[0][b]) > 1e-6             # under the weights of set 0 the reference is not met


@pytest.mark.parametrize("cs", [("HERMITE_SIMPSON", 3, 1, "HEUN", 2), ("SHOOTING", 3, 2, "HEUN", 2)], ids=["HS", "SHOOTING"])
def test_hvp_twin_with_a_weight_vector_per_instance(tmp_path, cs):
  lib = H.build_twin(tmp_path)
  tr, I, cpi, method, batch = cs
  P = NS_.weight_sets(3)
  for b, e in ((0, 1), (1, 2)):
    case, ref = NS_.hvp_reference(P[e], *cs)
    s = slice(b, b + 1)
    for wc in (1, 0):
      oz, op = H.twin_hvp(lib, tr, I, cpi, method, case["T"], case["z"][s], case["lam"][s], case["v"][s], P[e], wc)
      errs = (H.rel_error(oz[0], ref[wc][0][b]), H.rel_error(op[0], ref[wc][1][b]))
      print(tr, "instance", b, "set", e, "with_cost", wc, errs)
      assert max(errs) <= HVP_TWIN_TOL, errs
    _, other = H.twin_hvp(lib, tr, I, cpi, method, case["T"], case["z"][s], case["lam"][s], case["v"][s], P[0], 1)
    assert H.rel_error(other[0], ref[1][1][b]) > 1e-6
