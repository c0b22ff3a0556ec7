"""myr_fit_grad_sets on the device: E parameter sets of R trajectories each in one call (csrc/fit.h, csrc/myriad_hip.hip: dispatch_fit).

The contract is bit equality: set e of a sets call = myr_fit_grad on that set alone (B = R, the set's data, its parameters shared).  So every
comparison here is `tobytes()` against single calls; the one comparison with the oracle uses test_gpu_fit.py's bounds for the network kernel
(measured x 100: |dloss| / loss 3.0e-12, |dgrad| / max|grad| 8.3e-12), which apply because the bits are myr_fit_grad's.

Shapes: the smallest at which the mapping of sets to workgroups (network system: 4 wavefronts = trajectories per workgroup, a workgroup never
straddles two sets) and to lanes (closed-form systems: set boundaries inside and across 64-lane wavefronts) can go wrong."""
import functools

import numpy as np
import pytest
import torch

import fit_cases as F
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

NODE_LOSS_TOL, NODE_GRAD_TOL = 3.0e-12, 8.3e-12      # tests/test_gpu_fit.py: 100 x measured
NP_NODE = 4804


def _engine(name, method, S, T=None):
  return _lib.Engine(name, "SHOOTING", 1, F.horizon(name, S) if T is None else T, controls_per_interval=S, integration_method=method)


@functools.lru_cache(maxsize=None)
def _node_case(E, R, S, method):
  """E disturbed weight sets [E][4804] and E R trajectories of the true CARTPOLE field plus 1 % noise (as test_gpu_fit.py builds its network cases)"""
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping
  flat = flat_from_mapping(NeuralODE.load_fitted_cartpole().params)
  sysm = F.O.CartPole()
  rng = np.random.default_rng(1000 * E + 100 * R + 10 * S + F.METHODS.index(method))
  batch = E * R
  rows = 2 * S + 1 if method == "RK4" and R == 5 else S + 1       # RK4: its own control rows at R = 5, clamped rows otherwise
  us = F._controls(sysm, rng, batch, rows)
  x0 = 0.3 * rng.standard_normal((batch, 4))
  h = 0.1
  xs = np.stack([F.O.integrate_time_independent(sysm.dynamics, torch.tensor(x0[b]), torch.tensor(us[b]), h, S, method)[1].numpy() for b in range(batch)])
  xs_obs = xs + 0.01 * rng.standard_normal(xs.shape)
  xs_obs[:, 0] = x0
  P = flat[None] + 0.05 * rng.standard_normal((E, NP_NODE))
  out = (P, xs_obs.reshape(E, R, S + 1, 4), us.reshape(E, R, rows, 1), h * S)
  for a in out[:3]:
    a.setflags(write=False)
  return out


@functools.lru_cache(maxsize=None)
def _cartpole_case(E, R, S):
  xs_obs, us, params = F.inputs("CARTPOLE", "RK4", False, E * R, S, True)
  out = (np.ascontiguousarray(params[::R][:E]), xs_obs.reshape(E, R, S + 1, 4), us.reshape(E, R, S + 1, 1))
  for a in out:
    a.setflags(write=False)
  return out


def _bits(out):
  return out["loss"].tobytes() + (out["grad"].tobytes() if "grad" in out else b"")


def _assert_sets_equal_single_calls(eng, P, xs_obs, us, wt):
  rows = eng.fit_grad_sets(xs_obs, us, P, wt=wt)
  sums = eng.fit_grad_sets(xs_obs, us, P, wt=wt, reduce=True)
  E, R = xs_obs.shape[:2]
  assert rows["loss"].shape == (E, R) and rows["grad"].shape == (E, R, eng.np) and sums["grad"].shape == (E, eng.np)
  assert np.isfinite(rows["grad"]).all() and np.abs(rows["grad"]).max() > 0.0
  for e in range(E):
    one = eng.fit_grad(xs_obs[e], us[e], params=P[e], wt=wt)
    red = eng.fit_grad(xs_obs[e], us[e], params=P[e], wt=wt, reduce=True)
    assert rows["loss"][e].tobytes() == one["loss"].tobytes(), e
    assert rows["grad"][e].tobytes() == one["grad"].tobytes(), (e, np.argwhere(rows["grad"][e] != one["grad"])[:1])
    assert sums["loss"][e].tobytes() == red["loss"].tobytes(), e
    assert sums["grad"][e].tobytes() == red["grad"].tobytes(), (e, np.argwhere(sums["grad"][e] != red["grad"])[:1])
  return rows, sums


# ---- sets = single calls, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["HEUN", "RK4"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("R", [1, 4, 5])
def test_node_sets_equal_single_calls(R, S, method):
  """a lone wavefront, exactly one workgroup, a partial second workgroup per set; E = 3 and E = 1"""
  P, xs_obs, us, T = _node_case(3, R, S, method)
  eng = _engine("NODE_CARTPOLE", method, S, T)
  for wt in (None, F.decaying_wt(S)):
    _assert_sets_equal_single_calls(eng, P, xs_obs, us, wt)
  _assert_sets_equal_single_calls(eng, P[1:2], xs_obs[1:2], us[1:2], None)
  eng.close()


@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("E,R", [(3, 1), (3, 21), (5, 13), (2, 65)])
def test_closed_form_sets_equal_single_calls(E, R, S):
  """63, 65 and 130 lanes: set boundaries inside a wavefront, across wavefronts, padded lanes behind the last set"""
  P, xs_obs, us = _cartpole_case(E, R, S)
  eng = _engine("CARTPOLE", "RK4", S)
  _assert_sets_equal_single_calls(eng, P, xs_obs, us, F.decaying_wt(S))
  _assert_sets_equal_single_calls(eng, P[:1], xs_obs[:1], us[:1], None)
  eng.close()


@pytest.mark.parametrize("name", ["NODE_CARTPOLE", "CARTPOLE"])
def test_shared_data_equals_replicated_data(name):
  if name == "NODE_CARTPOLE":
    P, xs_obs, us, T = _node_case(3, 5, 3, "RK4")
    eng = _engine(name, "RK4", 3, T)
  else:
    P, xs_obs, us = _cartpole_case(5, 13, 7)
    eng = _engine(name, "RK4", 7)
  E = P.shape[0]
  x1, u1 = xs_obs[1], us[1]
  rep_x, rep_u = np.ascontiguousarray(np.broadcast_to(x1, (E,) + x1.shape)), np.ascontiguousarray(np.broadcast_to(u1, (E,) + u1.shape))
  for reduce in (False, True):
    shared = eng.fit_grad_sets(x1, u1, P, reduce=reduce)
    assert shared["loss"].shape == (E, x1.shape[0])
    assert _bits(shared) == _bits(eng.fit_grad_sets(rep_x, rep_u, P, reduce=reduce))
  assert _bits(eng.fit_grad_sets(x1, u1, P, want_grad=False)) == eng.fit_grad_sets(rep_x, rep_u, P)["loss"].tobytes()
  eng.close()


# ---- loss only ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["NODE_CARTPOLE", "CARTPOLE"])
def test_loss_only(name):
  if name == "NODE_CARTPOLE":
    P, xs_obs, us, T = _node_case(3, 5, 3, "HEUN")
    eng = _engine(name, "HEUN", 3, T)
  else:
    P, xs_obs, us = _cartpole_case(5, 13, 7)
    eng = _engine(name, "RK4", 7)
  E, R, S1 = xs_obs.shape[:3]
  full = eng.fit_grad_sets(xs_obs, us, P)
  only = eng.fit_grad_sets(xs_obs, us, P, want_grad=False)
  assert "grad" not in only and only["loss"].tobytes() == full["loss"].tobytes()
  # the raw entry point: no grad buffer at all
  loss = np.full((E, R), np.nan)
  args = (eng._h, E, R, S1 - 1, us.shape[2], xs_obs.ctypes.data, us.ctypes.data, 0, None, P.ctypes.data)
  assert eng.lib.myr_fit_grad_sets(*args, loss.ctypes.data, None, 0, _lib.MEM_HOST) == 0
  assert loss.tobytes() == full["loss"].tobytes()
  assert eng.lib.myr_fit_grad_sets(*args, loss.ctypes.data, None, eng.np, _lib.MEM_HOST) == 0
  assert loss.tobytes() == full["loss"].tobytes()
  rc = eng.lib.myr_fit_grad_sets(*args, None, None, 0, _lib.MEM_HOST)
  assert rc == -1 and b"both null" in eng.lib.myr_last_error()
  eng.close()


# ---- device memory ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["NODE_CARTPOLE", "CARTPOLE"])
def test_device_memory_gives_the_same_bits(name):
  if name == "NODE_CARTPOLE":
    P, xs_obs, us, T = _node_case(3, 5, 3, "HEUN")
    eng = _engine(name, "HEUN", 3, T)
  else:
    P, xs_obs, us = _cartpole_case(5, 13, 7)
    eng = _engine(name, "RK4", 7)
  E, R, S1 = xs_obs.shape[:3]
  npar, u_rows = eng.np, us.shape[2]
  wt = F.decaying_wt(S1 - 1)
  rows = eng.fit_grad_sets(xs_obs, us, P, wt=wt)
  sums = eng.fit_grad_sets(xs_obs, us, P, wt=wt, reduce=True)
  dev = torch.device("cuda:0")
  dx, du, dp, dw = (torch.tensor(np.array(a), device=dev) for a in (xs_obs, us, P, wt))      # (copies: the cached inputs are read-only)
  for rep in range(2):                                            # a second call: the same bits again
    dl = torch.full((E, R), float("nan"), dtype=torch.float64, device=dev)
    dg = torch.full((E, npar), float("nan"), dtype=torch.float64, device=dev)
    dgr = torch.full((E, R, npar), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.fit_grad_sets_device(E, R, S1 - 1, u_rows, dx, du, dp, grad=dg, grad_stride=0, wt=dw, loss=dl)
    eng.fit_grad_sets_device(E, R, S1 - 1, u_rows, dx, du, dp, grad=dgr, grad_stride=npar, wt=dw, loss=None)
    torch.cuda.synchronize()
    assert dl.cpu().numpy().tobytes() == sums["loss"].tobytes(), rep
    assert dg.cpu().numpy().tobytes() == sums["grad"].tobytes(), rep
    assert dgr.cpu().numpy().tobytes() == rows["grad"].tobytes(), rep
    dl2 = torch.full((E, R), float("nan"), dtype=torch.float64, device=dev)
    eng.fit_grad_sets_device(E, R, S1 - 1, u_rows, dx, du, dp, grad=None, wt=dw, loss=dl2)
    torch.cuda.synchronize()
    assert dl2.cpu().numpy().tobytes() == rows["loss"].tobytes(), rep
  eng.close()


# ---- chunks of whole sets -----------------------------------------------------------------------------------------------------------------
def test_chunked_equals_unchunked(monkeypatch):
  P, xs_obs, us, T = _node_case(3, 5, 3, "HEUN")
  eng = _engine("NODE_CARTPOLE", "HEUN", 3, T)
  monkeypatch.delenv("MYRIAD_FIT_ROWS_BYTES", raising=False)
  whole = eng.fit_grad_sets(xs_obs, us, P, reduce=True)
  rows_whole = eng.fit_grad_sets(xs_obs, us, P)
  one_set = 5 * NP_NODE * 8                                       # bytes of one set's rows
  for bound in (one_set, 2 * one_set + 8, 1000):                  # three chunks; two sets and one; below one set: still a set per chunk
    monkeypatch.setenv("MYRIAD_FIT_ROWS_BYTES", str(bound))
    assert _bits(eng.fit_grad_sets(xs_obs, us, P, reduce=True)) == _bits(whole), bound
    assert _bits(eng.fit_grad_sets(xs_obs[0], us[0], P, reduce=True)) == _bits(eng.fit_grad_sets(
        np.ascontiguousarray(np.broadcast_to(xs_obs[0], xs_obs.shape)), np.ascontiguousarray(np.broadcast_to(us[0], us.shape)), P, reduce=True)), bound
    assert _bits(eng.fit_grad_sets(xs_obs, us, P)) == _bits(rows_whole), bound      # (rows need no scratch: not chunked)
  eng.close()


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------
def test_node_sets_against_the_oracle():
  from myriad_amd.systems.neural_ode import mapping_from_flat
  E, R, S, method = 2, 2, 3, "HEUN"
  P, xs_obs, us, T = _node_case(E, R, S, method)
  eng = _engine("NODE_CARTPOLE", method, S, T)
  out = eng.fit_grad_sets(xs_obs, us, P)
  eng.close()
  keys = ("linear", "linear_1", "linear_2")
  for e in range(E):
    ref_loss, ref_grad = [], []
    for r in range(R):
      tp = {k: {f: torch.tensor(v, requires_grad=True) for f, v in d.items()} for k, d in mapping_from_flat(P[e]).items()}
      _, xh = F.O.integrate_time_independent(F.O.NodeCartPole(tp).dynamics, torch.tensor(xs_obs[e, r, 0]), torch.tensor(us[e, r]), T / S, S, method)
      l = ((xh - torch.tensor(xs_obs[e, r])) ** 2).sum()
      g = torch.autograd.grad(l, [tp[k][f] for k in keys for f in ("w", "b")])
      ref_loss.append(float(l.detach()))
      ref_grad.append(np.concatenate([gi.numpy().ravel() for gi in g]))
    el, eg = F.rel_errors(out["loss"][e], out["grad"][e], np.array(ref_loss), np.stack(ref_grad))
    print(f"set {e}: dloss {el:.2e} dgrad {eg:.2e}")
    assert el <= NODE_LOSS_TOL and eg <= NODE_GRAD_TOL, (e, el, eg)


# ---- what the registers held before the launch does not reach the result ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["CARTPOLE", "NODE_CARTPOLE"])
def test_inherited_state_does_not_reach_the_result(monkeypatch, name):
  if name == "CARTPOLE":
    P, xs_obs, us = _cartpole_case(5, 13, 7)
    T = F.horizon("CARTPOLE", 7)
  else:
    P, xs_obs, us, T = _node_case(3, 5, 3, "RK4")
  bits = {}
  for pat in ("zero", "nan", "random"):
    monkeypatch.setenv("MYRIAD_REG_FILL", pat)
    monkeypatch.setenv("MYRIAD_STACK_FILL", pat)
    eng = _engine(name, "RK4", xs_obs.shape[2] - 1, T)             # (the handle reads the fill at creation)
    out = eng.fit_grad_sets(xs_obs, us, P)
    red = eng.fit_grad_sets(xs_obs, us, P, reduce=True)
    only = eng.fit_grad_sets(xs_obs, us, P, want_grad=False)
    eng.close()
    assert np.isfinite(out["grad"]).all()
    bits[pat] = _bits(out) + _bits(red) + _bits(only)
  assert bits["nan"] == bits["zero"] and bits["random"] == bits["zero"]


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def test_errors():
  P, xs_obs, us = _cartpole_case(3, 1, 7)
  eng = _lib.Engine("CARTPOLE_ELASTIC", "HERMITE_SIMPSON", 7, 1.0)
  with pytest.raises(NotImplementedError, match="elastic"):
    eng.fit_grad_sets(xs_obs, np.zeros((3, 1, 8, eng.nu)), np.zeros((3, eng.np)))
  eng.close()
  eng = _lib.Engine("INVASIVEPLANT", "SHOOTING", 1, 10.0, controls_per_interval=7)
  with pytest.raises(NotImplementedError, match="INVASIVEPLANT"):
    eng.fit_grad_sets(np.zeros((3, 1, 8, eng.ns)), np.zeros((3, 1, 8, eng.nu)), np.zeros((3, eng.np)))
  eng.close()
  eng = _engine("CARTPOLE", "RK4", 7)
  with pytest.raises(ValueError):
    eng.fit_grad_sets(xs_obs, us, P[:2])                          # E of params and of the data differ
  with pytest.raises(ValueError):
    eng.fit_grad_sets(xs_obs, us[0], P)                           # one shared, one per set
  loss, grad = np.full((3, 1), 7.0), np.full((3, 1, 4), 7.0)
  call = lambda E, R, params, gs, shared: eng.lib.myr_fit_grad_sets(eng._h, E, R, 7, 8, xs_obs.ctypes.data, us.ctypes.data, shared, None, params,
                                                                   loss.ctypes.data, grad.ctypes.data, gs, _lib.MEM_HOST)
  # (the argument checks of the C call, with their full texts and their order: tests/test_gpu_api.py)
  assert call(0, 1, P.ctypes.data, 4, 0) == 0                    # E = 0: nothing is written
  assert (loss == 7.0).all() and (grad == 7.0).all()
  assert call(3, 1, P.ctypes.data, 4, 0) == 0 and (loss != 7.0).all() and np.isfinite(grad).all()
  eng.close()
  eng = _engine("NODE_CARTPOLE", "HEUN", 7, 0.7)                  # myr_fit_grad keeps its refusal of per-instance weights
  with pytest.raises(NotImplementedError, match="shared"):
    eng.fit_grad(xs_obs[:, 0], us[:, 0], params=np.zeros((3, NP_NODE)))
  eng.close()


# ---- ensemble training, end to end --------------------------------------------------------------------------------------------------------
def _training_hp(**kw):
  from myriad_amd.config import HParams, OptimizerType
  from myriad_amd.systems import SystemType
  base = dict(system=SystemType.CARTPOLE, optimizer=OptimizerType.SHOOTING, intervals=1, controls_per_interval=5, train_size=6, val_size=2,
              test_size=2, minibatch_size=3, num_epochs=6, loss_recording_frequency=1, early_stop_check_frequency=2, learning_rate=1e-3)
  base.update(kw)
  return HParams(**base)


def test_train_ensemble_equals_separate_trainings():
  import copy
  from myriad_amd.config import Config
  from myriad_amd.neural_ode import node_training
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping, mapping_from_flat
  from myriad_amd.utils import generate_dataset
  hp = _training_hp()
  assert hp.minibatch_size == 2
  datasets = []
  for e in range(3):
    hp_e = copy.copy(hp)
    hp_e.seed = hp.seed + 10 * e
    datasets.append(generate_dataset(hp_e, Config(verbose=False, plot=False)))
  data = np.stack(datasets)
  assert data.shape == (3, 10, 6, 5)
  T = hp.system().T
  rng = np.random.default_rng(11)
  P = flat_from_mapping(NeuralODE.load_fitted_cartpole().params)[None] + 0.05 * rng.standard_normal((3, NP_NODE))
  runs = node_training.train_ensemble(hp, T, P.copy(), data[:, :6], data[:, 6:8])
  for e in range(3):
    best, epoch, record = node_training.train(hp, T, mapping_from_flat(P[e]), data[e, :6], data[e, 6:8], rng=np.random.default_rng(hp.seed + e))
    assert runs[e][1] == epoch == 5 and runs[e][2] == record, (e, runs[e][2], record)
    assert flat_from_mapping(runs[e][0]).tobytes() == flat_from_mapping(best).tobytes(), e
    assert record[-1][1] < record[0][1], record


def test_node_noise_study():
  from myriad_amd.config import Config
  from myriad_amd.experiments import node_mle_sysid
  from myriad_amd.systems.neural_ode import NeuralODE, NodeSystem, flat_from_mapping
  from myriad_amd.trajectory_optimizers import get_optimizer
  from myriad_amd.utils import get_state_trajectory_and_cost
  cfg = Config(verbose=False, plot=False)
  hp = _training_hp(num_epochs=4, hidden_layers=(64, 64))
  fitted = NeuralODE.load_fitted_cartpole().params
  res = node_mle_sysid.run_node_noise_study(hp, cfg, noise_levels=(0.0, 0.01), params=fitted)
  assert res["noise_levels"] == [0.0, 0.01] and res["costs"].shape == (2,) and np.isfinite(res["costs"]).all()
  assert len(res["records"]) == 2 and [r[0] for r in res["records"][0]] == [0, 1, 2, 3]
  assert res["records"][0] != res["records"][1]                   # two datasets: two trainings
  true_system = hp.system()
  u = get_optimizer(hp, cfg, true_system).solve()['u']
  assert res["optimal_cost"] == get_state_trajectory_and_cost(hp, true_system, true_system.x_0, u)[1]
  assert res["costs"][0] != res["costs"][1]                        # two networks: two plans
  # costs[e] IS the cost of set e's own plan.  The batched plan goes through the start-state form of the solve (myr_solve_x0), the single plan
  # through myr_solve on the expanded arrays; tests/test_gpu_solve.py pins the two forms to each other bit for bit, and an instance's solve does
  # not depend on the batch it runs in -- so the comparison is equality, with solve_with_params and with a batch of that one set alone.
  opt = get_optimizer(hp, cfg, NodeSystem(NeuralODE(fitted, (64, 64)), true_system))
  for e in range(2):
    ue = opt.solve_with_params(res["params"][e])['u']
    ce = get_state_trajectory_and_cost(hp, true_system, true_system.x_0, ue)[1]
    ub = opt.solve_batch(params=flat_from_mapping(res["params"][e])[None])['u']
    print(f"level {res['noise_levels'][e]}: study cost {float(res['costs'][e])!r}, single plan {ce!r}, optimal {res['optimal_cost']!r}; "
          f"max |u - u_single| {np.abs(res['us'][e] - ue).max():.3e}, max |u - u_batch_of_one| {np.abs(res['us'][e] - ub[0]).max():.3e}")
    assert ub[0].tobytes() == res["us"][e].tobytes(), e
    assert np.asarray(ue, dtype=np.float64).reshape(res["us"][e].shape).tobytes() == res["us"][e].tobytes(), (e, np.argwhere(res["us"][e] != ue)[:1])
    assert res["costs"][e] == ce, (e, res["costs"][e], ce)
  with pytest.raises(NotImplementedError, match="64, 64"):
    node_mle_sysid.run_node_noise_study(_training_hp(), cfg, noise_levels=(0.0,))
  from myriad_amd.systems import SystemType
  with pytest.raises(NotImplementedError, match="CARTPOLE"):
    node_mle_sysid.run_node_mle_sysid(_training_hp(system=SystemType.VANDERPOL, hidden_layers=(64, 64)), cfg)


def test_closed_form_ensemble_equals_separate_fits():
  import copy
  from myriad_amd.config import Config, HParams, OptimizerType
  from myriad_amd.experiments import mle_sysid
  from myriad_amd.systems import SystemType
  from myriad_amd.utils import generate_dataset
  hp = HParams(system=SystemType.VANDERPOL, optimizer=OptimizerType.SHOOTING, intervals=1, controls_per_interval=20, train_size=8, val_size=3, test_size=3)
  cfg = Config(verbose=False, plot=False)
  datasets = []
  for level in (0.0, 0.01):
    hp_l = copy.copy(hp)
    hp_l.noise_level = level
    datasets.append(generate_dataset(hp_l, cfg))
  res = mle_sysid.run_mle_sysid_sets(hp, cfg, np.stack(datasets), num_updates=20)
  assert len(res) == 2 and res[0]["last_params"] != res[1]["last_params"]
  for e in range(2):
    one = mle_sysid.run_mle_sysid(hp, cfg, dataset=datasets[e], num_updates=20)
    assert res[e]["last_params"] == one["last_params"], (e, res[e]["last_params"], one["last_params"])      # the same arithmetic: within 0
    assert res[e]["params"] == one["params"] and res[e]["train_losses"] == one["train_losses"] and res[e]["val_losses"] == one["val_losses"]
