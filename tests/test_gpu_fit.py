"""myr_fit_grad on the device: trajectory-matching loss and its gradient in the model parameters (csrc/fit.h).

References as in test_fit_host_twin.py (tests/fit_cases.py): the oracle's autograd, or central differences (relative tolerance 1e-6)
for the systems whose constructors convert their arguments (of this file's subset: HIVTREATMENT).

Tolerances.  Closed-form systems: the host twin's measured bound x 10, since the device contracts FMAs and has its own libm:
  |dloss| / loss <= 2.7e-11,  |dgrad| / max|grad| <= 3.4e-10        (measured on an MI355X: 1.1e-14 / 4.0e-13 against the oracle,
  5.3e-14 / 2.0e-13 against the twin; HIVTREATMENT against central differences 2.0e-08; profiles/r11_fit/README.md)
Network system: no host twin, so the bound comes from the device's own measurement against `O.NodeCartPole` autograd over the matrix below,
as for the twin: measured |dloss| / loss 3.0e-14, |dgrad| / max|grad| 8.3e-14 (all 4 804 entries) -> asserted x 100: 3.0e-12 / 8.3e-12.
"""
import math

import numpy as np
import pytest
import torch

import fit_cases as F
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL = 2.7e-11, 3.4e-10
NODE_LOSS_TOL, NODE_GRAD_TOL = 3.0e-12, 8.3e-12      # 100 x measured
PARITY_SYSTEMS = ("CARTPOLE", "VANDERPOL", "CANCERTREATMENT", "PENDULUM", "MOUNTAINCAR", "HIVTREATMENT", "ROCKETLANDING", "PREDATORPREY", "HARVEST")


def _engine(name, method, S, T=None):
  return _lib.Engine(name, "SHOOTING", 1, F.horizon(name, S) if T is None else T, controls_per_interval=S, integration_method=method)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return F.build_twin(tmp_path_factory.mktemp("fit_twin"))


# ---- parity with the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY_SYSTEMS)
def test_parity_with_the_oracle(name):
  engines = {}
  for (_, method, long_u, weighted) in F.matrix((name,)):
    xs_obs, us, params = F.inputs(name, method, long_u)
    S = xs_obs.shape[1] - 1
    ref_loss, ref_grad = F.reference(name, method, long_u, weighted)
    eng = engines.setdefault(method, _engine(name, method, S))
    out = eng.fit_grad(xs_obs, us, params=params, wt=F.decaying_wt(S) if weighted else None)
    el, eg = F.rel_errors(out["loss"], out["grad"], ref_loss, ref_grad)
    print(f"{name} {method} u_rows={us.shape[1]} wt={'decaying' if weighted else 'none'}: dloss {el:.2e} dgrad {eg:.2e}")
    assert el <= LOSS_TOL, (method, long_u, weighted, el)
    assert eg <= (F.FD_RTOL if name in F.FD_SYSTEMS else GRAD_TOL), (method, long_u, weighted, eg)
    for k in F.COST_ONLY.get(name, ()):
      assert (out["grad"][:, F.O.SYSTEMS[name].param_names.index(k)] == 0.0).all()
  for e in engines.values():
    e.close()


# ---- device = host twin over the awkward shapes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 7])
@pytest.mark.parametrize("batch", [1, 63, 65, 130])
def test_device_equals_twin_over_awkward_shapes(twin, batch, S):
  """partial wavefront, wavefront boundary, several workgroups; one, two and seven steps; shared and per-instance parameters"""
  name, method = "CARTPOLE", "RK4"
  T = F.horizon(name, S)
  eng = _engine(name, method, S)
  for per_instance in (False, True):
    xs_obs, us, params = F.inputs(name, method, False, batch, S, per_instance)
    wt = F.decaying_wt(S)
    ref_loss, ref_grad = F.twin_loss_grad(twin, name, method, T, xs_obs, us, params, wt)
    out = eng.fit_grad(xs_obs, us, params=params, wt=wt)
    el, eg = F.rel_errors(out["loss"], out["grad"], ref_loss, ref_grad)
    print(f"B={batch} S={S} per_instance={per_instance}: dloss {el:.2e} dgrad {eg:.2e}")
    assert el <= LOSS_TOL and eg <= GRAD_TOL, (per_instance, el, eg)
    if per_instance:                                  # rows of the batched call = rows of B single calls, bit for bit
      for b in range(batch):
        one = eng.fit_grad(xs_obs[b:b + 1], us[b:b + 1], params=params[b], wt=wt)
        assert one["loss"][0] == out["loss"][b] and (one["grad"][0] == out["grad"][b]).all(), b
  eng.close()


# ---- the reduction over the batch ---------------------------------------------------------------------------------------------------
def _reduction_checks(eng, xs_obs, us, params, npar):
  rows = eng.fit_grad(xs_obs, us, params=params)
  red = eng.fit_grad(xs_obs, us, params=params, reduce=True)
  assert red["grad"].shape == (npar,)
  exact = np.array([math.fsum(rows["grad"][:, k]) for k in range(npar)])      # the correctly rounded sum of the rows
  scale = np.abs(rows["grad"]).sum(axis=0).max()
  assert np.abs(red["grad"] - exact).max() <= 1e-13 * scale
  assert (red["loss"] == rows["loss"]).all()
  again = eng.fit_grad(xs_obs, us, params=params, reduce=True)
  assert again["grad"].tobytes() == red["grad"].tobytes() and again["loss"].tobytes() == red["loss"].tobytes()
  # MYR_MEM_DEVICE on the same handle: the same bits
  B, S = xs_obs.shape[0], xs_obs.shape[1] - 1
  dev = torch.device("cuda:0")
  dx, du, dp = (torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (xs_obs, us, params))
  dl, dg = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(npar, dtype=torch.float64, device=dev)
  torch.cuda.synchronize()
  eng.fit_grad_device(B, S, us.shape[1], dx, du, dg, 0, params=dp, params_stride=0, loss=dl)
  torch.cuda.synchronize()
  assert dg.cpu().numpy().tobytes() == red["grad"].tobytes() and dl.cpu().numpy().tobytes() == red["loss"].tobytes()
  dgr = torch.empty((B, npar), dtype=torch.float64, device=dev)
  eng.fit_grad_device(B, S, us.shape[1], dx, du, dgr, npar, params=dp, params_stride=0, loss=None)
  torch.cuda.synchronize()
  assert dgr.cpu().numpy().tobytes() == rows["grad"].tobytes()


@pytest.mark.parametrize("batch", [1, 65, 600])
def test_reduction_is_deterministic_and_exact_enough(batch):
  name, method, S = "CARTPOLE", "HEUN", 3
  xs_obs, us, params = F.inputs(name, method, False, batch, S)
  eng = _engine(name, method, S)
  _reduction_checks(eng, xs_obs, us, params, 4)
  eng.close()


# ---- the network system ---------------------------------------------------------------------------------------------------------------
def _node_case(batch, S, method):
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping
  node = NeuralODE.load_fitted_cartpole()
  sysm = F.O.CartPole()
  rng = np.random.default_rng(100 * batch + 10 * S + F.METHODS.index(method))
  rows = 2 * S + 1 if method == "RK4" and batch == 5 else S + 1          # RK4: clamped rows at B = 1, its own rows at B = 5
  us = F._controls(sysm, rng, batch, rows)
  x0 = 0.3 * rng.standard_normal((batch, 4))
  h = 0.1
  xs = np.stack([F.O.integrate_time_independent(sysm.dynamics, torch.tensor(x0[b]), torch.tensor(us[b]), h, S, method)[1].numpy() for b in range(batch)])
  xs_obs = xs + 0.01 * rng.standard_normal(xs.shape)
  xs_obs[:, 0] = x0
  return node, flat_from_mapping(node.params), xs_obs, us, h * S


def _node_reference(node, method, xs_obs, us, T):
  S = xs_obs.shape[1] - 1
  keys = ("linear", "linear_1", "linear_2")
  loss, grad = [], []
  for b in range(xs_obs.shape[0]):
    tp = {k: {f: torch.tensor(np.asarray(node.params[k][f], dtype=np.float64), requires_grad=True) for f in ("w", "b")} for k in keys}
    sysm = F.O.NodeCartPole(tp)
    _, xh = F.O.integrate_time_independent(sysm.dynamics, torch.tensor(xs_obs[b, 0]), torch.tensor(us[b]), T / S, S, method)
    l = ((xh - torch.tensor(xs_obs[b])) ** 2).sum()
    leaves = [tp[k][f] for k in keys for f in ("w", "b")]
    g = torch.autograd.grad(l, leaves)
    loss.append(float(l.detach()))
    grad.append(np.concatenate([gi.numpy().ravel() for gi in g]))
  loss, grad = np.array(loss), np.stack(grad)
  assert np.isfinite(loss).all() and np.isfinite(grad).all()
  return loss, grad


@pytest.mark.parametrize("method", F.METHODS)
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("batch", [1, 5])
def test_node_parity_with_the_oracle(batch, S, method):
  node, flat, xs_obs, us, T = _node_case(batch, S, method)
  ref_loss, ref_grad = _node_reference(node, method, xs_obs, us, T)
  eng = _engine("NODE_CARTPOLE", method, S, T)
  out = eng.fit_grad(xs_obs, us, params=flat)
  assert out["grad"].shape == (batch, 4804)
  el, eg = F.rel_errors(out["loss"], out["grad"], ref_loss, ref_grad)
  print(f"NODE {method} B={batch} S={S} u_rows={us.shape[1]}: dloss {el:.2e} dgrad {eg:.2e}")
  assert el <= NODE_LOSS_TOL and eg <= NODE_GRAD_TOL, (el, eg)
  # the loss is that of myr_rollout's states
  xs, _ = eng.rollout(xs_obs[:, 0], us, S, params=flat)
  np.testing.assert_allclose(out["loss"], ((xs - xs_obs) ** 2).sum(axis=(1, 2)), rtol=1e-12)
  if batch == 5 and method == "HEUN":
    _reduction_checks(eng, xs_obs, us, flat, 4804)
  eng.close()


def test_node_training_loss_and_a_few_epochs():
  """neural_ode/node_training.py: loss(params, minibatch) is the plain mean over trajectories, steps and states of one fit_grad call, its gradient
  comes back in the Haiku layout, and a few epochs of minibatched Adam from disturbed weights bring the training loss down."""
  from myriad_amd.config import Config, HParams, OptimizerType
  from myriad_amd.neural_ode import node_training
  from myriad_amd.systems import SystemType
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping
  from myriad_amd.utils import generate_dataset
  hp = HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.SHOOTING, intervals=1, controls_per_interval=5, train_size=6, val_size=2,
               test_size=2, minibatch_size=3, num_epochs=6, loss_recording_frequency=1, early_stop_check_frequency=2, learning_rate=1e-3)
  data = generate_dataset(hp, Config(verbose=False, plot=False))
  assert data.shape == (10, 6, 5) and hp.minibatch_size == 2
  T = SystemType.CARTPOLE().T
  rng = np.random.default_rng(11)
  params = {k: {f: v + 0.05 * rng.standard_normal(v.shape) for f, v in d.items()} for k, d in NeuralODE.load_fitted_cartpole().params.items()}
  fit = node_training.NodeFitLoss(hp, T)
  mb = data[:4]
  value, grads = fit.value_and_grad(params, mb)
  wt = np.full(6, 1.0 / (4 * 6 * 4))
  ref = fit.engine.fit_grad(mb[:, :, :4], mb[:, :, 4:], params=flat_from_mapping(params), wt=wt, reduce=True)
  assert value == float(ref["loss"].sum()) and flat_from_mapping(grads).tobytes() == ref["grad"].tobytes()
  assert {k: {f: v.shape for f, v in d.items()} for k, d in grads.items()} == {k: {f: v.shape for f, v in d.items()} for k, d in params.items()}
  xs, _ = fit.engine.rollout(mb[:, 0, :4], mb[:, :, 4:], 5, params=flat_from_mapping(params))
  np.testing.assert_allclose(value, np.mean((xs - mb[:, :, :4]) ** 2), rtol=1e-12)
  assert node_training.loss(params, mb, hp=hp, T=T) == value
  assert node_training.loss(params, mb, hp=hp, T=T, engine=fit.engine) == value
  fit.engine.close()
  best, epoch, record = node_training.train(hp, T, params, data[:6], data[6:8])
  assert epoch == 5 and [r[0] for r in record] == [0, 1, 2, 3, 4, 5]
  assert record[-1][1] < record[0][1], record
  assert best is not None and set(best) == set(params) and flat_from_mapping(best).shape == (4804,)


# ---- the Adam path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", ["VANDERPOL", "CARTPOLE"])
def test_fifty_adam_steps_follow_torchs_on_the_oracles_loss(system):
  from myriad_amd.config import Config, HParams, OptimizerType
  from myriad_amd.defaults import param_guesses
  from myriad_amd.experiments import mle_sysid
  from myriad_amd.systems import SystemType
  from myriad_amd.utils import generate_dataset
  hp = HParams(system=SystemType[system], optimizer=OptimizerType.SHOOTING, intervals=1, controls_per_interval=20, train_size=8, val_size=3, test_size=3)
  cfg = Config(verbose=False, plot=False)
  dataset = generate_dataset(hp, cfg)
  assert dataset.shape == (14, 21, hp.state_size + hp.control_size)
  res = mle_sysid.run_mle_sysid(hp, cfg, dataset=dataset, num_updates=50)
  train = dataset[:8]
  names = F.O.SYSTEMS[system].param_names
  guess = param_guesses[SystemType[system]]
  assert guess == ({"a": 0.5} if system == "VANDERPOL" else {"g": 10., "m1": 1.5, "m2": 0.2, "length": 0.6})
  tp = {k: torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for k, v in guess.items()}
  opt = torch.optim.Adam(list(tp.values()), lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
  xs_t, us_t = torch.tensor(train[:, :, :hp.state_size]), torch.tensor(train[:, :, hp.state_size:])
  h = F.O.SYSTEMS[system]().T / 20

  def oracle_loss(epoch):
    sysm = F.make_system(system, [tp[k] if k in tp else float(F.O.SYSTEMS[system]().params()[i]) for i, k in enumerate(names)])
    _, xh = F.O.integrate_time_independent(sysm.dynamics, xs_t[:, 0], us_t.transpose(0, 1), h, 20, "HEUN")      # [21, 8, ns]
    wt = torch.tensor(mle_sysid.loss_weights(hp, 8, epoch))
    return (wt[:, None, None] * (xh - xs_t.transpose(0, 1)) ** 2).sum()

  first = float(oracle_loss(0).detach())
  for epoch in range(50):
    opt.zero_grad()
    oracle_loss(epoch).backward()
    opt.step()
  last = float(oracle_loss(50).detach())
  for k in guess:
    assert abs(res["last_params"][k] - float(tp[k].detach())) <= 1e-8, (k, res["last_params"][k], float(tp[k].detach()))
  fit = mle_sysid.FitLoss(hp)
  l0, l1 = fit(guess, train, 0), fit(res["last_params"], train, 50)
  fit.engine.close()
  assert abs(l0 - first) <= 1e-10 * first and abs(l1 - last) <= 1e-10 * last
  assert l1 < l0
  assert res["train_losses"][0] == l0


def test_cartpole_negative_guess_takes_the_sign_rule():
  """evaluate at |p|, multiply the gradient by sign(p) (cartpole.py:90-93): the gradient in a negative m1 is minus that in |m1|"""
  from myriad_amd.config import HParams, OptimizerType
  from myriad_amd.experiments import mle_sysid
  from myriad_amd.systems import SystemType
  hp = HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.SHOOTING, intervals=1, controls_per_interval=7)
  xs_obs, us, _ = F.inputs("CARTPOLE", "HEUN")
  data = np.concatenate([xs_obs, us], axis=2)
  fit = mle_sysid.FitLoss(hp)
  lp, gp = fit.value_and_grad({"g": 10., "m1": 1.5, "m2": 0.2, "length": 0.6}, data)
  ln, gn = fit.value_and_grad({"g": 10., "m1": -1.5, "m2": 0.2, "length": 0.6}, data)
  fit.engine.close()
  assert ln == lp and gn["m1"] == -gp["m1"] and gn["g"] == gp["g"] and gp["m1"] != 0.0


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_errors():
  xs_obs, us, _ = F.inputs("CARTPOLE", "HEUN")
  eng = _lib.Engine("CARTPOLE_ELASTIC", "HERMITE_SIMPSON", 7, 1.0)
  with pytest.raises(NotImplementedError, match="elastic"):
    eng.fit_grad(xs_obs, np.zeros((3, 8, eng.nu)))
  eng.close()
  eng = _lib.Engine("INVASIVEPLANT", "SHOOTING", 1, 10.0, controls_per_interval=7)
  with pytest.raises(NotImplementedError, match="INVASIVEPLANT"):
    eng.fit_grad(np.zeros((3, 8, eng.ns)), np.zeros((3, 8, eng.nu)))
  eng.close()
  eng = _engine("NODE_CARTPOLE", "HEUN", 7, 0.7)
  with pytest.raises(NotImplementedError, match="shared"):
    eng.fit_grad(xs_obs, us, params=np.zeros((3, 4804)))
  with pytest.raises(ValueError, match="weights"):
    eng.fit_grad(xs_obs, us)
  eng.close()
  # (the argument checks of the C call, with their full texts and their order: tests/test_gpu_api.py)


# ---- what the registers held before the launch does not reach the result --------------------------------------------------------
@pytest.mark.parametrize("name", ["CARTPOLE", "NODE_CARTPOLE"])
def test_inherited_registers_do_not_reach_the_result(monkeypatch, name):
  if name == "CARTPOLE":
    xs_obs, us, params = F.inputs("CARTPOLE", "RK4", False, 65, 7)
    T = F.horizon("CARTPOLE", 7)
  else:
    _, params, xs_obs, us, T = _node_case(5, 3, "RK4")
  bits = {}
  for pat in ("zero", "nan", "random"):
    monkeypatch.setenv("MYRIAD_REG_FILL", pat)
    monkeypatch.setenv("MYRIAD_STACK_FILL", pat)
    eng = _engine(name, "RK4", xs_obs.shape[1] - 1, T)             # (the handle reads the fill at creation)
    out = eng.fit_grad(xs_obs, us, params=params)
    red = eng.fit_grad(xs_obs, us, params=params, reduce=True)
    eng.close()
    assert np.isfinite(out["grad"]).all()
    bits[pat] = out["loss"].tobytes() + out["grad"].tobytes() + red["grad"].tobytes()
  assert bits["nan"] == bits["zero"] and bits["random"] == bits["zero"]
