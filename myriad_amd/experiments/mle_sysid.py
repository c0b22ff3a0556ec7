"""Parameter fitting by trajectory matching: /root/reference/myriad/experiments/mle_sysid.py:81-224.

The reference integrates a batch of recorded control sequences with `parametrized_dynamics`, takes the (discounted) mean squared
distance to the recorded states and descends jax.grad(loss) with optax.adam(1e-3).  Here loss and gradient are ONE device call
(myr_fit_grad, csrc/fit.h) and Adam runs in numpy on the host.  No plotting, pickling or CSV; the planning comparison that follows the fit
in the reference (:226-) is `useful_scripts.plan_with_params`' business."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from myriad_amd import _lib
from myriad_amd.config import Config, HParams
from myriad_amd.defaults import param_guesses
from myriad_amd.systems import SystemType
from myriad_amd.utils import generate_dataset

DISCOUNTED = (SystemType.BACTERIA, SystemType.MOUNTAINCAR, SystemType.CARTPOLE)      # mle_sysid.py:121


def loss_weights(hp, batch: int, epoch) -> np.ndarray:
  """wt [num_steps+1] of myr_fit_grad that makes sum_b loss[b] the reference's loss (:117-125): mean over batch and states per time
  step, times discount_t = (1 - 1 / (1 + exp(2 + 1e-6 epoch)))^t for BACTERIA, MOUNTAINCAR and CARTPOLE (1 otherwise), mean over time."""
  n = hp.num_steps + 1
  discount = (1.0 - 1.0 / (1.0 + np.exp(2.0 + 0.000001 * epoch))) ** np.arange(n) if hp.system in DISCOUNTED else np.ones(n)
  return discount / (n * batch * hp.state_size)


def split_params(system, params: Dict[str, float]):
  """(device parameter vector, sign [np]) of a parameter mapping.  CARTPOLE's parametrized dynamics take |p| (cartpole.py:90-93): the
  device evaluates at |p| and the chain rule multiplies the gradient by sign(p); other systems: the values themselves, sign 1."""
  raw = system.device_params()
  for i, k in enumerate(system.param_names):
    if k in params:
      raw[i] = float(params[k])
  p = system.params_from_mapping(params)
  sign = np.where(p == raw, 1.0, np.sign(raw))
  return p, sign


class FitLoss:
  """loss(params, dataset, epoch) and its gradient in the keys of `params`, on one device handle (HEUN, as the reference hard-codes)."""

  def __init__(self, hp, engine=None):
    self.hp = hp
    self.system = hp.system()
    self.engine = engine or _lib.Engine(self.system.name, "SHOOTING", 1, self.system.T, controls_per_interval=hp.num_steps,
                                        integration_method="HEUN")

  def value_and_grad(self, params: Dict[str, float], dataset, epoch=0):
    ns = self.hp.state_size
    dataset = np.asarray(dataset, dtype=np.float64)
    p, sign = split_params(self.system, params)
    out = self.engine.fit_grad(dataset[:, :, :ns], dataset[:, :, ns:], params=p, wt=loss_weights(self.hp, dataset.shape[0], epoch), reduce=True)
    names = self.system.param_names
    g = out["grad"] * sign
    return float(out["loss"].sum()), {k: float(g[names.index(k)]) for k in params}

  def __call__(self, params, dataset, epoch=0) -> float:
    return self.value_and_grad(params, dataset, epoch)[0]

  def values_and_grads(self, params_sets, datasets, epoch=0, want_grad=True):
    """value_and_grad for E parameter mappings at once (one myr_fit_grad_sets call): datasets [E,M,S+1,ns+nu], or [M,S+1,ns+nu] read by every
    set.  The sign rule of split_params applies per set.  Returns (values: E floats, grads: E mappings); want_grad=False: (values, None), no
    reverse sweep.  Entry e is value_and_grad(params_sets[e], datasets[e], epoch) to the bit."""
    ns = self.hp.state_size
    datasets = np.asarray(datasets, dtype=np.float64)
    split = [split_params(self.system, params) for params in params_sets]
    out = self.engine.fit_grad_sets(datasets[..., :ns], datasets[..., ns:], np.stack([p for p, _ in split]),
                                    wt=loss_weights(self.hp, datasets.shape[-3], epoch), reduce=True, want_grad=want_grad)
    values = [float(row.sum()) for row in out["loss"]]
    if not want_grad:
      return values, None
    names = self.system.param_names
    grads = []
    for params, (_, sign), row in zip(params_sets, split, out["grad"]):
      g = row * sign
      grads.append({k: float(g[names.index(k)]) for k in params})
    return values, grads


class Adam:
  """optax.adam(lr) with its defaults b1 = 0.9, b2 = 0.999, eps = 1e-8, eps_root = 0, on a mapping of floats."""

  def __init__(self, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    self.lr, self.b1, self.b2, self.eps = lr, b1, b2, eps
    self.m: Dict[str, float] = {}
    self.v: Dict[str, float] = {}
    self.t = 0

  def update(self, params, grads):
    self.t += 1
    new = {}
    for k, g in grads.items():
      g = np.asarray(g, dtype=np.float64)
      self.m[k] = self.b1 * self.m.get(k, 0.0) + (1.0 - self.b1) * g
      self.v[k] = self.b2 * self.v.get(k, 0.0) + (1.0 - self.b2) * g * g
      m_hat = self.m[k] / (1.0 - self.b1 ** self.t)
      v_hat = self.v[k] / (1.0 - self.b2 ** self.t)
      new[k] = params[k] - self.lr * m_hat / (np.sqrt(v_hat) + self.eps)
    return new


def run_mle_sysid(hp: HParams, cfg: Config, dataset=None, num_updates: Optional[int] = None, check_frequency: int = 500) -> dict:
  """mle_sysid.py:81-224: fit the keys of defaults.param_guesses[hp.system] to a dataset of hp.train_size / val_size / test_size
  trajectories; full-batch Adam(1e-3) for hp.num_epochs * 10 updates (or `num_updates`), train and validation loss every 500 updates,
  early stopping on the validation loss (:146-178).  Returns {"params": best_params, "last_params", "epochs", "train_losses", "val_losses"}."""
  if dataset is None:
    dataset = generate_dataset(hp, cfg)
  train_set, val_set = dataset[:hp.train_size], dataset[hp.train_size:-hp.test_size]
  fit = FitLoss(hp)
  params = dict(param_guesses[hp.system])
  opt = Adam(1e-3)
  epochs, train_losses, val_losses = [], [], []
  best_val_loss, best_params, count = None, None, 0
  for epoch in range(hp.num_epochs * 10 if num_updates is None else num_updates):
    if epoch % check_frequency == 0:
      cur_loss, val_loss = fit(params, train_set, epoch), fit(params, val_set, epoch)
      epochs.append(epoch); train_losses.append(cur_loss); val_losses.append(val_loss)
      if cfg.verbose:
        print("loss", cur_loss, "val loss", val_loss)
      if np.isnan(cur_loss):
        raise FloatingPointError(f"mle_sysid: the loss is NaN at params {params}")
      if best_val_loss is None or val_loss < best_val_loss:
        best_val_loss, best_params, count = val_loss, dict(params), 0
      elif count > hp.early_stop_threshold:
        if cfg.verbose:
          print("stopping early at epoch", epoch)
        break
      count += check_frequency
    _, grads = fit.value_and_grad(params, train_set, epoch)
    params = opt.update(params, grads)
  fit.engine.close()
  return {"params": best_params, "last_params": params, "epochs": epochs, "train_losses": train_losses, "val_losses": val_losses}


def run_mle_sysid_sets(hp: HParams, cfg: Config, datasets, guesses=None, num_updates: Optional[int] = None, check_frequency: int = 500) -> list:
  """run_mle_sysid for E datasets [E][train+val+test][S+1][ns+nu] at once (noise levels, seeds; `guesses`: E starting mappings, default
  defaults.param_guesses[hp.system] for every set): the fits run in lockstep, every update of all of them in one myr_fit_grad_sets call.  Each set has
  its own Adam state, best parameters and early-stop counter, and leaves the later calls once it has stopped.  Returns E dictionaries; entry e is
  what run_mle_sysid(hp, cfg, datasets[e]) returns (from guesses[e]): the same arithmetic, equal values."""
  datasets = np.asarray(datasets, dtype=np.float64)
  E = datasets.shape[0]
  train_sets, val_sets = datasets[:, :hp.train_size], datasets[:, hp.train_size:-hp.test_size]
  fit = FitLoss(hp)
  params = [dict(param_guesses[hp.system] if guesses is None else guesses[e]) for e in range(E)]
  opts = [Adam(1e-3) for _ in range(E)]
  out = [{"params": None, "last_params": None, "epochs": [], "train_losses": [], "val_losses": []} for _ in range(E)]
  best_val_loss, count = [None] * E, [0] * E
  live = list(range(E))
  for epoch in range(hp.num_epochs * 10 if num_updates is None else num_updates):
    if not live:
      break
    if epoch % check_frequency == 0:
      cur = [params[e] for e in live]
      cur_losses = fit.values_and_grads(cur, train_sets[live], epoch, want_grad=False)[0]
      val_losses = fit.values_and_grads(cur, val_sets[live], epoch, want_grad=False)[0]
      for e, cur_loss, val_loss in zip(list(live), cur_losses, val_losses):
        o = out[e]
        o["epochs"].append(epoch); o["train_losses"].append(cur_loss); o["val_losses"].append(val_loss)
        if cfg.verbose:
          print(e, "loss", cur_loss, "val loss", val_loss)
        if np.isnan(cur_loss):
          raise FloatingPointError(f"mle_sysid: the loss of set {e} is NaN at params {params[e]}")
        if best_val_loss[e] is None or val_loss < best_val_loss[e]:
          best_val_loss[e], o["params"], count[e] = val_loss, dict(params[e]), 0
        elif count[e] > hp.early_stop_threshold:
          if cfg.verbose:
            print(e, "stopping early at epoch", epoch)
          live.remove(e)
          continue
        count[e] += check_frequency
      if not live:
        break
    _, grads = fit.values_and_grads([params[e] for e in live], train_sets[live], epoch)
    for e, g in zip(live, grads):
      params[e] = opts[e].update(params[e], g)
  fit.engine.close()
  for e in range(E):
    out[e]["last_params"] = params[e]
  return out
