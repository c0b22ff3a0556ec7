"""Parameter fitting by trajectory matching: /root/reference/myriad/experiments/mle_sysid.py:81-224.

The reference integrates a batch of recorded control sequences with `parametrized_dynamics`, takes the (discounted) mean squared
distance to the recorded states and descends jax.grad(loss) with optax.adam(1e-3).  Here loss and gradient are ONE device call
(myr_fit_grad, csrc/fit.h) and Adam runs in numpy on the host.  No plotting, pickling or CSV; the planning comparison that follows the fit
in the reference (:226-) is `useful_scripts.plan_with_params`' business.

Beside the reference's recipe: the fit is a least-squares problem in a handful of unknowns, and myr_fit_gn (csrc/fit_gn.h) returns its Gauss-Newton
matrix with the loss and gradient -- run_mle_sysid_gn / run_mle_sysid_gn_sets fit the same keys by Levenberg-Marquardt in tens of device calls and
report the parameter covariance."""
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

  def _in_keys(self, params, sign, loss, grad=None, gn=None):
    """(value, grad mapping, gn [K,K]) in the keys of `params`, in their order: split_params' sign rule is d|p|/dp = sign on grad and
    sign_i sign_j on gn; the parameters that are not fitted drop out.  grad, gn: None where the call did not form them."""
    names = self.system.param_names
    idx = [names.index(k) for k in params]
    g = None if grad is None else {k: float(v) for k, v in zip(params, (grad * sign)[idx])}
    G = None if gn is None else (gn * np.outer(sign, sign))[np.ix_(idx, idx)]
    return float(loss.sum()), g, G

  def _one(self, fit, params, dataset, epoch):
    """one mapping on one dataset through `fit` (the engine's fit_grad or fit_gn): (value, grad mapping, gn or None)"""
    ns = self.hp.state_size
    dataset = np.asarray(dataset, dtype=np.float64)
    p, sign = split_params(self.system, params)
    out = fit(dataset[:, :, :ns], dataset[:, :, ns:], params=p, wt=loss_weights(self.hp, dataset.shape[0], epoch), reduce=True)
    return self._in_keys(params, sign, out["loss"], out["grad"], out.get("gn"))

  def _sets(self, fit, params_sets, datasets, epoch, **kw):
    """E mappings at once through `fit` (fit_grad_sets or fit_gn_sets), the sign rule per set: (values, grads, gns), E entries each (None where
    the call did not form them)"""
    ns = self.hp.state_size
    datasets = np.asarray(datasets, dtype=np.float64)
    split = [split_params(self.system, params) for params in params_sets]
    out = fit(datasets[..., :ns], datasets[..., ns:], np.stack([p for p, _ in split]), wt=loss_weights(self.hp, datasets.shape[-3], epoch),
              reduce=True, **kw)
    at = lambda k, e: out[k][e] if k in out else None
    rows = [self._in_keys(params, sign, out["loss"][e], at("grad", e), at("gn", e)) for e, (params, (_, sign)) in enumerate(zip(params_sets, split))]
    return tuple([r[c] for r in rows] for c in range(3))

  def value_and_grad(self, params: Dict[str, float], dataset, epoch=0):
    return self._one(self.engine.fit_grad, params, dataset, epoch)[:2]

  def __call__(self, params, dataset, epoch=0) -> float:
    return self.value_and_grad(params, dataset, epoch)[0]

  def values_and_grads(self, params_sets, datasets, epoch=0, want_grad=True):
    """value_and_grad for E parameter mappings at once (one myr_fit_grad_sets call): datasets [E,M,S+1,ns+nu], or [M,S+1,ns+nu] read by every
    set.  The sign rule of split_params applies per set.  Returns (values: E floats, grads: E mappings); want_grad=False: (values, None), no
    reverse sweep.  Entry e is value_and_grad(params_sets[e], datasets[e], epoch) to the bit."""
    values, grads, _ = self._sets(self.engine.fit_grad_sets, params_sets, datasets, epoch, want_grad=want_grad)
    return values, (grads if want_grad else None)

  # ---- with the Gauss-Newton matrix (myr_fit_gn, csrc/fit_gn.h) ---------------------------------------------------------------
  def value_grad_gn(self, params: Dict[str, float], dataset, epoch=0):
    """(loss, its gradient as a mapping, its Gauss-Newton matrix [K,K]) in the K keys of `params`, rows and columns in their order: one
    myr_fit_gn call.  loss(params + d) ~ loss + grad . d + d . gn d / 2."""
    return self._one(self.engine.fit_gn, params, dataset, epoch)

  def values_grads_gns(self, params_sets, datasets, epoch=0):
    """value_grad_gn for E parameter mappings at once (one myr_fit_gn_sets call): datasets [E,M,S+1,ns+nu], or [M,S+1,ns+nu] read by every
    set.  Returns (values, grads, gns): E floats, E mappings, E matrices; entry e is value_grad_gn(params_sets[e], datasets[e], epoch) to the bit."""
    return self._sets(self.engine.fit_gn_sets, params_sets, datasets, epoch)


def lm_accepts(value, loss) -> bool:
  """the project's one rule for a Levenberg-Marquardt trial point: it is taken only if its loss is lower"""
  return float(value) < float(loss)


def lm_next_lambda(lam, accepted):
  """... and for the damping: a third on acceptance, four times on rejection (LevenbergMarquardt below, node_training.LevenbergMarquardtCG)"""
  return lam / 3.0 if accepted else lam * 4.0


class LevenbergMarquardt:
  """Levenberg-Marquardt on a mapping of floats, driven from outside so that many fits can run in lockstep:
    begin(value, grad, gn) at the start point; then, until `done`, p = trial() and end(value, grad, gn) with the evaluation at p.
  A trial point is params + d with (G + lam diag(G)) d = -g on the keys whose diagonal entry of G is positive (a key the data do not move stays).
  It is accepted only if its loss is lower -- the evaluation is then the next iteration's: one call per iteration --, lam / 3 on acceptance, lam * 4
  on rejection, lam = 1e-3 at the start.  Stops on an accepted relative decrease of the loss below `rtol`, at `max_iter` trial points, or once the
  loss is below `ftol` times the loss at the start (residuals at the rounding level of the rollout: a decrease there is noise)."""

  def __init__(self, params: Dict[str, float], lam=1e-3, rtol=1e-12, max_iter=50, ftol=1e-24):
    self.params = dict(params)
    self.keys = list(params)
    self.lam, self.rtol, self.max_iter, self.ftol = float(lam), rtol, max_iter, ftol
    self.iterations, self.done = 0, False
    self.loss = self.loss0 = None
    self.grad = self.gn = self._trial = None

  def begin(self, value, grad, gn):
    self.loss = self.loss0 = float(value)
    self.grad, self.gn = np.array([grad[k] for k in self.keys], dtype=np.float64), np.array(gn, dtype=np.float64)
    self.done = self.max_iter < 1 or not self.loss > 0.0

  def step(self) -> np.ndarray:
    """d [K] of the current point, gradient, matrix and lam"""
    d = np.zeros(len(self.keys))
    diag = np.diag(self.gn)
    on = np.flatnonzero(diag > 0.0)
    if on.size:
      A = self.gn[np.ix_(on, on)] + self.lam * np.diag(diag[on])
      try:
        d[on] = np.linalg.solve(A, -self.grad[on])
      except np.linalg.LinAlgError:
        d[on] = np.linalg.lstsq(A, -self.grad[on], rcond=None)[0]
    return d

  def trial(self) -> Dict[str, float]:
    d = self.step()
    self._trial = {k: float(self.params[k] + d[i]) for i, k in enumerate(self.keys)}
    return dict(self._trial)

  def end(self, value, grad, gn) -> bool:
    """the evaluation at the last trial point; True: the point was accepted"""
    self.iterations += 1
    value = float(value)
    accepted = lm_accepts(value, self.loss)
    if accepted:
      decrease = (self.loss - value) / self.loss
      self.params, self.loss = self._trial, value
      self.grad, self.gn = np.array([grad[k] for k in self.keys], dtype=np.float64), np.array(gn, dtype=np.float64)
      if decrease < self.rtol or value <= self.ftol * self.loss0:
        self.done = True
    self.lam = lm_next_lambda(self.lam, accepted)
    if self.iterations >= self.max_iter:
      self.done = True
    return accepted


def parameter_covariance(gn, loss, n_residuals):
  """Covariance of the fitted parameters, sigma^2 (gn / 2)^+ with sigma^2 = loss / (n_residuals - rank): gn / 2 = J^T W J is the Fisher
  information of the fit up to the noise variance, which the residuals estimate.  The pseudo-inverse runs over the keys with a positive diagonal
  entry (the others get rows and columns of 0: the data say nothing about them); rank is that block's."""
  gn = np.asarray(gn, dtype=np.float64)
  cov = np.zeros_like(gn)
  on = np.flatnonzero(np.diag(gn) > 0.0)
  rank = 0
  if on.size:
    F = 0.5 * gn[np.ix_(on, on)]
    rank = int(np.linalg.matrix_rank(F, hermitian=True))
    dof = n_residuals - rank
    sigma2 = float(loss) / dof if dof > 0 else float("nan")
    cov[np.ix_(on, on)] = sigma2 * np.linalg.pinv(F, hermitian=True)
  return cov


def _gn_result(hp, lm, record, best_params, n_train):
  out = dict(record)
  out.update({"params": best_params, "last_params": dict(lm.params), "iterations": lm.iterations, "gn": lm.gn,
              "covariance": parameter_covariance(lm.gn, lm.loss, n_train * hp.num_steps * hp.state_size)})
  return out


def run_mle_sysid_gn(hp: HParams, cfg: Config, dataset=None, max_iter: int = 50, rtol: float = 1e-12, fit=None, guess=None) -> dict:
  """run_mle_sysid's fit by Levenberg-Marquardt on the Gauss-Newton matrix (myr_fit_gn): the same keys from the same start, the reference's loss at
  epoch 0 (fixed discount weights), tens of device calls where Adam makes hp.num_epochs * 10.  Train and validation loss are recorded at the start
  and after every accepted step ("epochs": the iteration it was accepted in); "params" are those with the lowest validation loss.  Returns
  run_mle_sysid's dictionary plus "iterations" (trial points evaluated), "gn" (at the last parameters, in the order of their keys) and "covariance"
  (parameter_covariance).  fit: a FitLoss to run on (tests: one with a host stand-in for the engine); it is left open.  guess: the starting
  mapping, whose keys are fitted (default: defaults.param_guesses[hp.system])."""
  if dataset is None:
    dataset = generate_dataset(hp, cfg)
  dataset = np.asarray(dataset, dtype=np.float64)
  train_set, val_set = dataset[:hp.train_size], dataset[hp.train_size:dataset.shape[0] - hp.test_size]
  own_fit = fit is None
  if own_fit:
    fit = FitLoss(hp)
  lm = LevenbergMarquardt(param_guesses[hp.system] if guess is None else guess, rtol=rtol, max_iter=max_iter)
  record = {"epochs": [], "train_losses": [], "val_losses": []}
  best = [None, None]                                             # lowest validation loss, its parameters

  def note(epoch):
    val_loss = fit(lm.params, val_set, 0) if val_set.shape[0] else lm.loss
    record["epochs"].append(epoch); record["train_losses"].append(lm.loss); record["val_losses"].append(val_loss)
    if cfg.verbose:
      print("loss", lm.loss, "val loss", val_loss, "lambda", lm.lam)
    if np.isnan(lm.loss):
      raise FloatingPointError(f"mle_sysid: the loss is NaN at params {lm.params}")
    if best[0] is None or val_loss < best[0]:
      best[0], best[1] = val_loss, dict(lm.params)

  lm.begin(*fit.value_grad_gn(lm.params, train_set, 0))
  note(0)
  while not lm.done:
    if lm.end(*fit.value_grad_gn(lm.trial(), train_set, 0)):
      note(lm.iterations)
  if own_fit:
    fit.engine.close()
  return _gn_result(hp, lm, record, best[1], train_set.shape[0])


def run_mle_sysid_gn_sets(hp: HParams, cfg: Config, datasets, guesses=None, max_iter: int = 50, rtol: float = 1e-12, fit=None) -> list:
  """run_mle_sysid_gn for E datasets [E][train+val+test][S+1][ns+nu] at once (`guesses`: E starting mappings, default
  defaults.param_guesses[hp.system] for every set): the fits run in lockstep, every iteration of all of them in one myr_fit_gn_sets call.  Each set
  has its own lambda, record and stopping state, and leaves the later calls once it has stopped.  Returns E dictionaries; entry e is what
  run_mle_sysid_gn(hp, cfg, datasets[e]) returns (from guesses[e]): the same arithmetic, equal values."""
  datasets = np.asarray(datasets, dtype=np.float64)
  E = datasets.shape[0]
  train_sets, val_sets = datasets[:, :hp.train_size], datasets[:, hp.train_size:datasets.shape[1] - hp.test_size]
  own_fit = fit is None
  if own_fit:
    fit = FitLoss(hp)
  lms = [LevenbergMarquardt(param_guesses[hp.system] if guesses is None else guesses[e], rtol=rtol, max_iter=max_iter) for e in range(E)]
  records = [{"epochs": [], "train_losses": [], "val_losses": []} for _ in range(E)]
  best = [[None, None] for _ in range(E)]

  def note(sets):
    if not sets:
      return
    if val_sets.shape[1]:
      val_losses = fit.values_and_grads([lms[e].params for e in sets], val_sets[sets], 0, want_grad=False)[0]
    else:
      val_losses = [lms[e].loss for e in sets]
    for e, val_loss in zip(sets, val_losses):
      lm, r = lms[e], records[e]
      r["epochs"].append(lm.iterations); r["train_losses"].append(lm.loss); r["val_losses"].append(val_loss)
      if cfg.verbose:
        print(e, "loss", lm.loss, "val loss", val_loss, "lambda", lm.lam)
      if np.isnan(lm.loss):
        raise FloatingPointError(f"mle_sysid: the loss of set {e} is NaN at params {lm.params}")
      if best[e][0] is None or val_loss < best[e][0]:
        best[e][0], best[e][1] = val_loss, dict(lm.params)

  live = list(range(E))
  for e, value, grad, gn in zip(live, *fit.values_grads_gns([lm.params for lm in lms], train_sets, 0)):
    lms[e].begin(value, grad, gn)
  note(live)
  live = [e for e in live if not lms[e].done]
  while live:
    evals = fit.values_grads_gns([lms[e].trial() for e in live], train_sets[live], 0)
    note([e for e, value, grad, gn in zip(live, *evals) if lms[e].end(value, grad, gn)])
    live = [e for e in live if not lms[e].done]
  if own_fit:
    fit.engine.close()
  return [_gn_result(hp, lms[e], records[e], best[e][1], train_sets.shape[1]) for e in range(E)]


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
