"""Training of the network system by trajectory matching: /root/reference/myriad/neural_ode/node_training.py:31-110, for the
architecture the device code is built for (NodeSystem over CARTPOLE, hidden layers (64, 64)).  loss and gradient are one myr_fit_grad
call (csrc/fit.h: node_fit_kernel); Adam(hp.learning_rate) runs in numpy on the host.  No plotting, no planning losses.

`train_ensemble` runs E independent trainings (noise levels, seeds, initialisations) in lockstep: every minibatch step of all of them is ONE
myr_fit_grad_sets call, whose set e has the bits of the myr_fit_grad call `train` makes for that model alone -- so each model's weights, losses
and stopping epoch are those of its own `train` run."""
from __future__ import annotations

import numpy as np

from myriad_amd import _lib
from myriad_amd.experiments.mle_sysid import Adam
from myriad_amd.systems.neural_ode import flat_from_mapping, mapping_from_flat
from myriad_amd.utils import yield_minibatches


class NodeFitLoss:
  """loss(params, minibatch) = mean((predicted - true)^2) over trajectories, time steps and states (:31-54), with hp.integration_method."""

  def __init__(self, hp, T, engine=None):
    self.hp = hp
    self.engine = engine or _lib.Engine("NODE_CARTPOLE", "SHOOTING", 1, T, controls_per_interval=hp.num_steps,
                                        integration_method=hp.integration_method.name)

  def value_and_grad(self, params, minibatch):
    ns = self.hp.state_size
    mb = np.asarray(minibatch, dtype=np.float64)
    wt = np.full(mb.shape[1], 1.0 / (mb.shape[0] * mb.shape[1] * ns))
    out = self.engine.fit_grad(mb[:, :, :ns], mb[:, :, ns:], params=flat_from_mapping(params), wt=wt, reduce=True)
    return float(out["loss"].sum()), mapping_from_flat(out["grad"])

  def __call__(self, params, minibatch) -> float:
    return self.value_and_grad(params, minibatch)[0]

  def values_and_grads(self, params_sets, minibatches, want_grad=True):
    """value_and_grad for E weight sets at once (one myr_fit_grad_sets call): params_sets [E,4804] flat rows; minibatches [E,n,S+1,ns+nu], or
    [n,S+1,ns+nu] read by every set.  Returns (values: E floats, grads [E,4804]); want_grad=False: (values, None), no reverse sweep.  Entry e is
    value_and_grad(params_sets[e], minibatches[e]) to the bit."""
    ns = self.hp.state_size
    mb = np.asarray(minibatches, dtype=np.float64)
    wt = np.full(mb.shape[-2], 1.0 / (mb.shape[-3] * mb.shape[-2] * ns))
    out = self.engine.fit_grad_sets(mb[..., :ns], mb[..., ns:], np.asarray(params_sets, dtype=np.float64), wt=wt, reduce=True, want_grad=want_grad)
    return [float(row.sum()) for row in out["loss"]], out.get("grad")      # (row.sum(): the summation value_and_grad applies to its [n] losses)

  def values(self, params_sets, minibatches):
    return self.values_and_grads(params_sets, minibatches, want_grad=False)[0]


def loss(params, minibatch, *, hp, T, engine=None) -> float:
  """node_training.py:31-54 as a function of (params, minibatch); hp and the horizon T are what the reference's closure takes from `node`."""
  fit = NodeFitLoss(hp, T, engine)
  try:
    return fit(params, minibatch)
  finally:
    if engine is None:
      fit.engine.close()


def train(hp, T, params, train_data, val_data, rng=None, verbose=False, fit=None):
  """node_training.py:24-110: hp.num_epochs passes of minibatched Adam(hp.learning_rate) over the first hp.train_size rows, validation
  loss every hp.early_stop_check_frequency epochs, early stopping after hp.early_stop_threshold epochs without improvement.
  Returns (best_params, last epoch, [(epoch, train loss, validation loss)]).  `fit`: the loss object to use (the caller's; default: a
  NodeFitLoss of its own, closed at the end)."""
  own_fit = fit is None
  fit = NodeFitLoss(hp, T) if own_fit else fit
  rng = rng or np.random.default_rng(hp.seed)
  flat_keys = [(k, f) for k in ("linear", "linear_1", "linear_2") for f in ("w", "b")]
  opt = Adam(hp.learning_rate)
  best_val_loss, best_params, count, epoch, record = 10e10, None, 0, None, []
  validation_loss = None
  for epoch in range(hp.num_epochs):
    if epoch % hp.loss_recording_frequency == 0 or epoch % hp.early_stop_check_frequency == 0:
      train_loss, validation_loss = fit(params, train_data[:hp.train_size]), fit(params, val_data)
      record.append((epoch, train_loss, validation_loss))
      if verbose:
        print(epoch, train_loss, validation_loss)
    if epoch % hp.early_stop_check_frequency == 0:
      if count >= hp.early_stop_threshold:
        break
      if validation_loss >= best_val_loss:
        count += hp.early_stop_check_frequency
      else:
        best_val_loss, best_params, count = validation_loss, {k: {f: np.array(v) for f, v in d.items()} for k, d in params.items()}, 0
    for mb in yield_minibatches(hp, hp.train_size, train_data, rng):
      _, grads = fit.value_and_grad(params, mb)
      new = opt.update({k + "/" + f: params[k][f] for k, f in flat_keys}, {k + "/" + f: grads[k][f] for k, f in flat_keys})
      params = {k: {f: new[k + "/" + f] for f in ("w", "b")} for k in ("linear", "linear_1", "linear_2")}
  if own_fit:
    fit.engine.close()
  return best_params, epoch, record


class AdamSets:
  """mle_sysid.Adam on the rows of an [E, np] array: every row is an optimiser of its own -- its moments and its step count --, in the elementwise
  arithmetic of Adam.update.  Rows left out of a step keep both.  lr: one learning rate, or one per row ([E])."""

  def __init__(self, shape, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    self.lr, self.b1, self.b2, self.eps = (lr if np.ndim(lr) == 0 else np.asarray(lr, dtype=np.float64).reshape(shape[0])), b1, b2, eps
    self.m, self.v, self.t = np.zeros(shape), np.zeros(shape), [0] * shape[0]

  def update(self, rows, params, grads):
    """params, grads [len(rows), np] of the listed rows -> their new parameters"""
    for r in rows:
      self.t[r] += 1
    g = np.asarray(grads, dtype=np.float64)
    self.m[rows] = self.b1 * self.m[rows] + (1.0 - self.b1) * g
    self.v[rows] = self.b2 * self.v[rows] + (1.0 - self.b2) * g * g
    c1 = np.array([1.0 - self.b1 ** self.t[r] for r in rows])[:, None]      # (Python's float power per row, as Adam.update takes it)
    c2 = np.array([1.0 - self.b2 ** self.t[r] for r in rows])[:, None]
    m_hat = self.m[rows] / c1
    v_hat = self.v[rows] / c2
    lr = self.lr if np.ndim(self.lr) == 0 else self.lr[rows][:, None]      # (a row's own rate times its row: the product Adam.update takes)
    return params - lr * m_hat / (np.sqrt(v_hat) + self.eps)


def train_ensemble(hp, T, params_sets, train_data, val_data, rngs=None, fit=None, verbose=False):
  """E independent `train` runs in lockstep, the fits of all of them in one device call per step.  params_sets: E Haiku mappings or [E,4804]
  flat rows; train_data [E][M][S+1][ns+nu], or [M][...] shared by all sets; val_data likewise; rngs: one generator per set for its minibatch
  order (default np.random.default_rng(hp.seed + e)); fit: the loss object (default: a NodeFitLoss of its own, closed at the end).
  Every set has its own Adam state, best parameters and early-stop counter; a set that has stopped is taken out of the later calls; validation
  and recorded losses are loss-only calls.  Returns [(best_params, last epoch, record)] -- entry e is what
  train(hp, T, params_sets[e], train_data[e], val_data[e], rngs[e]) returns: equal values, not just close ones."""
  own_fit = fit is None
  fit = NodeFitLoss(hp, T) if own_fit else fit
  P = np.stack([np.asarray(p, dtype=np.float64) if isinstance(p, np.ndarray) else flat_from_mapping(p) for p in params_sets]) if len(params_sets) else np.empty((0, 4804))
  E = P.shape[0]
  train_data, val_data = np.asarray(train_data, dtype=np.float64), np.asarray(val_data, dtype=np.float64)
  shared_train, shared_val = train_data.ndim == 3, val_data.ndim == 3
  if not shared_train and train_data.shape[0] != E or not shared_val and val_data.shape[0] != E:
    raise ValueError(f"train_data and val_data must be [E = {E}][rows][S+1][ns+nu], or [rows][S+1][ns+nu] shared by all sets")
  rngs = [np.random.default_rng(hp.seed + e) for e in range(E)] if rngs is None else list(rngs)
  if len(rngs) != E:
    raise ValueError(f"one rng per set: {E}")
  train_of = lambda e: train_data if shared_train else train_data[e]
  opt = AdamSets(P.shape, hp.learning_rate)
  best_val_loss, best_params, count, last_epoch = [10e10] * E, [None] * E, [0] * E, [None] * E
  records = [[] for _ in range(E)]
  live = list(range(E))
  for epoch in range(hp.num_epochs):
    if not live:
      break
    for e in live:
      last_epoch[e] = epoch
    if epoch % hp.loss_recording_frequency == 0 or epoch % hp.early_stop_check_frequency == 0:
      train_losses = fit.values(P[live], train_data[:hp.train_size] if shared_train else train_data[live, :hp.train_size])
      val_losses = fit.values(P[live], val_data if shared_val else val_data[live])
      for i, e in enumerate(live):
        records[e].append((epoch, train_losses[i], val_losses[i]))
        if verbose:
          print(e, epoch, train_losses[i], val_losses[i])
    if epoch % hp.early_stop_check_frequency == 0:
      for e in list(live):
        validation_loss = records[e][-1][2]
        if count[e] >= hp.early_stop_threshold:
          live.remove(e)
        elif validation_loss >= best_val_loss[e]:
          count[e] += hp.early_stop_check_frequency
        else:
          best_val_loss[e], best_params[e], count[e] = validation_loss, mapping_from_flat(P[e]), 0
    if not live:
      break
    for mbs in zip(*[yield_minibatches(hp, hp.train_size, train_of(e), rngs[e]) for e in live]):
      _, grads = fit.values_and_grads(P[live], np.stack(mbs))
      P[live] = opt.update(live, P[live], grads)
  if own_fit:
    fit.engine.close()
  return [(best_params[e], last_epoch[e], records[e]) for e in range(E)]
