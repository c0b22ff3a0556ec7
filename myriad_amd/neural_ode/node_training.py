"""Training of the network system by trajectory matching: /root/reference/myriad/neural_ode/node_training.py:31-110, for the
architecture the device code is built for (NodeSystem over CARTPOLE, hidden layers (64, 64)).  loss and gradient are one myr_fit_grad
call (csrc/fit.h: node_fit_kernel); Adam(hp.learning_rate) runs in numpy on the host.  No plotting, no planning losses."""
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


def loss(params, minibatch, *, hp, T, engine=None) -> float:
  """node_training.py:31-54 as a function of (params, minibatch); hp and the horizon T are what the reference's closure takes from `node`."""
  fit = NodeFitLoss(hp, T, engine)
  try:
    return fit(params, minibatch)
  finally:
    if engine is None:
      fit.engine.close()


def train(hp, T, params, train_data, val_data, rng=None, verbose=False):
  """node_training.py:24-110: hp.num_epochs passes of minibatched Adam(hp.learning_rate) over the first hp.train_size rows, validation
  loss every hp.early_stop_check_frequency epochs, early stopping after hp.early_stop_threshold epochs without improvement.
  Returns (best_params, last epoch, [(epoch, train loss, validation loss)])."""
  fit = NodeFitLoss(hp, T)
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
  fit.engine.close()
  return best_params, epoch, record
