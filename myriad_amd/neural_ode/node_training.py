"""Training of the network system by trajectory matching: /root/reference/myriad/neural_ode/node_training.py:31-110, for the
architecture the device code is built for (NodeSystem over CARTPOLE, hidden layers (64, 64)).  loss and gradient are one myr_fit_grad
call (csrc/fit.h: node_fit_kernel); Adam(hp.learning_rate) runs in numpy on the host.  No plotting, no planning losses.

`train_ensemble` runs E independent trainings (noise levels, seeds, initialisations) in lockstep: every minibatch step of all of them is ONE
myr_fit_grad_sets call, whose set e has the bits of the myr_fit_grad call `train` makes for that model alone -- so each model's weights, losses
and stopping epoch are those of its own `train` run."""
from __future__ import annotations

import numpy as np

from myriad_amd import _lib
from myriad_amd.experiments.mle_sysid import Adam, lm_accepts, lm_next_lambda
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

  def gn_product(self, params, v, minibatch):
    """G v [4804] for the Gauss-Newton matrix G = 2 J^T W J of this loss at `params` (a mapping or flat), v flat: one myr_fit_gnvp call, no matrix.
    loss(params + d) ~ loss + grad . d + d . G d / 2 with value_and_grad's loss and gradient."""
    ns = self.hp.state_size
    mb = np.asarray(minibatch, dtype=np.float64)
    wt = np.full(mb.shape[1], 1.0 / (mb.shape[0] * mb.shape[1] * ns))
    p = params if isinstance(params, np.ndarray) else flat_from_mapping(params)
    return self.engine.fit_gnvp(mb[:, :, :ns], mb[:, :, ns:], p, v, wt=wt, reduce=True)["out"]

  def gn_products(self, params_sets, vs, minibatches):
    """gn_product for E weight sets at once (one myr_fit_gnvp_sets call): params_sets, vs [E,4804]; minibatches as in values_and_grads.  Row e is
    gn_product(params_sets[e], vs[e], minibatches[e]) to the bit."""
    ns = self.hp.state_size
    mb = np.asarray(minibatches, dtype=np.float64)
    wt = np.full(mb.shape[-2], 1.0 / (mb.shape[-3] * mb.shape[-2] * ns))
    return self.engine.fit_gnvp_sets(mb[..., :ns], mb[..., ns:], np.asarray(params_sets, dtype=np.float64), np.asarray(vs, dtype=np.float64), wt=wt,
                                     reduce=True)["out"]


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


# ---- second-order training: Levenberg-Marquardt with a conjugate-gradient inner solve on the matrix-free Gauss-Newton product (myr_fit_gnvp) --------
class ConjugateGradient:
  """Conjugate gradients for A d = b from d = 0, A symmetric positive definite and known by its products only.  Driven from outside, so that many
  solves can share one device call per product:  while not cg.done: cg.feed(A @ cg.p).
  Truncated: it stops after `iters` products, once |b - A d| <= tol |b| (the recurrence's residual), or at a direction without positive curvature
  (A is positive definite: rounding).  d is `x`; `products` counts the feeds; `residual` is |b - A d| / |b|."""

  def __init__(self, b, iters, tol):
    b = np.array(b, dtype=np.float64)
    self.x, self.r, self.p = np.zeros_like(b), b.copy(), b.copy()
    self.rs = self.b2 = float(b @ b)
    self.iters, self.tol, self.products = int(iters), float(tol), 0
    self.done = self.iters < 1 or not self.rs > 0.0

  @property
  def residual(self) -> float:
    return float(np.sqrt(self.rs / self.b2)) if self.b2 > 0.0 else 0.0

  def feed(self, Ap):
    self.products += 1
    pAp = float(self.p @ Ap)
    if not pAp > 0.0:
      self.done = True
      return
    alpha = self.rs / pAp
    self.x = self.x + alpha * self.p
    self.r = self.r - alpha * Ap
    rs = float(self.r @ self.r)
    if rs <= self.tol * self.tol * self.b2 or self.products >= self.iters:
      self.done = True
    else:
      self.p = self.r + (rs / self.rs) * self.p
    self.rs = rs


def conjugate_gradient(op, b, iters, tol):
  """ConjugateGradient run on an operator callable op(v) = A v: (d, products made, |b - A d| / |b|)"""
  cg = ConjugateGradient(b, iters, tol)
  while not cg.done:
    cg.feed(op(cg.p))
  return cg.x, cg.products, cg.residual


class LevenbergMarquardtCG:
  """Levenberg-Marquardt on a flat parameter vector with the step from a truncated conjugate-gradient solve of (G + lam I) d = -g, G known by its
  products only.  Driven from outside, as mle_sysid.LevenbergMarquardt is:
    begin(value, grad) at the start point; then, until `done`:  while solving: feed(G @ direction());  then end(value, grad) with the evaluation at trial().
  Acceptance and the damping follow mle_sysid's rule (lm_accepts, lm_next_lambda; lam = 1e-3 at the start): the evaluation at an accepted trial point
  is the next iteration's, a rejected one is solved again from the same gradient with the larger lam.  Stops as LevenbergMarquardt does: on an accepted
  relative decrease below `rtol`, at `max_iter` trial points, or below `ftol` times the loss at the start.  `last`: the record of the last trial."""

  def __init__(self, params, lam=1e-3, cg_iters=20, cg_tol=1e-2, rtol=1e-12, max_iter=50, ftol=1e-24):
    self.params = np.array(params, dtype=np.float64)
    self.lam, self.cg_iters, self.cg_tol, self.rtol, self.max_iter, self.ftol = float(lam), cg_iters, cg_tol, rtol, max_iter, ftol
    self.iterations, self.done = 0, False
    self.loss = self.loss0 = self.grad = self.cg = self.last = None

  def begin(self, value, grad):
    self.loss = self.loss0 = float(value)
    self.grad = np.array(grad, dtype=np.float64)
    self.done = self.max_iter < 1 or not self.loss > 0.0
    self.cg = ConjugateGradient(-self.grad, self.cg_iters, self.cg_tol)

  @property
  def solving(self) -> bool:
    return not self.done and not self.cg.done

  def direction(self) -> np.ndarray:
    """the vector whose product the solve waits for; 0 where it waits for none (a model that rides along in a lockstep call)"""
    return self.cg.p if self.solving else np.zeros_like(self.params)

  def feed(self, Gv):
    self.cg.feed(np.asarray(Gv, dtype=np.float64) + self.lam * self.cg.p)

  def trial(self) -> np.ndarray:
    return self.params + self.cg.x

  def end(self, value, grad) -> bool:
    """the evaluation at trial(); True: the point was accepted"""
    self.iterations += 1
    value = float(value)
    accepted = lm_accepts(value, self.loss)
    self.last = {"params": self.params, "grad": self.grad, "lam": self.lam, "d": self.cg.x, "cg_products": self.cg.products,
                 "cg_residual": self.cg.residual, "loss": self.loss, "trial_loss": value, "accepted": accepted}
    if accepted:
      decrease = (self.loss - value) / self.loss
      self.params, self.loss, self.grad = self.trial(), value, np.array(grad, dtype=np.float64)
      if decrease < self.rtol or value <= self.ftol * self.loss0:
        self.done = True
    self.lam = lm_next_lambda(self.lam, accepted)
    if self.iterations >= self.max_iter:
      self.done = True
    self.cg = ConjugateGradient(-self.grad, self.cg_iters, self.cg_tol)
    return accepted


def _gn_lockstep(hp, lms, value_grads, products, val_losses, verbose, histories):
  """The loop train_gn and train_ensemble_gn share: the models `lms` (LevenbergMarquardtCG, at their start points) in lockstep.  An outer step -- one
  trial point -- is an epoch of train's bookkeeping: validation loss every hp.early_stop_check_frequency steps, the best parameters and the early-stop
  counter as train keeps them; the point a model ends at is checked too.  value_grads(sets, P) -> (values, grads); products(sets, P, V) -> [n,4804];
  val_losses(sets, P) -> values: the device calls, for the listed models.  Returns [(best_params, last step, record)]."""
  E = len(lms)
  best_val_loss, best_params, count, last_epoch = [10e10] * E, [None] * E, [0] * E, [None] * E
  records = [[] for _ in range(E)]
  live = list(range(E))

  def note(sets, epoch, check):
    new = [e for e in sets if not (records[e] and records[e][-1][0] == epoch)]      # (one record per model and epoch)
    if new:
      for e, validation_loss in zip(new, val_losses(new, np.stack([lms[e].params for e in new]))):
        records[e].append((epoch, lms[e].loss, validation_loss))
        if verbose:
          print(e, epoch, lms[e].loss, validation_loss, lms[e].lam)
    for e in sets if check else ():
      validation_loss = records[e][-1][2]
      if count[e] >= hp.early_stop_threshold:
        lms[e].done = True
      elif validation_loss >= best_val_loss[e]:
        count[e] += hp.early_stop_check_frequency
      else:
        best_val_loss[e], best_params[e], count[e] = validation_loss, mapping_from_flat(lms[e].params), 0

  if live:
    values, grads = value_grads(live, np.stack([lms[e].params for e in live]))
    for i, e in enumerate(live):
      lms[e].begin(values[i], grads[i])
  epoch = 0
  while live:
    for e in live:
      last_epoch[e] = epoch
    check = epoch % hp.early_stop_check_frequency == 0
    if check or epoch % hp.loss_recording_frequency == 0:
      note(live, epoch, check)
    ended = [e for e in live if lms[e].done]
    live = [e for e in live if not lms[e].done]
    if ended and not check:                            # the point a model ends at is recorded and compared too
      note(ended, epoch, True)
    if not live:
      break
    P = np.stack([lms[e].params for e in live])
    while any(lms[e].solving for e in live):           # the inner solves: one product call for all models; a finished solve rides along with 0
      Gv = products(live, P, np.stack([lms[e].direction() for e in live]))
      for i, e in enumerate(live):
        if lms[e].solving:
          lms[e].feed(Gv[i])
    values, grads = value_grads(live, np.stack([lms[e].trial() for e in live]))
    for i, e in enumerate(live):
      lms[e].end(values[i], grads[i])
      if histories is not None:
        histories[e].append(lms[e].last)
    epoch += 1
  return [(best_params[e], last_epoch[e], records[e]) for e in range(E)]


def train_gn(hp, T, params, train_data, val_data, max_iter=50, cg_iters=20, cg_tol=1e-2, lam=1e-3, rtol=1e-12, verbose=False, fit=None, history=None):
  """train's fit by Levenberg-Marquardt on the full training set (the first hp.train_size rows): per outer step one myr_fit_grad call (the loss and
  gradient at the trial point) and at most `cg_iters` myr_fit_gnvp calls (the truncated conjugate-gradient solve of (G + lam I) d = -g to the relative
  residual `cg_tol`); mle_sysid's rule for lam and for taking a step; train's validation and early-stop bookkeeping with an outer step as the epoch.
  Returns train's (best_params, last step, [(step, train loss, validation loss)]).  history: a list that receives one record per trial point
  (LevenbergMarquardtCG.last).  fit: the loss object to use (default: a NodeFitLoss of its own, closed at the end)."""
  own_fit = fit is None
  fit = NodeFitLoss(hp, T) if own_fit else fit
  data = np.asarray(train_data, dtype=np.float64)[:hp.train_size]
  val = np.asarray(val_data, dtype=np.float64)
  p0 = params if isinstance(params, np.ndarray) else flat_from_mapping(params)
  lm = LevenbergMarquardtCG(p0, lam=lam, cg_iters=cg_iters, cg_tol=cg_tol, rtol=rtol, max_iter=max_iter)

  def value_grads(sets, P):
    value, grad = fit.value_and_grad(mapping_from_flat(P[0]), data)
    return [value], [flat_from_mapping(grad)]

  out = _gn_lockstep(hp, [lm], value_grads, lambda sets, P, V: [fit.gn_product(P[0], V[0], data)], lambda sets, P: [fit(mapping_from_flat(P[0]), val)],
                     verbose, None if history is None else [history])
  if own_fit:
    fit.engine.close()
  return out[0]


def train_ensemble_gn(hp, T, params_sets, train_data, val_data, max_iter=50, cg_iters=20, cg_tol=1e-2, lam=1e-3, rtol=1e-12, verbose=False, fit=None,
                      histories=None):
  """E independent train_gn runs in lockstep on the sets calls: every product of all inner solves is ONE myr_fit_gnvp_sets call, every trial point of
  all models one myr_fit_grad_sets call.  Each model has its own lam and its own conjugate-gradient state; a model whose solve has ended rides along in
  the product calls with the direction 0, one that has stopped leaves the later calls.  params_sets, train_data, val_data as in train_ensemble;
  histories: E lists (train_gn's history).  Entry e of the result is what train_gn returns for that model alone: equal values."""
  own_fit = fit is None
  fit = NodeFitLoss(hp, T) if own_fit else fit
  P0 = np.stack([np.asarray(p, dtype=np.float64) if isinstance(p, np.ndarray) else flat_from_mapping(p) for p in params_sets]) if len(params_sets) else np.empty((0, 4804))
  E = P0.shape[0]
  train_data, val_data = np.asarray(train_data, dtype=np.float64), np.asarray(val_data, dtype=np.float64)
  shared_train, shared_val = train_data.ndim == 3, val_data.ndim == 3
  if not shared_train and train_data.shape[0] != E or not shared_val and val_data.shape[0] != E:
    raise ValueError(f"train_data and val_data must be [E = {E}][rows][S+1][ns+nu], or [rows][S+1][ns+nu] shared by all sets")
  data_of = lambda sets: train_data[:hp.train_size] if shared_train else train_data[sets, :hp.train_size]
  lms = [LevenbergMarquardtCG(P0[e], lam=lam, cg_iters=cg_iters, cg_tol=cg_tol, rtol=rtol, max_iter=max_iter) for e in range(E)]
  out = _gn_lockstep(hp, lms, lambda sets, P: fit.values_and_grads(P, data_of(sets)), lambda sets, P, V: fit.gn_products(P, V, data_of(sets)),
                     lambda sets, P: fit.values(P, val_data if shared_val else val_data[sets]), verbose, histories)
  if own_fit:
    fit.engine.close()
  return out
