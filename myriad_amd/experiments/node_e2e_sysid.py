"""End-to-end system identification of the network system: the reference's myriad/experiments/node_e2e_sysid.py:24-291.

The reference trains the weights of the (64, 64) MLP so that PLANNING THROUGH THE NETWORK reproduces the true optimal controls: a primal-dual
guess advances by hp.num_unrolled extragradient steps under the current weights (:276-277), then hp.num_unrolled further steps are
differentiated in the weights from the advanced point (`many_steps_grad`, :139-166), contracted with the gradient of the imitation loss taken at
that same point (`lookahead_update`, :187-196), and optax.adam(1e-4) -- hard-coded, :94 -- moves the weights.  Here the steps are one device call
(myr_exgd) and the contracted derivative another (myr_exgd_grad_node: one reverse sweep, csrc/node_exgd_grad.h; under SHOOTING
myr_exgd_grad_node_shoot, csrc/node_shoot_exgd_grad.h); loss and Adam run in numpy.

`run_node_endtoend_sets` trains E networks at once -- seeds, noise levels, learning rates --: an epoch of all of them is one myr_exgd call with a
weight row per instance and one myr_exgd_grad_node_sets call (E R workgroups in one launch where E runs launch E times one), with
node_training.AdamSets; entry e of its result is run_node_endtoend on network e alone, to the bit.

`run_node_endtoend(..., shooting=True)` with a SHOOTING optimizer -- the reference's default hyperparameters -- runs the same loop on
myr_exgd_grad_node_shoot.  Without it myr_exgd_grad_node is asked, which refuses every transcription but Hermite-Simpson before anything is solved.

As e2e_sysid.run_endtoend: nothing is pickled or plotted in the loop -- what the reference writes to disk is returned --, a run never resumes
from saved weights, and the guess a reset rebuilds (:231-234) is the deterministic one the run started from.  The imitation loss carries NO
discount (the reference's list at :181 is empty): weights 1 / (rows nu).  Recording: every epoch for the first ten after a reset, then every 10
(:211, :236-239).  `node=None` draws seeded initial weights in the shape Haiku's Linear uses (truncated normal of std 1 / sqrt(fan_in) cut at two
standard deviations, zero biases) from numpy's generator seeded with hp.seed; the reference's own draw comes from jax's generator and cannot be
reproduced.  EXTENSION: `start_states [B][ns]` runs B instances at once, as in e2e_sysid."""
from __future__ import annotations

from typing import Optional

import numpy as np

from myriad_amd.config import Config, HParams
from myriad_amd.defaults import param_guesses
from myriad_amd.experiments.mle_sysid import Adam
from myriad_amd.systems.neural_ode import NeuralODE, NodeSystem, flat_from_mapping, mapping_from_flat
from myriad_amd.trajectory_optimizers import get_optimizer

ADAM_LR = 1e-4                                                    # node_e2e_sysid.py:94


def initial_node(seed: int, sizes=(5, 64, 64, 4)) -> NeuralODE:
  """hk.Linear's default initialisers: w ~ truncated normal (|t| <= 2) of std 1 / sqrt(fan_in), b = 0"""
  rng = np.random.default_rng(seed)
  params = {}
  for k, a, b in zip(("linear", "linear_1", "linear_2"), sizes[:-1], sizes[1:]):
    w = rng.standard_normal((a, b))
    while (np.abs(w) > 2.0).any():                                # redraw the entries outside the cut
      bad = np.abs(w) > 2.0
      w[bad] = rng.standard_normal(int(bad.sum()))
    params[k] = {"w": w / np.sqrt(a), "b": np.zeros(b)}
  return NeuralODE(params, sizes[1:-1])


def imitation_weights(rows: int, nu: int) -> np.ndarray:
  """w [rows] with the loss = sum_t w[t] sum_c (u[t][c] - u_true[t][c])^2 (:174-185): the plain mean over controls and time"""
  return np.ones(rows) / (rows * nu)


def simple_imitation_loss(optimizer, xs_and_us, true_opt_us):
  """(loss, d loss / d xs_and_us) for one instance [n] or a batch [B][n] (the mean over the batch; the rows are the per-instance gradients)"""
  _, us = optimizer.unravel(np.asarray(xs_and_us, dtype=np.float64))
  diff = us - true_opt_us
  w = imitation_weights(us.shape[-2], us.shape[-1])
  loss = (w[:, None] * diff * diff).sum(axis=(-2, -1))
  grad = np.zeros(np.shape(xs_and_us))
  grad[..., grad.shape[-1] - us.shape[-2] * us.shape[-1]:] = (2.0 * w[:, None] * diff).reshape(diff.shape[:-2] + (-1,))
  return float(np.mean(loss)), grad


def lookahead_gradient(optimizer, true_optimizer, flat, xs_and_us, lmbdas, true_opt_us, lb, ub, eta_x, eta_v, nsteps) -> np.ndarray:
  """dJ/dweights of lookahead_update (:187-196) as the flat row: `nsteps` steps differentiated from (xs_and_us, lmbdas), contracted with the loss
  gradient taken at that same point; for a batch the gradient of the mean loss.  A SHOOTING optimizer goes through myr_exgd_grad_node_shoot."""
  _, dJ_dx = simple_imitation_loss(true_optimizer, xs_and_us, true_opt_us)
  B = 1 if np.ndim(xs_and_us) == 1 else np.shape(xs_and_us)[0]
  call = optimizer.engine.exgd_grad_node_shoot if optimizer.transcription == "SHOOTING" else optimizer.engine.exgd_grad_node
  g = call(xs_and_us, lmbdas, lb, ub, eta_x, eta_v, nsteps, dJ_dx, flat, reduce=True, want_start=False)["grad"]
  return g / B


def run_node_endtoend(hp: HParams, cfg: Config, num_epochs: int = 10_000, node: Optional[NeuralODE] = None, start_states=None,
                      save_and_reset_time: int = 1_000, shooting: bool = False) -> Optional[dict]:
  """node_e2e_sysid.py:24-291.  shooting=True admits a SHOOTING optimizer (myr_exgd_grad_node_shoot).  Returns {"params" (Haiku mapping), "saved_params" {epoch: mapping}, "ts", "imitation_losses", "primal_guesses",
  "dual_guesses", "true_opt_us"}; None for a system without parameter guesses (:25-27)."""
  if hp.system not in param_guesses:
    print("We do not currently support that kind of system for sysid. Exiting...")
    return None
  if node is None:
    node = initial_node(hp.seed)
  true_system = hp.system()
  true_optimizer = get_optimizer(hp, cfg, true_system)           # :49
  node_optimizer = get_optimizer(hp, cfg, NodeSystem(node=node, true_system=true_system))      # :50-51
  if shooting and node_optimizer.transcription == "SHOOTING":      # the library's own refusals, before the true optimum is solved for
    node_optimizer.engine.exgd_grad_node_shoot_probe()
  elif node_optimizer.transcription != "HERMITE_SIMPSON":      # (without the opt-in the weight gradient is asked of myr_exgd_grad_node: Hermite-Simpson only)
    node_optimizer.engine.exgd_grad_node_probe()
  batched = start_states is not None
  if batched:
    x0s = np.asarray(start_states, dtype=np.float64)
    B = x0s.shape[0]
    true_opt_us = true_optimizer.solve_batch(x0s=x0s)['u']
    guess, lb, ub = true_optimizer.batch_inputs(x0s, true_system.device_params())
  else:
    B = 1
    true_opt_us = true_optimizer.solve()['u']                    # :63-64
    guess, lb, ub = true_optimizer.guess, true_optimizer.bounds[:, 0], true_optimizer.bounds[:, 1]      # :82, :104
  flat = flat_from_mapping(node.params)
  xs_and_us = np.array(guess, dtype=np.float64)
  original_lmbdas = np.zeros(xs_and_us.shape[:-1] + (node_optimizer.engine.m,))      # :83
  lmbdas = original_lmbdas.copy()
  opt = Adam(ADAM_LR)
  eta_x, eta_v = true_optimizer.step_sizes()                     # :98-102
  ts, primal_guesses, dual_guesses, imitation_losses, saved = [], [], [], [], {}
  record_things_time = 10
  for epoch in range(num_epochs):
    if epoch % save_and_reset_time == 0:                         # :214-234: keep the weights, reset the guess
      record_things_time = 1
      saved[epoch] = mapping_from_flat(flat)
      xs_and_us, lmbdas = np.array(guess, dtype=np.float64), original_lmbdas.copy()
    if epoch % record_things_time == 0:                          # :236-273
      if epoch >= 10:
        record_things_time = 10
      ts.append(epoch); primal_guesses.append(xs_and_us.copy()); dual_guesses.append(lmbdas.copy())
      cur_loss, _ = simple_imitation_loss(true_optimizer, xs_and_us, true_opt_us)
      imitation_losses.append(cur_loss)
      if cfg.verbose:
        print(epoch, "loss", cur_loss)
    z, lam = node_optimizer.engine.exgd(xs_and_us, lmbdas, lb, ub, eta_x, eta_v, hp.num_unrolled, params=flat)      # :276-277
    xs_and_us, lmbdas = (z, lam) if batched else (z[0], lam[0])
    g = lookahead_gradient(node_optimizer, true_optimizer, flat, xs_and_us, lmbdas, true_opt_us, lb, ub, eta_x, eta_v, hp.num_unrolled)
    flat = opt.update({"weights": flat}, {"weights": g})["weights"]      # :280
  node.params = mapping_from_flat(flat)
  saved[num_epochs] = mapping_from_flat(flat)
  return {"params": node.params, "saved_params": saved, "ts": ts, "imitation_losses": imitation_losses, "primal_guesses": primal_guesses,
          "dual_guesses": dual_guesses, "true_opt_us": true_opt_us}


def advance_sets(engine, Z, L, lb, ub, eta_x, eta_v, nsteps, P):
  """`nsteps` extragradient steps of all E R iterates Z [E,R,n], L [E,R,m], set e under the weights P[e] of P [E,np]: ONE myr_exgd call with each
  set's row repeated R times (params_stride == np).  Under SHOOTING that stride takes the one-instance-per-pass route of
  csrc/node_shoot_products.h where a single run's shared-weights call takes the batched one; both give the same bits
  (tests/test_gpu_node_sets.py: the driver under SHOOTING).  Returns the new (Z, L)."""
  E, R = Z.shape[:2]
  wide = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), Z.shape)).reshape(E * R, -1)
  z, lam = engine.exgd(Z.reshape(E * R, -1), L.reshape(E * R, -1), wide(lb), wide(ub), eta_x, eta_v, nsteps, params=np.repeat(P, R, axis=0))
  return z.reshape(Z.shape), lam.reshape(L.shape)


def run_node_endtoend_sets(hp: HParams, cfg: Config, nodes, num_epochs: int = 10_000, start_states=None, save_and_reset_time: int = 1_000,
                           shooting: bool = False, lrs=None) -> Optional[list]:
  """run_node_endtoend for E networks at once (`nodes`: E NeuralODE of the (64, 64) architecture -- different seeds, noise levels, learning
  rates): every epoch is ONE advance of all E R iterates (myr_exgd with a weight row per instance) and ONE myr_exgd_grad_node_sets call with the
  per-set sums, where E separate runs launch E workgroups one after the other; Adam is node_training.AdamSets, a row per network, with the
  learning rate lrs[e] (default ADAM_LR for all).  R = the number of start states (1 without them); the true optimum, the guess and the bounds
  are the same for every network.  Returns a list of E dicts with run_node_endtoend's keys; entry e equals run_node_endtoend on nodes[e] alone
  (with ADAM_LR = lrs[e]), to the bit.  None for a system without parameter guesses."""
  from myriad_amd.neural_ode.node_training import AdamSets
  if hp.system not in param_guesses:
    print("We do not currently support that kind of system for sysid. Exiting...")
    return None
  nodes = list(nodes)
  E = len(nodes)
  if E == 0:
    return []
  true_system = hp.system()
  true_optimizer = get_optimizer(hp, cfg, true_system)
  node_optimizer = get_optimizer(hp, cfg, NodeSystem(node=nodes[0], true_system=true_system))      # one handle serves every set: the weights go in per call
  engine = node_optimizer.engine
  is_shoot = node_optimizer.transcription == "SHOOTING"
  if is_shoot and not shooting:      # (as run_node_endtoend: without the opt-in the single-set Hermite-Simpson call is asked, which refuses)
    engine.exgd_grad_node_probe()
  engine.exgd_grad_node_sets_probe()      # the library's own refusals, before the true optimum is solved for
  batched = start_states is not None
  if batched:
    x0s = np.asarray(start_states, dtype=np.float64)
    B = x0s.shape[0]
    true_opt_us = true_optimizer.solve_batch(x0s=x0s)['u']
    guess, lb, ub = true_optimizer.batch_inputs(x0s, true_system.device_params())
  else:
    B = 1
    true_opt_us = true_optimizer.solve()['u']
    guess, lb, ub = true_optimizer.guess, true_optimizer.bounds[:, 0], true_optimizer.bounds[:, 1]
  guess = np.array(guess, dtype=np.float64).reshape(B, -1)
  own = (lambda a: a) if batched else (lambda a: a[0])           # a set's iterate in the shape run_node_endtoend keeps it: [B][n], or [n]
  P = np.stack([flat_from_mapping(node.params) for node in nodes])
  Z0 = np.ascontiguousarray(np.broadcast_to(guess, (E,) + guess.shape))
  L0 = np.zeros((E, B, engine.m))
  Z, L = Z0.copy(), L0.copy()
  opt = AdamSets(P.shape, ADAM_LR if lrs is None else np.asarray(lrs, dtype=np.float64))
  every = list(range(E))
  eta_x, eta_v = true_optimizer.step_sizes()
  runs = [{"ts": [], "primal_guesses": [], "dual_guesses": [], "imitation_losses": [], "saved_params": {}} for _ in range(E)]
  record_things_time = 10
  for epoch in range(num_epochs):
    if epoch % save_and_reset_time == 0:
      record_things_time = 1
      for e in every:
        runs[e]["saved_params"][epoch] = mapping_from_flat(P[e])
      Z, L = Z0.copy(), L0.copy()
    if epoch % record_things_time == 0:
      if epoch >= 10:
        record_things_time = 10
      for e in every:
        r = runs[e]
        r["ts"].append(epoch); r["primal_guesses"].append(own(Z[e]).copy()); r["dual_guesses"].append(own(L[e]).copy())
        cur_loss, _ = simple_imitation_loss(true_optimizer, own(Z[e]), true_opt_us)
        r["imitation_losses"].append(cur_loss)
        if cfg.verbose:
          print(e, epoch, "loss", cur_loss)
    Z, L = advance_sets(engine, Z, L, lb, ub, eta_x, eta_v, hp.num_unrolled, P)
    dJ = np.stack([simple_imitation_loss(true_optimizer, own(Z[e]), true_opt_us)[1].reshape(B, -1) for e in every])
    g = engine.exgd_grad_node_sets(Z, L, lb, ub, eta_x, eta_v, hp.num_unrolled, dJ, P, reduce=True, want_start=False)["grad"] / B
    P = opt.update(every, P, g)
  out = []
  for e, node in enumerate(nodes):
    node.params = mapping_from_flat(P[e])
    runs[e]["saved_params"][num_epochs] = mapping_from_flat(P[e])
    out.append({"params": node.params, "saved_params": runs[e]["saved_params"], "ts": runs[e]["ts"], "imitation_losses": runs[e]["imitation_losses"],
                "primal_guesses": runs[e]["primal_guesses"], "dual_guesses": runs[e]["dual_guesses"], "true_opt_us": true_opt_us})
  return out
