"""End-to-end system identification: /root/reference/myriad/experiments/e2e_sysid.py:29-297.

The reference fits the model parameters so that PLANNING WITH THE MODEL reproduces the true optimal controls: it advances a primal-dual
guess by NUM_UNROLLED extragradient steps under the current parameters, then differentiates NUM_UNROLLED further steps from the advanced
point in the parameters (`many_steps_grad`, forward mode, :148-177), contracts with the gradient of the imitation loss taken AT THAT SAME
advanced point (`lookahead_update`, :209-218) and lets optax.adam(hp.adam_lr) move the parameters.  Here the steps are one device call
(myr_exgd) and the contracted derivative another (myr_exgd_grad: one reverse sweep, csrc/exgd_grad.h; under SHOOTING myr_exgd_grad_shoot,
csrc/shoot_exgd_grad.h); the loss, its gradient and Adam run in numpy on the host.  Two deviations from the reference's loop: nothing is
pickled -- what it writes to disk every `save_and_reset_time` epochs is
returned instead, and a run never resumes from saved parameters (:233-241) --; and at a reset (:257-262) the reference splits hp.key and rebuilds the
optimizer, which the reference's collocation optimisers answer with the same deterministic guess (no key enters hermite_simpson.py:37-48 /
trapezoidal.py:34-50; nor the shooting guess: shooting.py:47 has its noise commented out): the driver reuses the guess it started from.

EXTENSION: `start_states [B][ns]` runs B instances at once, each with its own true optimum (one batched solve) and its own guess; the loss is
the mean over the batch and its gradient the batch sum of myr_exgd_grad (grad_stride 0) divided by B.

The reference's default hyperparameters select SHOOTING (intervals = 1, controls_per_interval = 100, HEUN).  That route is opt-in:
`run_endtoend(..., shooting=True)` with a SHOOTING optimizer runs the same loop on myr_exgd_grad_shoot.  Without it myr_exgd_grad is asked, which
refuses SHOOTING (NotImplementedError with its message) before anything is solved; the driver does not switch transcription on its own.

EXTENSION: `run_endtoend_gn` fits the same keys by Levenberg-Marquardt on the imitation loss.  Its Jacobian is what many_steps_grad carries forward
before lookahead_update contracts it -- d x_n / d p itself, one myr_exgd_jac call (csrc/exgd_jac.h) per trial point, which also returns x_n --, and the
driver is mle_sysid's LevenbergMarquardt.  Collocation transcriptions, closed-form systems; `run_endtoend` is unchanged."""
from __future__ import annotations

from typing import Optional

import numpy as np

from myriad_amd.config import Config, HParams
from myriad_amd.defaults import param_guesses
from myriad_amd.experiments.mle_sysid import Adam, split_params
from myriad_amd.systems import SystemType
from myriad_amd.trajectory_optimizers import get_optimizer

NUM_UNROLLED = 10                                                                                          # e2e_sysid.py:21
DISCOUNTED = (SystemType.BACTERIA, SystemType.MOUNTAINCAR, SystemType.CARTPOLE, SystemType.PENDULUM)       # :203


def imitation_weights(hp, rows: int, nu: int, epoch) -> np.ndarray:
  """w [rows] with simple_imitation_loss = sum_t w[t] sum_c (u[t][c] - u_true[t][c])^2 (:195-207): mean over the controls, the discount
  (1 - 1 / (1 + exp(2 + 1e-6 epoch)))^t for BACTERIA, MOUNTAINCAR, CARTPOLE and PENDULUM (1 otherwise), mean over time."""
  discount = (1.0 - 1.0 / (1.0 + np.exp(2.0 + 0.000001 * epoch))) ** np.arange(rows) if hp.system in DISCOUNTED else np.ones(rows)
  return discount / (rows * nu)


def simple_imitation_loss(optimizer, xs_and_us, true_opt_us, epoch):
  """(loss, d loss / d xs_and_us) for one instance [n] or a batch [B][n] (the mean over the batch, and the gradient OF THAT MEAN'S TERM of each
  instance times B: the rows are the per-instance gradients)."""
  _, us = optimizer.unravel(np.asarray(xs_and_us, dtype=np.float64))
  diff = us - true_opt_us
  w = imitation_weights(optimizer.hp, us.shape[-2], us.shape[-1], epoch)
  loss = (w[:, None] * diff * diff).sum(axis=(-2, -1))
  grad = np.zeros(np.shape(xs_and_us))
  grad[..., grad.shape[-1] - us.shape[-2] * us.shape[-1]:] = (2.0 * w[:, None] * diff).reshape(diff.shape[:-2] + (-1,))
  return float(np.mean(loss)), grad


def lookahead_gradient(optimizer, params, xs_and_us, lmbdas, true_opt_us, epoch, lb, ub, eta_x, eta_v) -> dict:
  """dJ/dp of lookahead_update (:209-218) in the keys of `params`: NUM_UNROLLED steps differentiated from (xs_and_us, lmbdas), contracted with
  the loss gradient taken at that same point; for a batch the gradient of the mean loss (the batch sum of myr_exgd_grad divided by B).  A SHOOTING
  optimizer goes through myr_exgd_grad_shoot."""
  system = optimizer.system
  p, sign = split_params(system, params)
  _, dJ_dx = simple_imitation_loss(optimizer, xs_and_us, true_opt_us, epoch)
  B = 1 if np.ndim(xs_and_us) == 1 else np.shape(xs_and_us)[0]
  call = optimizer.engine.exgd_grad_shoot if optimizer.transcription == "SHOOTING" else optimizer.engine.exgd_grad
  g = call(xs_and_us, lmbdas, lb, ub, eta_x, eta_v, NUM_UNROLLED, dJ_dx, params=p, reduce=True, want_start=False)["grad"]
  g = g * sign / B
  return {k: float(g[system.param_names.index(k)]) for k in params}


def imitation_normal_equations(keys, names, u_n, jz, true_opt_us, weights):
  """(loss, gradient mapping, Gauss-Newton matrix [K,K], J^T J [K,K]) of the imitation loss sum_b r_b . r_b with r = sqrt(w) o (u_n - u_true), in
  the LevenbergMarquardt convention (loss(p + d) ~ loss + grad . d + d . gn d / 2: grad = 2 J^T r, gn = 2 J^T J), summed over the batch.
  u_n [B][rows nu]: the control part of the iterate; jz [B][np][n]: its Jacobian rows (myr_exgd_jac), of which the control part of the rows of
  `keys` (`names`: the device order) is J^T; weights [rows]."""
  B, width = u_n.shape
  sw = np.sqrt(np.repeat(np.asarray(weights, dtype=np.float64), width // len(weights)))
  r = sw * (u_n - np.reshape(true_opt_us, (B, width)))
  Jt = jz[:, [names.index(k) for k in keys], jz.shape[2] - width:] * sw      # [B][K][rows nu]
  jtr = np.einsum("bki,bi->k", Jt, r)
  jtj = np.einsum("bki,bli->kl", Jt, Jt)
  return float((r * r).sum()), {k: 2.0 * float(v) for k, v in zip(keys, jtr)}, 2.0 * jtj, jtj


def fit_imitation_gn(evaluate, guess, max_iter=50, rtol=1e-12):
  """Levenberg-Marquardt (mle_sysid.LevenbergMarquardt, the driver of run_mle_sysid_gn) on `evaluate(params) -> (loss, grad mapping, gn, jtj)`
  from the mapping `guess`: one evaluation per trial point.  Returns {"params", "losses" (at the start and after every accepted step),
  "device_calls", "iterations", "jtj" (J^T J at the last accepted point, in the order of the keys), "first" (the evaluation at the start)}."""
  from myriad_amd.experiments.mle_sysid import LevenbergMarquardt
  lm = LevenbergMarquardt(guess, rtol=rtol, max_iter=max_iter)
  calls, jtj = 1, None
  first = evaluate(lm.params)
  lm.begin(*first[:3])
  jtj, losses = first[3], [lm.loss]
  while not lm.done:
    ev = evaluate(lm.trial())
    calls += 1
    if lm.end(*ev[:3]):
      jtj = ev[3]
      losses.append(lm.loss)
  return {"params": dict(lm.params), "losses": losses, "device_calls": calls, "iterations": lm.iterations, "jtj": jtj, "first": first}


def run_endtoend_gn(hp: HParams, cfg: Config, nsteps: int = NUM_UNROLLED, max_iter: int = 50, start_states=None, rtol: float = 1e-12,
                    true_opt_us=None, guess=None) -> Optional[dict]:
  """The end-to-end fit by Levenberg-Marquardt instead of Adam: the keys of param_guesses[hp.system] (or of `guess`, the starting mapping) so that
  `nsteps` extragradient steps from the optimizer's guess with lmbda = 0 reproduce the true optimal controls.  Residual
  r(p) = sqrt(w) o (u_n(p) - u_true) with w = imitation_weights at epoch 0; its Jacobian is the control part of d z_n / d p, which the reference's
  many_steps_grad carries forward (:148-177) and ONE myr_exgd_jac call per trial point gives together with u_n.  start_states [B][ns]: a batch of
  instances, their normal equations summed.  true_opt_us: the controls to imitate ([rows][nu], [B][rows][nu] for a batch; default: the true
  system's optimum, one solve).  Returns fit_imitation_gn's dictionary plus "true_opt_us"; None for a system without parameter guesses.
  run_endtoend (Adam on the reverse-mode gradient, the reference's loop) is unchanged."""
  if hp.system not in param_guesses and guess is None:
    print("We do not currently support that kind of system for sysid. Exiting...")
    return None
  true_system = hp.system()
  optimizer = get_optimizer(hp, cfg, true_system)
  optimizer.engine.exgd_jac_probe()                        # the library's own refusal, before the true optimum is solved for
  if start_states is not None:
    x0s = np.asarray(start_states, dtype=np.float64)
    if true_opt_us is None:
      true_opt_us = optimizer.solve_batch(x0s=x0s)['u']
    z0, lb, ub = optimizer.batch_inputs(x0s, true_system.device_params())
  else:
    if true_opt_us is None:
      true_opt_us = optimizer.solve()['u']
    z0, lb, ub = optimizer.guess[None], optimizer.bounds[None, :, 0], optimizer.bounds[None, :, 1]
  z0 = np.array(z0, dtype=np.float64)
  true_opt_us = np.asarray(true_opt_us, dtype=np.float64)
  lam0 = np.zeros((z0.shape[0], optimizer.engine.m))
  eta_x, eta_v = optimizer.step_sizes()
  start = dict(param_guesses[hp.system] if guess is None else guess)
  rows, nu = true_opt_us.shape[-2:]
  weights = imitation_weights(hp, rows, nu, 0)

  def evaluate(params):
    out = optimizer.unrolled_jacobian(z0, lam0, params, nsteps, eta_x, eta_v, lb, ub, want=("zn", "jz"))
    return imitation_normal_equations(list(start), true_system.param_names, out["zn"][:, z0.shape[1] - rows * nu:], out["jz"], true_opt_us, weights)

  res = fit_imitation_gn(evaluate, start, max_iter=max_iter, rtol=rtol)
  if cfg.verbose:
    print("losses", res["losses"])
    print("params", res["params"])
  res["true_opt_us"] = true_opt_us
  return res


def run_endtoend(hp: HParams, cfg: Config, num_epochs: int = 10_000, start_states=None, save_and_reset_time: int = 1_000,
                 shooting: bool = False) -> Optional[dict]:
  """e2e_sysid.py:29-297.  shooting=True admits a SHOOTING optimizer (myr_exgd_grad_shoot).  Returns {"params", "saved_params" {epoch: params}, "ts",
  "imitation_losses", "primal_guesses", "dual_guesses",
  "true_opt_us"}; None for a system without parameter guesses (:30-32)."""
  if hp.system not in param_guesses:
    print("We do not currently support that kind of system for sysid. Exiting...")
    return None
  true_system = hp.system()
  optimizer = get_optimizer(hp, cfg, true_system)
  if shooting and optimizer.transcription == "SHOOTING":   # the library's own refusal (SHOOTING without the opt-in, ...), before the true optimum is solved for
    optimizer.engine.exgd_grad_shoot_probe()
  else:
    optimizer.engine.exgd_grad_probe()
  batched = start_states is not None
  if batched:
    x0s = np.asarray(start_states, dtype=np.float64)
    B = x0s.shape[0]
    true_opt_us = optimizer.solve_batch(x0s=x0s)['u']      # [B][u_rows][nu]: every instance's own true optimum
    guess, lb, ub = optimizer.batch_inputs(x0s, true_system.device_params())
  else:
    B = 1
    true_opt_us = optimizer.solve()['u']
    guess, lb, ub = optimizer.guess, optimizer.bounds[:, 0], optimizer.bounds[:, 1]
  params = dict(param_guesses[hp.system])                  # :87
  xs_and_us = np.array(guess, dtype=np.float64)            # :93-98
  original_lmbdas = np.zeros(xs_and_us.shape[:-1] + (optimizer.engine.m,))
  lmbdas = original_lmbdas.copy()
  opt = Adam(hp.adam_lr)                                   # :101
  eta_x, eta_v = optimizer.step_sizes()                    # :104-109
  ts, primal_guesses, dual_guesses, imitation_losses, saved = [], [], [], [], {}
  record_things_time = 10
  for epoch in range(num_epochs):
    if epoch % save_and_reset_time == 0:                   # :232-262: keep the parameters, reset the guess
      record_things_time = 1
      saved[epoch] = dict(params)
      xs_and_us, lmbdas = np.array(guess, dtype=np.float64), original_lmbdas.copy()
    if epoch % record_things_time == 0:                    # :264-279
      if epoch >= 10:
        record_things_time = 50
      ts.append(epoch); primal_guesses.append(xs_and_us.copy()); dual_guesses.append(lmbdas.copy())
      cur_loss, _ = simple_imitation_loss(optimizer, xs_and_us, true_opt_us, epoch)
      imitation_losses.append(cur_loss)
      if cfg.verbose:
        print("loss", cur_loss)
        print("params", params)
    p, _ = split_params(true_system, params)
    z, lam = optimizer.engine.exgd(xs_and_us, lmbdas, lb, ub, eta_x, eta_v, NUM_UNROLLED, params=p)      # :282-283
    xs_and_us, lmbdas = (z, lam) if batched else (z[0], lam[0])
    params = opt.update(params, lookahead_gradient(optimizer, params, xs_and_us, lmbdas, true_opt_us, epoch, lb, ub, eta_x, eta_v))      # :286
  saved[num_epochs] = dict(params)
  out = {"params": params, "saved_params": saved, "ts": ts, "imitation_losses": imitation_losses, "primal_guesses": primal_guesses,
         "dual_guesses": dual_guesses, "true_opt_us": true_opt_us}
  if cfg.plot:
    try:
      import matplotlib
      matplotlib.use("Agg")
      import matplotlib.pyplot as plt
      from pathlib import Path
      plot_path = f'plots/{hp.system.name}/e2e_sysid/'
      Path(plot_path).mkdir(parents=True, exist_ok=True)
      plt.figure(figsize=(4, 3.3))
      plt.plot(ts, imitation_losses)
      plt.xlabel("epoch"); plt.ylabel("imitation loss"); plt.yscale("log"); plt.tight_layout()
      plt.savefig(plot_path + "imitation_loss.png"); plt.close()
    except Exception as e:  # plotting is presentation only
      print("plot skipped:", e)
  return out
