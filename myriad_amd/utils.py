"""Host mirror of the hot-path helpers of /root/reference/myriad/utils.py.
The numerics run on the GPU through the C-ABI (myr_rollout); only array plumbing and random draws happen here."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from myriad_amd import _lib


def _engine_for(hp, system, device=0):
  from myriad_amd.config import OptimizerType, QuadratureRule
  if hp.optimizer == OptimizerType.COLLOCATION:
    tr = "HERMITE_SIMPSON" if hp.quadrature_rule == QuadratureRule.HERMITE_SIMPSON else "TRAPEZOIDAL"
  else:
    tr = "SHOOTING"
  return _lib.Engine(system.name, tr, hp.intervals, system.T, controls_per_interval=hp.controls_per_interval,
                     integration_method=hp.integration_method.name, device=device)


def get_state_trajectory_and_cost(hp, system, start_state, us, params=None, engine=None) -> Tuple[np.ndarray, float]:
  """utils.py:258-298: integrate [x; cost] of the TRUE dynamics under `us` with hp.integration_method over
  hp.intervals*hp.controls_per_interval steps.  Batched when start_state is [B,ns] / us is [B,rows,nu]."""
  if getattr(system, "discrete", False):
    # DEVIATION: the reference integrates the next-state map of a discrete system as if it were an ODE right-hand side
    # (utils.py:262-298 has no discrete branch), which has no meaning; here the recurrence x_{i+1} = dynamics(x_i, u_i)
    # is applied over the rows of `us` and the running cost summed (host loop: int(T) steps).
    x = np.asarray(start_state, dtype=np.float64)
    xs, c = [x], 0.0
    for u_t in np.asarray(us, dtype=np.float64):
      c += system.cost(x, u_t)
      x = system.dynamics(x, u_t)
      xs.append(x)
    return np.stack(xs), float(c)
  eng = engine or _engine_for(hp, system)
  num_steps = hp.intervals * hp.controls_per_interval
  x0 = np.asarray(start_state, dtype=np.float64)
  us = np.asarray(us, dtype=np.float64)
  single = x0.ndim == 1
  if us.ndim == 1:
    us = us[:, None]
  p = system.device_params() if params is None else params
  xs, cost = eng.rollout(x0, us, num_steps, params=p)
  if engine is None:
    eng.close()
  return (xs[0], float(cost[0])) if single else (xs, cost)


def get_defect(system, learned_xs) -> Optional[np.ndarray]:
  """utils.py:313-324."""
  if system.x_T is None:
    return None
  last = np.asarray(learned_xs)[-1]
  return np.array([last[i] - system.x_T[i] for i in range(len(system.x_T)) if system.x_T[i] is not None])


def integrate_time_independent(dynamics, x_0, interval_us, h, N, integration_method):
  """utils.py:80-131 on the host, for the handful of coarse steps the reference's initial guesses take
  (shooting.py:56-74, trapezoidal.py:36-50).  `interval_us` indexing clamps like jnp (quirk Q6)."""
  name = integration_method if isinstance(integration_method, str) else integration_method.name
  x = np.asarray(x_0, dtype=np.float64)
  us = np.asarray(interval_us, dtype=np.float64)
  g = lambda i: us[min(i, len(us) - 1)]
  out = [x]
  for i in range(N):
    if name == "EULER":
      x = x + h * dynamics(x, g(i))
    elif name == "HEUN":
      k1 = dynamics(x, g(i)); k2 = dynamics(x + h * k1, g(i + 1)); x = x + h / 2 * (k1 + k2)
    elif name == "MIDPOINT":
      x_mid = x + h * dynamics(x, g(i)); x = x + h * dynamics(x_mid, (g(i) + g(i + 1)) / 2)
    elif name == "RK4":
      u1, u2, u3 = g(2 * i), g(2 * i + 1), g(2 * i + 2)
      k1 = dynamics(x, u1); k2 = dynamics(x + h * k1 / 2, u2); k3 = dynamics(x + h * k2 / 2, u2); k4 = dynamics(x + h * k3, u3)
      x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    else:
      raise KeyError(name)
    out.append(x)
  return x, np.stack(out)


def smooth(curve, its: int) -> np.ndarray:
  """utils.py:300-309: `its` passes of a five-tap Gaussian blur along the time axis of [B, rows, dim], edges repeated."""
  curve = np.array(curve, dtype=np.float64)
  kernel = np.array([0.15286624, 0.22292994, 0.24840764, 0.22292994, 0.15286624])
  for _ in range(its):
    padded = np.pad(curve, ((0, 0), (2, 2), (0, 0)), mode="edge")
    curve = sum(kernel[k] * padded[:, k:k + curve.shape[1], :] for k in range(5))
  return curve


def generate_dataset(hp, cfg, given_us=None, engine=None) -> np.ndarray:
  """utils.py:327-444: train_size + val_size + test_size control sequences (RANDOM_WALK, UNIFORM, or noise around `given_us`), start
  states around x_0, the TRUE system's states under them by hp.integration_method (one myr_rollout call for the whole set), observation
  noise, clipping to the state bounds.  Returns [total, num_steps+1, ns+nu]: states, then controls.  Every draw comes from one numpy
  Generator seeded by hp.seed (the reference mixes jax keys and numpy's global state); a system with an infinite state or control
  bound raises, as there."""
  from myriad_amd.config import SamplingApproach
  system = hp.system()
  rng = np.random.default_rng(hp.seed)
  total_size = hp.train_size + hp.val_size + hp.test_size
  ns, nu, S = hp.state_size, hp.control_size, hp.num_steps
  u_lower, u_upper = system.bounds[ns:, 0], system.bounds[ns:, 1]
  x_lower, x_upper = system.bounds[:ns, 0], system.bounds[:ns, 1]
  if np.isinf(u_lower).any() or np.isinf(u_upper).any():
    raise Exception("infinite control bounds, aborting")
  if np.isinf(x_lower).any() or np.isinf(x_upper).any():
    raise Exception("infinite state bounds, aborting")
  spread = (u_upper - u_lower) * hp.sample_spread
  if hp.sampling_approach == SamplingApproach.RANDOM_WALK:
    all_us = np.empty((total_size, S + 1, nu))
    all_us[:, 0] = rng.uniform(u_lower, u_upper, (total_size, nu))
    for i in range(S):
      all_us[:, i + 1] = np.clip(all_us[:, i] + rng.normal(0.0, spread, (total_size, nu)), u_lower, u_upper)
  elif hp.sampling_approach == SamplingApproach.UNIFORM or given_us is None and hp.sampling_approach in (
      SamplingApproach.TRUE_OPTIMAL, SamplingApproach.CURRENT_OPTIMAL):
    all_us = rng.uniform(u_lower, u_upper, (total_size, S + 1, nu)) * 0.75      # (the factor is the reference's)
  elif hp.sampling_approach in (SamplingApproach.TRUE_OPTIMAL, SamplingApproach.CURRENT_OPTIMAL):
    noise = rng.standard_normal((total_size, S + 1, nu)) * spread
    all_us = np.clip(np.asarray(given_us, dtype=np.float64).reshape(1, S + 1, nu) + noise, u_lower, u_upper)
  else:
    raise Exception("Unknown sampling approach, please choose among", [m.name for m in SamplingApproach])
  if hp.to_smooth:
    all_us = smooth(all_us, 2)
  start_states = np.tile(system.x_0, (total_size, 1))
  if hp.start_spread > 0.:
    start_states = np.clip(start_states + rng.standard_normal(start_states.shape) * hp.start_spread, x_lower, x_upper)
  eng = engine or _lib.Engine(system.name, "SHOOTING", 1, system.T, controls_per_interval=S, integration_method=hp.integration_method.name)
  all_xs, _ = eng.rollout(start_states, all_us, S, params=system.device_params())
  if engine is None:
    eng.close()
  all_xs = all_xs + rng.standard_normal(all_xs.shape) * (x_upper - x_lower) * hp.noise_level
  all_xs = np.clip(all_xs, x_lower, x_upper)
  xs_and_us = np.concatenate((all_xs, all_us), axis=2)
  if cfg.verbose:
    print("generated", xs_and_us.shape, "between control bounds", u_lower, u_upper)
  assert np.isfinite(xs_and_us).all()
  return xs_and_us


def yield_minibatches(hp, total_size: int, dataset, rng=None):
  """utils.py:447-455: the first `total_size` rows of a fresh permutation of the dataset, hp.minibatch_size at a time (the last one shorter)."""
  assert total_size <= dataset.shape[0]
  tmp_dataset = (rng or np.random).permutation(dataset)
  num_minibatches = total_size // hp.minibatch_size + (1 if total_size % hp.minibatch_size > 0 else 0)
  for i in range(num_minibatches):
    n = min((i + 1) * hp.minibatch_size, total_size) - i * hp.minibatch_size
    yield tmp_dataset[i * hp.minibatch_size: i * hp.minibatch_size + n]
