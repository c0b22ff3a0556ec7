"""System identification of the network system by trajectory matching: the reference's myriad/experiments/node_mle_sysid.py:21-201, and
`study_noise` for 'node_mle_sysid' (study_scripts.py:26-64).

The reference generates a dataset on the true system, trains the (64, 64) MLP on it (neural_ode/node_training.py), plans with the learned
network (`solve_with_params`) and rolls the planned controls out on the true system; its noise study repeats that once per noise level, one
training after the other.  Here the trainings of a study are ONE ensemble (node_training.train_ensemble: every minibatch step of all networks is
one myr_fit_grad_sets call) and the plans ONE batched solve (`solve_batch(params=[E, np])`).

Nothing is pickled, plotted or written to disk: what the reference saves is returned.  A run never resumes from saved weights.  Out of scope: the
dataset augmentation between experiments (`node.augment_datasets`, :71-74 -- hp.num_experiments > 1 trains on the one dataset again from the weights
it reached, each time as a fresh `train` run; every run's record is returned) and `study_vector_field`.  `params=None` draws the initial weights of node_e2e_sysid.initial_node(hp.seed).

The device code has one architecture: NodeSystem over CARTPOLE with hidden layers (64, 64).  Any other hp.system or hp.hidden_layers raises
NotImplementedError."""
from __future__ import annotations

import copy

import numpy as np

from myriad_amd.config import Config, HParams
from myriad_amd.experiments.node_e2e_sysid import initial_node
from myriad_amd.neural_ode.node_training import train, train_ensemble
from myriad_amd.systems import SystemType
from myriad_amd.systems.neural_ode import NeuralODE, NodeSystem, flat_from_mapping
from myriad_amd.trajectory_optimizers import get_optimizer
from myriad_amd.utils import generate_dataset, get_defect, get_state_trajectory_and_cost

NOISE_LEVELS = (0.0, 0.001, 0.01, 0.1, 0.2, 0.5, 1., 2., 5.)      # study_scripts.py:28


def _check_architecture(hp: HParams) -> None:
  if hp.system != SystemType.CARTPOLE or tuple(hp.hidden_layers) != (64, 64):
    raise NotImplementedError(f"node_mle_sysid: the device code is built for NodeSystem over CARTPOLE with hidden_layers (64, 64) only; "
                              f"got system {hp.system.name}, hidden_layers {tuple(hp.hidden_layers)}")


def _split(hp: HParams, data):
  """(train rows, validation rows) of a dataset [..., train + val + test, S+1, ns+nu]"""
  return data[..., :hp.train_size, :, :], data[..., hp.train_size:hp.train_size + hp.val_size, :, :]


def _true_plan(hp: HParams, cfg: Config, true_system):
  """controls planned with the true model, and their state trajectory and cost on the true system (:25-26, :105)"""
  us = get_optimizer(hp, cfg, true_system).solve()['u']
  xs, cost = get_state_trajectory_and_cost(hp, true_system, true_system.x_0, us)
  return us, xs, cost


def run_node_mle_sysid(hp: HParams, cfg: Config, params=None) -> dict:
  """node_mle_sysid.py:21-151: generate a dataset, train the network on it (early stopping on the validation rows), plan with the learned network,
  roll the planned controls out on the true system.  hp.num_experiments trainings follow one another on the ONE dataset (no augmentation between
  them): each is a `train` run of its own -- the minibatch order of default_rng(hp.seed) and a fresh Adam state, as a run of the reference that
  reloads saved weights -- from the best weights of the one before; with num_experiments == 0 nothing is trained and the initial weights plan.
  Returns {"params" (the weights planned with, Haiku mapping), "last_epoch", "record" [(epoch, train loss, validation loss)] (the last training's;
  None without one), "last_epochs", "records" (every training's), "true_cost", "learned_cost", "true_defect", "learned_defect", "u", "learned_u"}."""
  _check_architecture(hp)
  true_system = hp.system()
  node = NeuralODE(initial_node(hp.seed).params if params is None else params, (64, 64))
  train_data, val_data = _split(hp, generate_dataset(hp, cfg))
  last_epochs, records = [], []
  for _ in range(hp.num_experiments):
    best, last_epoch, record = train(hp, true_system.T, node.params, train_data, val_data, verbose=cfg.verbose)
    last_epochs.append(last_epoch); records.append(record)
    if best is not None:
      node.params = best
  true_us, true_x, true_c = _true_plan(hp, cfg, true_system)
  learned_us = get_optimizer(hp, cfg, NodeSystem(node, true_system)).solve_with_params(node.params)['u']      # :103
  learned_x, learned_c = get_state_trajectory_and_cost(hp, true_system, true_system.x_0, learned_us)            # :115
  return {"params": node.params, "last_epoch": last_epochs[-1] if last_epochs else None, "record": records[-1] if records else None,
          "last_epochs": last_epochs, "records": records, "true_cost": true_c, "learned_cost": learned_c,
          "true_defect": get_defect(true_system, true_x), "learned_defect": get_defect(true_system, learned_x), "u": true_us, "learned_u": learned_us}


def run_node_noise_study(hp: HParams, cfg: Config, noise_levels=NOISE_LEVELS, params=None) -> dict:
  """study_noise(hp, cfg, 'node_mle_sysid'): one dataset per noise level, ALL networks trained in one train_ensemble (from the same initial
  weights, as the reference's fresh NeuralODE per level), planned with in one solve_batch, their controls rolled out on the true system.
  Returns {"noise_levels", "costs" [E], "defects" (E arrays, or None where the system has no terminal state), "optimal_cost", "records",
  "params" (E Haiku mappings: the best weights), "last_epochs", "us" [E][rows][nu]}."""
  _check_architecture(hp)
  true_system = hp.system()
  init = initial_node(hp.seed).params if params is None else params
  datasets = []
  for level in noise_levels:
    hp_level = copy.copy(hp)
    hp_level.noise_level = level
    datasets.append(generate_dataset(hp_level, cfg))
  train_data, val_data = _split(hp, np.stack(datasets))
  E = len(datasets)
  runs = train_ensemble(hp, true_system.T, [init] * E, train_data, val_data, rngs=[np.random.default_rng(hp.seed) for _ in range(E)], verbose=cfg.verbose)
  best = [init if b is None else b for b, _, _ in runs]
  node_optimizer = get_optimizer(hp, cfg, NodeSystem(NeuralODE(init, (64, 64)), true_system))
  us = node_optimizer.solve_batch(params=np.stack([flat_from_mapping(b) for b in best]))['u']
  xs, costs = get_state_trajectory_and_cost(hp, true_system, np.tile(true_system.x_0, (E, 1)), us)
  defects = [get_defect(true_system, x) for x in xs]
  _, _, optimal_cost = _true_plan(hp, cfg, true_system)            # study_scripts.py:76-79
  return {"noise_levels": list(noise_levels), "costs": np.asarray(costs), "defects": None if true_system.x_T is None else defects,
          "optimal_cost": optimal_cost, "records": [r for _, _, r in runs], "params": best, "last_epochs": [ep for _, ep, _ in runs], "us": us}
