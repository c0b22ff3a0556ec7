#!/usr/bin/env python3
"""The Gauss-Newton product of the network fit (myr_fit_gnvp*, csrc/fit.h: node_fit_gnvp_kernel) against the gradient call it stands beside.

1. One call, at the shapes of tools/bench_fit_sets.py: NODE_CARTPOLE, HEUN, S = 100 steps, R = 16 trajectories per model, E in {1, 8, 64} models with
   weights and data of their own.  myr_fit_grad_sets (losses and per-set gradient sums) against myr_fit_gnvp_sets (per-set product sums; with and
   without `jv`; the forward tangent alone) on the same handle and the same device-resident arrays (MYR_MEM_DEVICE: no copies inside the window).  And
   the single-set pair myr_fit_grad / myr_fit_gnvp at B = 16 and 1024.  A host clock around `--calls` repetitions that end in a device synchronise;
   3 warm-up repetitions per case; `--windows` such windows, reported as the median with the smallest and the largest window.
2. One training: neural_ode/node_training.train (minibatched Adam, `--epochs` epochs) against train_gn (Levenberg-Marquardt with a truncated
   conjugate-gradient inner solve) on the same CARTPOLE dataset (utils.generate_dataset with the default hyperparameters: 100 training trajectories
   of 100 steps) from the same start (the committed weights plus 5 % noise): device calls and wall time that each needs, and those that train_gn
   needs to reach the best validation loss `train` records.

Needs a GPU: it does not fall back.    python tools/bench_fit_gnvp.py [--calls 10] [--windows 7] [--epochs 100] [--max-iter 30] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

S, T, R = 100, 2.0, 16


def windows(run, sync, calls, n):
  for _ in range(3):
    run()
  sync()
  out = []
  for _ in range(n):
    t0 = time.perf_counter()
    for _ in range(calls):
      run()
    sync()
    out.append((time.perf_counter() - t0) / calls * 1e3)
  return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


class Counting:
  """an Engine that counts its fit calls by name"""
  def __init__(self, engine):
    self._engine, self.calls = engine, {}

  def __getattr__(self, name):
    attr = getattr(self._engine, name)
    if not name.startswith("fit_"):
      return attr
    def counted(*args, **kw):
      self.calls[name] = self.calls.get(name, 0) + 1
      return attr(*args, **kw)
    return counted


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--calls", type=int, default=10)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--epochs", type=int, default=100)
  ap.add_argument("--max-iter", type=int, default=30)
  ap.add_argument("--cg-iters", type=int, default=20)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import torch
  if not torch.cuda.is_available():
    raise SystemExit("bench_fit_gnvp: no GPU")
  torch.cuda.init()
  from myriad_amd import _lib
  from myriad_amd.config import Config, HParams, OptimizerType
  from myriad_amd.neural_ode import node_training
  from myriad_amd.systems import SystemType
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping, mapping_from_flat
  from myriad_amd.utils import generate_dataset
  version = _lib.load().myr_version().decode()
  flat = flat_from_mapping(NeuralODE.load_fitted_cartpole().params)
  rng = np.random.default_rng(0)
  dev = torch.device("cuda:0")
  sync = torch.cuda.synchronize
  results = []

  def emit(r):
    r.update({"version": version})
    print(json.dumps(r), flush=True)
    results.append(r)

  roll = _lib.Engine("CARTPOLE", "SHOOTING", 1, T, controls_per_interval=S, integration_method="HEUN")      # the recorded states: the true system's
  eng = _lib.Engine("NODE_CARTPOLE", "SHOOTING", 1, T, controls_per_interval=S, integration_method="HEUN")
  npar = eng.np

  def data(B):
    us = -5.0 + 10.0 * rng.random((B, S + 1, 1))
    xs, _ = roll.rollout(0.1 * rng.standard_normal((B, 4)), us, S)
    return xs, us

  new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
  for B in (16, 1024):                                            # the single-set pair
    xs, us = data(B)
    dx, du, dp, dv = (torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (xs, us, flat, rng.standard_normal(npar)))
    dl, dg, do = new(B), new(npar), new(npar)
    rg = windows(lambda: eng.fit_grad_device(B, S, S + 1, dx, du, dg, 0, params=dp, loss=dl), sync, a.calls, a.windows)
    rp = windows(lambda: eng.fit_gnvp_device(B, S, S + 1, dx, du, dp, dv, out=do, out_stride=0), sync, a.calls, a.windows)
    assert bool(torch.isfinite(do).all())
    emit({"part": "call", "mode": "single", "S": S, "B": B, "calls": a.calls, "windows": a.windows, "fit_grad": rg, "fit_gnvp": rp,
          "fit_gnvp_over_fit_grad": rp["median_ms"] / rg["median_ms"]})
  for E in (1, 8, 64):                                            # E models at once
    xs, us = data(E * R)
    P, V = flat[None] + 0.05 * rng.standard_normal((E, npar)), rng.standard_normal((E, npar))
    dx, du, dP, dV = (torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (xs, us, P, V))
    dl, dg, do, dj = new(E, R), new(E, npar), new(E, npar), new(E, R, S + 1, 4)
    rg = windows(lambda: eng.fit_grad_sets_device(E, R, S, S + 1, dx, du, dP, grad=dg, grad_stride=0, loss=dl), sync, a.calls, a.windows)
    rp = windows(lambda: eng.fit_gnvp_sets_device(E, R, S, S + 1, dx, du, dP, dV, out=do, out_stride=0), sync, a.calls, a.windows)
    rj = windows(lambda: eng.fit_gnvp_sets_device(E, R, S, S + 1, dx, du, dP, dV, jv=dj, out=do, out_stride=0), sync, a.calls, a.windows)
    rf = windows(lambda: eng.fit_gnvp_sets_device(E, R, S, S + 1, dx, du, dP, dV, jv=dj), sync, a.calls, a.windows)
    assert bool(torch.isfinite(do).all()) and bool(torch.isfinite(dj).all())
    emit({"part": "call", "mode": "sets", "S": S, "E": E, "R": R, "calls": a.calls, "windows": a.windows, "fit_grad_sets": rg, "fit_gnvp_sets": rp,
          "fit_gnvp_sets_with_jv": rj, "fit_gnvp_sets_forward_only": rf, "fit_gnvp_sets_over_fit_grad_sets": rp["median_ms"] / rg["median_ms"]})
  roll.close()
  eng.close()

  hp = HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.SHOOTING, num_epochs=a.epochs)
  dataset = generate_dataset(hp, Config(verbose=False, plot=False))
  train_data, val_data = dataset[:hp.train_size], dataset[hp.train_size:hp.train_size + hp.val_size]
  start = mapping_from_flat(flat + 0.05 * np.random.default_rng(1).standard_normal(npar))
  Tsys = SystemType.CARTPOLE().T
  fit = node_training.NodeFitLoss(hp, Tsys)
  fit.engine = Counting(fit.engine)
  t0 = time.perf_counter()
  _, adam_last, adam_record = node_training.train(hp, Tsys, start, train_data, val_data, fit=fit)
  t_adam = time.perf_counter() - t0
  adam_calls, fit.engine.calls = dict(fit.engine.calls), {}
  target = min(r[2] for r in adam_record)

  def run_gn(max_iter):
    hp_gn = HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.SHOOTING, loss_recording_frequency=1, early_stop_check_frequency=1)
    history = []
    fit.engine.calls = {}
    t0 = time.perf_counter()
    _, last, record = node_training.train_gn(hp_gn, Tsys, start, train_data, val_data, max_iter=max_iter, cg_iters=a.cg_iters, fit=fit, history=history)
    return time.perf_counter() - t0, dict(fit.engine.calls), last, record, history

  t_gn, gn_calls, gn_last, gn_record, history = run_gn(a.max_iter)
  reached = next((r[0] for r in gn_record if r[2] <= target), None)
  to_target = None
  if reached is not None:                                         # the same run cut at the step that reaches Adam's validation loss (deterministic: the same points)
    t_cut, cut_calls, _, cut_record, _ = run_gn(reached)
    assert cut_record[-1][2] <= target
    to_target = {"outer_steps": reached, "device_calls": cut_calls, "device_calls_total": sum(cut_calls.values()), "wall_s": t_cut}
  emit({"part": "training", "train_size": hp.train_size, "val_size": hp.val_size, "S": hp.num_steps, "minibatch_size": hp.minibatch_size,
        "adam_epochs": a.epochs, "adam_last_epoch": adam_last, "adam_device_calls": adam_calls, "adam_device_calls_total": sum(adam_calls.values()),
        "adam_wall_s": t_adam, "adam_first_record": adam_record[0], "adam_best_val_loss": target, "adam_last_record": adam_record[-1],
        "gn_max_iter": a.max_iter, "gn_cg_iters": a.cg_iters, "gn_last_step": gn_last, "gn_device_calls": gn_calls,
        "gn_device_calls_total": sum(gn_calls.values()), "gn_wall_s": t_gn, "gn_record": gn_record,
        "gn_steps": [{k: s[k] for k in ("lam", "cg_products", "cg_residual", "loss", "trial_loss", "accepted")} for s in history],
        "gn_to_adams_best_val_loss": to_target})
  fit.engine.close()
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      json.dump(results, f, indent=1)


if __name__ == "__main__":
  main()
