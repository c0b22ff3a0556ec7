#!/usr/bin/env python3
"""The Gauss-Newton fit (myr_fit_gn, csrc/fit_gn.h) against the first-order path it stands beside.

1. One call: myr_fit_gn (loss, gradient and Gauss-Newton matrix by forward sensitivities) against myr_fit_grad (loss and gradient by a reverse sweep)
   on the same handle -- CARTPOLE, HEUN, S = 100 steps, B = 128 / 1024 / 4096 trajectories, sums over the batch, device-resident arrays
   (MYR_MEM_DEVICE: no copies inside the window).  A host clock around `--calls` repetitions that end in a device synchronise; 3 warm-up
   repetitions per case; `--windows` such windows, reported as the median with the smallest and the largest window.
2. One fit: experiments/mle_sysid.run_mle_sysid (full-batch Adam(1e-3), `--updates` updates, the reference's recipe) against run_mle_sysid_gn
   (Levenberg-Marquardt) on the same dataset (CARTPOLE, the default hyperparameters: 100 training trajectories of 100 steps): device calls and wall
   time that Levenberg-Marquardt needs to reach the best validation loss Adam reaches.  The validation loss compared is the one both record (the
   reference's loss; Adam's discount at its epoch, Levenberg-Marquardt's at epoch 0 -- they differ by less than 1e-3 relative over 2000 epochs).

Needs a GPU: it does not fall back.    python tools/bench_fit_gn.py [--calls 20] [--windows 7] [--updates 2000] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

S, T = 100, 2.0


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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--calls", type=int, default=20)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--updates", type=int, default=2000)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import torch
  if not torch.cuda.is_available():
    raise SystemExit("bench_fit_gn: no GPU")
  torch.cuda.init()
  from myriad_amd import _lib
  from myriad_amd.config import Config, HParams, OptimizerType
  from myriad_amd.experiments import mle_sysid
  from myriad_amd.systems import SystemType
  from myriad_amd.utils import generate_dataset
  version = _lib.load().myr_version().decode()
  rng = np.random.default_rng(0)
  dev = torch.device("cuda:0")
  sync = torch.cuda.synchronize
  results = []

  def emit(r):
    r.update({"version": version})
    print(json.dumps(r), flush=True)
    results.append(r)

  eng = _lib.Engine("CARTPOLE", "SHOOTING", 1, T, controls_per_interval=S, integration_method="HEUN")
  npar = eng.np
  for B in (128, 1024, 4096):
    us = -5.0 + 10.0 * rng.random((B, S + 1, 1))
    xs, _ = eng.rollout(0.1 * rng.standard_normal((B, 4)), us, S)
    p = np.array([10.0, 1.5, 0.2, 0.6])
    dx, du, dp = (torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (xs, us, p))
    dl, dg, dn = (torch.empty(s, dtype=torch.float64, device=dev) for s in ((B,), (npar,), (npar, npar)))
    rg = windows(lambda: eng.fit_grad_device(B, S, S + 1, dx, du, dg, 0, params=dp, loss=dl), sync, a.calls, a.windows)
    grad_rev = dg.cpu().numpy().copy()
    rn = windows(lambda: eng.fit_gn_device(B, S, S + 1, dx, du, dn, 0, params=dp, loss=dl, grad=dg), sync, a.calls, a.windows)
    assert bool(torch.isfinite(dn).all())
    agree = float(np.abs(dg.cpu().numpy() - grad_rev).max() / np.abs(grad_rev).max())
    emit({"part": "call", "system": "CARTPOLE", "S": S, "B": B, "calls": a.calls, "windows": a.windows, "fit_grad": rg, "fit_gn": rn,
          "fit_gn_over_fit_grad": rn["median_ms"] / rg["median_ms"], "forward_against_reverse_grad": agree})
  eng.close()

  hp = HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.SHOOTING)
  cfg = Config(verbose=False, plot=False)
  dataset = generate_dataset(hp, cfg)
  t0 = time.perf_counter()
  adam = mle_sysid.run_mle_sysid(hp, cfg, dataset=dataset, num_updates=a.updates)
  t_adam = time.perf_counter() - t0
  target = min(adam["val_losses"])
  adam_calls = a.updates + 2 * len(adam["epochs"])
  t0 = time.perf_counter()
  lm = mle_sysid.run_mle_sysid_gn(hp, cfg, dataset=dataset)
  t_lm = time.perf_counter() - t0
  reached = next((i for i, v in enumerate(lm["val_losses"]) if v <= target), None)
  emit({"part": "fit", "system": "CARTPOLE", "train_size": hp.train_size, "S": hp.num_steps, "adam_updates": a.updates, "adam_device_calls": adam_calls,
        "adam_wall_s": t_adam, "adam_best_val_loss": target, "adam_params": adam["params"],
        "lm_iterations": lm["iterations"], "lm_device_calls": 1 + lm["iterations"] + len(lm["epochs"]), "lm_wall_s": t_lm,
        "lm_val_losses": lm["val_losses"], "lm_epochs": lm["epochs"], "lm_params": lm["last_params"],
        "lm_iteration_that_reaches_adams_val_loss": None if reached is None else lm["epochs"][reached],
        "lm_device_calls_to_adams_val_loss": None if reached is None else 1 + lm["epochs"][reached] + reached + 1,
        "lm_parameter_std": [float(v) for v in np.sqrt(np.diag(lm["covariance"]))]})
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      json.dump(results, f, indent=1)


if __name__ == "__main__":
  main()
