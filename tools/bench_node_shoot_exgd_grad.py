#!/usr/bin/env python3
"""Kernel time of myr_exgd_grad_node_shoot (myr_kernel_time, MYR_K_PROD: HIP events around the launches) at NODE_CARTPOLE under SHOOTING,
nsteps = 5 (hp.num_unrolled's default): 1 x 100 HEUN -- the reference's default hyperparameters -- and 20 x 5 RK4, each at B = 1 / 64 / 1 024.
Per shape: 3 warm-up calls, then 10 timed calls on device arrays with a gradient row per instance; myr_exgd of the same steps beside it.
Prints one JSON line per (shape, B), with the stage-point visits of a call (second-order pair passes only: (2 nsteps + 1) I cpi stages) and the
time per visit of ONE wavefront (the visits a wavefront makes one after the other).  Run it twice: the two runs must agree.
Run: python tools/bench_node_shoot_exgd_grad.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from myriad_amd import _lib  # noqa: E402
from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping  # noqa: E402

NSTEPS, T, BATCHES = 5, 2.0, (1, 64, 1024)
SHAPES = ((1, 100, "HEUN"), (20, 5, "RK4"))
STAGES = {"EULER": 1, "HEUN": 2, "MIDPOINT": 2, "RK4": 4}


def main():
  torch.cuda.init()
  dev = "cuda:0"
  flat = flat_from_mapping(NeuralODE.load_fitted_cartpole().params)
  p = torch.tensor(flat, device=dev)
  for I, cpi, method in SHAPES:
    eng = _lib.Engine("NODE_CARTPOLE", "SHOOTING", I, T, controls_per_interval=cpi, integration_method=method)
    nx = (I + 1) * 4
    wpi = 4 if I >= 4 else (2 if I >= 2 else 1)
    for B in BATCHES:
      rng = np.random.default_rng(B)
      z0 = np.concatenate([0.3 * rng.standard_normal((B, nx)), rng.uniform(-1.0, 1.0, (B, eng.n - nx))], axis=1)
      lb0, ub0 = np.full_like(z0, -10.0), np.full_like(z0, 10.0)
      lb0[:, :4] = z0[:, :4]; ub0[:, :4] = z0[:, :4]
      z, lb, ub = (torch.tensor(a, device=dev) for a in (z0, lb0, ub0))
      lam = torch.tensor(0.1 * rng.standard_normal((B, eng.m)), device=dev)
      seed = torch.tensor(rng.standard_normal((B, eng.n)), device=dev)
      g = torch.empty((B, eng.np), dtype=torch.float64, device=dev)
      out = {"intervals": I, "cpi": cpi, "method": method, "nsteps": NSTEPS, "B": B, "wavefronts_per_instance": wpi}
      for rep in range(13):
        if rep == 3:
          eng.kernel_time_reset()
        eng.exgd_grad_node_shoot_device(B, z, lam, lb, ub, 0.01, 0.01, NSTEPS, seed, g, eng.np, p)
      ms, n = eng.kernel_time(_lib.K_PROD)
      out["exgd_grad_node_shoot_ms"] = round(ms, 4)      # (myr_kernel_time returns the average over the calls)
      out["calls"] = n
      visits = (2 * NSTEPS + 1) * I * cpi * STAGES[method]
      out["stage_visits_per_instance"] = visits
      out["us_per_visit_of_a_wavefront"] = round(1e3 * ms / (visits / min(wpi, I)), 3)
      z0h, lamh = z0.copy(), lam.cpu().numpy()
      for rep in range(6):
        if rep == 1:
          eng.kernel_time_reset()
        eng.exgd(z0h, lamh, lb0, ub0, 0.01, 0.01, NSTEPS, params=flat)
      ms, n = eng.kernel_time(_lib.K_PROD)
      out["exgd_ms"] = round(ms, 4)
      out["finite"] = bool(torch.isfinite(g).all())
      print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
  main()
