#!/usr/bin/env python3
"""Kernel time of myr_exgd_grad_node (myr_kernel_time, MYR_K_PROD: HIP events around the launches) at NODE_CARTPOLE, Hermite-Simpson, N = 100,
nsteps = 5 (hp.num_unrolled's default), B = 1 / 64 / 1 024, for every number of wavefronts per instance the library builds
(MYRIAD_NODE_EXGD_WPI = 1, 2, 4; the handle reads it at creation).  Per shape: 3 warm-up calls, then 10 timed calls on device arrays with a
gradient row per instance; myr_exgd of the same steps beside it.  Prints one JSON line per (WPI, B).  Run: python tools/bench_node_exgd_grad.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from myriad_amd import _lib  # noqa: E402
from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping  # noqa: E402

N, NSTEPS, T, BATCHES, WPIS = 100, 5, 2.0, (1, 64, 1024), (1, 2, 4)


def main():
  torch.cuda.init()
  dev = "cuda:0"
  flat = flat_from_mapping(NeuralODE.load_fitted_cartpole().params)
  p = torch.tensor(flat, device=dev)
  for wpi in WPIS:
    os.environ["MYRIAD_NODE_EXGD_WPI"] = str(wpi)
    eng = _lib.Engine("NODE_CARTPOLE", "HERMITE_SIMPSON", N, T)
    for B in BATCHES:
      rng = np.random.default_rng(B)
      z0 = np.concatenate([0.3 * rng.standard_normal((B, (2 * N + 1) * 4)), rng.uniform(-1.0, 1.0, (B, 2 * N + 1))], axis=1)
      lb0, ub0 = np.full_like(z0, -10.0), np.full_like(z0, 10.0)
      lb0[:, :4] = z0[:, :4]; ub0[:, :4] = z0[:, :4]
      z, lb, ub = (torch.tensor(a, device=dev) for a in (z0, lb0, ub0))
      lam = torch.tensor(0.1 * rng.standard_normal((B, eng.m)), device=dev)
      seed = torch.tensor(rng.standard_normal((B, eng.n)), device=dev)
      g = torch.empty((B, eng.np), dtype=torch.float64, device=dev)
      out = {"wpi": wpi, "intervals": N, "nsteps": NSTEPS, "B": B}
      for rep in range(13):
        if rep == 3:
          eng.kernel_time_reset()
        eng.exgd_grad_node_device(B, z, lam, lb, ub, 0.01, 0.01, NSTEPS, seed, g, eng.np, p)
      ms, n = eng.kernel_time(_lib.K_PROD)
      out["exgd_grad_node_ms"] = round(ms, 4)      # (myr_kernel_time returns the average over the calls)
      out["calls"] = n
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
