#!/usr/bin/env python3
"""Device time of myr_fit_grad (csrc/fit.h): the lane kernel on CARTPOLE and the one-wavefront-per-trajectory kernel on the network
system, Heun, S = 100.  One GPU process; per case a warm-up of 3 calls, then `--launches` timed calls on device-resident arrays
(MYR_MEM_DEVICE: no copies inside the window), time from the handle's HIP events (myr_kernel_time, slot MYR_K_FIT: lane / wavefront
kernel plus the reduction).  Reports ms per call and trajectories x steps per second, and -- for information, on the host -- the
oracle's autograd time for B = 128.  Needs a GPU: it does not fall back.

  python tools/fit_probe.py [--launches 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def case(system, B, S, rng):
  from oracle import myriad_oracle as O
  sysm = O.CartPole()
  lo, hi = sysm.bounds[4:, 0], sysm.bounds[4:, 1]
  us = lo + (0.25 + 0.5 * rng.random((B, S + 1, 1))) * (hi - lo)
  x0 = 0.1 * rng.standard_normal((B, 4))
  return x0, us


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--launches", type=int, default=20)
  ap.add_argument("--out", default=None)
  ap.add_argument("--no-oracle", action="store_true")
  a = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    raise SystemExit("fit_probe: no GPU")
  torch.cuda.init()
  from myriad_amd import _lib
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping
  S, T = 100, 2.0
  rng = np.random.default_rng(0)
  flat = flat_from_mapping(NeuralODE.load_fitted_cartpole().params)
  dev = torch.device("cuda:0")
  results = []
  roll = _lib.Engine("CARTPOLE", "SHOOTING", 1, T, controls_per_interval=S, integration_method="HEUN")      # the recorded states: the true system's
  for system, batches in (("CARTPOLE", (128, 4096, 65536)), ("NODE_CARTPOLE", (128, 1024))):
    eng = _lib.Engine(system, "SHOOTING", 1, T, controls_per_interval=S, integration_method="HEUN")
    params = flat if system == "NODE_CARTPOLE" else np.array([10.0, 1.5, 0.2, 0.6])
    for B in batches:
      x0, us = case(system, B, S, rng)
      xs, _ = roll.rollout(x0, us, S)
      dx, du, dp = (torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (xs, us, params))
      dl = torch.empty(B, dtype=torch.float64, device=dev)
      dg = torch.empty(eng.np, dtype=torch.float64, device=dev)
      torch.cuda.synchronize()
      for _ in range(3):
        eng.fit_grad_device(B, S, S + 1, dx, du, dg, 0, params=dp, loss=dl)
      eng.kernel_time_reset()
      t0 = time.perf_counter()
      for _ in range(a.launches):
        eng.fit_grad_device(B, S, S + 1, dx, du, dg, 0, params=dp, loss=dl)
      wall = (time.perf_counter() - t0) / a.launches * 1e3
      ms, n = eng.kernel_time(_lib.K_FIT)
      assert n == a.launches and bool(torch.isfinite(dg).all())
      r = {"system": system, "B": B, "S": S, "method": "HEUN", "launches": n, "kernel_ms": ms, "wall_ms": wall,
           "traj_steps_per_s": B * S / (ms * 1e-3)}
      print(json.dumps(r), flush=True)
      results.append(r)
    eng.close()
  if not a.no_oracle:      # information: the oracle's autograd on the host, B = 128, closed-form CARTPOLE
    from oracle import myriad_oracle as O
    x0, us = case("CARTPOLE", 128, S, rng)
    pt = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (10.0, 1.5, 0.2, 0.6)]
    sysm = O.CartPole(*pt)
    xo = torch.zeros(S + 1, 128, 4, dtype=torch.float64)
    t0 = time.perf_counter()
    _, xh = O.integrate_time_independent(sysm.dynamics, torch.tensor(x0), torch.tensor(us).transpose(0, 1), T / S, S, "HEUN")
    torch.autograd.grad(((xh - xo) ** 2).sum(), pt)
    r = {"system": "CARTPOLE", "B": 128, "S": S, "oracle_autograd_host_ms": (time.perf_counter() - t0) * 1e3}
    print(json.dumps(r), flush=True)
    results.append(r)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      json.dump(results, f, indent=1)


if __name__ == "__main__":
  main()
