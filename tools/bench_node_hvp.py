#!/usr/bin/env python3
"""Kernel time of myr_hvp_node (myr_kernel_time, MYR_K_HVP_NODE / MYR_K_HVP_NODE_SHOOT: HIP events around the launches) at NODE_CARTPOLE:
Hermite-Simpson N = 100 and SHOOTING 20 x 5 under HEUN and RK4, each at B = 1 / 64 / 1 024, with and without out_p (a row per instance).
Per (shape, B, form): 3 warm-up calls, then `--calls` timed calls on device arrays; the figure is the average of the timed calls.  Beside it
myr_exgd_grad_node / myr_exgd_grad_node_shoot with nsteps = 1 on the same inputs (MYR_K_PROD): one unrolled step holds two second-order point
passes plus the first-order ones, so the product must not take longer than it.  `--only exgd --root DIR` measures that call alone with the
package and library of another tree (one without myr_hvp_node: the parent commit).  Prints one JSON line per (shape, B).  Run it twice: the two runs must agree.
Run: python tools/bench_node_hvp.py [--calls 10] [--only exgd --root DIR]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

T, BATCHES = 2.0, (1, 64, 1024)
SHAPES = (("HERMITE_SIMPSON", 100, 1, "HEUN"), ("SHOOTING", 20, 5, "HEUN"), ("SHOOTING", 20, 5, "RK4"))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--calls", type=int, default=10)
  ap.add_argument("--only", choices=("all", "exgd"), default="all")
  ap.add_argument("--root", default=HERE, help="the tree whose package and library are measured (default: this one)")
  a = ap.parse_args()
  sys.path.insert(0, os.path.abspath(a.root))
  from myriad_amd import _lib
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping
  torch.cuda.init()
  dev = "cuda:0"
  flat = flat_from_mapping(NeuralODE.load_fitted_cartpole().params)
  p = torch.tensor(flat, device=dev)
  for tr, I, cpi, method in SHAPES:
    shoot = tr == "SHOOTING"
    eng = (_lib.Engine("NODE_CARTPOLE", tr, I, T, controls_per_interval=cpi, integration_method=method) if shoot
           else _lib.Engine("NODE_CARTPOLE", tr, I, T))
    nx = 4 * ((I + 1) if shoot else (2 * I + 1))
    kid = None if a.only == "exgd" else (_lib.K_HVP_NODE_SHOOT if shoot else _lib.K_HVP_NODE)      # (a parent tree's package has neither)
    for B in BATCHES:
      rng = np.random.default_rng(B)
      z0 = np.concatenate([0.3 * rng.standard_normal((B, nx)), rng.uniform(-1.0, 1.0, (B, eng.n - nx))], axis=1)
      z = torch.tensor(z0, device=dev)
      lam = torch.tensor(0.1 * rng.standard_normal((B, eng.m)), device=dev)
      v = torch.tensor(rng.standard_normal((B, eng.n)), device=dev)
      lb, ub = torch.full_like(z, -10.0), torch.full_like(z, 10.0)
      hz = torch.empty_like(z); hp = torch.empty((B, eng.np), dtype=torch.float64, device=dev)
      out = {"transcription": tr, "intervals": I, "cpi": cpi, "method": method, "B": B, "calls": a.calls}
      if a.only == "all":
        for name, rows in (("hvp_node_z_ms", None), ("hvp_node_z_and_p_ms", hp)):
          for rep in range(3 + a.calls):
            if rep == 3:
              eng.kernel_time_reset()
            eng.hvp_node_device(B, z, lam, v, p, out_z=hz, out_p=rows, p_stride=eng.np)
          ms, n = eng.kernel_time(kid)
          assert n == a.calls
          out[name] = round(ms, 4)      # (myr_kernel_time returns the average over the calls)
          out[name.replace("_ms", "_products_per_s")] = round(B / (ms * 1e-3), 1)
        out["finite"] = bool(torch.isfinite(hz).all() and torch.isfinite(hp).all())
      call = eng.exgd_grad_node_shoot_device if shoot else eng.exgd_grad_node_device
      for rep in range(3 + a.calls):
        if rep == 3:
          eng.kernel_time_reset()
        call(B, z, lam, lb, ub, 0.01, 0.01, 1, v, hp, eng.np, p)
      ms, n = eng.kernel_time(_lib.K_PROD)
      out["exgd_grad_node_one_step_ms"] = round(ms, 4)
      print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
  main()
