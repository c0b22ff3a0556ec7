#!/usr/bin/env python3
"""Kernel time of myr_exgd_grad_shoot beside myr_hvp and myr_exgd on the same handle at the same shape (myr_kernel_time, MYR_K_PROD: HIP events
around the launches).  Shapes: CARTPOLE, nsteps = 10, at 1 x 100 HEUN (the reference's default hyperparameters) and 20 x 5 RK4, B = 1 / 64 /
1 024 / 16 384.  Per shape: 2 warm-up calls, then 5 timed calls of each entry point (device arrays for the derivative and the product; myr_exgd
through its host binding -- the events bracket the launches only).  `expected_ms` = (2 nsteps + 1) hvp + exgd: a pass is myr_hvp's pair pass and
the forward phase is myr_exgd's launch sequence; `ratio` = measured / expected.  Prints one JSON line per shape.
Run: python tools/bench_shoot_exgd_grad.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from myriad_amd import _lib  # noqa: E402

NSTEPS = 10
SHAPES = [("CARTPOLE", 1, 100, "HEUN", 2.0, (1, 64, 1024, 16384)), ("CARTPOLE", 20, 5, "RK4", 2.0, (1, 64, 1024, 16384))]


def main():
  torch.cuda.init()
  rng = np.random.default_rng(0)
  dev = "cuda:0"
  for name, I, cpi, method, T, batches in SHAPES:
    eng = _lib.Engine(name, "SHOOTING", I, T, controls_per_interval=cpi, integration_method=method)
    for B in batches:
      zh = 0.3 + 0.1 * rng.standard_normal((B, eng.n))
      lamh = 0.1 * rng.standard_normal((B, eng.m))
      z, lam = torch.tensor(zh, device=dev), torch.tensor(lamh, device=dev)
      lb, ub = z - 1.0, z + 1.0
      v = torch.tensor(rng.standard_normal((B, eng.n)), device=dev)
      hz, dz = torch.empty_like(z), torch.empty_like(z)
      dl = torch.empty_like(lam)
      rows = torch.empty((B, eng.np), dtype=torch.float64, device=dev)
      out = {"system": name, "intervals": I, "cpi": cpi, "method": method, "B": B, "nsteps": NSTEPS}
      for what in ("exgd_grad_shoot", "hvp", "exgd"):
        for rep in range(7):
          if rep == 2:
            eng.kernel_time_reset()
          if what == "exgd_grad_shoot":
            eng.exgd_grad_shoot_device(B, z, lam, lb, ub, 1e-3, 1e-3, NSTEPS, v, rows, eng.np, seed_lam=lam, dz0=dz, dlam0=dl)
          elif what == "hvp":
            eng.hvp_device(B, z, lam, v, out_z=hz, out_p=rows, p_stride=eng.np)
          else:
            eng.exgd(zh, lamh, zh - 1.0, zh + 1.0, 1e-3, 1e-3, NSTEPS)
        ms, n = eng.kernel_time(_lib.K_PROD)
        out[what + "_ms"] = round(ms, 4)
        if what == "exgd_grad_shoot":
          torch.cuda.synchronize()
          out["finite"] = bool(torch.isfinite(rows).all()) and bool(torch.isfinite(dz).all()) and bool(torch.isfinite(dl).all())
      out["expected_ms"] = round((2 * NSTEPS + 1) * out["hvp_ms"] + out["exgd_ms"], 4)
      out["ratio"] = round(out["exgd_grad_shoot_ms"] / out["expected_ms"], 2)
      print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
  main()
