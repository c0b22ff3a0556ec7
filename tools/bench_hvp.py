#!/usr/bin/env python3
"""Kernel time of myr_hvp beside myr_vjp (add_gradf = 1) at the same shape (myr_kernel_time, MYR_K_PROD: HIP events around the launches).
Shapes: CARTPOLE Hermite-Simpson N = 100 and shooting 20 x 5 RK4 at B = 128 / 1 024 / 4 096, ROCKETLANDING shooting 20 x 5 RK4 at B = 1 024.
Per shape: 3 warm-up calls, then 10 timed calls of each entry point on device arrays (out_z and a parameter row per instance); prints one JSON
line per shape.  Run: python tools/bench_hvp.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from myriad_amd import _lib  # noqa: E402

SHAPES = [("CARTPOLE", "HERMITE_SIMPSON", 100, 1, "HEUN", 2.0, (128, 1024, 4096)), ("CARTPOLE", "SHOOTING", 20, 5, "RK4", 2.0, (128, 1024, 4096)),
          ("ROCKETLANDING", "SHOOTING", 20, 5, "RK4", 2.0, (1024,))]


def main():
  torch.cuda.init()
  rng = np.random.default_rng(0)
  dev = "cuda:0"
  for name, tr, N, cpi, method, T, batches in SHAPES:
    eng = _lib.Engine(name, tr, N, T, controls_per_interval=cpi, integration_method=method)
    for B in batches:
      z = torch.tensor(0.3 + 0.1 * rng.standard_normal((B, eng.n)), device=dev)
      lam = torch.tensor(0.1 * rng.standard_normal((B, eng.m)), device=dev)
      v = torch.tensor(rng.standard_normal((B, eng.n)), device=dev)
      hz, g = torch.empty_like(z), torch.empty_like(z)
      hp = torch.empty((B, eng.np), dtype=torch.float64, device=dev)
      out = {"system": name, "transcription": tr, "intervals": N, "cpi": cpi, "method": method, "B": B}
      for what in ("hvp", "vjp"):
        for rep in range(13):
          if rep == 3:
            eng.kernel_time_reset()
          if what == "hvp":
            eng.hvp_device(B, z, lam, v, out_z=hz, out_p=hp, p_stride=eng.np)
          else:
            eng.products_device("vjp", B, z, lam, g, add_gradf=1)
        ms, n = eng.kernel_time(_lib.K_PROD)
        out[what + "_ms"] = round(ms, 4)
        out[what + "_launches"] = n
      out["finite"] = bool(torch.isfinite(hz).all()) and bool(torch.isfinite(hp).all())
      out["ratio"] = round(out["hvp_ms"] / out["vjp_ms"], 2)
      print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
  main()
