#!/usr/bin/env python3
"""Kernel time of myr_exgd_grad beside myr_exgd (myr_kernel_time, MYR_K_PROD) at CARTPOLE, Hermite-Simpson, N = 100, nsteps = 10.
Per batch size: 3 warm-up calls, then 10 timed calls of each entry point on device arrays; prints one JSON line per batch size.
Run: python tools/bench_exgd_grad.py [B ...]   (default 1 128 4096)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from myriad_amd import _lib  # noqa: E402


def main():
  N, nsteps, T = 100, 10, 2.0
  eng = _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", N, T)
  rng = np.random.default_rng(0)
  for B in [int(a) for a in sys.argv[1:]] or [1, 128, 4096]:
    dev = "cuda:0"
    z = torch.tensor(0.1 * rng.standard_normal((B, eng.n)), device=dev)
    lam = torch.tensor(0.1 * rng.standard_normal((B, eng.m)), device=dev)
    lb, ub = torch.full_like(z, -2.0), torch.full_like(z, 2.0)
    seed = torch.tensor(rng.standard_normal((B, eng.n)), device=dev)
    grad = torch.empty((B, eng.np), dtype=torch.float64, device=dev)
    out = {"B": B, "N": N, "nsteps": nsteps}
    for what in ("exgd_grad", "exgd"):
      for rep in range(13):
        if rep == 3:
          eng.kernel_time_reset()
        if what == "exgd":
          zz, ll = z.clone(), lam.clone()
          _lib._chk(eng.lib.myr_exgd(eng._h, B, zz.data_ptr(), ll.data_ptr(), lb.data_ptr(), ub.data_ptr(), None, 0, 0.01, 1e-4, nsteps, _lib.MEM_DEVICE), "myr_exgd")
        else:
          eng.exgd_grad_device(B, z, lam, lb, ub, 0.01, 1e-4, nsteps, seed, grad, eng.np)
      ms, n = eng.kernel_time(_lib.K_PROD)
      out[what + "_ms"] = round(ms, 4)
      out[what + "_launches"] = n
    out["ratio"] = round(out["exgd_grad_ms"] / out["exgd_ms"], 2)
    print(json.dumps(out), flush=True)
  eng.close()


if __name__ == "__main__":
  main()
