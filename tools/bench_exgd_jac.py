#!/usr/bin/env python3
"""The forward-mode Jacobian of the unrolled extragradient steps (myr_exgd_jac, csrc/exgd_jac.h) against the calls it stands beside.

CARTPOLE, Hermite-Simpson, N = 100, a parameter row per instance, device-resident arrays (MYR_MEM_DEVICE: no copies inside the window):
1. nsteps = 10, B = 1 / 128 / 1024: myr_exgd_jac (all four columns of jz and jlam, and the iterate) against myr_exgd_grad (one seeded row by a reverse
   sweep) and myr_exgd (the steps alone; it works in place, so every repetition advances the same buffers -- the time does not depend on the values).
2. nsteps = 1000, the same batches: myr_exgd_jac in one launch against myr_exgd_grad, whose history (nsteps (2 n + m) + n doubles per instance: 22.5 MB)
   passes its 1 GiB bound from B = 48 on and runs in chunks of instances.
A host clock around `--calls` repetitions that end in a device synchronise; 3 warm-up repetitions per case; `--windows` such windows, reported as
the median with the smallest and the largest window.

Needs a GPU: it does not fall back.    python tools/bench_exgd_jac.py [--calls 10] [--windows 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

N, T = 100, 5.0


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
  ap.add_argument("--calls", type=int, default=10)
  ap.add_argument("--windows", type=int, default=5)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  import torch
  if not torch.cuda.is_available():
    raise SystemExit("bench_exgd_jac: no GPU")
  torch.cuda.init()
  from myriad_amd import _lib
  version = _lib.load().myr_version().decode()
  dev = torch.device("cuda:0")
  sync = torch.cuda.synchronize
  results = []
  eng = _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", N, T)
  n, m, npar = eng.n, eng.m, eng.np
  K = 2 * N + 1
  for nsteps, calls in ((10, a.calls), (1000, max(1, a.calls // 5))):
    for B in (1, 128, 1024):
      rng = np.random.default_rng(B + nsteps)
      z = np.concatenate([0.2 * rng.standard_normal((B, K * 4)), rng.uniform(-1.0, 1.0, (B, K))], axis=1)
      box = rng.random((B, n)) < 0.3
      lb, ub = np.where(box, z - 1e-3, -np.inf), np.where(box, z + 1e-3, np.inf)
      lb[:, :4] = z[:, :4]; ub[:, :4] = z[:, :4]
      p = np.array([9.8, 1.0, 0.1, 0.5]) * (1.0 + 0.05 * (2.0 * rng.random((B, npar)) - 1.0))
      eta = 0.02 if nsteps == 10 else 0.002
      t = {k: torch.as_tensor(np.ascontiguousarray(v), device=dev) for k, v in
           dict(z=z, lam=0.1 * rng.standard_normal((B, m)), lb=lb, ub=ub, p=p, seed=rng.standard_normal((B, n))).items()}
      o = {k: torch.empty(s, dtype=torch.float64, device=dev) for k, s in
           dict(zn=(B, n), lamn=(B, m), jz=(B, npar, n), jlam=(B, npar, m), grad=(B, npar)).items()}
      rj = windows(lambda: eng.exgd_jac_device(B, t["z"], t["lam"], t["lb"], t["ub"], eta, eta, nsteps, params=t["p"], params_stride=npar, zn=o["zn"],
                                               lamn=o["lamn"], jz=o["jz"], jlam=o["jlam"]), sync, calls, a.windows)
      assert bool(torch.isfinite(o["jz"]).all())
      rg = windows(lambda: eng.exgd_grad_device(B, t["z"], t["lam"], t["lb"], t["ub"], eta, eta, nsteps, t["seed"], o["grad"], npar, params=t["p"],
                                                params_stride=npar), sync, calls, a.windows)
      agree = float((torch.einsum("bi,bki->bk", t["seed"], o["jz"]) - o["grad"]).abs().max() / o["grad"].abs().max())
      zw, lw = t["z"].clone(), t["lam"].clone()
      rs = windows(lambda: _lib._chk(eng.lib.myr_exgd(eng._h, B, zw.data_ptr(), lw.data_ptr(), t["lb"].data_ptr(), t["ub"].data_ptr(), t["p"].data_ptr(),
                                                      npar, eta, eta, nsteps, _lib.MEM_DEVICE), "myr_exgd"), sync, calls, a.windows)
      r = {"system": "CARTPOLE", "scheme": "HERMITE_SIMPSON", "N": N, "nsteps": nsteps, "B": B, "calls": calls, "windows": a.windows, "exgd_jac": rj,
           "exgd_grad": rg, "exgd": rs, "exgd_jac_over_exgd_grad": rj["median_ms"] / rg["median_ms"], "exgd_jac_over_exgd": rj["median_ms"] / rs["median_ms"],
           "seeded_jac_against_exgd_grad": agree, "version": version}
      print(json.dumps(r), flush=True)
      results.append(r)
  eng.close()
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      json.dump(results, f, indent=1)


if __name__ == "__main__":
  main()
