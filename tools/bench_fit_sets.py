#!/usr/bin/env python3
"""Many independent network trainings' worth of trajectory-matching gradients: E sequential myr_fit_grad calls against one myr_fit_grad_sets call.

Workload: NODE_CARTPOLE, HEUN, S = 100 steps, R = 16 trajectories per model (the reference's minibatch, config.py:84), E in {1, 8, 64} models with
weights of their own on data of their own.  Two modes, on device-resident arrays (MYR_MEM_DEVICE: no copies inside the window):
  (a) "sequential": E calls fit_grad(reduce) one after the other -- the existing entry point only, so this mode runs on any earlier checkout
      (`--tree DIR` imports the package of another checkout, with the library built there);
  (b) "sets": one fit_grad_sets call (skipped where the package has none).
And `fit_grad` itself at B = 16 and B = 1024, the same S, and the closed-form lane kernel (CARTPOLE, B = 128, 4 096, 65 536, one parameter vector and a
row per trajectory), for the comparison of one checkout with another.

Timing: a host clock around `--calls` repetitions that end in a device synchronise; 3 warm-up repetitions per shape and mode; `--windows` such
windows per case, reported as the median with the smallest and the largest window (the run-to-run spread inside one process).  With --digest
the script also prints a SHA-256 of the outputs of the fit_grad cases, to compare the bits of two checkouts.  Needs a GPU: it does not fall back.

  python tools/bench_fit_sets.py [--calls 20] [--windows 7] [--tree DIR] [--out FILE.json]
"""
import argparse
import hashlib
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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--calls", type=int, default=20)
  ap.add_argument("--windows", type=int, default=7)
  ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  ap.add_argument("--label", default="")
  ap.add_argument("--digest", action="store_true")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  sys.path.insert(0, os.path.abspath(a.tree))
  import torch
  if not torch.cuda.is_available():
    raise SystemExit("bench_fit_sets: no GPU")
  torch.cuda.init()
  from myriad_amd import _lib
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping
  version = _lib.load().myr_version().decode()
  flat = flat_from_mapping(NeuralODE.load_fitted_cartpole().params)
  rng = np.random.default_rng(0)
  dev = torch.device("cuda:0")
  sync = torch.cuda.synchronize
  roll = _lib.Engine("CARTPOLE", "SHOOTING", 1, T, controls_per_interval=S, integration_method="HEUN")      # the recorded states: the true system's
  eng = _lib.Engine("NODE_CARTPOLE", "SHOOTING", 1, T, controls_per_interval=S, integration_method="HEUN")
  npar = eng.np
  results = []

  def data(B):
    us = -5.0 + 10.0 * rng.random((B, S + 1, 1))
    xs, _ = roll.rollout(0.1 * rng.standard_normal((B, 4)), us, S)
    return xs, us

  def emit(r):
    r.update({"label": a.label, "version": version, "S": S, "calls": a.calls, "windows": a.windows})
    print(json.dumps(r), flush=True)
    results.append(r)

  digest = hashlib.sha256()
  for B in (16, 1024):                                            # fit_grad itself
    xs, us = data(B)
    dx, du, dp = (torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (xs, us, flat))
    dl, dg = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(npar, dtype=torch.float64, device=dev)
    r = windows(lambda: eng.fit_grad_device(B, S, S + 1, dx, du, dg, 0, params=dp, loss=dl), sync, a.calls, a.windows)
    assert bool(torch.isfinite(dg).all())
    digest.update(dl.cpu().numpy().tobytes() + dg.cpu().numpy().tobytes())
    emit({"mode": "fit_grad", "B": B, **r})
  # the closed-form systems' lane kernel through the same entry point (CARTPOLE; one parameter vector, and a row per trajectory)
  lane = _lib.Engine("CARTPOLE", "SHOOTING", 1, T, controls_per_interval=S, integration_method="HEUN")
  for B in (128, 4096, 65536):
    xs, us = data(B)
    rows = np.array([10.0, 1.5, 0.2, 0.6])[None] * (1.0 + 0.05 * (2.0 * rng.random((B, 4)) - 1.0))
    dx, du, dp, dr = (torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (xs, us, rows[0], rows))
    dl, dg = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(lane.np, dtype=torch.float64, device=dev)
    for what, prm, stride in (("shared", dp, 0), ("per_trajectory", dr, lane.np)):
      r = windows(lambda: lane.fit_grad_device(B, S, S + 1, dx, du, dg, 0, params=prm, params_stride=stride, loss=dl), sync, a.calls, a.windows)
      assert bool(torch.isfinite(dg).all())
      digest.update(dl.cpu().numpy().tobytes() + dg.cpu().numpy().tobytes())
      emit({"mode": "fit_grad_lane", "system": "CARTPOLE", "params": what, "B": B, **r})
  lane.close()
  if a.digest:
    print(json.dumps({"label": a.label, "version": version, "fit_grad_outputs_sha256": digest.hexdigest()}), flush=True)
  for E in (1, 8, 64):
    xs, us = data(E * R)
    P = flat[None] + 0.05 * rng.standard_normal((E, npar))
    dx, du, dP = (torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (xs, us, P))
    dl = torch.empty((E, R), dtype=torch.float64, device=dev)
    dg = torch.empty((E, npar), dtype=torch.float64, device=dev)

    def sequential():
      for e in range(E):
        eng.fit_grad_device(R, S, S + 1, dx[e * R:(e + 1) * R], du[e * R:(e + 1) * R], dg[e], 0, params=dP[e], loss=dl[e])

    ra = windows(sequential, sync, a.calls, a.windows)
    seq_bits = dl.cpu().numpy().tobytes() + dg.cpu().numpy().tobytes()
    emit({"mode": "sequential", "E": E, "R": R, **ra})
    if hasattr(eng, "fit_grad_sets_device"):
      dl.zero_(); dg.zero_()
      rb = windows(lambda: eng.fit_grad_sets_device(E, R, S, S + 1, dx, du, dP, grad=dg, grad_stride=0, loss=dl), sync, a.calls, a.windows)
      assert dl.cpu().numpy().tobytes() + dg.cpu().numpy().tobytes() == seq_bits, "sets and sequential calls differ"
      emit({"mode": "sets", "E": E, "R": R, **rb, "sequential_over_sets": ra["median_ms"] / rb["median_ms"]})
  eng.close(); roll.close()
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      json.dump(results, f, indent=1)


if __name__ == "__main__":
  main()
