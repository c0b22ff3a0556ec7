#!/usr/bin/env python3
"""End-to-end identification of many networks: E sequential single-set calls against one weight-set call, for the three kernels' own workloads.

Workloads, NODE_CARTPOLE, T = 2, one instance per network (R = 1: the reference's node_e2e_sysid.py loop has one start state), E in {1, 8, 64}
networks with weights of their own (the committed set plus 5 % noise), on device-resident arrays (MYR_MEM_DEVICE: no copies inside the window):
  "exgd_grad_hs"     myr_exgd_grad_node, Hermite-Simpson N = 100, nsteps = 5 (hp.num_unrolled's default), the per-set sum (grad_stride 0)
  "exgd_grad_shoot"  myr_exgd_grad_node_shoot, SHOOTING 20 x 5 HEUN, the same
  "hvp"              myr_hvp_node, Hermite-Simpson N = 100, out_z and the per-set sum of out_p
Two modes:
  (a) "sequential": E single-set calls one after the other -- the existing entry points only, so this mode runs on any earlier checkout
      (`--tree DIR` imports the package of another checkout, with the library built there);
  (b) "sets": one myr_exgd_grad_node_sets / myr_hvp_node_sets call (skipped where the package has none).  The tool checks that (b) has the
      bytes of (a).
And the single-set entry points themselves at B = 1 and B = 64, for the comparison of one checkout with another; with --digest a SHA-256 over
their outputs, which must be equal for two checkouts that compute the same.

Timing: a host clock around `--calls` repetitions that end in a device synchronise; 3 warm-up repetitions per shape and mode; `--windows` such
windows per case, reported as the median with the smallest and the largest window.  Needs a GPU: it does not fall back.

  python tools/bench_node_sets.py [--calls 20] [--windows 7] [--digest] [--single-only] [--tree DIR] [--label NAME] [--out FILE.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

T, NSTEPS, ETA = 2.0, 5, 0.01
WORKLOADS = (("exgd_grad_hs", "HERMITE_SIMPSON", 100, 1, "HEUN"), ("exgd_grad_shoot", "SHOOTING", 20, 5, "HEUN"), ("hvp", "HERMITE_SIMPSON", 100, 1, "HEUN"))


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
  ap.add_argument("--single-only", action="store_true", help="the single-set entry points only: the comparison of two checkouts")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  sys.path.insert(0, os.path.abspath(a.tree))
  import torch
  if not torch.cuda.is_available():
    raise SystemExit("bench_node_sets: no GPU")
  torch.cuda.init()
  from myriad_amd import _lib
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping
  version = _lib.load().myr_version().decode()
  flat = flat_from_mapping(NeuralODE.load_fitted_cartpole().params)
  dev = torch.device("cuda:0")
  sync = torch.cuda.synchronize
  results = []
  digest = hashlib.sha256()

  def emit(r):
    r.update({"label": a.label, "version": version, "calls": a.calls, "windows": a.windows})
    print(json.dumps(r), flush=True)
    results.append(r)

  def instances(eng, B, seed):
    rng = np.random.default_rng(seed)
    nx = eng.x_rows * eng.ns
    z = np.concatenate([0.3 * rng.standard_normal((B, nx)), rng.uniform(-1.0, 1.0, (B, eng.n - nx))], axis=1)
    lb, ub = np.full_like(z, -10.0), np.full_like(z, 10.0)
    lb[:, :4] = z[:, :4]; ub[:, :4] = z[:, :4]
    host = dict(z=z, lb=lb, ub=ub, lam=0.1 * rng.standard_normal((B, eng.m)), seed=rng.standard_normal((B, eng.n)), v=rng.standard_normal((B, eng.n)))
    return {k: torch.as_tensor(np.ascontiguousarray(x), device=dev) for k, x in host.items()}

  for name, tr, I, cpi, method in WORKLOADS:
    eng = _lib.Engine("NODE_CARTPOLE", tr, I, T, controls_per_interval=cpi, integration_method=method)
    npar = eng.np
    hvp = name == "hvp"
    single = eng.hvp_node_device if hvp else (eng.exgd_grad_node_shoot_device if tr == "SHOOTING" else eng.exgd_grad_node_device)

    def one(B, d, p, g, oz):
      """the single-set call on the B instances of d (slices of device tensors), weights p [np], the sum into g [np]"""
      if hvp:
        single(B, d["z"], d["lam"], d["v"], p, out_z=oz, out_p=g, p_stride=0)
      else:
        single(B, d["z"], d["lam"], d["lb"], d["ub"], ETA, ETA, NSTEPS, d["seed"], g, 0, p)

    # the single-set entry points themselves: one checkout against another
    dp = torch.as_tensor(flat, device=dev)
    for B in (1, 64):
      d = instances(eng, B, 10 + B)
      g, oz = torch.empty(npar, dtype=torch.float64, device=dev), torch.empty((B, eng.n), dtype=torch.float64, device=dev)
      r = windows(lambda: one(B, d, dp, g, oz), sync, a.calls, a.windows)
      assert bool(torch.isfinite(g).all())
      digest.update(g.cpu().numpy().tobytes() + (oz.cpu().numpy().tobytes() if hvp else b""))
      emit({"workload": name, "mode": "single_set", "B": B, **r})
    # E networks: sequential single-set calls against one sets call
    for E in (() if a.single_only else (1, 8, 64)):
      d = instances(eng, E, 100 + E)
      P = torch.as_tensor(flat[None] * (1.0 + 0.05 * np.random.default_rng(E).standard_normal((E, npar))), device=dev)
      g, oz = torch.zeros((E, npar), dtype=torch.float64, device=dev), torch.zeros((E, eng.n), dtype=torch.float64, device=dev)
      rows = [{k: x[e:e + 1] for k, x in d.items()} for e in range(E)]

      def sequential():
        for e in range(E):
          one(1, rows[e], P[e], g[e], oz[e:e + 1])

      ra = windows(sequential, sync, a.calls, a.windows)
      seq_bits = g.cpu().numpy().tobytes() + oz.cpu().numpy().tobytes()
      emit({"workload": name, "mode": "sequential", "E": E, "R": 1, **ra})
      sets = getattr(eng, "hvp_node_sets_device" if hvp else "exgd_grad_node_sets_device", None)
      if sets is not None:
        g.zero_(); oz.zero_()
        if hvp:
          run = lambda: sets(E, 1, d["z"], d["lam"], d["v"], P, out_z=oz, out_p=g, p_stride=0)
        else:
          run = lambda: sets(E, 1, d["z"], d["lam"], d["lb"], d["ub"], ETA, ETA, NSTEPS, d["seed"], g, 0, P)
        rb = windows(run, sync, a.calls, a.windows)
        assert g.cpu().numpy().tobytes() + oz.cpu().numpy().tobytes() == seq_bits, "sets and sequential calls differ"
        emit({"workload": name, "mode": "sets", "E": E, "R": 1, **rb, "sequential_over_sets": ra["median_ms"] / rb["median_ms"]})
    eng.close()
  if a.digest:
    print(json.dumps({"label": a.label, "version": version, "single_set_outputs_sha256": digest.hexdigest()}), flush=True)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      json.dump(results, f, indent=1)


if __name__ == "__main__":
  main()
