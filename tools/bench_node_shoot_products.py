#!/usr/bin/env python
"""Timing of myr_vjp / myr_jvp / myr_exgd (nsteps = 10) of the network system under SHOOTING: the matrix-core form (node_shoot_products.h)
against the per-lane form of the same build (MYRIAD_PROD_MODE=lane), and one Hermite-Simpson myr_exgd call as orientation.  A project tool, not
part of bench.py.

The parent never opens the GPU: every measurement is a child process of its own under `timeout`, the two forms alternate, and nothing starts
after a child has failed.  Per child: `--warm` warm calls, then `--calls` timed ones (fewer of the slow lane form: `--lane-warm`, `--lane-calls`); reported are the median of myr_kernel_time(MYR_K_PROD) and of
the wall clock per call.  Over `--reps` alternating children the parent prints the median and the min - max spread, one JSON line per
(shape, form), and the ratio lane / matrix-core of the kernel-time medians.

  python tools/bench_node_shoot_products.py --reps 3 --out timings.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, transcription, B, intervals, cpi): the reference's default (single shooting, 100 controls, HEUN) at three batch sizes, the multiple-shooting
# shape of tests/test_gpu_node.py::test_node_shooting_batch, and Hermite-Simpson N = 100 (myr_exgd only; no lane form)
SHAPES = (("default_B1", "SHOOTING", 1, 1, 100), ("default_B64", "SHOOTING", 64, 1, 100), ("default_B1024", "SHOOTING", 1024, 1, 100),
          ("multi_20x5_B1024", "SHOOTING", 1024, 20, 5), ("hs_N100_B1024", "HERMITE_SIMPSON", 1024, 100, 1))
NSTEPS = 10


def child(a):
  sys.path.insert(0, ROOT)
  import numpy as np
  from myriad_amd import _lib
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping
  p = np.ascontiguousarray(flat_from_mapping(NeuralODE.load_fitted_cartpole().params), dtype=np.float64)
  T = 2.0
  eng = _lib.Engine("NODE_CARTPOLE", a.transcription, a.intervals, T, controls_per_interval=a.cpi, integration_method="HEUN", max_batch=max(64, a.B))
  rng = np.random.default_rng(1)
  z = 0.2 * rng.standard_normal((a.B, eng.n)); lam = rng.standard_normal((a.B, eng.m)); v = rng.standard_normal((a.B, eng.n))
  lb, ub = np.full(eng.n, -10.0), np.full(eng.n, 10.0)
  calls = {"exgd": lambda: eng.exgd(z, np.ones_like(lam), lb, ub, 1e-2, 1e-3, NSTEPS, params=p)}
  if a.transcription == "SHOOTING":
    calls["vjp"] = lambda: eng.vjp(z, lam, params=p, add_gradf=True)
    calls["jvp"] = lambda: eng.jvp(z, v, params=p)
  out = {}
  for name, f in calls.items():
    for _ in range(a.warm):
      f()
    ker, wall = [], []
    for _ in range(a.calls):
      eng.kernel_time_reset()
      t0 = time.perf_counter(); f(); wall.append((time.perf_counter() - t0) * 1e3)
      ms, n = eng.kernel_time(_lib.K_PROD)
      ker.append(ms * n)
    out[name] = {"kernel_ms": statistics.median(ker), "wall_ms": statistics.median(wall)}
  eng.close()
  print("RESULT " + json.dumps(out), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--reps", type=int, default=3)
  ap.add_argument("--calls", type=int, default=5)
  ap.add_argument("--warm", type=int, default=2)
  ap.add_argument("--lane-calls", type=int, default=2, help="timed calls of the (slow) lane form")
  ap.add_argument("--lane-warm", type=int, default=1)
  ap.add_argument("--limit", type=int, default=300, help="seconds per child")
  ap.add_argument("--out", default=None)
  ap.add_argument("--shapes", default=None, help="comma-separated names (default: all)")
  ap.add_argument("--child", action="store_true")
  ap.add_argument("--transcription"); ap.add_argument("--B", type=int); ap.add_argument("--intervals", type=int); ap.add_argument("--cpi", type=int)
  a = ap.parse_args()
  if a.child:
    return child(a)
  shapes = [s for s in SHAPES if a.shapes is None or s[0] in a.shapes.split(",")]
  runs = {}
  for rep in range(a.reps):
    for name, tr, B, I, cpi in shapes:
      for form in (("mfma", "lane") if tr == "SHOOTING" else ("mfma",)):      # alternating
        env = dict(os.environ)
        env.pop("MYRIAD_PROD_MODE", None)
        if form == "lane":
          env["MYRIAD_PROD_MODE"] = "lane"
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--transcription", tr, "--B", str(B),
               "--intervals", str(I), "--cpi", str(cpi), "--calls", str(a.lane_calls if form == "lane" else a.calls), "--warm", str(a.lane_warm if form == "lane" else a.warm)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
          print(f"{name} {form}: child failed (exit {r.returncode}); nothing further is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
          return r.returncode or 1
        runs.setdefault((name, form), []).append(json.loads(line[0][7:]))
  table = []
  for (name, form), rs in runs.items():
    row = {"shape": name, "form": form, "reps": len(rs)}
    for call in rs[0]:
      for k in ("kernel_ms", "wall_ms"):
        vals = [r[call][k] for r in rs]
        row[f"{call}_{k}"] = {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}
    table.append(row)
    print(json.dumps(row), flush=True)
  for name, tr, *_ in shapes:
    if tr == "SHOOTING":
      m, l = (next(r for r in table if r["shape"] == name and r["form"] == f) for f in ("mfma", "lane"))
      print(json.dumps({"shape": name, "lane_over_mfma_kernel": {c: l[f"{c}_kernel_ms"]["median"] / m[f"{c}_kernel_ms"]["median"] for c in ("vjp", "jvp", "exgd")},
                        "beats_spread": {c: l[f"{c}_kernel_ms"]["min"] > m[f"{c}_kernel_ms"]["max"] for c in ("vjp", "jvp", "exgd")}}), flush=True)
  if a.out:
    with open(a.out, "w") as f:
      json.dump(table, f, indent=1)
  return 0


if __name__ == "__main__":
  sys.exit(main())
