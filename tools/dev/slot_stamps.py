# dev tool: where the slots of the two-phase launch idle.  Runs the bench workload with the slot-stamp build (-DMYR_SLOT_STAMPS: every slot of the fused
# kernel writes the wall clock at entry, after each ticket and at exit) once per launch form -- phase-1 fill on, fill off -- and prints for launch 1 and
# launch 2 the IDLE SHARE: mean over slots of (last exit - own exit) / duration of the launch (first entry to last exit).
#   tools/dev/build_variant.sh "" libstamps.so -DMYR_SLOT_STAMPS && MYRIAD_VARIANT_LIB=variants/libstamps.so python tools/dev/slot_stamps.py [B] [repeats]
# Each form runs in a process of its own (the knobs are read once per handle, the library once per process).
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child(B, repeats, path):
  import numpy as np
  sys.path.insert(0, ROOT)
  from myriad_amd import _lib
  _lib.LIB_PATH = os.path.abspath(os.environ.get("MYRIAD_VARIANT_LIB") or os.path.join(ROOT, "variants", "libstamps.so"))
  from bench import build_workload
  x0, z0, lb, ub, T = build_workload(B, 100, 2019)
  eng = _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", 100, T, max_batch=B)
  eng.solve(z0, lb, ub)        # warm-up: allocations, code upload
  rows = []
  for _ in range(repeats):
    res = eng.solve(z0, lb, ub)
    d = np.fromfile(path, dtype=np.int64)
    slots, words = int(d[0]), int(d[1])
    st = d[2:].reshape(2, slots, words)
    row = []
    for ph in range(2):
      entry, exit_, nt = st[ph, :, 0], st[ph, :, 1], st[ph, :, 2]
      span = float(exit_.max() - entry.min())
      row += [span, float((exit_.max() - exit_).mean()) / span, float(nt.mean()), int(nt.max())]
    rows.append(row)
  rows = np.array(rows)
  plan = eng.solve_plan()
  print("  plan: park_iter %d, %d launches, %d slots; converged %.3f, iterations median %g max %g" %
        (plan["park_iter"], plan["launches_per_solve"], plan["slots"], (res["status"] == 0).mean(), np.median(res["iters"]), res["iters"].max()))
  for ph in range(2):
    c = rows[:, 4 * ph:4 * ph + 4]
    print("  launch %d: idle share %s  (mean %.4f)   span [ticks of the 100 MHz wall clock] %s   tickets per slot mean %.2f max %d" %
          (ph + 1, " ".join("%.4f" % v for v in c[:, 1]), c[:, 1].mean(), " ".join("%.0f" % v for v in c[:, 0]), c[:, 2].mean(), int(c[:, 3].max())))
  tot = rows[:, 0] + rows[:, 4]
  print("  launch-1 idle as a share of both launches: %.4f;  launch-2 idle: %.4f" %
        ((rows[:, 1] * rows[:, 0] / tot).mean(), (rows[:, 5] * rows[:, 4] / tot).mean()))


if __name__ == "__main__":
  if len(sys.argv) > 1 and sys.argv[1] == "--child":
    child(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
  else:
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    for fill in ("0", "1"):
      with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "stamps.bin")
        print("MYRIAD_PARK_FILL=%s  B = %d" % (fill, B), flush=True)
        env = dict(os.environ, MYRIAD_PARK_FILL=fill, MYRIAD_SLOT_STAMPS=path)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(B), str(repeats), path], env=env, timeout=300)
        if r.returncode != 0:
          sys.exit(r.returncode)       # (nothing more on the device after a failure)
