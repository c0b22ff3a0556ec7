#!/usr/bin/env python3
"""Device-code comparison of two source trees: has a refactor changed what the compiler emits?

Every translation unit of the library (the job list of __graft_entry__.build()) is compiled from both trees with the build's flags
plus --cuda-device-only -S.  The only text that depends on where a tree lies is the __hip_cuid_<hash> symbol: it is replaced by a
fixed token.  Per job the tool prints `identical`, or the functions whose text differs.

  python tools/dev/cmp_device_code.py TREE_A TREE_B [-DNAME=V ...] [--only REGEX] [--normalise [--max-ranges N]] [--listings DIR] [--reuse] [-j N]

  -DNAME=V      an extra define for both compiles (e.g. the fallback form: -DMYR_FUSED_SPEC=0 -DMYR_SWEEP_CALL_W=0)
  --only        jobs whose name matches (e.g. 'SysCARTPOLE.p[13]')
  --normalise   compare instruction sequences: comments and directives dropped, register names and .LBB labels replaced.  Per
                differing function: the index ranges that differ, the indices of the first and the last v_mfma, and whether the
                sequence between those two is unchanged (the stage code of a sweep lies there); --max-ranges N prints the first N ranges
                and the number of the others (a re-allocated kernel has thousands)
  --listings    where the listings go (DIR/a, DIR/b; default build/cmp); --reuse keeps a listing that is already there
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

# the flags of __graft_entry__.build()
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form"]


def listing(tree, out, job, extra, reuse):
  name, defs = job
  path = os.path.join(out, name + "".join(extra) + ".s")
  if not (reuse and os.path.exists(path)):
    src = os.path.join(tree, "myriad_amd", "csrc", "myriad_hip.hip")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + defs + extra + ["--cuda-device-only", "-S", src, "-o", path],
                       capture_output=True, text=True)
    if r.returncode != 0:
      raise RuntimeError(f"hipcc failed for {name} in {tree}:\n{r.stderr[-4000:]}")
  return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())


def functions(text):
  """{symbol: lines} of every function of a listing"""
  d, cur = {}, None
  for ln in text.split("\n"):
    m = re.match(r"^(_Z\w+):", ln)
    if m:
      cur = m.group(1); d[cur] = []
    elif ln.startswith(".Lfunc_end"):
      cur = None
    elif cur:
      d[cur].append(ln)
  return d


def norm(lines):
  out = []
  for l in lines:
    if not l.startswith("\t") or l.startswith("\t."):
      continue
    l = l.split(";")[0].rstrip()
    l = re.sub(r"\b[vsa]\[\d+:\d+\]", "R", l); l = re.sub(r"\b[vsa]\d+\b", "R", l); l = re.sub(r"\.LBB\d+_\d+", "L", l)
    out.append(l)
  return out


def mfma_span(x):
  k = [i for i, l in enumerate(x) if l.lstrip().startswith("v_mfma")]
  return (k[0], k[-1]) if k else (0, -1)


def compare(name, ta, tb, normalise, max_ranges=0):
  """report lines of one job"""
  if ta == tb:
    return [f"{name}: identical"]
  a, b = functions(ta), functions(tb)
  rep = [f"  gone: {k[:150]}" for k in a if k not in b] + [f"  new:  {k[:150]}" for k in b if k not in a]
  for k in a:
    if k not in b or a[k] == b[k]:
      continue
    if not normalise:
      rep.append(f"  differs: {k[:150]}")
      continue
    x, y = norm(a[k]), norm(b[k])
    if x == y:
      continue
    ops = [o for o in difflib.SequenceMatcher(None, x, y, autojunk=False).get_opcodes() if o[0] != "equal"]
    (fa, la), (fb, lb) = mfma_span(x), mfma_span(y)
    same = x[fa:la + 1] == y[fb:lb + 1]
    rep.append(f"  differs: {k[:150]}\n    instructions {len(x)} -> {len(y)}; v_mfma first / last {fa} / {la} -> {fb} / {lb}; "
               f"first to last v_mfma {'unchanged' if same else 'CHANGED'}\n    ranges: " +
               ", ".join(f"a[{o[1]}:{o[2]}] b[{o[3]}:{o[4]}]" for o in (ops[:max_ranges] if max_ranges else ops)) +
               (f", ... {len(ops) - max_ranges} more, the last a[{ops[-1][1]}:{ops[-1][2]}] b[{ops[-1][3]}:{ops[-1][4]}]" if max_ranges and len(ops) > max_ranges else ""))
  if not rep:
    return [f"{name}: identical" + (" after normalising" if normalise else " in every function (text outside the functions differs)")]
  return [f"{name}: {len(rep)} function(s) differ"] + rep


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument("tree_a"); ap.add_argument("tree_b")
  ap.add_argument("-D", dest="defs", action="append", default=[])
  ap.add_argument("--only", default=".")
  ap.add_argument("--normalise", action="store_true")
  ap.add_argument("--max-ranges", type=int, default=0)
  ap.add_argument("--listings", default=os.path.join(ROOT, "build", "cmp"))
  ap.add_argument("--reuse", action="store_true")
  ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 4))
  args = ap.parse_args()
  extra = ["-D" + d for d in args.defs]
  jobs = [j for j in entry._jobs() if re.search(args.only, j[0])]
  work = [(tree, os.path.join(args.listings, side), j) for j in jobs for side, tree in (("a", args.tree_a), ("b", args.tree_b))]
  for _, out, _ in work:
    os.makedirs(out, exist_ok=True)
  with ThreadPoolExecutor(min(16, args.j)) as ex:
    texts = list(ex.map(lambda w: listing(w[0], w[1], w[2], extra, args.reuse), work))
  print(f"# {len(jobs)} jobs{' ' + ' '.join(extra) if extra else ''}{', normalised' if args.normalise else ''}")
  differing = 0
  for i, (name, _) in enumerate(jobs):
    rep = compare(name + "".join(" " + e for e in extra), texts[2 * i], texts[2 * i + 1], args.normalise, args.max_ranges)
    differing += len(rep) > 1
    print("\n".join(rep), flush=True)
  print(f"# {len(jobs) - differing} of {len(jobs)} jobs identical")
  sys.exit(1 if differing else 0)


if __name__ == "__main__":
  main()
