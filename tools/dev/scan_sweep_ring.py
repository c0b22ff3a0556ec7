#!/usr/bin/env python3
"""Listing gate for the prefetch ring of the Riccati sweeps (DESIGN.md sections 4 and 10.5).

The sweeps (HsFused::riccati_tile, riccati_tile_trap, each as the plain sweep and as a chunk; compiled into the functions sweep_call and
chunk_call) keep PF stages of point records in flight: a stage refills its ring slot with the records of the stage PF further down and
reads the slot's other half (the midpoint records) PF - 1 stages after the refill.  That only hides the memory latency if the compiled
stage loop
  * loads through global_load (a flat_load counts against LGKM as well and drains with lgkmcnt(0) at the next LDS or scalar wait),
  * never waits with s_waitcnt vmcnt(n) for a ring load that has fewer than (PF - 2) stages' worth of ring loads behind it -- i.e. that
    was issued less than PF - 1 stages earlier,
  * never copies a ring register that a load has just written (a copy out of a load's destination waits for that load: the form the
    compiler took when a slot was refilled in front of its last reader).
The loop is the innermost loop of the function that holds the most loads, its body the blocks the compiler's listing annotates as its
members ("in Loop: Header=..."), every block assumed executed.  vmcnt counts stores as well, so the simulation walks two iterations of every
vector memory operation in issue order.

  python tools/dev/scan_sweep_ring.py LISTING.s [--pf 4]     lists the violations per function (exit status 1 when there are any)
"""
import re
import sys

FUNC_RE = re.compile(r"^(_Z\S*?(?:10sweep_call|10chunk_call)\S*):")
LOAD_RE = re.compile(r"^\s*(global_load|flat_load|buffer_load)\w*\s+(\S+?),")
STORE_RE = re.compile(r"^\s*(global_store|flat_store|buffer_store|global_atomic|flat_atomic|buffer_atomic)\w*")
WAIT_RE = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\((\d+)\)")
COPY_RE = re.compile(r"^\s*(v_mov_b32|v_mov_b64|v_accvgpr_write_b32|v_accvgpr_read_b32|v_accvgpr_mov_b32)\w*\s+(\S+),\s*(\S+)")


def regs(op):
  """v[4:5] -> {v4, v5}; a7 -> {a7}; anything else -> empty"""
  m = re.fullmatch(r"([va])\[(\d+):(\d+)\]", op)
  if m:
    return {f"{m.group(1)}{i}" for i in range(int(m.group(2)), int(m.group(3)) + 1)}
  m = re.fullmatch(r"([va])(\d+)", op)
  return {op} if m else set()


def functions(lines):
  """(name, first line, lines) of every sweep_call / chunk_call in the listing"""
  out, cur, start = [], None, 0
  for i, l in enumerate(lines):
    m = FUNC_RE.match(l)
    if m:
      cur, start = m.group(1), i
    elif cur and l.startswith(".Lfunc_end"):
      out.append((cur, start, lines[start:i]))
      cur = None
  return out


BLOCK_RE = re.compile(r"^(?:\.L(BB\w+)|; %bb\.\d+):")
HEADER_RE = re.compile(r"=>This (?:Inner )?Loop Header: Depth=(\d+)")
MEMBER_RE = re.compile(r"in Loop: Header=(BB\w+) Depth=(\d+)")


def stage_loop(body):
  """line indices of the stage loop's body in execution order: the blocks the compiler annotates as members of the innermost loop that
  holds the most loads, from the header on (blocks placed in front of the header -- latches, flow blocks -- run after the ones behind it)"""
  starts = [i for i, l in enumerate(body) if BLOCK_RE.match(l)] + [len(body)]
  blocks = []                                                # (first line, end, header name or None, member-of header or None)
  for a, b in zip(starts, starts[1:]):
    head = " ".join(body[a:a + 2])
    m = BLOCK_RE.match(body[a])
    hdr = m.group(1) if HEADER_RE.search(head) else None
    mem = MEMBER_RE.search(head)
    blocks.append((a, b, hdr, mem.group(1) if mem else None))
  best, best_n = None, 0
  for a, b, hdr, _ in blocks:
    if not hdr:
      continue
    member = [(x, y) for x, y, h, mh in blocks if h == hdr or mh == hdr]
    n = sum(1 for x, y in member for l in body[x:y] if LOAD_RE.match(l))
    if n > best_n:
      after = [(x, y) for x, y in member if x >= a]
      before = [(x, y) for x, y in member if x < a]
      best, best_n = [i for x, y in after + before for i in range(x, y)], n
  return best


def scan_loop(loop, pf):
  """violations (line offset in the loop, text) of one stage loop"""
  ops = []            # (index in loop, 'L' / 'S', destination registers)
  for i, l in enumerate(loop):
    m = LOAD_RE.match(l)
    if m:
      ops.append((i, "L", regs(m.group(2))))
    elif STORE_RE.match(l):
      ops.append((i, "S", set()))
  loads = [o for o in ops if o[1] == "L"]
  hits = []
  if not loads:
    return [(0, "no ring loads in the stage loop")]
  for i, l in enumerate(loop):
    if re.match(r"^\s*flat_load", l):
      hits.append((i, "flat_load in the stage loop: " + l.strip()))
  if len(loads) % pf:
    hits.append((0, f"{len(loads)} loads in the stage loop: not a multiple of PF = {pf}"))
    return hits
  per_stage = len(loads) // pf
  need = (pf - 2) * per_stage
  # vmcnt: two iterations of the memory operations in issue order, the waits of the second one
  for i, l in enumerate(loop):
    m = WAIT_RE.match(l)
    if not m:
      continue
    n = int(m.group(1))
    seq = [o[1] for o in ops] + [o[1] for o in ops if o[0] < i]       # oldest first: the previous iteration, then this one up to the wait
    forced = seq[:max(0, len(seq) - n)]
    if "L" not in forced:
      continue
    y = max(k for k, t in enumerate(forced) if t == "L")
    younger = sum(1 for t in seq[y + 1:] if t == "L")
    if younger < need:
      hits.append((i, f"{l.strip()}: waits for a ring load with {younger} ring loads behind it (< {need} = (PF - 2) x {per_stage}: issued "
                      f"less than PF - 1 stages earlier)"))
  # copies of a just-loaded register: the first reader of a load's destination, in the loop's cyclic order, must not be a copy
  for k, (i, _, dst) in enumerate(loads):
    order = list(range(i + 1, len(loop))) + list(range(0, i))
    for j in order:
      l = loop[j]
      if LOAD_RE.match(l) and regs(LOAD_RE.match(l).group(2)) & dst:
        break                                               # reloaded before anyone read it
      m = COPY_RE.match(l)
      if m and regs(m.group(3)) & dst:
        hits.append((j, f"{l.strip()}: copies the destination of the ring load at loop line {i} ({loop[i].strip()})"))
        break
      toks = re.split(r"[\s,]+", l.strip())
      if len(toks) > 1 and not toks[0].startswith(("s_", ";", ".")) and any(regs(t) & dst for t in toks[2:]):
        break                                               # first reader is a real consumer
  return hits


def scan(path, pf=4):
  """{function: [(listing line, text)]} for every sweep_call / chunk_call of the listing (an empty list: the function passes)"""
  lines = open(path).read().split("\n")
  out = {}
  for name, start, body in functions(lines):
    idx = stage_loop(body)
    if idx is None:
      out[name] = [(start, "no stage loop with loads found")]
      continue
    out[name] = [(start + idx[i], msg) for i, msg in scan_loop([body[k] for k in idx], pf)]
  return out


def default_pf():
  import os
  src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "myriad_amd", "csrc", "hs_solver_wave.h")
  m = re.search(r"#define MYR_RICCATI_PF (\d+)", open(src).read())
  return int(m.group(1))


if __name__ == "__main__":
  args = sys.argv[1:]
  pf = default_pf()
  if "--pf" in args:
    k = args.index("--pf"); pf = int(args[k + 1]); del args[k:k + 2]
  bad = 0
  for path in args:
    for fn, hits in scan(path, pf).items():
      print(f"{path}: {fn[:90]}: {'ok' if not hits else str(len(hits)) + ' violation(s)'}")
      for ln, msg in hits[:12]:
        print(f"  line {ln + 1}: {msg}")
      bad += len(hits)
  sys.exit(1 if bad else 0)
