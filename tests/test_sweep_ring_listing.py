"""Listing gate for the prefetch ring of the Riccati sweeps (tools/dev/scan_sweep_ring.py; DESIGN.md sections 4 and 10.5): the stage loops
of sweep_call / chunk_call load through global_load, wait only for ring loads issued at least PF - 1 stages earlier, and never copy a
register that a ring load has just written.  Synthetic listings check the scanner; the real ones are compiled with the build's flags."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _scanner():
  spec = importlib.util.spec_from_file_location("scan_sweep_ring", os.path.join(ROOT, "tools", "dev", "scan_sweep_ring.py"))
  m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
  return m


def _listing(stages):
  """a sweep_call whose stage loop holds the given stage texts (PF = len(stages))"""
  body = "".join(stages)
  return ("_ZN6myriad7HsFusedI1SELi1ELi0EE10sweep_callENS_6SwArgsE:\n"
          "\tglobal_load_dwordx2 v[10:11], v[0:1], off\n"
          ".LBB0_1:                               ; %loop\n"
          "                                        ; =>This Inner Loop Header: Depth=1\n"
          + body +
          "\ts_cbranch_scc1 .LBB0_1\n"
          "; %bb.2:\n"
          "\ts_setpc_b64 s[30:31]\n"
          ".Lfunc_end0:\n")


def _stage(slot, wait=None, flat=False, copy=False):
  """one stage: waits for its operands, three products, a gain store, the refill of its slot (two loads into v[20+4s : ...])"""
  r0, r1 = 20 + 4 * slot, 22 + 4 * slot
  ld = "flat_load_dwordx2" if flat else "global_load_dwordx2"
  w = f"\ts_waitcnt vmcnt({wait})\n" if wait is not None else ""
  dst1 = f"v[{r1 + 40}:{r1 + 41}]" if copy else f"v[{r1}:{r1 + 1}]"
  txt = (w + f"\tv_mfma_f64_16x16x4_f64 v[2:9], v[{r0}:{r0 + 1}], v[{r1}:{r1 + 1}], v[2:9]\n"
         "\tglobal_store_dwordx2 v[0:1], v[2:3], off\n"
         f"\t{ld} v[{r0}:{r0 + 1}], v[12:13], off\n"
         f"\t{ld} {dst1}, v[14:15], off\n")
  if copy:
    txt += f"\tv_mov_b64_e32 v[{r1}:{r1 + 1}], v[{r1 + 40}:{r1 + 41}]\n"
  return txt


def test_scanner_passes_a_ring_in_flight(tmp_path):
  # PF = 4, 2 loads + 1 store per stage: a wait for the slot refilled 3 stages ago leaves 2 stages (6 operations) in flight
  f = tmp_path / "good.s"
  f.write_text(_listing([_stage(u, wait=6) for u in range(4)]))
  assert _scanner().scan(str(f), pf=4) == {"_ZN6myriad7HsFusedI1SELi1ELi0EE10sweep_callENS_6SwArgsE": []}


def test_scanner_flags_a_wait_for_the_stages_own_loads(tmp_path):
  f = tmp_path / "bad.s"
  f.write_text(_listing([_stage(u, wait=6) for u in range(3)] + [_stage(3, wait=1)]))
  (hits,) = _scanner().scan(str(f), pf=4).values()
  assert len(hits) == 1 and "vmcnt(1)" in hits[0][1]


def test_scanner_flags_flat_loads_and_copies(tmp_path):
  f = tmp_path / "flat.s"
  f.write_text(_listing([_stage(u, wait=6, flat=(u == 2)) for u in range(4)]))
  (hits,) = _scanner().scan(str(f), pf=4).values()
  assert len(hits) == 2 and all("flat_load" in h[1] for h in hits)
  f = tmp_path / "copy.s"
  f.write_text(_listing([_stage(u, wait=6, copy=(u == 1)) for u in range(4)]))
  (hits,) = _scanner().scan(str(f), pf=4).values()
  assert len(hits) == 1 and "copies the destination" in hits[0][1]


def _compile(tmp_path, part):
  """the build's compile of SysCARTPOLE part `part` (__graft_entry__.build), listing kept"""
  base = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
  probe = tmp_path / "probe.hip"
  probe.write_text("#include <hip/hip_runtime.h>\n__global__ void k(double* p) { p[0] = 1.0; }\n")
  if subprocess.run(base + ["-mllvm", "-amdgpu-mfma-vgpr-form", "-c", str(probe), "-o", os.devnull], capture_output=True).returncode == 0:
    base += ["-mllvm", "-amdgpu-mfma-vgpr-form"]
  d = tmp_path / f"p{part}"
  d.mkdir()
  subprocess.run(base + ["-DMYR_TU_SYSTEM=SysCARTPOLE", f"-DMYR_TU_PART={part}", "-save-temps=obj", "-c",
                         os.path.join(ROOT, "myriad_amd", "csrc", "myriad_hip.hip"), "-o", str(d / "p.o")],
                 check=True, capture_output=True, cwd=d)
  (s,) = [f for f in os.listdir(d) if f.endswith("gfx950.s")]
  return str(d / s)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_hermite_simpson_sweeps_keep_the_ring_in_flight(tmp_path):
  """part 1: the headline sweep (W = 1) and the two-level chunk sweep (W = 2)"""
  sc = _scanner()
  res = sc.scan(_compile(tmp_path, 1), pf=sc.default_pf())
  assert any("Li1ELi0EE10sweep_call" in f for f in res) and any("Li2ELi0EE10chunk_call" in f for f in res), list(res)
  bad = {f[:80]: h[:4] for f, h in res.items() if h}
  assert not bad, bad


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_trapezoidal_sweeps_load_globally_into_the_ring(tmp_path):
  """part 3: the chunk sweep passes in full; the one-wavefront sweep loads through global_load and copies no ring register (its first stage
  still waits for the slot the compiler refills at the loop's top -- DESIGN.md section 10.5)"""
  sc = _scanner()
  res = sc.scan(_compile(tmp_path, 3), pf=sc.default_pf())
  sweep = [h for f, h in res.items() if "Li1ELi1EE10sweep_call" in f]
  chunk = [h for f, h in res.items() if "Li2ELi1EE10chunk_call" in f]
  assert len(sweep) == 1 and len(chunk) == 1, list(res)
  assert chunk[0] == [], chunk[0][:4]
  assert not [h for h in sweep[0] if "flat_load" in h[1] or "copies" in h[1] or "no stage loop" in h[1]], sweep[0][:4]
