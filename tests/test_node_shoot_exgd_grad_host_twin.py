"""The derivative of the unrolled extragradient steps in the network weights under SHOOTING (myriad_amd/csrc/node_shoot_exgd_grad.h:
NodeShootExgd, node_shoot_exgd_grad_host) against the oracle, on the host.

The twin (tests/hostsim/node_shoot_exgd_grad_twin.cpp) is the header's pair and step algebra compiled with g++, the network in plain loops; the
reference is torch autograd through the oracle's shooting transcription of NodeCartPole and the step restated with torch.clamp
(tests/node_shoot_exgd_grad_cases.py).  Tolerance: 100 x the largest rel_error of grad, dz0 and dlam0 measured on the host with the cases as they
stand -- 5.3e-15 at (4, 3, HEUN, 2, 37); the others 4.3e-16 ... 4.1e-15.  A row is a sum of a few thousand fp64 products: a figure above
1e-11 would be a bug.  Fused against unfused order: 4.7e-15 at the same case (K13's twin: ~1e-15), the same bound.
"""
import os
import subprocess

import numpy as np
import pytest

import node_shoot_exgd_grad_cases as E

ORACLE_MEASURED = 5.3e-15
ORACLE_TOL = 100.0 * ORACLE_MEASURED
ALL = E.CASES + (E.CHUNKED,)
IDS = ["-".join(map(str, c)) for c in ALL]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return E.build_twin(tmp_path_factory.mktemp("node_shoot_exgd_grad_twin"))


@pytest.mark.parametrize("cs", ALL, ids=IDS)
def test_twin_matches_the_oracle_and_the_unfused_order(twin, cs):
  case, *ref = E.reference(*cs)
  rows = case["rows"]
  tw, un = E.twin_of_case(twin, case), E.twin_of_case(twin, case, fused=False)
  if case["nsteps"] == 0:
    for out in (tw, un):
      assert (out[0] == 0.0).all() and (out[1] == case["seed_z"]).all() and (out[2] == case["seed_lam"]).all()
    return
  eo = [E.rel_error(a[rows], r[rows]) for a, r in zip(tw, ref)]
  ef = [E.rel_error(a, r) for a, r in zip(un, tw)]
  print(cs, f"seed {case['seed']} tie {case['tie']:.2e} clipped {case['clipped']:.2f}: twin-oracle {max(eo):.2e} unfused-fused {max(ef):.2e}")
  assert (ref[0][rows] != 0.0).all() and np.abs(ref[0][rows]).max() > 1e-2       # every weight takes part
  assert max(eo) <= ORACLE_TOL, eo
  assert max(ef) <= ORACLE_TOL, ef


def test_null_seed_lam_is_a_zero_seed_lam(twin):
  case, *_ = E.reference(*E.CASES[1])
  a = E.twin_of_case(twin, case, seed_lam=None)
  b = E.twin_of_case(twin, case, seed_lam=np.zeros_like(case["seed_lam"]))
  assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_sanitized_stand_alone_program(tmp_path):
  """tests/hostsim/node_shoot_exgd_grad_check.cpp, its own main, under AddressSanitizer and UBSan: compiled and run directly"""
  exe = str(tmp_path / "node_shoot_exgd_grad_check")
  subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                  os.path.join(E.ROOT, "tests", "hostsim", "node_shoot_exgd_grad_check.cpp"), "-o", exe], check=True, timeout=600)
  r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  print(r.stdout, r.stderr)
  assert r.returncode == 0, r.stdout + r.stderr
  assert r.stdout.count(": ok") == 2
