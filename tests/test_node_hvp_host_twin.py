"""The Lagrangian Hessian-vector product of the network system (myriad_amd/csrc/node_hvp.h: node_hvp_host) against the oracle, on the host.

The twin (tests/hostsim/node_hvp_twin.cpp) is the header's point and pair algebra compiled with g++, the network in plain loops; the reference is
torch's double backward through the oracle's transcriptions of NodeCartPole (tests/node_hvp_cases.py).  Tolerances: 100 x the largest rel_error
measured on the host with the cases as they stand (the figures stand beside the constants below).  A row is a sum of a few thousand fp64
products: a figure above 1e-11 would be a bug, not a tolerance.
"""
import os
import subprocess

import numpy as np
import pytest

import node_hvp_cases as H

ORACLE_MEASURED = 3.1e-15      # twin against torch: out_z of (HERMITE_SIMPSON, 3, 1, HEUN, 2) without the cost; the others 1.9e-16 ... 2.2e-15
SYMMETRY_MEASURED = 1.6e-16    # |u.Hv - v.Hu| / (|u| |Hv| + |v| |Hu|) on the twin: (SHOOTING, 1, 12, MIDPOINT, 1); the others 1.8e-17 ... 9.7e-17
POINT_MEASURED = 4.8e-14       # the layer-by-layer block against SysNODE::hessian d, relative to max|W d| (the five terms of a row cancel)
ORACLE_TOL = 100.0 * ORACLE_MEASURED
SYMMETRY_TOL = 100.0 * SYMMETRY_MEASURED
POINT_TOL = 100.0 * POINT_MEASURED
CEILING = 1e-11
assert max(ORACLE_TOL, SYMMETRY_TOL, POINT_TOL) <= CEILING


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return H.build_twin(tmp_path_factory.mktemp("node_hvp_twin"))


@pytest.mark.parametrize("cs", H.CASES, ids=H.IDS)
def test_twin_matches_the_oracle(twin, cs):
  case, ref = H.reference(*cs)
  rows = case["rows"]
  worst = 0.0
  for wc in (1, 0):
    oz, op = H.twin_of_case(twin, case, wc)
    ez, ep = H.rel_error(oz[rows], ref[wc][0][rows]), H.rel_error(op[rows], ref[wc][1][rows])
    print(cs, f"seed {case['seed']} with_cost {wc}: out_z {ez:.2e} out_p {ep:.2e} (with_cost changes out_z by {case['flag']:.2e})")
    worst = max(worst, ez, ep)
  assert worst <= ORACLE_TOL, worst


@pytest.mark.parametrize("cs", (H.HS_CASES[1], H.SHOOT_CASES[1], H.SHOOT_CASES[2], H.SHOOT_CASES[3]), ids=lambda c: "-".join(map(str, c)))
def test_the_product_is_symmetric(twin, cs):
  case, _ = H.reference(*cs)
  rng = np.random.default_rng(5)
  u = rng.standard_normal(case["v"].shape)
  for wc in (1, 0):
    hv = H.twin_of_case(twin, case, wc)[0]
    hu = H.twin_of_case(twin, case, wc, v=u)[0]
    a, b = (u * hv).sum(axis=1), (case["v"] * hu).sum(axis=1)
    scale = np.linalg.norm(u, axis=1) * np.linalg.norm(hv, axis=1) + np.linalg.norm(case["v"], axis=1) * np.linalg.norm(hu, axis=1)
    err = float((np.abs(a - b) / scale).max())
    print(cs, f"with_cost {wc}: u.Hv {a[0]:.12g} v.Hu {b[0]:.12g} relative {err:.2e}")
    assert np.abs(a).min() > 0 and err <= SYMMETRY_TOL


def test_the_point_block_is_the_dense_hessian_contracted(twin):
  """NodeExgdHost::second + cost_hd at a point against SysNODE::hessian (the 5 x 5 block of the solvers) times d"""
  rng = np.random.default_rng(7)
  p = np.ascontiguousarray(H.weights()[1])
  worst = 0.0
  for wq in (0.0, 0.05):
    for _ in range(8):
      w = np.concatenate([0.5 * rng.standard_normal(4), rng.uniform(-5.0, 5.0, 1)])
      mu, d = 0.1 * rng.standard_normal(4), rng.standard_normal(5)
      a, b = np.empty(5), np.empty(5)
      twin.node_hvp_point_two_ways(w.ctypes.data, p.ctypes.data, mu.ctypes.data, wq, d.ctypes.data, a.ctypes.data, b.ctypes.data)
      assert np.isfinite(a).all() and np.abs(b).max() > 0
      worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
  print(f"layer by layer against the dense block: {worst:.2e}")
  assert worst <= POINT_TOL


def test_null_lam_is_a_zero_lam_and_out_p_does_not_touch_out_z(twin):
  for cs in (H.HS_CASES[1], H.SHOOT_CASES[2]):
    c, _ = H.reference(*cs)
    a = H.twin_of_case(twin, c, 1, lam=None)
    b = H.twin_of_case(twin, c, 1, lam=np.zeros_like(c["lam"]))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    full = H.twin_of_case(twin, c, 1)
    only_z = H.twin_hvp(twin, c["tr"], c["I"], c["cpi"], c["method"], c["T"], c["z"], c["lam"], c["v"], c["params"], 1, want_p=False)
    assert only_z[1] is None and only_z[0].tobytes() == full[0].tobytes()


def test_sanitized_stand_alone_program(tmp_path):
  """tests/hostsim/node_hvp_check.cpp, its own main, under AddressSanitizer and UBSan: compiled and run directly"""
  exe = str(tmp_path / "node_hvp_check")
  subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                  os.path.join(H.ROOT, "tests", "hostsim", "node_hvp_check.cpp"), "-o", exe], check=True, timeout=600)
  r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  print(r.stdout, r.stderr)
  assert r.returncode == 0, r.stdout + r.stderr
  assert r.stdout.count(": ok") == 6
