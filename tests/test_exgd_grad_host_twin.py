"""Derivative of the unrolled extragradient steps (myriad_amd/csrc/exgd_grad.h: ExgdGradPoint, exgd_grad_host) against the oracle, on the host.

The twin (tests/hostsim/exgd_grad_twin.cpp) is the device code's own point algebra compiled with g++ and looped over a batch; the reference is
torch autograd through the oracle's transcription and the step formulas (tests/exgd_grad_cases.py), central differences for the parameter
gradient of HIVTREATMENT, SEIR and TUMOUR.  Matrix: 20 systems x {Hermite-Simpson, trapezoidal}, N = 3, nsteps 1 and 3, B = 2, a parameter
row per instance; the first point's state is pinned, 29 ... 32 % of the other variables of every instance clip in a half-step (asserted: at
least 15 %), and a case whose oracle run
comes within 1e-6 of a bound (or 1e-3 of a kink of PENDULUM / MOUNTAINCAR) fails.

Measured over this matrix (the 17 autograd systems; two exact derivatives in fp64, they differ by rounding through at most 3 steps):
  largest |dgrad| / max|grad|                          2.9e-15   -> asserted 1e-12 (100 x measured, floor 1e-12)
  largest |ddz0| / max|dz0|, |ddlam0| / max|dlam0|     6.4e-16   -> asserted 1e-12 (the floor)
(profiles/r15_exgd_grad/README.md).  The three central-difference systems: the same bound for dz0 / dlam0, which are autograd for them too; the
parameter gradient to the relative tolerance 1e-6 the differences resolve (measured 1.8e-07 at worst).
"""
import os
import subprocess

import numpy as np
import pytest

import exgd_grad_cases as E

MEASURED_GRAD = 2.9e-15        # largest |dgrad| / max|grad| over the matrix
MEASURED_START = 6.4e-16       # largest of the same figure for dz0 and dlam0
GRAD_TOL = max(100.0 * MEASURED_GRAD, 1e-12)
START_TOL = max(100.0 * MEASURED_START, 1e-12)
HOSTSIM = os.path.join(E.ROOT, "tests", "hostsim")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return E.build_twin(tmp_path_factory.mktemp("exgd_grad_twin"))


@pytest.mark.parametrize("name", E.SYSTEMS)
def test_twin_matches_oracle(twin, name):
  for scheme in E.SCHEMES:
    for nsteps in (1, 3):
      case, ref_grad, ref_dz0, ref_dlam0 = E.reference(name, scheme, 3, nsteps, 2)      # (asserts the tie condition and finite references)
      grad, dz0, dlam0 = E.twin_of_case(twin, case)
      eg, ez, el = E.rel_error(grad, ref_grad), E.rel_error(dz0, ref_dz0), E.rel_error(dlam0, ref_dlam0)
      print(f"{name} {scheme} nsteps={nsteps} clipped={case['clipped']:.2f}: dgrad {eg:.2e} ddz0 {ez:.2e} ddlam0 {el:.2e}")
      assert np.abs(ref_grad).max() > 0 and np.abs(ref_dz0).max() > 0 and np.abs(ref_dlam0).max() > 0
      assert E.MIN_CLIPPED <= case["clipped"] <= 0.75, case["clipped"]      # of the free variables, in every instance
      assert (case["lb"][:, :case["ns"]] == case["ub"][:, :case["ns"]]).all()
      assert eg <= (E.FD_RTOL if name in E.FD_SYSTEMS else GRAD_TOL), (scheme, nsteps, eg)
      assert ez <= START_TOL and el <= START_TOL, (scheme, nsteps, ez, el)


def test_zero_steps_and_null_seed(twin):
  """nsteps == 0: grad = 0, dz0 = seed_z, dlam0 = seed_lam; a null seed_lam is a zero seed_lam, bit for bit"""
  case, _, _, _ = E.reference("CARTPOLE", "HERMITE_SIMPSON", 3, 3, 2)
  c = dict(case)
  c["nsteps"] = 0
  grad, dz0, dlam0 = E.twin_of_case(twin, c)
  assert (grad == 0.0).all() and (dz0 == c["seed_z"]).all() and (dlam0 == c["seed_lam"]).all()
  a = E.twin_grad(twin, c["name"], c["scheme"], c["N"], c["T"], c["z"], c["lam"], c["lb"], c["ub"], c["params"], c["eta_x"], c["eta_v"], 3, c["seed_z"], None)
  b = E.twin_grad(twin, c["name"], c["scheme"], c["N"], c["T"], c["z"], c["lam"], c["lb"], c["ub"], c["params"], c["eta_x"], c["eta_v"], 3, c["seed_z"],
                  np.zeros_like(c["seed_lam"]))
  for u, v in zip(a, b):
    assert (u == v).all()


def test_cost_only_parameters_have_real_entries(twin):
  """the running cost is in the mixed derivative: a cost-only parameter (a zero of myr_fit_grad) moves the steps"""
  for name in ("CANCERTREATMENT", "GLUCOSE", "BEARPOPULATIONS"):
    case, ref_grad, _, _ = E.reference(name, "HERMITE_SIMPSON", 3, 3, 2)
    grad, _, _ = E.twin_of_case(twin, case)
    names = E.F.O.SYSTEMS[name].param_names
    for k in E.F.COST_ONLY[name]:
      assert (grad[:, names.index(k)] != 0.0).all() and (ref_grad[:, names.index(k)] != 0.0).all(), (name, k)


def test_sanitized_stand_alone_program(tmp_path):
  """tests/hostsim/exgd_grad_check.cpp, its own main, under AddressSanitizer and UBSan: compiled and run directly"""
  exe = str(tmp_path / "exgd_grad_check")
  subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                  os.path.join(HOSTSIM, "exgd_grad_check.cpp"), "-o", exe], check=True, timeout=300)
  r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  print(r.stdout, r.stderr)
  assert r.returncode == 0, r.stdout + r.stderr
  assert r.stdout.count(": ok") == 3
