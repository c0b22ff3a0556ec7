"""Lagrangian Hessian-vector product (myriad_amd/csrc/shoot_hvp.h: ShootHvp; colloc_hvp.h: CollocHvp) against the oracle, on the host.

The twin (tests/hostsim/hvp_twin.cpp) is the device code's own algebra compiled with g++ and looped over a batch; the reference is torch
double-backward through the oracle's transcription (tests/hvp_cases.py), central differences for out_p of HIVTREATMENT, SEIR and TUMOUR.
Matrix: 20 systems x {Hermite-Simpson N = 3, trapezoidal N = 3, shooting 3 x 2 under Euler / Heun / midpoint / RK4, single shooting 1 x 4 RK4},
B = 2, a parameter row per instance, with_cost 1 and 0: 280 cases.

Measured over this matrix (two exact derivatives in fp64; they differ by rounding):
  largest |d out_z| / max|out_z|                          3.2e-15 (BACTERIA, 1 x 4 RK4)             -> asserted 1e-12 (the floor)
  largest |d out_p| / max|out_p|, the 17 autograd systems 2.7e-14 (SIMPLECASEWITHBOUNDS, 3 x 2 Heun) -> asserted 2.7e-12 (100 x measured)
  out_p of the three central-difference systems           9.5e-09 (SEIR, 3 x 2 RK4)                 -> the relative tolerance 1e-6 such differences resolve
  symmetry |u^T H v - v^T H u| / (sum|u_i (Hv)_i| + sum|v_i (Hu)_i|)   2.0e-16                       -> asserted 1e-13 (the floor)
  the stage rule against ShootCore::slin's step Hessian   3.5e-16                                   -> the out_z bound
(profiles/r17_hvp/README.md).  With with_cost = 0 the systems with linear dynamics (GLUCOSE, MOUNTAINCAR, ...) have out_z = 0 exactly, in the oracle and
in the twin: the references are asserted non-zero with the cost in.
"""
import os
import subprocess

import numpy as np
import pytest

import hvp_cases as H

MEASURED_Z = 3.2e-15           # largest |d out_z| / max|out_z| over the matrix
MEASURED_P = 2.7e-14           # largest |d out_p| / max|out_p| over the matrix (autograd systems)
MEASURED_SYM = 2.0e-16
Z_TOL = max(100.0 * MEASURED_Z, 1e-12)
P_TOL = max(100.0 * MEASURED_P, 1e-12)
SYM_TOL = max(100.0 * MEASURED_SYM, 1e-13)
HOSTSIM = os.path.join(H.ROOT, "tests", "hostsim")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return H.build_twin(tmp_path_factory.mktemp("hvp_twin"))


@pytest.mark.parametrize("name", H.SYSTEMS)
def test_twin_matches_oracle(twin, name):
  for tr, N, cpi, method in H.HOST_SHAPES:
    for wc in (1, 0):
      case, ref_z, ref_p = H.reference(name, tr, N, cpi, method, 2, wc)      # (asserts finite references away from the kinks)
      oz, op = H.twin_of_case(twin, case, wc)
      ez, ep = H.rel_error(oz, ref_z), H.rel_error(op, ref_p)
      print(f"{name} {tr} {N}x{cpi} {method} with_cost={wc}: dz {ez:.2e} dp {ep:.2e}")
      if wc:
        assert np.abs(ref_z).max() > 0 and np.abs(ref_p).max() > 0
      assert ez <= Z_TOL, (tr, N, cpi, method, wc, ez)
      assert ep <= (H.FD_RTOL if name in H.FD_SYSTEMS else P_TOL), (tr, N, cpi, method, wc, ep)


@pytest.mark.parametrize("name", ("CARTPOLE", "BEARPOPULATIONS", "BACTERIA", "HARVEST", "ROCKETLANDING"))
def test_symmetry(twin, name):
  """u^T (H v) = v^T (H u) for two random directions"""
  worst = 0.0
  for tr, N, cpi, method in H.HOST_SHAPES:
    case = H.inputs(name, tr, N, cpi, method, 2)
    u = np.random.default_rng(5).standard_normal(case["v"].shape)
    hv, _ = H.twin_of_case(twin, case)
    hu, _ = H.twin_of_case(twin, case, v=u)
    for b in range(2):
      a, c = u[b] @ hv[b], case["v"][b] @ hu[b]
      scale = np.abs(u[b] * hv[b]).sum() + np.abs(case["v"][b] * hu[b]).sum()
      assert scale > 0
      worst = max(worst, abs(a - c) / scale)
      assert abs(a - c) <= SYM_TOL * scale, (tr, N, cpi, method, a, c)
  print(f"{name}: symmetry {worst:.2e}")


def test_linearity(twin):
  """v = 0 gives exact zeros; H (2 v) == 2 H v bit for bit"""
  for name in ("CARTPOLE", "PREDATORPREY", "TIMBERHARVEST"):
    for tr, N, cpi, method in H.HOST_SHAPES:
      case = H.inputs(name, tr, N, cpi, method, 2)
      for wc in (1, 0):
        oz, op = H.twin_of_case(twin, case, wc, v=np.zeros_like(case["v"]))
        assert (oz == 0.0).all() and (op == 0.0).all()
        z1, p1 = H.twin_of_case(twin, case, wc)
        z2, p2 = H.twin_of_case(twin, case, wc, v=2.0 * case["v"])
        assert (z2 == 2.0 * z1).all() and (p2 == 2.0 * p1).all(), (name, tr, method, wc)


def test_null_lam_is_zero_lam(twin):
  for tr, N, cpi, method in H.HOST_SHAPES:
    case = H.inputs("VANDERPOL", tr, N, cpi, method, 2)
    a = H.twin_of_case(twin, case, lam=None)
    b = H.twin_of_case(twin, case, lam=np.zeros_like(case["lam"]))
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    assert np.abs(a[0]).max() > 0                                            # the objective's own Hessian


@pytest.mark.parametrize("name", ("CARTPOLE", "BEARPOPULATIONS", "HARVEST"))
def test_stage_rule_against_the_solvers_step_hessian(twin, name):
  """ShootCore::slin(..., pin = a, ...)'s Hs times the step's tangent equals what ShootHvp::step_back hands back for ad = 0, for every integrator
  (BEARPOPULATIONS: two controls; HARVEST: time in the cost)"""
  from myriad_amd._lib import INT_IDS, SYS_IDS
  sysm = H.O.SYSTEMS[name]()
  rng = np.random.default_rng(11)
  worst = 0.0
  for method in H.METHODS:
    ny = sysm.ns + (3 if method == "RK4" else 2) * sysm.nu
    x = sysm.x_0 * (1.0 + 0.05 * rng.standard_normal(sysm.ns)) + 0.05 * rng.standard_normal(sysm.ns) * (0.0 if name in H.F.LENHART else 1.0)
    y = np.concatenate([x, H.F._controls(sysm, rng, 1, ny)[0].ravel()[:ny - sysm.ns]])
    yd, a = rng.standard_normal(ny), rng.standard_normal(sysm.ns)
    p = sysm.params() * (1.0 + 0.05 * (2.0 * rng.random(sysm.params().size) - 1.0))
    hs, rule = np.empty(ny), np.empty(ny)
    rc = twin.hvp_step_two_ways(SYS_IDS[name], INT_IDS[method], 0.05, 0.35, y.ctypes.data, yd.ctypes.data, p.ctypes.data, a.ctypes.data,
                                hs.ctypes.data, rule.ctypes.data)
    assert rc == ny
    e = H.rel_error(rule[None], hs[None])
    worst = max(worst, e)
    assert np.abs(hs).max() > 0 and e <= Z_TOL, (method, e, hs, rule)
  print(f"{name}: stage rule against slin {worst:.2e}")


def test_cost_only_parameters(twin):
  """a parameter that enters the running cost only has a real entry in out_p with the cost in, and a literal 0.0 without"""
  for name, keys in (("CANCERTREATMENT", ("a",)), ("GLUCOSE", ("A", "l")), ("BEARPOPULATIONS", ("c_p", "c_f"))):
    names = H.O.SYSTEMS[name].param_names
    for tr, N, cpi, method in H.HOST_SHAPES:
      case, _, ref_p = H.reference(name, tr, N, cpi, method, 2, 1)
      _, p1 = H.twin_of_case(twin, case, 1)
      _, p0 = H.twin_of_case(twin, case, 0)
      for k in keys:
        i = names.index(k)
        assert (p1[:, i] != 0.0).all() and (ref_p[:, i] != 0.0).all(), (name, k, tr, method)
        assert (p0[:, i] == 0.0).all(), (name, k, tr, method)


def test_sanitized_stand_alone_program(tmp_path):
  """tests/hostsim/hvp_check.cpp, its own main, under AddressSanitizer and UBSan: compiled and run directly"""
  exe = str(tmp_path / "hvp_check")
  subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                  os.path.join(HOSTSIM, "hvp_check.cpp"), "-o", exe], check=True, timeout=600)
  r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  print(r.stdout, r.stderr)
  assert r.returncode == 0, r.stdout + r.stderr
  assert r.stdout.count(": ok") == 7


def test_integration_block_compiles_and_matches_the_header():
  """the SciPy callbacks INTEGRATION.md shows: the block compiles and calls myr_hvp with the number of arguments the header declares, which is the
  number the binding's argtypes list"""
  import re
  import test_integration_stub as S
  txt = open(os.path.join(H.ROOT, "INTEGRATION.md")).read()
  blk = [b for b in re.findall(r"```python\n(.*?)```", txt, re.S) if "def hip_hessians" in b]
  assert len(blk) == 1
  compile(blk[0], "INTEGRATION.md:hip_hessians", "exec")
  calls = S._call_arity(blk[0])
  assert [c for c, _ in calls] == ["myr_hvp"]
  assert calls[0][1] == S._header_arity()["myr_hvp"] == 12
  from myriad_amd import _lib      # (the signature table load() declares the functions from; importing it loads no library)
  assert len(_lib._SIGNATURES["myr_hvp"][0]) == 12
