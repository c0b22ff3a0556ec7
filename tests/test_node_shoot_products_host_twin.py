"""Lagrangian products and extragradient steps of the network system under SHOOTING (myriad_amd/csrc/node_shoot_products.h: NodeShootProd,
node_shoot_grad_host / jvp_host / exgd_host) against the oracle, on the host.

The twin (tests/hostsim/node_shoot_products_twin.cpp) is the header's pair algebra compiled with g++, the network by SysNODE::lin / f in plain
loops; the reference is the oracle's autodiff through O.shooting(O.NodeCartPole(params), I, cpi, method) (tests/node_shoot_products_cases.py).
Tolerances: those of tests/test_gpu_products.py::test_shooting_products_match_autodiff.

Measured twin - oracle over the six shapes (largest |d| / max(1, largest |ref|)): grad L and J^T lam 3.8e-14 (single shooting, 10 midpoint
steps), J v 1.5e-14, ten extragradient steps 3.3e-16; <J v, lam> against <v, J^T lam> 5.9e-15 relative.
"""
import os
import subprocess

import numpy as np
import pytest

import node_shoot_products_cases as E

SHAPE_IDS = ["-".join(map(str, s)) for s in E.SHAPES]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return E.build_twin(tmp_path_factory.mktemp("node_shoot_products_twin"))


@pytest.mark.parametrize("sh", E.SHAPES, ids=SHAPE_IDS)
def test_twin_products_match_oracle_autodiff(twin, sh):
  c, ref = E.case(*sh), E.ref_products(*sh)
  gL, jt, jv = E.twin_vjp(twin, c, True), E.twin_vjp(twin, c, False), E.twin_jvp(twin, c)
  for b in E.checked(sh[0]):
    rg, rj, rv = ref[b]
    sc = max(1.0, np.abs(rg).max())
    print(sh, b, "gradL", E.rel(gL[b], rg), "JTlam", E.rel(jt[b], rj), "Jv", E.rel(jv[b], rv))
    np.testing.assert_allclose(gL[b], rg, rtol=1e-10, atol=1e-12 * sc)
    np.testing.assert_allclose(jt[b], rj, rtol=1e-9, atol=1e-11 * sc)
    np.testing.assert_allclose(jv[b], rv, rtol=1e-10, atol=1e-12 * max(1.0, np.abs(rv).max()))
  for b in range(sh[0]):                                     # every instance: <J v, lam> == <v, J^T lam>
    lhs, rhs = jv[b] @ c["lam"][b], c["v"][b] @ jt[b]
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs), (b, lhs, rhs)


@pytest.mark.parametrize("sh", E.SHAPES, ids=SHAPE_IDS)
def test_twin_extragradient_steps_match_the_oracle(twin, sh):
  c, ref = E.case(*sh), E.ref_exgd(*sh)
  rows = E.checked(sh[0])
  z, lam = E.twin_exgd(twin, c, rows=rows)
  for i, b in enumerate(rows):
    x, lm = ref[b]
    print(sh, b, "z", E.rel(z[i], x), "lam", E.rel(lam[i], lm))
    np.testing.assert_allclose(z[i], x, rtol=1e-9, atol=1e-10 * max(1.0, np.abs(x).max()))
    np.testing.assert_allclose(lam[i], lm, rtol=1e-9, atol=1e-10)


def test_twin_no_steps_and_nine_plus_one(twin):
  c = E.case(*E.SHAPES[0])
  z0, l0 = E.twin_exgd(twin, c, nsteps=0)
  assert (z0 == c["z"]).all() and (l0 == 1.0).all()
  z10, l10 = E.twin_exgd(twin, c, tight=True)
  ref = E.ref_exgd(*E.SHAPES[0], True)
  lb, ub = E.clip_bounds(c, True)
  for b in range(c["B"]):                                    # the active clip: the same variables exactly on a bound as the oracle's iterate
    assert ((z10[b] == lb) == (ref[b][0] == lb)).all() and ((z10[b] == ub) == (ref[b][0] == ub)).all()
    assert (((ref[b][0] == lb) | (ref[b][0] == ub)) & (lb < ub)).any()


def test_sanitized_stand_alone_program(tmp_path):
  """tests/hostsim/node_shoot_products_check.cpp, its own main, under AddressSanitizer and UBSan: compiled and run directly"""
  exe = str(tmp_path / "node_shoot_products_check")
  subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                  os.path.join(E.ROOT, "tests", "hostsim", "node_shoot_products_check.cpp"), "-o", exe], check=True, timeout=600)
  r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  print(r.stdout, r.stderr)
  assert r.returncode == 0, r.stdout + r.stderr
  assert r.stdout.count(": ok") == 2
