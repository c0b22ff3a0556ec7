"""Derivative of the unrolled extragradient steps in the network weights (myriad_amd/csrc/node_exgd_grad.h: NodeExgdHost, node_exgd_grad_host)
against the oracle, on the host.

The twin (tests/hostsim/node_exgd_grad_twin.cpp) is the header's plain-loop point algebra compiled with g++; the reference is torch autograd
through oracle.NodeCartPole and the step formulas (tests/node_exgd_grad_cases.py).  Cases (N, nsteps, B), Hermite-Simpson, the committed weights:
(1, 1, 1), (3, 3, 2), (2, 0, 2), (33, 2, 1) and (7, 2, 3); 27 ... 30 % of the free variables of every instance clip in a half-step (asserted: at
least 15 %).

Measured over these cases (two exact derivatives in fp64; a row is a sum of a few thousand products):
  largest |dgrad| / max|grad|                          3.6e-15
  largest |ddz0| / max|dz0|, |ddlam0| / max|dlam0|     5.0e-15
asserted: 100 x the larger, 5.0e-13 (profiles/r18_node_exgd_grad/README.md).
"""
import numpy as np
import pytest

import node_exgd_grad_cases as E

MEASURED = 5.0e-15             # largest rel_error of grad, dz0, dlam0 over the cases (grad alone: 3.6e-15)
TWIN_TOL = 100.0 * MEASURED


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return E.build_twin(tmp_path_factory.mktemp("node_exgd_grad_twin"))


@pytest.mark.parametrize("N,nsteps,batch", E.CASES + (E.CHUNKED,))
def test_twin_matches_oracle(twin, N, nsteps, batch):
  case, ref_grad, ref_dz0, ref_dlam0 = E.reference(N, nsteps, batch)      # (asserts the tie condition and finite references)
  grad, dz0, dlam0 = E.twin_of_case(twin, case)
  eg, ez, el = E.rel_error(grad, ref_grad), E.rel_error(dz0, ref_dz0), E.rel_error(dlam0, ref_dlam0)
  print(f"NODE N={N} nsteps={nsteps} B={batch} clipped={case['clipped']:.2f}: dgrad {eg:.2e} ddz0 {ez:.2e} ddlam0 {el:.2e}")
  assert (case["lb"][:, :4] == case["ub"][:, :4]).all()
  if nsteps == 0:
    assert (grad == 0.0).all() and (dz0 == case["seed_z"]).all() and (dlam0 == case["seed_lam"]).all()
    return
  assert (ref_grad != 0.0).all() and np.abs(ref_dz0).max() > 0 and np.abs(ref_dlam0).max() > 0      # every one of the 4 804 weights moves the steps
  assert E.MIN_CLIPPED <= case["clipped"] <= 0.75, case["clipped"]
  assert eg <= TWIN_TOL and ez <= TWIN_TOL and el <= TWIN_TOL, (eg, ez, el)


def test_null_seed_lam_is_a_zero_seed(twin):
  c, _, _, _ = E.reference(3, 3, 2)
  args = (c["N"], c["T"], c["z"], c["lam"], c["lb"], c["ub"], c["params"], c["eta_x"], c["eta_v"], 3, c["seed_z"])
  for u, v in zip(E.twin_grad(twin, *args, None), E.twin_grad(twin, *args, np.zeros_like(c["seed_lam"]))):
    assert (u == v).all()


def test_initial_weights_have_haiku_linear_shape():
  """node=None of run_node_endtoend: truncated normal of std 1 / sqrt(fan_in) cut at two standard deviations, zero biases, seeded"""
  from myriad_amd.experiments.node_e2e_sysid import initial_node
  from myriad_amd.systems.neural_ode import flat_from_mapping
  a, b = initial_node(3), initial_node(3)
  assert flat_from_mapping(a.params).shape == (4804,) and (flat_from_mapping(a.params) == flat_from_mapping(b.params)).all()
  assert (flat_from_mapping(initial_node(4).params) != flat_from_mapping(a.params)).any()
  for k, fan_in, out in (("linear", 5, 64), ("linear_1", 64, 64), ("linear_2", 64, 4)):
    w, bias = a.params[k]["w"], a.params[k]["b"]
    assert w.shape == (fan_in, out) and (bias == 0.0).all() and bias.shape == (out,)
    assert np.abs(w).max() <= 2.0 / np.sqrt(fan_in) and 0.5 / np.sqrt(fan_in) < w.std() < 1.0 / np.sqrt(fan_in)
