"""Trajectory-matching loss and parameter gradient (myriad_amd/csrc/fit.h: FitLane<Sys>) against the oracle, on the host.

The twin (tests/hostsim/fit_twin.cpp) is the device code's own FitLane<Sys> compiled with g++ and looped over a batch; the references are
the oracle's autograd through its integrators, or central differences of the oracle's loss for the systems whose constructors convert
their arguments (tests/fit_cases.py).  Matrix: all 20 closed-form systems x 4 integrators, B = 3, S = 7 (40 for the Lenhart systems),
u_rows = S+1 (RK4 clamps: quirk Q6) and, for RK4, u_rows = 2S+1; unweighted and with a decaying wt.  No system is left out: BACTERIA has
finite references on the horizon tests/fit_cases.py:horizon gives it.

Measured over this matrix (the 17 autograd systems; both sides fp64, they differ in the order of their sums):
  largest |dloss| / loss          2.7e-14   -> asserted 2.7e-12
  largest |dgrad| / max|grad|     3.4e-13   -> asserted 3.4e-11
The three central-difference systems (HIVTREATMENT, SEIR, TUMOUR): the same loss bound; gradient to the relative
tolerance 1e-6 the differences resolve (measured 9.6e-08 at worst).
"""
import numpy as np
import pytest

import fit_cases as F

LOSS_TOL = 2.7e-12      # 100 x measured
GRAD_TOL = 3.4e-11      # 100 x measured


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return F.build_twin(tmp_path_factory.mktemp("fit_twin"))


@pytest.mark.parametrize("name", F.SYSTEMS)
def test_twin_matches_oracle(twin, name):
  for (_, method, long_u, weighted) in F.matrix((name,)):
    xs_obs, us, params = F.inputs(name, method, long_u)
    S = xs_obs.shape[1] - 1
    assert us.shape[1] == (2 * S + 1 if long_u else S + 1)
    ref_loss, ref_grad = F.reference(name, method, long_u, weighted)      # (asserts that the oracle's values are finite)
    wt = F.decaying_wt(S) if weighted else None
    loss, grad = F.twin_loss_grad(twin, name, method, F.horizon(name), xs_obs, us, params, wt)
    el, eg = F.rel_errors(loss, grad, ref_loss, ref_grad)
    print(f"{name} {method} u_rows={us.shape[1]} wt={'decaying' if weighted else 'none'}: dloss {el:.2e} dgrad {eg:.2e}")
    assert (ref_loss > 0).all() and np.abs(ref_grad).max() > 0
    assert el <= LOSS_TOL, (method, long_u, weighted, el)
    assert eg <= (F.FD_RTOL if name in F.FD_SYSTEMS else GRAD_TOL), (method, long_u, weighted, eg)


@pytest.mark.parametrize("name", sorted(F.COST_ONLY))
def test_cost_only_parameters_get_exact_zeros(twin, name):
  xs_obs, us, params = F.inputs(name, "RK4")
  _, grad = F.twin_loss_grad(twin, name, "RK4", F.horizon(name), xs_obs, us, params)
  names = F.O.SYSTEMS[name].param_names
  for k in F.COST_ONLY[name]:
    col = grad[:, names.index(k)]
    assert (col == 0.0).all() and not np.signbit(col).any(), (k, col)
  others = [i for i, k in enumerate(names) if k not in F.COST_ONLY[name]]
  assert (grad[:, others] != 0.0).any()


def test_per_instance_parameters_and_defaults(twin):
  """a parameter row per trajectory gives the rows of single calls; params = the defaults reproduces the call without params"""
  xs_obs, us, params = F.inputs("CARTPOLE", "HEUN", per_instance=True)
  T = F.horizon("CARTPOLE")
  loss, grad = F.twin_loss_grad(twin, "CARTPOLE", "HEUN", T, xs_obs, us, params)
  for b in range(F.B):
    l1, g1 = F.twin_loss_grad(twin, "CARTPOLE", "HEUN", T, xs_obs[b:b + 1], us[b:b + 1], params[b])
    assert l1[0] == loss[b] and (g1[0] == grad[b]).all()
  ref_loss, ref_grad = F.reference("CARTPOLE", "HEUN", per_instance=True)
  el, eg = F.rel_errors(loss, grad, ref_loss, ref_grad)
  assert el <= LOSS_TOL and eg <= GRAD_TOL
