"""Derivative of the unrolled extragradient steps under SHOOTING (myriad_amd/csrc/shoot_exgd_grad.h: ShootExgdGrad, ShootHvp::interval<true>)
against the oracle, on the host.

The twin (tests/hostsim/shoot_exgd_grad_twin.cpp) is the device code's own pair algebra and pass schedule compiled with g++ and looped over a
batch; the reference is torch autograd through the oracle's shooting transcription and `Lagrangian.step` restated with torch.clamp
(tests/shoot_exgd_grad_cases.py), central differences for the parameter gradient of HIVTREATMENT, SEIR and TUMOUR.
Matrix: 20 systems x {3 x 2 under Euler / Heun / midpoint / RK4, single shooting 1 x 4 RK4}, nsteps = 3, B = 2, a parameter row per instance.

Measured over this matrix (largest |d| / max|row| over grad, dz0 and dlam0; two exact derivatives in fp64, they differ by rounding):
  twin against the oracle, the 17 autograd systems        5.2e-15 (SIMPLECASEWITHBOUNDS, 1 x 4 RK4) -> asserted 1e-11, the project's ORACLE_TOL
  dz0, dlam0 of the three central-difference systems      4.9e-16 (TUMOUR, 3 x 2 Euler)             -> the same
  grad of the three central-difference systems            2.1e-07 (TUMOUR, 3 x 2 midpoint, seed 3)  -> the relative tolerance 1e-6 such differences resolve
  the fused schedule against items 1 .. 5 as three passes 1.4e-15 (EPIDEMICSEIRN, 3 x 2 midpoint)   -> asserted 10 x measured
(profiles/r20_shoot_exgd_grad/README.md).  Every draw is seed 0 except BEARPOPULATIONS 3 x 2 midpoint (seed 1: at seed 0 an unclipped value lies 9.6e-7 from its bound, inside TIE), TUMOUR 3 x 2
midpoint (seed 3) and TUMOUR 1 x 4 RK4 (seed 1): at the seeds before, TUMOUR's central difference does not resolve 1e-6 (shoot_exgd_grad_cases:
FD_SELF; at seed 0 of 1 x 4 RK4 it is 1.5e-6 away from the twin, which the difference with step 1e-5 |p| confirms to 4e-9).
"""
import numpy as np
import pytest

import shoot_exgd_grad_cases as S

ORACLE_TOL = 1e-11
FUSION_MEASURED = 1.4e-15      # the largest |fused - unfused| / max|row| over the matrix (EPIDEMICSEIRN, 3 x 2 midpoint)
FUSION_TOL = 10.0 * FUSION_MEASURED


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return S.build_twin(tmp_path_factory.mktemp("shoot_exgd_grad_twin"))


@pytest.mark.parametrize("name", S.SYSTEMS)
def test_twin_matches_oracle(twin, name):
  worst = 0.0
  for I, cpi, method in S.HOST_SHAPES:
    case, *ref = S.reference(name, I, cpi, method, 3, 2)      # (asserts a finite draw that meets the tie, kink and clip conditions)
    out = S.twin_of_case(twin, case)
    eg, ez, el = (S.rel_error(a, r) for a, r in zip(out, ref))
    print(f"{name} {I}x{cpi} {method} seed {case['seed']} clipped {case['clipped']:.2f} tie {case['tie']:.1e}: grad {eg:.2e} dz0 {ez:.2e} dlam0 {el:.2e}")
    worst = max(worst, ez, el, 0.0 if name in S.FD_SYSTEMS else eg)
    assert np.abs(ref[0]).max() > 0 and np.abs(ref[1]).max() > 0 and np.abs(ref[2]).max() > 0
    assert eg <= (S.FD_RTOL if name in S.FD_SYSTEMS else ORACLE_TOL), (I, cpi, method, eg)
    assert ez <= ORACLE_TOL and el <= ORACLE_TOL, (I, cpi, method, ez, el)
  print(f"{name}: worst {worst:.2e}")


@pytest.mark.parametrize("name", S.SYSTEMS)
def test_fused_schedule_agrees_with_the_items_in_order(twin, name):
  """2 nsteps + 1 passes (item 5 of step s and item 1 of step s - 1 in one pass at x_s) against items 1 .. 5 as three passes a step"""
  worst = 0.0
  for I, cpi, method in S.HOST_SHAPES:
    case = S.reference(name, I, cpi, method, 3, 2)[0]
    a, b = S.twin_of_case(twin, case), S.twin_of_case(twin, case, fused=False)
    e = max(S.rel_error(x, y) for x, y in zip(a, b))
    worst = max(worst, e)
    assert e <= FUSION_TOL, (I, cpi, method, e)
  print(f"{name}: fused against unfused {worst:.2e}")


def test_no_steps_is_the_identity(twin):
  for name in ("CARTPOLE", "PREDATORPREY"):
    for I, cpi, method in S.HOST_SHAPES:
      case = S.reference(name, I, cpi, method, 0, 2)[0]
      for sl in (case["seed_lam"], None):
        grad, dz0, dlam0 = S.twin_of_case(twin, case, seed_lam=sl)
        assert (grad == 0.0).all() and (dz0 == case["seed_z"]).all() and (dlam0 == (0.0 if sl is None else sl)).all()


def test_null_seed_lam_is_zero_seed_lam(twin):
  for I, cpi, method in S.HOST_SHAPES:
    case = S.reference("VANDERPOL", I, cpi, method, 3, 2)[0]
    a = S.twin_of_case(twin, case, seed_lam=None)
    b = S.twin_of_case(twin, case, seed_lam=np.zeros_like(case["seed_lam"]))
    for x, y in zip(a, b):
      assert x.tobytes() == y.tobytes()
    assert np.abs(a[0]).max() > 0
