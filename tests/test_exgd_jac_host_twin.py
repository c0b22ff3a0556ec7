"""Forward-mode Jacobian of the unrolled extragradient steps (myriad_amd/csrc/exgd_jac.h: ExgdJacPoint, exgd_jac_host) against the oracle and against
K10's reverse sweep, on the host.

The twin (tests/hostsim/exgd_jac_twin.cpp) is the device code's own point algebra compiled with g++ and looped over a batch; the reference is torch
autograd through the oracle's transcription, one backward pass per entry of (z_n, lam_n) (tests/exgd_jac_cases.py), central differences for
HIVTREATMENT, SEIR and TUMOUR.  Matrix: K10's -- 20 systems x {Hermite-Simpson, trapezoidal}, N = 3, nsteps 1 and 3, B = 2, a parameter row per
instance, the same draws (pinned first point, at least 15 % of the free variables clipping, no ties: asserted by exgd_grad_cases.reference).

Measured over this matrix, largest |d row| / max|row| over the rows jz[b][k], jlam[b][k]:
  twin against the oracle, the 17 autograd systems      2.2e-15 (CARTPOLE Hermite-Simpson, nsteps 1)   -> asserted 1e-12 (100 x measured, floor 1e-12)
  ... the three central-difference systems              1.4e-07 (TUMOUR Hermite-Simpson, nsteps 1)      -> asserted FD_RTOL = 1e-6
  the iterate zn, lamn against the oracle's             2.1e-15                                         -> asserted 1e-12
  seed . J against K10's twin (grad)                    2.4e-15                                         -> asserted 1e-12 (at most 2e-11: both are
                                                                                                          held to 1e-11 of the oracle)
  the Levenberg-Marquardt driver on the twin (CANCERTREATMENT trapezoidal N = 10, 10 steps, keys r and delta): cond(J) = 1.96 at p*, the keys
  recovered to 7.0e-14 relative from param_guesses + 5 % in 6 evaluations                                -> asserted 1e-10 cond = 1.97e-10
"""
import os
import subprocess

import numpy as np
import pytest

import exgd_grad_cases as E
import exgd_jac_cases as J

MEASURED_JAC = 2.2e-15         # twin against the oracle, autograd systems
MEASURED_ITERATE = 2.1e-15     # zn, lamn against the oracle's
MEASURED_K10 = 2.4e-15         # seed . J against K10's twin
JAC_TOL = max(100.0 * MEASURED_JAC, 1e-12)
ITERATE_TOL = max(100.0 * MEASURED_ITERATE, 1e-12)
K10_TOL = max(100.0 * MEASURED_K10, 1e-12)
HOSTSIM = os.path.join(E.ROOT, "tests", "hostsim")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return J.build_twin(tmp_path_factory.mktemp("exgd_jac_twin"))


@pytest.fixture(scope="module")
def grad_twin(tmp_path_factory):
  return E.build_twin(tmp_path_factory.mktemp("exgd_grad_twin_for_jac"))


@pytest.mark.parametrize("name", J.SYSTEMS)
def test_twin_matches_oracle_and_k10(twin, grad_twin, name):
  assert K10_TOL <= 2e-11
  for scheme in J.SCHEMES:
    for nsteps in (1, 3):
      case, ref_jz, ref_jlam, ref_zn, ref_lamn = J.reference_jac(name, scheme, 3, nsteps, 2)
      out = J.twin_of_case(twin, case)
      ez, el = J.rel_error_rows(out["jz"], ref_jz), J.rel_error_rows(out["jlam"], ref_jlam)
      en = max(E.rel_error(out["zn"], ref_zn), E.rel_error(out["lamn"], ref_lamn))
      ek = E.rel_error(J.seeded(case, out), E.twin_of_case(grad_twin, case)[0])
      print(f"{name} {scheme} nsteps={nsteps}: djz {ez:.2e} djlam {el:.2e} iterate {en:.2e} seed.J - K10 {ek:.2e}")
      assert np.abs(ref_jz).max() > 0 and np.abs(ref_jlam).max() > 0
      tol = J.FD_RTOL if name in J.FD_SYSTEMS else JAC_TOL
      assert ez <= tol and el <= tol, (scheme, nsteps, ez, el)
      assert en <= ITERATE_TOL, (scheme, nsteps, en)
      assert ek <= K10_TOL, (scheme, nsteps, ek)
      # a pinned variable, and one that the last half-step left on a bound, has a zero row entry in every column
      on_bound = ~((out["zn"] > case["lb"]) & (out["zn"] < case["ub"]))
      assert on_bound[:, :case["ns"]].all() and on_bound.sum() > 2 * case["ns"]
      assert (out["jz"][np.broadcast_to(on_bound[:, None, :], out["jz"].shape)] == 0.0).all()
      assert (ref_jz[np.broadcast_to(on_bound[:, None, :], ref_jz.shape)] == 0.0).all()


def test_cost_only_parameters_have_real_columns(twin):
  """the running cost is in the mixed derivative: a cost-only parameter (a zero of myr_fit_grad) moves the steps"""
  for name in ("CANCERTREATMENT", "GLUCOSE", "BEARPOPULATIONS"):
    case, ref_jz, _, _, _ = J.reference_jac(name, "HERMITE_SIMPSON", 3, 3, 2)
    out = J.twin_of_case(twin, case)
    names = E.F.O.SYSTEMS[name].param_names
    for k in E.F.COST_ONLY[name]:
      i = names.index(k)
      assert (np.abs(out["jz"][:, i]).max(axis=-1) > 0).all() and (np.abs(ref_jz[:, i]).max(axis=-1) > 0).all(), (name, k)


def _same(a, b):
  return all(a[k].tobytes() == b[k].tobytes() for k in ("zn", "lamn", "jz", "jlam"))


def test_zero_steps_null_start_chaining_and_groups(twin):
  case = J.reference_jac("CARTPOLE", "HERMITE_SIMPSON", 3, 3, 2)[0]
  rng = np.random.default_rng(3)
  B, npar = case["z"].shape[0], case["params"].shape[1]
  jz0, jlam0 = rng.standard_normal((B, npar, case["n"])), rng.standard_normal((B, npar, case["m"]))
  # nsteps == 0: the inputs come back
  out = J.twin_of_case(twin, case, nsteps=0, jz0=jz0, jlam0=jlam0)
  assert (out["jz"] == jz0).all() and (out["jlam"] == jlam0).all() and (out["zn"] == case["z"]).all() and (out["lamn"] == case["lam"]).all()
  out = J.twin_of_case(twin, case, nsteps=0)
  assert (out["jz"] == 0.0).all() and (out["jlam"] == 0.0).all()
  # a null start is a zero start, bit for bit
  assert _same(J.twin_of_case(twin, case, nsteps=3), J.twin_of_case(twin, case, nsteps=3, jz0=np.zeros_like(jz0), jlam0=np.zeros_like(jlam0)))
  # 2 steps, then 3 from the returned iterate and tangents = 5 steps, bit for bit; a start's tangents do move the result
  five = J.twin_of_case(twin, case, nsteps=5)
  two = J.twin_of_case(twin, case, nsteps=2)
  c2 = dict(case, z=two["zn"], lam=two["lamn"])
  assert _same(J.twin_of_case(twin, c2, nsteps=3, jz0=two["jz"], jlam0=two["jlam"]), five)
  assert not _same(J.twin_of_case(twin, c2, nsteps=3), five)
  # columns do not interact: one, two, three columns to a group have the bits of all four at once
  for g in (1, 2, 3):
    assert _same(J.twin_of_case(twin, case, nsteps=5, gcols=g), five)


def test_driver_recovers_the_parameters_on_the_twin(twin):
  """myriad_amd.experiments.e2e_sysid.fit_imitation_gn (run_endtoend_gn's loop) with the twin in the device call's place, on the zero-residual
  problem of tests/test_gpu_exgd_jac.py: CANCERTREATMENT trapezoidal N = 10, 10 steps, keys r and delta.  cond(J) at p* measured 1.96."""
  from myriad_amd.experiments import e2e_sysid
  hp, c = J.driver_case()
  w = e2e_sysid.imitation_weights(hp, c["rows"], c["nu"], 0)
  width = c["rows"] * c["nu"]
  u_true = J.twin_driver_run(twin, c, c["true"])["zn"][:, -width:].reshape(1, c["rows"], c["nu"])

  def evaluate(params):
    out = J.twin_driver_run(twin, c, params)
    return e2e_sysid.imitation_normal_equations(c["keys"], list(c["names"]), out["zn"][:, -width:], out["jz"], u_true, w)

  at_true = evaluate(c["true"])
  assert at_true[0] == 0.0
  sv = np.sqrt(np.linalg.eigvalsh(at_true[3]))
  cond = sv.max() / sv.min()
  print("cond(J) at p*", cond)
  assert sv.min() > 0 and cond < 1e6 and cond <= J.DRIVER_COND
  res = e2e_sysid.fit_imitation_gn(evaluate, c["start"], max_iter=30)
  err = max(abs(res["params"][k] - c["true"][k]) / abs(c["true"][k]) for k in c["keys"])
  print("losses", res["losses"], "relative error", err, "evaluations", res["device_calls"])
  assert all(b < a for a, b in zip(res["losses"], res["losses"][1:])) and len(res["losses"]) > 2
  assert res["device_calls"] <= 31 and err <= J.DRIVER_RTOL


def test_sanitized_stand_alone_program(tmp_path):
  """tests/hostsim/exgd_jac_check.cpp, its own main, under AddressSanitizer and UBSan: compiled and run directly"""
  exe = str(tmp_path / "exgd_jac_check")
  subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                  os.path.join(HOSTSIM, "exgd_jac_check.cpp"), "-o", exe], check=True, timeout=300)
  r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  print(r.stdout, r.stderr)
  assert r.returncode == 0, r.stdout + r.stderr
  assert r.stdout.count(": ok") == 4
