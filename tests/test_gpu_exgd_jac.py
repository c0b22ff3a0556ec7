"""myr_exgd_jac on the device (myriad_amd/csrc/exgd_jac.h: colloc_exgd_jac_kernel) against its host twin, the oracle, K10's reverse sweep, central
differences of myr_exgd, myr_exgd's own bits, and itself across the forms of the call; the Levenberg-Marquardt end-to-end driver
(myriad_amd/experiments/e2e_sysid.py: run_endtoend_gn) on a zero-residual problem.

Tolerances (profiles/r29_exgd_jac/README.md; the figures are the largest |d row| / max|row| over the rows of jz and jlam, measured on an MI355X with
the cases as they stand):
  device against twin     parity cases (N = 3, nsteps = 3, B = 3): 10 x 2.6e-15 (ROCKETLANDING Hermite-Simpson; the others 2.2e-16 ... 6.7e-16)
                          shape cases: 10 x 7.7e-15 (CARTPOLE Hermite-Simpson N = 1; the others 1.6e-15 ... 2.0e-15)
                          The two run the same point algebra and differ by the compiler's FMA contraction.
  device against oracle   10 x the host twin's bound against the oracle (tests/test_exgd_jac_host_twin.py: 1e-12) = 1e-11 (measured 2.1e-15 at worst,
                          ROCKETLANDING Hermite-Simpson; the iterate 5.4e-16)
  seed . J against K10    the CPU test's bound (tests/test_exgd_jac_host_twin.py: K10_TOL = 1e-12; measured 1.4e-15 against myr_exgd_grad, 1e-16 relative
                          between the driver's first 2 J^T r and lookahead_gradient)
  the driver              CANCERTREATMENT trapezoidal N = 10, 10 steps, keys r and delta (chosen on the CPU with the twin, tests/exgd_jac_cases.py:
                          cond(J) at p* = 1.96; the twin-driven fit recovers the keys to 7.0e-14): relative error at most 1e-10 cond = 1.97e-10 (measured
                          7.0e-14 on the device, 6 device calls)
"""
import numpy as np
import pytest
import torch

import exgd_grad_cases as E
import exgd_jac_cases as J
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

PARITY_TWIN_MEASURED = 2.6e-15  # the parity cases: ROCKETLANDING Hermite-Simpson, the largest
SHAPE_TWIN_MEASURED = 7.7e-15   # the shape cases: CARTPOLE Hermite-Simpson N = 1, the largest
PARITY_TWIN_TOL = 10.0 * PARITY_TWIN_MEASURED
SHAPE_TWIN_TOL = 10.0 * SHAPE_TWIN_MEASURED
ORACLE_TOL = 1e-11
K10_TOL = 1e-12
PARITY = ("CARTPOLE", "VANDERPOL", "CANCERTREATMENT", "BACTERIA", "TIMBERHARVEST", "BEARPOPULATIONS", "ROCKETLANDING")
OUT = ("zn", "lamn", "jz", "jlam")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return J.build_twin(tmp_path_factory.mktemp("exgd_jac_twin_gpu"))


def _device(eng, c, **kw):
  a = dict(z=c["z"], lam=c["lam"], lb=c["lb"], ub=c["ub"], eta_x=c["eta_x"], eta_v=c["eta_v"], nsteps=c["nsteps"], params=c["params"])
  a.update(kw)
  return eng.exgd_jac(**a)


def _errs(out, ref):
  return tuple(J.rel_error_rows(out[k], ref[k]) for k in ("jz", "jlam"))


def _same(a, b, keys=OUT):
  return all(a[k].tobytes() == b[k].tobytes() for k in keys)


def shape_case(scheme, N, nsteps, B, name="CARTPOLE"):
  """inputs without an oracle run (the recipe of tests/test_gpu_exgd_grad.py): states around x_0, a third of the variables in a box of 1e-3 that the
  steps leave, the first point pinned, a parameter row per instance"""
  sysm = E.O.SYSTEMS[name]()
  K, n, m = E.dims(name, scheme, N)
  rng = np.random.default_rng(11 + 1000 * N + 10 * nsteps + B + E.SCHEMES.index(scheme))
  xs = np.tile(sysm.x_0, (B, K, 1)) + 0.2 * rng.standard_normal((B, K, sysm.ns))
  us = rng.uniform(-1.0, 1.0, (B, K, sysm.nu))
  z = np.concatenate([xs.reshape(B, -1), us.reshape(B, -1)], axis=1)
  box = rng.random((B, n)) < 0.3
  lb = np.where(box, z - 1e-3, -np.inf)
  ub = np.where(box, z + 1e-3, np.inf)
  lb[:, :sysm.ns] = z[:, :sysm.ns]; ub[:, :sysm.ns] = z[:, :sysm.ns]
  params = sysm.params() * (1.0 + 0.05 * (2.0 * rng.random((B, sysm.params().size)) - 1.0))
  return dict(name=name, scheme=scheme, N=N, T=0.05 * N, nsteps=nsteps, z=z, lam=0.1 * rng.standard_normal((B, m)), lb=lb, ub=ub, params=params,
              eta_x=0.02, eta_v=0.02, seed_z=rng.standard_normal((B, n)), seed_lam=rng.standard_normal((B, m)), K=K, n=n, m=m, ns=sysm.ns, nu=sysm.nu)


# ---- parity with the oracle and the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", E.SCHEMES)
@pytest.mark.parametrize("name", PARITY)
def test_parity_with_the_oracle_and_the_twin(twin, name, scheme):
  case, ref_jz, ref_jlam, ref_zn, ref_lamn = J.reference_jac(name, scheme, 3, 3, 3)
  eng = _lib.Engine(name, scheme, 3, case["T"])
  out = _device(eng, case)
  eng.close()
  tw = J.twin_of_case(twin, case)
  eo, et = _errs(out, dict(jz=ref_jz, jlam=ref_jlam)), _errs(out, tw)
  ei = max(E.rel_error(out["zn"], ref_zn), E.rel_error(out["lamn"], ref_lamn))
  print(f"{name} {scheme}: device-oracle {max(eo):.2e} device-twin {max(et):.2e} iterate-oracle {ei:.2e}")
  assert np.abs(ref_jz).max() > 0 and np.abs(ref_jlam).max() > 0
  assert max(et) <= PARITY_TWIN_TOL, et
  assert max(eo) <= ORACLE_TOL and ei <= ORACLE_TOL, (eo, ei)


# ---- awkward shapes against the twin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,N", [("HERMITE_SIMPSON", N) for N in (1, 31, 32, 33, 100)] + [("TRAPEZOIDAL", N) for N in (63, 64, 65)])
def test_awkward_shapes_against_the_twin(twin, scheme, N):
  eng = _lib.Engine("CARTPOLE", scheme, N, 0.05 * N)
  worst = 0.0
  for nsteps in (0, 1, 10):
    for B in (1, 130):
      c = shape_case(scheme, N, nsteps, B)
      out = _device(eng, c)
      tw = J.twin_of_case(twin, c)
      et = _errs(out, tw)
      worst = max(worst, *et)
      assert max(et) <= SHAPE_TWIN_TOL, (nsteps, B, et)
      if nsteps == 0:
        assert (out["jz"] == 0.0).all() and (out["jlam"] == 0.0).all() and (out["zn"] == c["z"]).all() and (out["lamn"] == c["lam"]).all()
      else:
        assert np.abs(out["jz"]).max() > 0 and np.abs(out["jlam"]).max() > 0
        assert (out["jz"][:, :, :c["ns"]] == 0.0).all()      # the pinned first point
  eng.close()
  print(f"{scheme} N={N}: device-twin {worst:.2e}")


# ---- the iterate has the bits of myr_exgd ----------------------------------------------------------------------------------------------
def test_the_iterate_has_the_bits_of_myr_exgd():
  c = shape_case("HERMITE_SIMPSON", 5, 4, 70)
  eng = _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", 5, c["T"])
  out = _device(eng, c)
  z, lam = eng.exgd(c["z"], c["lam"], c["lb"], c["ub"], c["eta_x"], c["eta_v"], 4, params=c["params"])
  eng.close()
  assert np.array_equal(out["zn"], z) and np.array_equal(out["lamn"], lam)
  assert not np.array_equal(z, c["z"])


# ---- forms of the call -----------------------------------------------------------------------------------------------------------------
def test_forms_of_the_call():
  c = shape_case("HERMITE_SIMPSON", 5, 4, 70)
  eng = _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", 5, c["T"])
  z_in, lam_in = c["z"].copy(), c["lam"].copy()
  rows = _device(eng, c)
  assert (c["z"] == z_in).all() and (c["lam"] == lam_in).all()
  # repeated calls
  assert _same(_device(eng, c), rows)
  # an instance alone against inside the batch
  for b in (0, 37, 69):
    one = _device(eng, {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()})
    assert all(one[k][0].tobytes() == rows[k][b].tobytes() for k in OUT), b
  # each subset of the optional outputs
  for want in (("jz",), ("jlam",), ("jz", "jlam"), ("zn", "jz"), ("lamn", "jlam"), ("zn", "lamn", "jz"), ("zn", "lamn", "jlam")):
    sub = _device(eng, c, want=want)
    assert set(sub) == set(want) and _same(sub, rows, want), want
  # shared parameters = the same row for every instance
  assert _same(_device(eng, c, params=c["params"][0]), _device(eng, c, params=np.tile(c["params"][0], (70, 1))))
  # after an unrelated call on the handle
  eng.exgd_grad(c["z"], c["lam"], c["lb"], c["ub"], c["eta_x"], c["eta_v"], 2, c["seed_z"], params=c["params"])
  eng.vjp(c["z"], c["lam"])
  assert _same(_device(eng, c), rows)
  # device arrays: the same bits as host arrays, inputs untouched; a start's tangents on the device
  dev = "cuda:0"
  t = {k: torch.tensor(c[k], device=dev) for k in ("z", "lam", "lb", "ub", "params")}
  o = {k: torch.full(rows[k].shape, float("nan"), dtype=torch.float64, device=dev) for k in OUT}
  eng.exgd_jac_device(70, t["z"], t["lam"], t["lb"], t["ub"], c["eta_x"], c["eta_v"], 4, params=t["params"], params_stride=eng.np, **o)
  torch.cuda.synchronize()
  assert all(o[k].cpu().numpy().tobytes() == rows[k].tobytes() for k in OUT)
  assert (t["z"].cpu().numpy() == z_in).all() and (t["lam"].cpu().numpy() == lam_in).all()
  eng.close()


# ---- groups of columns -------------------------------------------------------------------------------------------------------------------
def test_column_groups_have_the_same_bits_and_capacity_is_refused(monkeypatch):
  c = shape_case("HERMITE_SIMPSON", 20, 3, 5, name="HIVTREATMENT")
  c["params"] = 0.5 + np.random.default_rng(2).random(c["params"].shape)      # (parameters of order one, as the oracle cases of this system)
  c["z"] = np.abs(c["z"]) * 0.0 + 1.0 + 0.05 * np.random.default_rng(3).standard_normal(c["z"].shape)
  c["lb"], c["ub"] = np.where(np.isfinite(c["lb"]), c["z"] - 1e-3, -np.inf), np.where(np.isfinite(c["ub"]), c["z"] + 1e-3, np.inf)
  c["lb"][:, :c["ns"]] = c["z"][:, :c["ns"]]; c["ub"][:, :c["ns"]] = c["z"][:, :c["ns"]]
  eng = _lib.Engine("HIVTREATMENT", "HERMITE_SIMPSON", 20, c["T"])
  assert eng.np == 9
  full = _device(eng, c)
  assert np.isfinite(full["jz"]).all() and all(np.abs(full["jz"][:, k]).max() > 0 for k in range(9))
  record = (2 * c["n"] + c["m"] + c["K"] * c["ns"]) * 8      # the iterate's bytes, and one column's
  for cols in (1, 2, 4):                                      # nine groups of one, five of two, three of three
    monkeypatch.setenv("MYRIAD_EXGD_JAC_LDS_BYTES", str((1 + cols) * record + 16))
    assert _same(_device(eng, c), full), cols
  # a budget below one column: MYR_E_CAPACITY, nothing written
  monkeypatch.setenv("MYRIAD_EXGD_JAC_LDS_BYTES", str(2 * record + 15))
  out = {k: np.full(full[k].shape, 7.0) for k in OUT}
  rc = eng.lib.myr_exgd_jac(eng._h, 5, *(np.ascontiguousarray(c[k]).ctypes.data for k in ("z", "lam", "lb", "ub", "params")), 9, c["eta_x"], c["eta_v"], 3,
                            None, None, *(out[k].ctypes.data for k in OUT), _lib.MEM_HOST)
  assert rc == -4 and b"one tangent column" in eng.lib.myr_last_error()
  assert all((out[k] == 7.0).all() for k in OUT)
  monkeypatch.delenv("MYRIAD_EXGD_JAC_LDS_BYTES")
  assert _same(_device(eng, c), full)
  eng.close()


# ---- chaining, long unrolls ------------------------------------------------------------------------------------------------------------
def test_chained_calls_have_the_bits_of_one():
  c = shape_case("HERMITE_SIMPSON", 5, 7, 6)
  eng = _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", 5, c["T"])
  seven = _device(eng, c)
  three = _device(eng, c, nsteps=3)
  four = _device(eng, c, z=three["zn"], lam=three["lamn"], nsteps=4, jz0=three["jz"], jlam0=three["jlam"])
  held = _device(eng, c, z=three["zn"], lam=three["lamn"], nsteps=4)
  eng.close()
  assert _same(four, seven)
  assert _same(held, seven, ("zn", "lamn")) and not _same(held, seven, ("jz",))


def test_long_unroll():
  """2 000 steps from a fixed start: finite, and the bits of 1 000 + 1 000 chained.  No history exists: the handle's scratch does not grow."""
  c = shape_case("HERMITE_SIMPSON", 10, 2000, 4)
  c["eta_x"], c["eta_v"] = 0.005, 0.005
  eng = _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", 10, c["T"])
  whole = _device(eng, c)
  first = _device(eng, c, nsteps=1000)
  second = _device(eng, c, z=first["zn"], lam=first["lamn"], nsteps=1000, jz0=first["jz"], jlam0=first["jlam"])
  eng.close()
  assert all(np.isfinite(whole[k]).all() for k in OUT) and np.abs(whole["jz"]).max() > 0
  assert _same(second, whole)


# ---- against K10 and against differences of myr_exgd --------------------------------------------------------------------------------------
def test_seeded_rows_are_myr_exgd_grad():
  worst = 0.0
  for scheme, N in (("HERMITE_SIMPSON", 5), ("TRAPEZOIDAL", 7)):
    c = shape_case(scheme, N, 4, 9)
    eng = _lib.Engine("CARTPOLE", scheme, N, c["T"])
    out = _device(eng, c)
    g = eng.exgd_grad(c["z"], c["lam"], c["lb"], c["ub"], c["eta_x"], c["eta_v"], 4, c["seed_z"], seed_lam=c["seed_lam"], params=c["params"], want_start=False)
    eng.close()
    worst = max(worst, E.rel_error(J.seeded(c, out), g["grad"]))
  print(f"seed . J against myr_exgd_grad: {worst:.2e}")
  assert worst <= K10_TOL


def test_central_differences_of_myr_exgd():
  """(z_n(p + d) - z_n(p - d)) / 2 d from two myr_exgd calls per parameter, d = 1e-6 |p|, against the columns of jz"""
  c = shape_case("HERMITE_SIMPSON", 10, 10, 1)
  c["params"] = c["params"][0]
  eng = _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", 10, c["T"])
  out = _device(eng, c, want=("jz",))
  for k in range(c["params"].size):
    d = 1e-6 * abs(c["params"][k])
    zs = []
    for sgn in (1.0, -1.0):
      p = c["params"].copy(); p[k] += sgn * d
      zs.append(eng.exgd(c["z"], c["lam"], c["lb"], c["ub"], c["eta_x"], c["eta_v"], 10, params=p)[0])
    fd = (zs[0][0] - zs[1][0]) / (2.0 * d)
    print("column", k, "largest", np.abs(fd).max(), "difference", np.abs(out["jz"][0, k] - fd).max())
    np.testing.assert_allclose(out["jz"][0, k], fd, rtol=1e-6, atol=1e-6 * np.abs(fd).max())
  eng.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors_in_the_documented_order():
  c = shape_case("HERMITE_SIMPSON", 3, 2, 2)
  for name, tr, kw, word in (("CARTPOLE", "SHOOTING", dict(controls_per_interval=5), "myr_exgd_grad_shoot"),
                             ("NODE_CARTPOLE", "HERMITE_SIMPSON", {}, "myr_exgd_grad_node"),
                             ("CARTPOLE_ELASTIC", "HERMITE_SIMPSON", {}, "elastic twin"),
                             ("INVASIVEPLANT", "SHOOTING", dict(controls_per_interval=7), "INVASIVEPLANT")):
    eng = _lib.Engine(name, tr, 3, 1.0, **kw)
    with pytest.raises(NotImplementedError, match=word):
      eng.exgd_jac_probe()
    eng.close()
  eng = _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", 3, c["T"])
  a = {k: np.ascontiguousarray(c[k]).ctypes.data for k in ("z", "lam", "lb", "ub", "params")}
  jz, jlam = np.full((2, 4, c["n"]), 7.0), np.full((2, 4, c["m"]), 7.0)

  def call(h=eng._h, B=2, nsteps=2, stride=4, mem=_lib.MEM_HOST, jz_=jz.ctypes.data, jlam_=jlam.ctypes.data, **ptr):
    q = dict(a); q.update(ptr)
    rc = eng.lib.myr_exgd_jac(h, B, q["z"], q["lam"], q["lb"], q["ub"], q["params"], stride, 0.02, 0.02, nsteps, None, None, None, None, jz_, jlam_, mem)
    return rc, eng.lib.myr_last_error().decode()

  for kw, word in ((dict(h=None), "null handle or array"), (dict(z=None), "null handle or array"), (dict(lam=None), "null handle or array"),
                   (dict(lb=None), "null handle or array"), (dict(ub=None), "null ub"), (dict(jz_=None, jlam_=None), "jz and jlam are both null"),
                   (dict(B=-1), "negative batch"), (dict(nsteps=-1), "negative nsteps"), (dict(stride=3), "params_stride"), (dict(mem=5), "bad mem")):
    rc, msg = call(**kw)
    assert rc == -1 and word in msg and msg.startswith("myr_exgd_jac"), (kw, rc, msg)
  # the order: an earlier class wins over a later one
  assert "null ub" in call(ub=None, jz_=None, jlam_=None, B=-1)[1]
  assert "both null" in call(jz_=None, jlam_=None, B=-1, nsteps=-1)[1]
  assert "negative batch" in call(B=-1, nsteps=-1, stride=3, mem=5)[1]
  assert "negative nsteps" in call(nsteps=-1, stride=3, mem=5)[1]
  assert "params_stride" in call(stride=3, mem=5)[1]
  assert (jz == 7.0).all() and (jlam == 7.0).all()
  assert call(B=0)[0] == 0 and (jz == 7.0).all()               # B == 0 writes nothing
  assert call()[0] == 0 and np.isfinite(jz).all() and not (jz == 7.0).all()
  eng.close()
  sh = _lib.Engine("CARTPOLE", "SHOOTING", 3, 1.0, controls_per_interval=5)      # MYR_E_ARG before MYR_E_UNSUPPORTED
  rc = sh.lib.myr_exgd_jac(sh._h, -1, a["z"], a["lam"], a["lb"], a["ub"], None, 0, 0.02, 0.02, 1, None, None, None, None, jz.ctypes.data, None, _lib.MEM_HOST)
  assert rc == -1 and "negative batch" in sh.lib.myr_last_error().decode()
  sh.close()
  eng = _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", 700, 2.0)     # the iterate and one column: 2 (2 n + m + K ns) doubles = 403 KB
  with pytest.raises(_lib.MyriadHipError, match="one tangent column"):
    eng.exgd_jac(np.zeros((1, eng.n)), np.zeros((1, eng.m)), -np.ones(eng.n), np.ones(eng.n), 0.01, 0.01, 1)
  eng.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def test_driver_recovers_the_parameters_of_a_zero_residual_problem():
  """CANCERTREATMENT, trapezoidal, N = 10, 10 steps, keys r and delta (param_guesses): chosen on the CPU with the twin, where J at p* has full column
  rank with cond(J) = 1.96 (tests/test_exgd_jac_host_twin.py asserts it) and the twin-driven fit recovers the keys to 7.0e-14.  u_true is Engine.exgd's
  own result from the guess with the true parameters, so r(p*) = 0 exactly; the start is param_guesses + 5 %."""
  from myriad_amd.config import Config
  from myriad_amd.experiments import e2e_sysid
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp, c = J.driver_case()
  cfg = Config(verbose=False, plot=False)
  nsteps, max_iter = J.DRIVER["nsteps"], 30
  opt = get_optimizer(hp, cfg, hp.system())
  eta_x, eta_v = opt.step_sizes()
  assert (eta_x, eta_v) == (c["eta_x"], c["eta_v"]) and np.allclose(opt.guess, c["z0"][0], rtol=1e-12, atol=1e-12)      # the problem the twin was asked
  z, _ = opt.engine.exgd(opt.guess, np.zeros(opt.engine.m), opt.bounds[:, 0], opt.bounds[:, 1], eta_x, eta_v, nsteps, params=opt.system.device_params())
  width = c["rows"] * c["nu"]
  u_true = z[0, -width:].reshape(c["rows"], c["nu"])
  res = e2e_sysid.run_endtoend_gn(hp, cfg, nsteps=nsteps, max_iter=max_iter, true_opt_us=u_true, guess=c["start"])
  err = max(abs(res["params"][k] - c["true"][k]) / abs(c["true"][k]) for k in c["keys"])
  print("losses", res["losses"], "relative error", err, "device calls", res["device_calls"])
  assert set(res["params"]) == set(c["keys"]) and res["jtj"].shape == (2, 2)
  assert all(b < a for a, b in zip(res["losses"], res["losses"][1:])) and len(res["losses"]) > 2
  assert res["device_calls"] <= max_iter + 1
  assert err <= J.DRIVER_RTOL
  sv = np.sqrt(np.linalg.eigvalsh(res["jtj"]))
  assert sv.max() / sv.min() <= J.DRIVER_COND
  # J^T r of the first iteration against lookahead_gradient's reverse sweep from the same point (the guess, lmbda = 0) with the same weights (epoch 0)
  # and the same NUM_UNROLLED steps.  lookahead_gradient takes its loss gradient AT THE POINT IT STARTS FROM; the controls it is asked to imitate
  # are shifted so that this gradient is the residual at the END of the steps, 2 w (u_n - u_true): its result is then 2 J^T r, the driver's gradient
  assert e2e_sysid.NUM_UNROLLED == nsteps
  fwd = res["first"][1]
  zn = opt.unrolled_jacobian(opt.guess, np.zeros(opt.engine.m), c["start"], nsteps, eta_x, eta_v, want=("zn", "jz"))["zn"]
  u_start, u_n = opt.guess[-width:].reshape(c["rows"], c["nu"]), zn[-width:].reshape(c["rows"], c["nu"])
  rev = e2e_sysid.lookahead_gradient(opt, c["start"], opt.guess, np.zeros(opt.engine.m), u_start - (u_n - u_true), 0, opt.bounds[:, 0], opt.bounds[:, 1],
                                     eta_x, eta_v)
  scale = max(abs(fwd[k]) for k in c["keys"])
  print("forward 2 J^T r", fwd, "lookahead_gradient", rev)
  assert scale > 0 and all(abs(fwd[k] - rev[k]) <= K10_TOL * scale for k in c["keys"])
  opt.engine.close()
