"""myr_exgd_grad on the device (myriad_amd/csrc/exgd_grad.h: colloc_exgd_grad_kernel) against its host twin, the oracle, central differences of
myr_exgd, and itself across the forms of the call; the end-to-end driver (myriad_amd/experiments/e2e_sysid.py) against a torch restatement of
the reference's forward-mode many_steps_grad + lookahead_update.

Tolerances (profiles/r15_exgd_grad/README.md; the figures are the largest |d| / max|row| over grad, dz0 and dlam0, measured on an MI355X with
the cases as they stand):
  device against twin     parity cases (N = 3, nsteps = 3): 10 x 7.3e-15 (ROCKETLANDING Hermite-Simpson; the others 2e-16 ... 3.1e-15)
                          shape cases: 10 x 1.5e-14 (CARTPOLE Hermite-Simpson N = 100, nsteps = 10, B = 130; the others 3.2e-15 ... 9.1e-15)
                          The two run the same point algebra and differ by the compiler's FMA contraction and the order of the parameter sums.
  device against oracle   10 x the host twin's bound against the oracle (tests/test_exgd_grad_host_twin.py: 1e-12) = 1e-11 (measured 9.8e-15
                          at worst, VANDERPOL trapezoidal)
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import exgd_grad_cases as E
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

PARITY_TWIN_MEASURED = 7.3e-15  # the parity cases (N = 3, nsteps = 3): ROCKETLANDING Hermite-Simpson, the largest
SHAPE_TWIN_MEASURED = 1.5e-14   # the shape cases: CARTPOLE Hermite-Simpson N = 100, nsteps = 10, B = 130
PARITY_TWIN_TOL = 10.0 * PARITY_TWIN_MEASURED
SHAPE_TWIN_TOL = 10.0 * SHAPE_TWIN_MEASURED
ORACLE_TOL = 1e-11
PARITY = ("CARTPOLE", "VANDERPOL", "CANCERTREATMENT", "BACTERIA", "TIMBERHARVEST", "BEARPOPULATIONS", "ROCKETLANDING")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return E.build_twin(tmp_path_factory.mktemp("exgd_grad_twin_gpu"))


def _engine(name, scheme, N, T):
  return _lib.Engine(name, scheme, N, T)


def _device(eng, c, **kw):
  a = dict(z=c["z"], lam=c["lam"], lb=c["lb"], ub=c["ub"], eta_x=c["eta_x"], eta_v=c["eta_v"], nsteps=c["nsteps"], seed_z=c["seed_z"],
           seed_lam=c["seed_lam"], params=c["params"])
  a.update(kw)
  return eng.exgd_grad(**a)


def _errs(out, ref):
  return tuple(E.rel_error(out[k], r) for k, r in zip(("grad", "dz0", "dlam0"), ref))


# ---- parity with the oracle and the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", E.SCHEMES)
@pytest.mark.parametrize("name", PARITY)
def test_parity_with_the_oracle_and_the_twin(twin, name, scheme):
  case, *ref = E.reference(name, scheme, 3, 3, 3)
  eng = _engine(name, scheme, 3, case["T"])
  out = _device(eng, case)
  eng.close()
  tw = E.twin_of_case(twin, case)
  eo, et = _errs(out, ref), _errs(out, tw)
  print(f"{name} {scheme}: device-oracle {max(eo):.2e} device-twin {max(et):.2e}")
  assert max(et) <= PARITY_TWIN_TOL, et
  assert max(eo) <= ORACLE_TOL, eo


# ---- awkward shapes against the twin -------------------------------------------------------------------------------------------------
def shape_case(scheme, N, nsteps, B, name="CARTPOLE"):
  """inputs without an oracle run: states around x_0, a third of the variables in a box of 1e-3 that the steps leave, the first point pinned"""
  sysm = E.O.SYSTEMS[name]()
  K, n, m = E.dims(name, scheme, N)
  rng = np.random.default_rng(7 + 1000 * N + 10 * nsteps + B + E.SCHEMES.index(scheme))
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


@pytest.mark.parametrize("scheme,N", [("HERMITE_SIMPSON", N) for N in (1, 31, 32, 33, 100)] + [("TRAPEZOIDAL", N) for N in (63, 64, 65)])
def test_awkward_shapes_against_the_twin(twin, scheme, N):
  eng = _engine("CARTPOLE", scheme, N, 0.05 * N)
  worst = 0.0
  for nsteps in (0, 1, 10):
    for B in (1, 130):
      c = shape_case(scheme, N, nsteps, B)
      out = _device(eng, c)
      tw = E.twin_of_case(twin, c)
      et = _errs(out, tw)
      worst = max(worst, *et)
      assert max(et) <= SHAPE_TWIN_TOL, (nsteps, B, et)
      if nsteps == 0:
        assert (out["grad"] == 0.0).all() and (out["dz0"] == c["seed_z"]).all() and (out["dlam0"] == c["seed_lam"]).all()
      else:
        assert np.abs(out["grad"]).max() > 0
  eng.close()
  print(f"{scheme} N={N}: device-twin {worst:.2e}")


# ---- independent of the oracle and the twin ------------------------------------------------------------------------------------------
def test_central_differences_of_myr_exgd():
  """seed . (z_n(p + d) - z_n(p - d)) / 2 d from two myr_exgd calls per parameter, d = 1e-6 |p|, against grad"""
  c = shape_case("HERMITE_SIMPSON", 10, 10, 1)
  c["params"] = c["params"][0]
  eng = _engine("CARTPOLE", "HERMITE_SIMPSON", 10, c["T"])
  out = _device(eng, c, seed_lam=None)
  fd = np.empty(c["params"].size)
  for k in range(fd.size):
    d = 1e-6 * abs(c["params"][k])
    zs = []
    for sgn in (1.0, -1.0):
      p = c["params"].copy(); p[k] += sgn * d
      zs.append(eng.exgd(c["z"], c["lam"], c["lb"], c["ub"], c["eta_x"], c["eta_v"], 10, params=p)[0])
    fd[k] = float(c["seed_z"][0] @ (zs[0][0] - zs[1][0])) / (2.0 * d)
  eng.close()
  print("grad", out["grad"][0], "central differences", fd)
  np.testing.assert_allclose(out["grad"][0], fd, rtol=1e-6)


# ---- forms of the call -----------------------------------------------------------------------------------------------------------------
def test_forms_of_the_call(monkeypatch):
  c = shape_case("HERMITE_SIMPSON", 5, 4, 70)
  eng = _engine("CARTPOLE", "HERMITE_SIMPSON", 5, c["T"])
  z_in, lam_in = c["z"].copy(), c["lam"].copy()
  rows = _device(eng, c)
  assert (c["z"] == z_in).all() and (c["lam"] == lam_in).all()
  # shared parameters = the same row for every instance
  shared = _device(eng, c, params=c["params"][0])
  tiled = _device(eng, c, params=np.tile(c["params"][0], (70, 1)))
  for k in ("grad", "dz0", "dlam0"):
    assert shared[k].tobytes() == tiled[k].tobytes()
  # the batch sum: within 1e-13 scale of the exact row sum, the same bits on every call
  s1, s2 = _device(eng, c, reduce=True), _device(eng, c, reduce=True)
  exact = np.array([float(sum(Fraction(float(v)) for v in rows["grad"][:, k])) for k in range(eng.np)])
  scale = np.abs(rows["grad"]).sum(axis=0)
  assert (np.abs(s1["grad"] - exact) <= 1e-13 * scale).all()
  assert s1["grad"].tobytes() == s2["grad"].tobytes() and s1["dz0"].tobytes() == rows["dz0"].tobytes()
  # a null seed_lam is a zero seed_lam
  a, b = _device(eng, c, seed_lam=None), _device(eng, c, seed_lam=np.zeros_like(c["seed_lam"]))
  for k in ("grad", "dz0", "dlam0"):
    assert a[k].tobytes() == b[k].tobytes()
  # device arrays: the same bits as host arrays, inputs untouched
  dev = "cuda:0"
  t = {k: torch.tensor(c[k], device=dev) for k in ("z", "lam", "lb", "ub", "params", "seed_z", "seed_lam")}
  g = torch.empty((70, eng.np), dtype=torch.float64, device=dev); gs = torch.empty(eng.np, dtype=torch.float64, device=dev)
  dz = torch.empty_like(t["z"]); dl = torch.empty_like(t["lam"])
  eng.exgd_grad_device(70, t["z"], t["lam"], t["lb"], t["ub"], c["eta_x"], c["eta_v"], 4, t["seed_z"], g, eng.np, seed_lam=t["seed_lam"],
                       params=t["params"], params_stride=eng.np, dz0=dz, dlam0=dl)
  eng.exgd_grad_device(70, t["z"], t["lam"], t["lb"], t["ub"], c["eta_x"], c["eta_v"], 4, t["seed_z"], gs, 0, seed_lam=t["seed_lam"],
                       params=t["params"], params_stride=eng.np)
  torch.cuda.synchronize()
  assert g.cpu().numpy().tobytes() == rows["grad"].tobytes() and gs.cpu().numpy().tobytes() == s1["grad"].tobytes()
  assert dz.cpu().numpy().tobytes() == rows["dz0"].tobytes() and dl.cpu().numpy().tobytes() == rows["dlam0"].tobytes()
  assert (t["z"].cpu().numpy() == z_in).all() and (t["lam"].cpu().numpy() == lam_in).all()
  eng.close()
  # chunks of instances (the history bound set low: 70 instances in chunks of 3): the same bits
  per = (4 * (2 * c["n"] + c["m"]) + c["n"]) * 8
  monkeypatch.setenv("MYRIAD_EXGD_GRAD_HIST_BYTES", str(3 * per + 8))
  eng = _engine("CARTPOLE", "HERMITE_SIMPSON", 5, c["T"])
  ch, chs = _device(eng, c), _device(eng, c, reduce=True)
  eng.close()
  for k in ("grad", "dz0", "dlam0"):
    assert ch[k].tobytes() == rows[k].tobytes()
  assert chs["grad"].tobytes() == s1["grad"].tobytes()


@pytest.mark.parametrize("scheme", E.SCHEMES)
def test_inherited_registers_do_not_reach_the_result(monkeypatch, scheme):
  c = shape_case(scheme, 40, 3, 65)
  bits = {}
  for pat in ("zero", "nan", "random"):
    monkeypatch.setenv("MYRIAD_REG_FILL", pat)
    monkeypatch.setenv("MYRIAD_STACK_FILL", pat)
    eng = _engine("CARTPOLE", scheme, 40, c["T"])            # (the handle reads the fill at creation)
    out, red = _device(eng, c), _device(eng, c, reduce=True)
    eng.close()
    assert np.isfinite(out["grad"]).all()
    bits[pat] = out["grad"].tobytes() + out["dz0"].tobytes() + out["dlam0"].tobytes() + red["grad"].tobytes()
  assert bits["zero"] == bits["nan"] == bits["random"]


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors():
  c = shape_case("HERMITE_SIMPSON", 3, 2, 2)
  for name, tr, kw, word in (("CARTPOLE", "SHOOTING", dict(controls_per_interval=5), "SHOOTING"), ("CARTPOLE_ELASTIC", "HERMITE_SIMPSON", {}, "elastic twin"),
                             ("INVASIVEPLANT", "SHOOTING", dict(controls_per_interval=7), "INVASIVEPLANT")):
    eng = _lib.Engine(name, tr, 3, 1.0, **kw)
    with pytest.raises(NotImplementedError, match=word):
      eng.exgd_grad_probe()
    eng.close()
  # (the argument checks of the C call, with their full texts and their order: tests/test_gpu_api.py)
  eng = _engine("CARTPOLE", "HERMITE_SIMPSON", 3, c["T"])
  grad = np.empty((2, 4))
  rc = eng.lib.myr_exgd_grad(eng._h, 2, *(c[k].ctypes.data for k in ("z", "lam", "lb", "ub", "params")), 0, 0.02, 0.02, 2, c["seed_z"].ctypes.data, None,
                             grad.ctypes.data, 4, None, None, _lib.MEM_HOST)
  assert rc == 0
  eng.close()
  eng = _engine("CARTPOLE", "HERMITE_SIMPSON", 400, 2.0)     # (3 n + 2 m + K NS) doubles = 195 KB
  with pytest.raises(_lib.MyriadHipError, match="too large for the LDS"):
    eng.exgd_grad(np.zeros((1, eng.n)), np.zeros((1, eng.m)), -np.ones(eng.n), np.ones(eng.n), 0.01, 0.01, 1, np.zeros((1, eng.n)))
  eng.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def _hp():
  from myriad_amd.config import HParams, OptimizerType, QuadratureRule
  from myriad_amd.systems import SystemType
  return HParams(system=SystemType.VANDERPOL, optimizer=OptimizerType.COLLOCATION, quadrature_rule=QuadratureRule.TRAPEZOIDAL, intervals=5)


def _torch_lookahead(a, x, lam, true_us, epoch, eta_x, eta_v, lb, ub, weights, N, T):
  """dJ/da of the reference's lookahead_update (e2e_sysid.py:209-218) in torch: many_steps_grad's forward-mode recursion (:148-177) on the
  Jacobians of step_x / step_lmbda, contracted with the gradient of simple_imitation_loss at (x, lam)"""
  lo, hi = torch.tensor(lb), torch.tensor(ub)

  def lagr_parts(p):
    _, tr = E._transcription("VANDERPOL", "TRAPEZOIDAL", N, T, [p[0]])
    return lambda xx, ll: tr.objective(xx) + ll @ tr.constraints(xx), tr

  def step_x(xx, ll, p):
    L, _ = lagr_parts(p)
    g = lambda v: torch.autograd.grad(L(v, ll), v, create_graph=True)[0]
    xi = xx * 1.0
    xb = torch.clamp(xi - eta_x * g(xi), lo, hi)
    return torch.clamp(xi - eta_x * g(xb), lo, hi)

  def step_l(xx, ll, p):
    _, tr = lagr_parts(p)
    return ll + eta_v * tr.constraints(xx)

  J = torch.autograd.functional.jacobian
  p = torch.tensor([a], dtype=torch.float64)
  x, lam = torch.tensor(x), torch.tensor(lam)
  zx, zl = torch.zeros(x.numel(), 1, dtype=torch.float64), torch.zeros(lam.numel(), 1, dtype=torch.float64)
  from myriad_amd.experiments.e2e_sysid import NUM_UNROLLED
  x0 = x
  for _ in range(NUM_UNROLLED):
    dx, dl, dp = J(step_x, (x, lam, p))
    zx = dp + dx @ zx + dl @ zl
    x = step_x(x.clone().requires_grad_(True), lam, p).detach()
    dx, dl, dp = J(step_l, (x, lam, p))
    zl = dp + dx @ zx + dl @ zl
    lam = step_l(x, lam, p).detach()
  nu_part = torch.tensor(true_us).numel()
  dJ = torch.zeros(x0.numel(), dtype=torch.float64)
  dJ[-nu_part:] = (2.0 * torch.tensor(weights)[:, None] * (x0[-nu_part:].reshape(true_us.shape) - torch.tensor(true_us))).reshape(-1)
  return float(dJ @ zx[:, 0])


def test_driver_follows_the_reference_loop():
  from myriad_amd.config import Config
  from myriad_amd.experiments import e2e_sysid
  from myriad_amd.experiments.mle_sysid import Adam
  hp, cfg = _hp(), Config(verbose=False, plot=False)
  res = e2e_sysid.run_endtoend(hp, cfg, num_epochs=3)
  assert set(res["params"]) == {"a"} and res["ts"] == [0, 1, 2] and sorted(res["saved_params"]) == [0, 3]
  # the same three epochs on the oracle: steps by Lagrangian.step, gradient by the forward-mode recursion, the driver's Adam
  sysm = E.O.SYSTEMS["VANDERPOL"]()
  T, N = float(sysm.T), 5
  tr = E.O.make_transcription(sysm, "COLLOCATION", N, quadrature_rule="TRAPEZOIDAL")
  lb, ub = tr.bounds[:, 0].copy(), tr.bounds[:, 1].copy()
  x, lam = tr.guess.copy(), np.zeros(N * sysm.ns)
  a, opt = 0.5, Adam(hp.adam_lr)
  for epoch in range(3):
    _, trp = E._transcription("VANDERPOL", "TRAPEZOIDAL", N, T, [a])
    trp.bounds = tr.bounds
    lagr = E.O.Lagrangian(trp)
    for _ in range(e2e_sysid.NUM_UNROLLED):
      x, lam = lagr.step(x, lam, hp.eta_x, hp.eta_lmbda)
    w = e2e_sysid.imitation_weights(hp, N + 1, sysm.nu, epoch)
    g = _torch_lookahead(a, x, lam, res["true_opt_us"], epoch, hp.eta_x, hp.eta_lmbda, lb, ub, w, N, T)
    a = opt.update({"a": a}, {"a": g})["a"]
  print("driver", res["params"]["a"], "oracle", a)
  assert abs(res["params"]["a"] - a) <= 1e-8
  assert abs(res["params"]["a"] - 0.5) > 1e-4


def test_batched_gradient_is_the_mean_of_the_single_ones():
  from myriad_amd.config import Config
  from myriad_amd.experiments import e2e_sysid
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp, cfg = _hp(), Config(verbose=False, plot=False)
  opt = get_optimizer(hp, cfg, hp.system())
  x0s = np.array([[0.0, 1.0], [0.3, 0.8]])
  z, lb, ub = opt.batch_inputs(x0s, opt.system.device_params())
  rng = np.random.default_rng(5)
  lam = 0.1 * rng.standard_normal((2, opt.engine.m))
  true_us = rng.uniform(-0.5, 0.5, (2,) + opt._u_shape)
  both = e2e_sysid.lookahead_gradient(opt, {"a": 0.5}, z, lam, true_us, 0, lb, ub, hp.eta_x, hp.eta_lmbda)
  one = [e2e_sysid.lookahead_gradient(opt, {"a": 0.5}, z[b:b + 1], lam[b:b + 1], true_us[b:b + 1], 0, lb[b:b + 1], ub[b:b + 1], hp.eta_x, hp.eta_lmbda)
         for b in range(2)]
  mean = 0.5 * (one[0]["a"] + one[1]["a"])
  assert one[0]["a"] != one[1]["a"] and abs(both["a"] - mean) <= 1e-13 * (abs(one[0]["a"]) + abs(one[1]["a"]))
  res = e2e_sysid.run_endtoend(hp, cfg, num_epochs=2, start_states=x0s)
  assert res["true_opt_us"].shape == (2,) + opt._u_shape and np.isfinite(res["params"]["a"])


def test_default_hyperparameters_are_refused_by_the_library():
  from myriad_amd.config import Config, HParams
  from myriad_amd.experiments import e2e_sysid
  from myriad_amd.systems import SystemType
  with pytest.raises(NotImplementedError, match="SHOOTING"):
    e2e_sysid.run_endtoend(HParams(system=SystemType.VANDERPOL), Config(verbose=False, plot=False), num_epochs=1)
