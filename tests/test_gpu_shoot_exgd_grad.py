"""myr_exgd_grad_shoot on the device (myriad_amd/csrc/shoot_exgd_grad.h: shoot_exgd_grad_pair_kernel, shoot_exgd_grad_mask_kernel) against its
host twin, the oracle, a composition of the existing entry points, central differences of myr_exgd, and itself across the forms of the call; the
end-to-end driver's SHOOTING route (run_endtoend(..., shooting=True)) against a torch restatement of the reference's forward-mode many_steps_grad +
lookahead_update.

Tolerances (profiles/r20_shoot_exgd_grad/README.md; the figures are the largest |d| / max|row| over grad, dz0 and dlam0, measured on an MI355X with
the cases as they stand):
  device against twin     parity cases (3 x 2, nsteps = 3): 10 x 2.2e-15 (VANDERPOL Heun; the others 1.7e-16 ... 1.5e-15)
                          shape cases: 10 x 1.3e-15 (1 x 4 RK4, B = 130; the others 1.9e-16 ... 9.0e-16)
                          The two run the same pair algebra and differ by the compiler's FMA contraction.
  device against oracle   1e-11, the project's ORACLE_TOL (measured 7.1e-15 at worst, ROCKETLANDING RK4)
  device against the composition of myr_exgd / myr_vjp / myr_hvp / myr_jvp (dz0, dlam0): 10 x 1.7e-16 (RK4 dz0; Heun 1.4e-16): the composition
                          runs the device's own pair algebra through myr_hvp, so the two differ only where the sums are taken in another order
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import hvp_cases as H
import shoot_exgd_grad_cases as S
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

PARITY_TWIN_MEASURED = 2.2e-15  # the parity cases (3 x 2, nsteps = 3, B = 3): VANDERPOL Heun, the largest
SHAPE_TWIN_MEASURED = 1.3e-15   # the shape cases: 1 x 4 RK4, nsteps <= 10, B = 130
COMPOSITION_MEASURED = 1.72e-16 # CARTPOLE 4 x 3 RK4, nsteps = 3, B = 2: dz0
PARITY_TWIN_TOL = 10.0 * PARITY_TWIN_MEASURED
SHAPE_TWIN_TOL = 10.0 * SHAPE_TWIN_MEASURED
COMPOSITION_TOL = 10.0 * COMPOSITION_MEASURED
ORACLE_TOL = 1e-11
PARITY = ("CARTPOLE", "VANDERPOL", "CANCERTREATMENT", "BACTERIA", "PREDATORPREY", "BEARPOPULATIONS", "ROCKETLANDING")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return S.build_twin(tmp_path_factory.mktemp("shoot_exgd_grad_twin_gpu"))


def _engine(c, name=None):
  return _lib.Engine(name or c["name"], "SHOOTING", c["I"], c["T"], controls_per_interval=c["cpi"], integration_method=c["method"])


def _device(eng, c, **kw):
  a = dict(z=c["z"], lam=c["lam"], lb=c["lb"], ub=c["ub"], eta_x=c["eta_x"], eta_v=c["eta_v"], nsteps=c["nsteps"], seed_z=c["seed_z"],
           seed_lam=c["seed_lam"], params=c["params"])
  a.update(kw)
  return eng.exgd_grad_shoot(**a)


def _errs(out, ref):
  return tuple(S.rel_error(out[k], r) for k, r in zip(("grad", "dz0", "dlam0"), ref))


# ---- parity with the oracle and the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("HEUN", "RK4"))
@pytest.mark.parametrize("name", PARITY)
def test_parity_with_the_oracle_and_the_twin(twin, name, method):
  case, *ref = S.reference(name, 3, 2, method, 3, 3)
  eng = _engine(case)
  out = _device(eng, case)
  eng.close()
  tw = S.twin_of_case(twin, case)
  eo, et = _errs(out, ref), _errs(out, tw)
  print(f"{name} {method}: device-oracle {max(eo):.2e} device-twin {max(et):.2e}")
  assert max(et) <= PARITY_TWIN_TOL, et
  assert max(eo) <= ORACLE_TOL, eo


# ---- awkward shapes against the twin -------------------------------------------------------------------------------------------------
# 1 x 4: one pair per instance, no control row shared by two intervals, B = 130: three wavefronts of pairs, 62 idle lanes; 65 x 1 at B = 1: an instance
# across two wavefronts; 2 x 3; 64 x 2 at B = 2: two full wavefronts; 3 x 2 under every integrator
SHAPES = [(1, 4, m, 130) for m in ("HEUN", "RK4")] + [(65, 1, m, 1) for m in ("HEUN", "RK4")] + [(2, 3, m, 5) for m in ("HEUN", "RK4")] + \
         [(64, 2, m, 2) for m in ("HEUN", "RK4")] + [(3, 2, m, 3) for m in S.METHODS]


@pytest.mark.parametrize("I,cpi,method,B", SHAPES)
def test_awkward_shapes_against_the_twin(twin, I, cpi, method, B):
  worst = 0.0
  eng = None
  for nsteps in (0, 1, 10):
    c = S.shape_case(I, cpi, method, nsteps, B)
    eng = eng or _engine(c)
    out = _device(eng, c)
    tw = S.twin_of_case(twin, c)
    et = _errs(out, tw)
    worst = max(worst, *et)
    assert max(et) <= SHAPE_TWIN_TOL, (nsteps, et)
    if nsteps == 0:
      assert (out["grad"] == 0.0).all() and (out["dz0"] == c["seed_z"]).all() and (out["dlam0"] == c["seed_lam"]).all()
    else:
      assert np.abs(out["grad"]).max() > 0
  eng.close()
  print(f"{I}x{cpi} {method} B={B}: device-twin {worst:.2e}")


# ---- independent of the oracle and the twin ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("RK4", "HEUN"))
def test_composition_from_existing_entry_points(method):
  """dz0 and dlam0 in numpy from myr_exgd one step at a time (the history), myr_vjp (x_bar; J^T a_lam), myr_hvp, myr_jvp and the masks: items 1 .. 5"""
  c = S.shape_case(4, 3, method, 3, 2)
  eng = _engine(c)
  out = _device(eng, c)
  ex, ev, lb, ub, p = c["eta_x"], c["eta_v"], c["lb"], c["ub"], c["params"]
  inside = lambda x: (x > lb) & (x < ub)
  xs, lams, xbars = [c["z"]], [c["lam"]], []
  for _ in range(3):
    xbars.append(np.clip(xs[-1] - ex * eng.vjp(xs[-1], lams[-1], params=p, add_gradf=True), lb, ub))
    x, lam = eng.exgd(xs[-1], lams[-1], lb, ub, ex, ev, 1, params=p)
    xs.append(x); lams.append(lam)
  ax, al = c["seed_z"].copy(), c["seed_lam"].copy()
  for s in (2, 1, 0):
    ax = ax + ev * eng.vjp(xs[s + 1], al, params=p, add_gradf=False)                    # 1
    m2 = np.where(inside(xs[s + 1]), ax, 0.0); ax = m2; t = -ex * m2                    # 2
    r = eng.hvp(xbars[s], lams[s], t, params=p)["hz"]; al = al + eng.jvp(xbars[s], t, params=p)      # 3
    m1 = np.where(inside(xbars[s]), r, 0.0); ax = ax + m1; d = -ex * m1                 # 4
    ax = ax + eng.hvp(xs[s], lams[s], d, params=p)["hz"]; al = al + eng.jvp(xs[s], d, params=p)      # 5
  eng.close()
  e = (S.rel_error(out["dz0"], ax), S.rel_error(out["dlam0"], al))
  print(f"{method}: device against the composition: dz0 {e[0]:.2e} dlam0 {e[1]:.2e}")
  assert np.abs(ax).max() > 0 and np.abs(al).max() > 0
  assert max(e) <= COMPOSITION_TOL, e


def test_central_differences_of_myr_exgd():
  """seed . (z_n(p + d) - z_n(p - d)) / 2 d from two myr_exgd calls per parameter, d = 1e-6 |p|, against grad"""
  c = S.shape_case(4, 5, "RK4", 10, 1)
  p0 = c["params"][0]
  eng = _engine(c)
  out = _device(eng, c, seed_lam=None, params=p0)
  fd = np.empty(p0.size)
  for k in range(fd.size):
    d = 1e-6 * abs(p0[k])
    zs = []
    for sgn in (1.0, -1.0):
      p = p0.copy(); p[k] += sgn * d
      zs.append(eng.exgd(c["z"], c["lam"], c["lb"], c["ub"], c["eta_x"], c["eta_v"], 10, params=p)[0])
    fd[k] = float(c["seed_z"][0] @ (zs[0][0] - zs[1][0])) / (2.0 * d)
  eng.close()
  print("grad", out["grad"][0], "central differences", fd)
  np.testing.assert_allclose(out["grad"][0], fd, rtol=1e-6)


# ---- forms of the call -----------------------------------------------------------------------------------------------------------------
def test_forms_of_the_call(monkeypatch):
  B = 70
  c = S.shape_case(4, 3, "RK4", 4, B)
  eng = _engine(c)
  z_in, lam_in = c["z"].copy(), c["lam"].copy()
  rows = _device(eng, c)
  assert (c["z"] == z_in).all() and (c["lam"] == lam_in).all()
  # shared parameters = the same row for every instance
  shared = _device(eng, c, params=c["params"][0])
  tiled = _device(eng, c, params=np.tile(c["params"][0], (B, 1)))
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
  g = torch.empty((B, eng.np), dtype=torch.float64, device=dev); gs = torch.empty(eng.np, dtype=torch.float64, device=dev)
  dz = torch.empty_like(t["z"]); dl = torch.empty_like(t["lam"])
  eng.exgd_grad_shoot_device(B, t["z"], t["lam"], t["lb"], t["ub"], c["eta_x"], c["eta_v"], 4, t["seed_z"], g, eng.np, seed_lam=t["seed_lam"],
                             params=t["params"], params_stride=eng.np, dz0=dz, dlam0=dl)
  eng.exgd_grad_shoot_device(B, t["z"], t["lam"], t["lb"], t["ub"], c["eta_x"], c["eta_v"], 4, t["seed_z"], gs, 0, seed_lam=t["seed_lam"],
                             params=t["params"], params_stride=eng.np)
  torch.cuda.synchronize()
  assert g.cpu().numpy().tobytes() == rows["grad"].tobytes() and gs.cpu().numpy().tobytes() == s1["grad"].tobytes()
  assert dz.cpu().numpy().tobytes() == rows["dz0"].tobytes() and dl.cpu().numpy().tobytes() == rows["dlam0"].tobytes()
  assert (t["z"].cpu().numpy() == z_in).all() and (t["lam"].cpu().numpy() == lam_in).all()
  eng.close()
  # chunks of instances (the history bound set low: 70 instances in chunks of 3): the same bits
  per = (4 * (2 * c["n"] + c["m"]) + c["n"]) * 8
  monkeypatch.setenv("MYRIAD_EXGD_GRAD_HIST_BYTES", str(3 * per + 8))
  eng = _engine(c)
  ch, chs = _device(eng, c), _device(eng, c, reduce=True)
  eng.close()
  for k in ("grad", "dz0", "dlam0"):
    assert ch[k].tobytes() == rows[k].tobytes()
  assert chs["grad"].tobytes() == s1["grad"].tobytes()


@pytest.mark.parametrize("name", ("CARTPOLE", "ROCKETLANDING"))
def test_inherited_registers_do_not_reach_the_result(monkeypatch, name):
  c = S.shape_case(4, 3, "RK4", 3, 65, name=name)
  bits = {}
  for pat in ("zero", "nan", "random"):
    monkeypatch.setenv("MYRIAD_REG_FILL", pat)
    monkeypatch.setenv("MYRIAD_STACK_FILL", pat)
    eng = _engine(c)                                           # (the handle reads the fill at creation)
    out, red = _device(eng, c), _device(eng, c, reduce=True)
    eng.close()
    assert np.isfinite(out["grad"]).all() and np.abs(out["grad"]).max() > 0
    bits[pat] = out["grad"].tobytes() + out["dz0"].tobytes() + out["dlam0"].tobytes() + red["grad"].tobytes()
  assert bits["zero"] == bits["nan"] == bits["random"]


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors():
  c = S.shape_case(3, 2, "HEUN", 2, 2)
  for name, tr, kw, word in (("CARTPOLE", "HERMITE_SIMPSON", {}, "use myr_exgd_grad"), ("CARTPOLE", "TRAPEZOIDAL", {}, "use myr_exgd_grad"),
                             ("CARTPOLE_ELASTIC", "HERMITE_SIMPSON", {}, "elastic twin"),
                             ("INVASIVEPLANT", "SHOOTING", dict(controls_per_interval=7), "INVASIVEPLANT")):
    eng = _lib.Engine(name, tr, 3, 1.0, **kw)
    with pytest.raises(NotImplementedError, match=word):
      eng.exgd_grad_shoot_probe()
    eng.close()
  # (the argument checks of the C call, with their full texts and their order: tests/test_gpu_api.py)
  eng = _engine(c)
  eng.exgd_grad_shoot_probe()
  grad = np.empty((2, 4))
  rc = eng.lib.myr_exgd_grad_shoot(eng._h, 2, *(c[k].ctypes.data for k in ("z", "lam", "lb", "ub", "params")), 0, 0.02, 0.02, 2, c["seed_z"].ctypes.data,
                                   None, grad.ctypes.data, 4, None, None, _lib.MEM_HOST)
  assert rc == 0
  # myr_exgd_grad keeps its refusal of SHOOTING
  with pytest.raises(NotImplementedError, match="SHOOTING is not built"):
    eng.exgd_grad_probe()
  eng.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def _hp():
  from myriad_amd.config import HParams, IntegrationMethod, OptimizerType
  from myriad_amd.systems import SystemType
  return HParams(system=SystemType.VANDERPOL, optimizer=OptimizerType.SHOOTING, integration_method=IntegrationMethod.HEUN, intervals=3,
                 controls_per_interval=2)


def _torch_lookahead(a, x, lam, true_us, eta_x, eta_v, lb, ub, weights, I, cpi, method, T, nsteps):
  """dJ/da of the reference's lookahead_update (e2e_sysid.py:209-218) in torch over the shooting transcription: many_steps_grad's forward-mode
  recursion (:148-177) on the Jacobians of step_x / step_lmbda, contracted with the gradient of simple_imitation_loss at (x, lam)"""
  lo, hi = torch.tensor(lb), torch.tensor(ub)
  tr_of = lambda p: H._transcription("VANDERPOL", "SHOOTING", I, cpi, method, T, [p[0]])[1]

  def step_x(xx, ll, p):
    tr = tr_of(p)
    L = lambda v: tr.objective(v) + ll @ tr.constraints(v)
    g = lambda v: torch.autograd.grad(L(v), v, create_graph=True)[0]
    xi = xx * 1.0
    xb = torch.clamp(xi - eta_x * g(xi), lo, hi)
    return torch.clamp(xi - eta_x * g(xb), lo, hi)

  def step_l(xx, ll, p):
    return ll + eta_v * tr_of(p).constraints(xx)

  J = torch.autograd.functional.jacobian
  p = torch.tensor([a], dtype=torch.float64)
  x, lam = torch.tensor(x), torch.tensor(lam)
  zx, zl = torch.zeros(x.numel(), 1, dtype=torch.float64), torch.zeros(lam.numel(), 1, dtype=torch.float64)
  x0 = x
  for _ in range(nsteps):
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


def test_driver_follows_the_reference_loop_under_shooting():
  from myriad_amd.config import Config
  from myriad_amd.experiments import e2e_sysid
  from myriad_amd.experiments.mle_sysid import Adam
  hp, cfg = _hp(), Config(verbose=False, plot=False)
  with pytest.raises(NotImplementedError, match="SHOOTING"):      # the route is opt-in
    e2e_sysid.run_endtoend(hp, cfg, num_epochs=1)
  res = e2e_sysid.run_endtoend(hp, cfg, num_epochs=3, shooting=True)
  assert set(res["params"]) == {"a"} and res["ts"] == [0, 1, 2] and sorted(res["saved_params"]) == [0, 3]
  # the same three epochs on the oracle: steps by Lagrangian.step, gradient by the forward-mode recursion, the driver's Adam
  sysm = S.O.SYSTEMS["VANDERPOL"]()
  T, I, cpi = float(sysm.T), 3, 2
  tr = S.O.make_transcription(sysm, "SHOOTING", I, cpi, integration_method="HEUN")
  lb, ub = tr.bounds[:, 0].copy(), tr.bounds[:, 1].copy()
  x, lam = tr.guess.copy(), np.zeros(I * sysm.ns)
  a, opt = 0.5, Adam(hp.adam_lr)
  for epoch in range(3):
    trp = H._transcription("VANDERPOL", "SHOOTING", I, cpi, "HEUN", T, [a])[1]
    trp.bounds = tr.bounds
    lagr = S.O.Lagrangian(trp)
    for _ in range(e2e_sysid.NUM_UNROLLED):
      x, lam = lagr.step(x, lam, hp.eta_x, hp.eta_lmbda)
    w = e2e_sysid.imitation_weights(hp, I * cpi + 1, sysm.nu, epoch)
    g = _torch_lookahead(a, x, lam, res["true_opt_us"], hp.eta_x, hp.eta_lmbda, lb, ub, w, I, cpi, "HEUN", T, e2e_sysid.NUM_UNROLLED)
    a = opt.update({"a": a}, {"a": g})["a"]
  print("driver", res["params"]["a"], "oracle", a)
  assert abs(res["params"]["a"] - a) <= 1e-8
  assert abs(res["params"]["a"] - 0.5) > 1e-4


def test_unrolled_grad_goes_through_the_shooting_call():
  from myriad_amd.config import Config
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp, cfg = _hp(), Config(verbose=False, plot=False)
  opt = get_optimizer(hp, cfg, hp.system())
  rng = np.random.default_rng(3)
  z = opt.guess + 0.05 * rng.standard_normal(opt.guess.size)
  lam = 0.1 * rng.standard_normal(opt.engine.m)
  seed = rng.standard_normal(opt.guess.size)
  ex, ev = opt.step_sizes()
  g = opt.unrolled_grad(z, lam, {"a": 0.7}, seed, 4)
  ref = opt.engine.exgd_grad_shoot(z, lam, opt.bounds[:, 0], opt.bounds[:, 1], ex, ev, 4, seed, params=np.array([0.7]), want_start=False)["grad"][0]
  assert g.tobytes() == ref.tobytes() and np.abs(g).max() > 0
