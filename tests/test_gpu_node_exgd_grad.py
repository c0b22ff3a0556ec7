"""myr_exgd_grad_node on the device (myriad_amd/csrc/node_exgd_grad.h: node_exgd_grad_kernel) against the oracle, its host twin, central
differences of myr_exgd (the per-lane network code: an independent implementation), and itself across the forms of the call; the driver
(myriad_amd/experiments/node_e2e_sysid.py) against a restatement of its loop made of the engine calls.

Cases (N, nsteps, B) of tests/node_exgd_grad_cases.py, Hermite-Simpson, the committed weights.  Tolerances: 100 x the largest rel_error of grad,
dz0 and dlam0 measured on an MI355X with the cases as they stand (profiles/r18_node_exgd_grad/README.md); a row is a sum of a few thousand fp64
products, so a figure above 1e-11 would be a bug.
"""
import numpy as np
import pytest
import torch

import node_exgd_grad_cases as E
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

ORACLE_MEASURED = 3.9e-15      # device against torch, the largest over the cases: (7, 2, 3); the others 4.3e-16 ... 3.6e-15
TWIN_MEASURED = 5.7e-15        # device against the host twin, the same case; the others 3.8e-16 ... 1.3e-15.  The same for 1, 2 and 4 wavefronts
ORACLE_TOL = 100.0 * ORACLE_MEASURED
TWIN_TOL = 100.0 * TWIN_MEASURED
KEYS = ("grad", "dz0", "dlam0")


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return E.build_twin(tmp_path_factory.mktemp("node_exgd_grad_twin_gpu"))


def _engine(N, T, scheme="HERMITE_SIMPSON"):
  return _lib.Engine("NODE_CARTPOLE", scheme, N, T)


def _device(eng, c, **kw):
  a = dict(z=c["z"], lam=c["lam"], lb=c["lb"], ub=c["ub"], eta_x=c["eta_x"], eta_v=c["eta_v"], nsteps=c["nsteps"], seed_z=c["seed_z"],
           seed_lam=c["seed_lam"], params=c["params"])
  a.update(kw)
  return eng.exgd_grad_node(**a)


def _errs(out, ref):
  return tuple(E.rel_error(out[k], r) for k, r in zip(KEYS, ref))


def _same(a, b, keys=KEYS):
  return all(a[k].tobytes() == b[k].tobytes() for k in keys)


# ---- parity with the oracle and the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nsteps,batch", E.CASES + (E.CHUNKED,))
def test_parity_with_the_oracle_and_the_twin(twin, monkeypatch, N, nsteps, batch):
  case, *ref = E.reference(N, nsteps, batch)
  if (N, nsteps, batch) == E.CHUNKED:
    monkeypatch.setenv("MYRIAD_EXGD_GRAD_HIST_BYTES", str(E.CHUNKED_HIST_BYTES))      # one instance's history is 3 896 bytes: chunks of one
  eng = _engine(N, case["T"])
  z_in, lam_in = case["z"].copy(), case["lam"].copy()
  out = _device(eng, case)
  eng.close()
  assert (case["z"] == z_in).all() and (case["lam"] == lam_in).all()
  tw = E.twin_of_case(twin, case)
  if nsteps == 0:
    assert (out["grad"] == 0.0).all() and (out["dz0"] == case["seed_z"]).all() and (out["dlam0"] == case["seed_lam"]).all()
    return
  eo, et = _errs(out, ref), _errs(out, tw)
  print(f"NODE N={N} nsteps={nsteps} B={batch}: device-oracle {max(eo):.2e} device-twin {max(et):.2e}")
  assert max(eo) <= ORACLE_TOL, eo
  assert max(et) <= TWIN_TOL, et


# ---- independent of the oracle and the twin ------------------------------------------------------------------------------------------
def test_central_differences_of_myr_exgd():
  """seed . (z_n(p + d) - z_n(p - d)) / 2 from two myr_exgd calls per direction, d = 1e-6 |p| o r with r uniform in [-1, 1] -- the step of
  test_gpu_exgd_grad.test_central_differences_of_myr_exgd in every entry at once --, against grad . (|p| o r), to its rtol of 1e-6.  Inputs as
  that test's shape_case: a third of the variables in a box of 1e-3 that the steps leave, the first state pinned."""
  N, nsteps = 5, 3
  K, n, m = E.dims(N)
  rng = np.random.default_rng(11)
  z = np.concatenate([0.5 * rng.standard_normal(K * 4), rng.uniform(-5.0, 5.0, K)])[None]
  box = rng.random((1, n)) < 0.3
  lb, ub = np.where(box, z - 1e-3, -np.inf), np.where(box, z + 1e-3, np.inf)
  lb[:, :4] = z[:, :4]; ub[:, :4] = z[:, :4]
  lam, seed_z = 0.1 * rng.standard_normal((1, m)), rng.standard_normal((1, n))
  p = E.weights()[1]
  eta_x, eta_v = 0.5, 0.5
  eng = _engine(N, 0.1 * N)
  grad = eng.exgd_grad_node(z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, p, want_start=False)["grad"][0]
  for _ in range(3):
    delta = np.abs(p) * rng.uniform(-1.0, 1.0, p.size)
    zs = [eng.exgd(z, lam, lb, ub, eta_x, eta_v, nsteps, params=p + sgn * 1e-6 * delta)[0][0] for sgn in (1.0, -1.0)]
    fd = float(seed_z[0] @ (zs[0] - zs[1])) / 2e-6
    print("grad . delta", float(grad @ delta), "central differences", fd)
    np.testing.assert_allclose(float(grad @ delta), fd, rtol=1e-6)
  eng.close()


# ---- forms of the call -----------------------------------------------------------------------------------------------------------------
def test_forms_of_the_call(monkeypatch):
  from fractions import Fraction
  c, *_ = E.reference(*E.CHUNKED)
  B = c["z"].shape[0]
  eng = _engine(c["N"], c["T"])
  rows, again = _device(eng, c), _device(eng, c)
  assert _same(rows, again)                                                       # two calls: the same bits
  s1, s2 = _device(eng, c, reduce=True), _device(eng, c, reduce=True)             # rows against grad_stride == 0
  exact = np.array([float(sum(Fraction(float(v)) for v in rows["grad"][:, k])) for k in range(eng.np)])
  assert (np.abs(s1["grad"] - exact) <= 1e-13 * np.abs(rows["grad"]).sum(axis=0)).all()
  assert s1["grad"].tobytes() == s2["grad"].tobytes() and s1["dz0"].tobytes() == rows["dz0"].tobytes()
  a, b = _device(eng, c, seed_lam=None), _device(eng, c, seed_lam=np.zeros_like(c["seed_lam"]))      # a null seed_lam is a zero seed_lam
  assert _same(a, b)
  nostart = _device(eng, c, want_start=False)                                     # dz0, dlam0 null
  assert set(nostart) == {"grad"} and nostart["grad"].tobytes() == rows["grad"].tobytes()
  # device arrays: the same bits as host arrays, inputs untouched
  dev = "cuda:0"
  t = {k: torch.tensor(np.array(c[k]), device=dev) for k in ("z", "lam", "lb", "ub", "params", "seed_z", "seed_lam")}
  g = torch.empty((B, eng.np), dtype=torch.float64, device=dev); gs = torch.empty(eng.np, dtype=torch.float64, device=dev)
  dz = torch.empty_like(t["z"]); dl = torch.empty_like(t["lam"])
  eng.exgd_grad_node_device(B, t["z"], t["lam"], t["lb"], t["ub"], c["eta_x"], c["eta_v"], c["nsteps"], t["seed_z"], g, eng.np, t["params"],
                            seed_lam=t["seed_lam"], dz0=dz, dlam0=dl)
  eng.exgd_grad_node_device(B, t["z"], t["lam"], t["lb"], t["ub"], c["eta_x"], c["eta_v"], c["nsteps"], t["seed_z"], gs, 0, t["params"],
                            seed_lam=t["seed_lam"])
  torch.cuda.synchronize()
  assert g.cpu().numpy().tobytes() == rows["grad"].tobytes() and gs.cpu().numpy().tobytes() == s1["grad"].tobytes()
  assert dz.cpu().numpy().tobytes() == rows["dz0"].tobytes() and dl.cpu().numpy().tobytes() == rows["dlam0"].tobytes()
  assert (t["z"].cpu().numpy() == c["z"]).all() and (t["lam"].cpu().numpy() == c["lam"]).all()
  eng.close()
  # the chunked path (a 4 KB history bound: chunks of one instance) against the unchunked: the same bits
  monkeypatch.setenv("MYRIAD_EXGD_GRAD_HIST_BYTES", str(E.CHUNKED_HIST_BYTES))
  eng = _engine(c["N"], c["T"])
  ch, chs = _device(eng, c), _device(eng, c, reduce=True)
  eng.close()
  assert _same(ch, rows) and chs["grad"].tobytes() == s1["grad"].tobytes()


def test_inherited_registers_do_not_reach_the_result(monkeypatch):
  c, *_ = E.reference(33, 2, 1)
  bits = {}
  for pat in ("zero", "nan", "random"):
    monkeypatch.setenv("MYRIAD_REG_FILL", pat)
    monkeypatch.setenv("MYRIAD_STACK_FILL", pat)
    eng = _engine(c["N"], c["T"])                              # (the handle reads the fill at creation)
    out, red = _device(eng, c), _device(eng, c, reduce=True)
    eng.close()
    assert np.isfinite(out["grad"]).all()
    bits[pat] = out["grad"].tobytes() + out["dz0"].tobytes() + out["dlam0"].tobytes() + red["grad"].tobytes()
  assert bits["zero"] == bits["nan"] == bits["random"]


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors():
  c, *_ = E.reference(3, 3, 2)
  p = np.array(c["params"])
  grad = np.empty((2, 4804))
  ptr = {k: c[k].ctypes.data for k in ("z", "lam", "lb", "ub", "seed_z")}
  ptr.update(params=p.ctypes.data, grad=grad.ctypes.data)

  def call(eng, B=2, nsteps=3, grad_stride=4804, mem=_lib.MEM_HOST, **null):
    a = dict(ptr); a.update(null)
    return eng.lib.myr_exgd_grad_node(eng._h, B, a["z"], a["lam"], a["lb"], a["ub"], a["params"], c["eta_x"], c["eta_v"], nsteps, a["seed_z"], None,
                                      a["grad"], grad_stride, None, None, mem)

  # (the argument checks of the C call, with their full texts and their order: tests/test_gpu_api.py)
  eng = _engine(3, c["T"])
  assert call(eng) == 0
  assert call(eng, B=0) == 0
  eng.close()
  eng = _engine(400, 2.0)                                          # (5 064 + 54 N + 19) doubles = 213 KB
  with pytest.raises(_lib.MyriadHipError, match="too large for the LDS"):
    eng.exgd_grad_node(np.zeros((1, eng.n)), np.zeros((1, eng.m)), -np.ones(eng.n), np.ones(eng.n), 0.01, 0.01, 1, np.zeros((1, eng.n)), p)
  eng.close()


# ---- the optimizer's method and the driver ---------------------------------------------------------------------------------------------
def _hp(**kw):
  from myriad_amd.config import HParams, OptimizerType, QuadratureRule
  from myriad_amd.systems import SystemType
  return HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.COLLOCATION, quadrature_rule=QuadratureRule.HERMITE_SIMPSON, intervals=5,
                 num_unrolled=2, **kw)


def test_unrolled_grad_returns_the_mapping_of_the_flat_row():
  from myriad_amd.config import Config
  from myriad_amd.systems.neural_ode import NeuralODE, NodeSystem, flat_from_mapping
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp = _hp()
  node = NeuralODE.load_fitted_cartpole()
  opt = get_optimizer(hp, Config(verbose=False, plot=False), NodeSystem(node, hp.system()))
  rng = np.random.default_rng(3)
  lam, seed = 0.1 * rng.standard_normal(opt.engine.m), rng.standard_normal(opt.engine.n)
  g = opt.unrolled_grad(opt.guess, lam, node.params, seed, 2)
  ex, ev = opt.step_sizes()
  row = opt.engine.exgd_grad_node(opt.guess, lam, opt.bounds[:, 0], opt.bounds[:, 1], ex, ev, 2, seed, flat_from_mapping(node.params),
                                  want_start=False)["grad"][0]
  assert set(g) == {"linear", "linear_1", "linear_2"} and g["linear_1"]["w"].shape == (64, 64)
  assert flat_from_mapping(g).tobytes() == row.tobytes() and np.abs(row).max() > 0


def test_driver_follows_the_reference_loop():
  """two epochs of run_node_endtoend (N = 5, num_unrolled = 2) against the same loop made of the engine calls and the driver's Adam"""
  from myriad_amd.config import Config
  from myriad_amd.experiments import node_e2e_sysid as D
  from myriad_amd.experiments.mle_sysid import Adam
  from myriad_amd.systems.neural_ode import NeuralODE, NodeSystem, flat_from_mapping
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp, cfg = _hp(), Config(verbose=False, plot=False)
  res = D.run_node_endtoend(hp, cfg, num_epochs=2, node=NeuralODE.load_fitted_cartpole())
  assert res["ts"] == [0, 1] and sorted(res["saved_params"]) == [0, 2] and len(res["imitation_losses"]) == 2
  node = NeuralODE.load_fitted_cartpole()
  true_opt = get_optimizer(hp, cfg, hp.system())
  eng = get_optimizer(hp, cfg, NodeSystem(node, hp.system())).engine
  true_us = true_opt.solve()["u"]
  assert (true_us == res["true_opt_us"]).all()
  lb, ub = true_opt.bounds[:, 0], true_opt.bounds[:, 1]
  eta_x, eta_v = true_opt.step_sizes()
  x, lam, flat, adam = np.array(true_opt.guess, dtype=np.float64), np.zeros(eng.m), flat_from_mapping(node.params), Adam(1e-4)
  K = 2 * 5 + 1
  for epoch in range(2):
    z, l = eng.exgd(x, lam, lb, ub, eta_x, eta_v, 2, params=flat)
    x, lam = z[0], l[0]
    seed = np.zeros(eng.n)
    seed[-K:] = 2.0 * (x[-K:] - true_us.ravel()) / K              # no discount: weights 1 / (rows nu)
    g = eng.exgd_grad_node(x, lam, lb, ub, eta_x, eta_v, 2, seed, flat, reduce=True, want_start=False)["grad"]
    flat = adam.update({"w": flat}, {"w": g})["w"]
  got = flat_from_mapping(res["params"])
  assert np.abs(got - flat).max() <= 1e-12
  assert np.abs(got - flat_from_mapping(node.params)).max() > 1e-5      # Adam's first steps are lr-sized: the weights moved
