"""myr_exgd_grad_node_shoot on the device (myriad_amd/csrc/node_shoot_exgd_grad.h: node_shoot_exgd_grad_kernel) against the oracle, its host twin,
central differences of myr_exgd on the same handle (K14's matrix-core passes: an independent implementation), and itself across the forms of
the call; TrajectoryOptimizer.unrolled_grad and the driver (myriad_amd/experiments/node_e2e_sysid.py, shooting=True) against a restatement of
its loop made of the engine calls.

Cases (I, cpi, method, nsteps, B) of tests/node_shoot_exgd_grad_cases.py, the committed weights.  Tolerances: 100 x the largest rel_error of
grad, dz0 and dlam0 measured on an MI355X with the cases as they stand (profiles/r22_node_shoot_exgd_grad/README.md); a row is a sum of a few
thousand fp64 products, so a figure above 1e-11 would be a bug.
"""
import numpy as np
import pytest
import torch

import node_shoot_exgd_grad_cases as E
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

ORACLE_MEASURED = 4.3e-15      # device against torch, the largest over the cases: (1, 12, MIDPOINT, 2, 1); the others 5.1e-16 ... 4.2e-15
TWIN_MEASURED = 1.3e-14        # device against the host twin: all 37 instances of (4, 3, HEUN, 2, 37); the others 2.9e-16 ... 3.9e-15
ORACLE_TOL = 100.0 * ORACLE_MEASURED
TWIN_TOL = 100.0 * TWIN_MEASURED
KEYS = ("grad", "dz0", "dlam0")
ALL = E.CASES + (E.CHUNKED,)
IDS = ["-".join(map(str, c)) for c in ALL]
BATCH = E.CASES[5]             # (4, 3, HEUN, 2, 37)
WIDE = E.CASES[4]              # (70, 1, HEUN, 2, 1)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return E.build_twin(tmp_path_factory.mktemp("node_shoot_exgd_grad_twin_gpu"))


def _engine(c, scheme="SHOOTING", system="NODE_CARTPOLE"):
  return _lib.Engine(system, scheme, c["I"], c["T"], controls_per_interval=c["cpi"], integration_method=c["method"])


def _device(eng, c, rows=None, **kw):
  r = slice(None) if rows is None else list(rows)
  a = dict(z=c["z"][r], lam=c["lam"][r], lb=c["lb"][r], ub=c["ub"][r], eta_x=c["eta_x"], eta_v=c["eta_v"], nsteps=c["nsteps"], seed_z=c["seed_z"][r],
           seed_lam=c["seed_lam"][r], params=c["params"])
  a.update(kw)
  return eng.exgd_grad_node_shoot(**a)


def _same(a, b, keys=KEYS):
  return all(a[k].tobytes() == b[k].tobytes() for k in keys)


# ---- parity with the oracle and the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", ALL, ids=IDS)
def test_parity_with_the_oracle_and_the_twin(twin, monkeypatch, cs):
  case, *ref = E.reference(*cs)
  rows = case["rows"]
  if cs == E.CHUNKED:
    monkeypatch.setenv("MYRIAD_EXGD_GRAD_HIST_BYTES", str(E.CHUNKED_HIST_BYTES))
  eng = _engine(case)
  z_in, lam_in = case["z"].copy(), case["lam"].copy()
  out = _device(eng, case)
  eng.close()
  assert (case["z"] == z_in).all() and (case["lam"] == lam_in).all()
  if case["nsteps"] == 0:
    assert (out["grad"] == 0.0).all() and (out["dz0"] == case["seed_z"]).all() and (out["dlam0"] == case["seed_lam"]).all()
    return
  tw = E.twin_of_case(twin, case)
  eo = [E.rel_error(out[k][rows], r[rows]) for k, r in zip(KEYS, ref)]
  et = [E.rel_error(out[k], r) for k, r in zip(KEYS, tw)]
  print(f"NODE SHOOTING {cs}: device-oracle {max(eo):.2e} device-twin {max(et):.2e}")
  assert max(eo) <= ORACLE_TOL, eo
  assert max(et) <= TWIN_TOL, et


# ---- independent of the oracle and the twin ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,cpi,method", [(3, 2, "HEUN"), (2, 2, "RK4")])
def test_central_differences_of_myr_exgd(I, cpi, method):
  """seed . (z_n(p + d) - z_n(p - d)) / 2e-6 from two myr_exgd calls per direction, d = 1e-6 |p| o r with r uniform in [-1, 1], against
  grad . (|p| o r), at the rtol of 1e-6 of test_gpu_node_exgd_grad.test_central_differences_of_myr_exgd.  A third of the variables sit in a
  box of 1e-3 that the steps leave, the first node is pinned."""
  c = E.shape_case(I, cpi, method, 3, 1)
  p = c["params"]
  rng = np.random.default_rng(11)
  eng = _engine(c)
  grad = _device(eng, c, seed_lam=None, want_start=False)["grad"][0]
  zn = eng.exgd(c["z"], c["lam"], c["lb"], c["ub"], c["eta_x"], c["eta_v"], 3, params=p)[0][0]
  on = (zn == c["lb"][0]) | (zn == c["ub"][0])
  assert on[4:].any() and not on[4:].all()                       # the clip is active at the end for some variables, not for all
  for _ in range(3):
    delta = np.abs(p) * rng.uniform(-1.0, 1.0, p.size)
    zs = [eng.exgd(c["z"], c["lam"], c["lb"], c["ub"], c["eta_x"], c["eta_v"], 3, params=p + sgn * 1e-6 * delta)[0][0] for sgn in (1.0, -1.0)]
    fd = float(c["seed_z"][0] @ (zs[0] - zs[1])) / 2e-6
    print(I, cpi, method, "grad . delta", float(grad @ delta), "central differences", fd)
    np.testing.assert_allclose(float(grad @ delta), fd, rtol=1e-6)
  eng.close()


# ---- forms of the call -----------------------------------------------------------------------------------------------------------------
def test_forms_of_the_call(monkeypatch):
  from fractions import Fraction
  c, *_ = E.reference(*E.CHUNKED)
  B = c["z"].shape[0]
  eng = _engine(c)
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
  eng.exgd_grad_node_shoot_device(B, t["z"], t["lam"], t["lb"], t["ub"], c["eta_x"], c["eta_v"], c["nsteps"], t["seed_z"], g, eng.np, t["params"],
                                  seed_lam=t["seed_lam"], dz0=dz, dlam0=dl)
  eng.exgd_grad_node_shoot_device(B, t["z"], t["lam"], t["lb"], t["ub"], c["eta_x"], c["eta_v"], c["nsteps"], t["seed_z"], gs, 0, t["params"],
                                  seed_lam=t["seed_lam"])
  torch.cuda.synchronize()
  assert g.cpu().numpy().tobytes() == rows["grad"].tobytes() and gs.cpu().numpy().tobytes() == s1["grad"].tobytes()
  assert dz.cpu().numpy().tobytes() == rows["dz0"].tobytes() and dl.cpu().numpy().tobytes() == rows["dlam0"].tobytes()
  assert (t["z"].cpu().numpy() == c["z"]).all() and (t["lam"].cpu().numpy() == c["lam"]).all()
  eng.close()
  # the chunked path (a 4 KB history bound: chunks of one instance) against the unchunked: the same bits
  monkeypatch.setenv("MYRIAD_EXGD_GRAD_HIST_BYTES", str(E.CHUNKED_HIST_BYTES))
  eng = _engine(c)
  ch, chs = _device(eng, c), _device(eng, c, reduce=True)
  eng.close()
  assert _same(ch, rows) and chs["grad"].tobytes() == s1["grad"].tobytes()


def test_an_instance_alone_gives_the_bits_it_gives_inside_the_batch():
  c, *_ = E.reference(*BATCH)
  eng = _engine(c)
  whole, alone = _device(eng, c), _device(eng, c, rows=[21])
  eng.close()
  assert np.isfinite(whole["grad"]).all()
  for k in KEYS:
    assert whole[k][21].tobytes() == alone[k][0].tobytes(), k


def test_inherited_registers_do_not_reach_the_result(monkeypatch):
  c, *_ = E.reference(*WIDE)
  bits = {}
  for pat in ("zero", "nan", "random"):
    monkeypatch.setenv("MYRIAD_REG_FILL", pat)
    monkeypatch.setenv("MYRIAD_STACK_FILL", pat)
    eng = _engine(c)                                             # (the handle reads the fill at creation)
    out, red = _device(eng, c), _device(eng, c, reduce=True)
    eng.close()
    assert np.isfinite(out["grad"]).all()
    bits[pat] = out["grad"].tobytes() + out["dz0"].tobytes() + out["dlam0"].tobytes() + red["grad"].tobytes()
  assert bits["zero"] == bits["nan"] == bits["random"]


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors():
  c, *_ = E.reference(*E.CASES[1])
  p = np.array(c["params"])
  grad = np.empty((2, 4804))
  ptr = {k: c[k].ctypes.data for k in ("z", "lam", "lb", "ub", "seed_z")}
  ptr.update(params=p.ctypes.data, grad=grad.ctypes.data)

  def call(eng, B=2, nsteps=3, grad_stride=4804, mem=_lib.MEM_HOST, fn="myr_exgd_grad_node_shoot", **null):
    a = dict(ptr); a.update(null)
    return getattr(eng.lib, fn)(eng._h, B, a["z"], a["lam"], a["lb"], a["ub"], a["params"], c["eta_x"], c["eta_v"], nsteps, a["seed_z"], None,
                                a["grad"], grad_stride, None, None, mem)

  # (the argument checks of the C call, with their full texts and their order, and the refusals that stay -- myr_exgd_grad_node on a shooting
  # handle, myr_exgd_grad_shoot on the network: tests/test_gpu_api.py)
  eng = _engine(c)
  grad[:] = 7.0
  assert call(eng, B=0) == 0 and (grad == 7.0).all()             # an empty batch writes nothing
  assert call(eng) == 0 and np.isfinite(grad).all()
  eng.close()
  eng = _lib.Engine("NODE_CARTPOLE", "SHOOTING", 1, 2.0, controls_per_interval=2000, integration_method="HEUN")      # 5 064 + 24 035 doubles = 233 KB
  with pytest.raises(_lib.MyriadHipError, match="too large for the LDS"):
    eng.exgd_grad_node_shoot(np.zeros((1, eng.n)), np.zeros((1, eng.m)), -np.ones(eng.n), np.ones(eng.n), 0.01, 0.01, 1, np.zeros((1, eng.n)), p)
  eng.close()


# ---- the optimizer's method and the driver ---------------------------------------------------------------------------------------------
def _hp(**kw):
  from myriad_amd.config import HParams, OptimizerType
  from myriad_amd.systems import SystemType
  return HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.SHOOTING, intervals=4, controls_per_interval=3, hidden_layers=(64, 64),
                 num_unrolled=2, **kw)


def test_unrolled_grad_returns_the_mapping_of_the_flat_row():
  from myriad_amd.config import Config
  from myriad_amd.systems.neural_ode import NeuralODE, NodeSystem, flat_from_mapping
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp = _hp()
  node = NeuralODE.load_fitted_cartpole()
  opt = get_optimizer(hp, Config(verbose=False, plot=False), NodeSystem(node, hp.system()))
  assert opt.transcription == "SHOOTING"
  rng = np.random.default_rng(3)
  lam, seed = 0.1 * rng.standard_normal(opt.engine.m), rng.standard_normal(opt.engine.n)
  g = opt.unrolled_grad(opt.guess, lam, node.params, seed, 2)
  ex, ev = opt.step_sizes()
  row = opt.engine.exgd_grad_node_shoot(opt.guess, lam, opt.bounds[:, 0], opt.bounds[:, 1], ex, ev, 2, seed, flat_from_mapping(node.params),
                                        want_start=False)["grad"][0]
  assert set(g) == {"linear", "linear_1", "linear_2"} and g["linear_1"]["w"].shape == (64, 64)
  assert flat_from_mapping(g).tobytes() == row.tobytes() and np.abs(row).max() > 0


@pytest.mark.parametrize("batched", [False, True], ids=["single", "start_states"])
def test_driver_follows_the_reference_loop(batched):
  """two epochs of run_node_endtoend(hp, cfg, shooting=True) (4 x 3 HEUN, num_unrolled = 2) against the same loop made of the engine calls and
  the driver's Adam"""
  from myriad_amd.config import Config
  from myriad_amd.experiments import node_e2e_sysid as D
  from myriad_amd.experiments.mle_sysid import Adam
  from myriad_amd.systems.neural_ode import NeuralODE, NodeSystem, flat_from_mapping
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp, cfg = _hp(), Config(verbose=False, plot=False)
  true_system = hp.system()
  x0s = np.asarray(true_system.x_0, dtype=np.float64)[None] + np.array([[0.0, 0.0, 0.0, 0.0], [0.05, -0.05, 0.02, 0.0]]) if batched else None
  res = D.run_node_endtoend(hp, cfg, num_epochs=2, node=NeuralODE.load_fitted_cartpole(), start_states=x0s, shooting=True)
  assert res["ts"] == [0, 1] and sorted(res["saved_params"]) == [0, 2] and len(res["imitation_losses"]) == 2
  node = NeuralODE.load_fitted_cartpole()
  true_opt = get_optimizer(hp, cfg, true_system)
  eng = get_optimizer(hp, cfg, NodeSystem(node, hp.system())).engine
  if batched:
    true_us = true_opt.solve_batch(x0s=x0s)["u"]
    guess, lb, ub = true_opt.batch_inputs(x0s, true_system.device_params())
  else:
    true_us = true_opt.solve()["u"]
    guess, lb, ub = true_opt.guess, true_opt.bounds[:, 0], true_opt.bounds[:, 1]
  assert (true_us == res["true_opt_us"]).all()
  B = 2 if batched else 1
  eta_x, eta_v = true_opt.step_sizes()
  x = np.array(guess, dtype=np.float64).reshape(B, -1)
  lam, flat, adam = np.zeros((B, eng.m)), flat_from_mapping(node.params), Adam(1e-4)
  K = 4 * 3 + 1                                                   # control rows of 4 x 3 HEUN
  for epoch in range(2):
    x, lam = eng.exgd(x, lam, lb, ub, eta_x, eta_v, 2, params=flat)
    seed = np.zeros((B, eng.n))
    seed[:, -K:] = 2.0 * (x[:, -K:] - true_us.reshape(B, -1)) / K      # no discount: weights 1 / (rows nu)
    g = eng.exgd_grad_node_shoot(x, lam, lb, ub, eta_x, eta_v, 2, seed, flat, reduce=True, want_start=False)["grad"] / B
    flat = adam.update({"w": flat}, {"w": g})["w"]
  got = flat_from_mapping(res["params"])
  assert np.abs(got - flat).max() <= 1e-12
  assert np.abs(got - flat_from_mapping(node.params)).max() > 1e-5      # Adam's first steps are lr-sized: the weights moved
