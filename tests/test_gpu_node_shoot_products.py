"""myr_vjp, myr_jvp and myr_exgd of the network system under SHOOTING (myriad_amd/csrc/node_shoot_products.h) on the device: against the oracle's
autodiff, the host twin, the per-lane form (MYRIAD_PROD_MODE=lane) and myr_eval's Jacobian blocks; the active clip; bit-exactness over calls,
batches, memory kinds and inherited state; argument errors; the extragradient solver branch and the refusal of the weight gradient.

Shapes, points and references: tests/node_shoot_products_cases.py.  Tolerances against the oracle are those of
tests/test_gpu_products.py::test_shooting_products_match_autodiff; against the lane form that of
tests/test_gpu_node.py::test_node_shooting_eval_matches_oracle_autodiff.

Measured device - twin distance over the six shapes (largest |d| / max(1, largest |ref|); two evaluations of the same algebra, the network once by
matrix-core passes and once by plain loops): products 9.1e-15 (J v of the batch of 37), ten extragradient steps 4.4e-16.  Asserted: 100 x the
larger, 9.1e-13.
"""
import numpy as np
import pytest
import torch

import node_shoot_products_cases as E
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

MEASURED = 9.1e-15
TWIN_TOL = 100.0 * MEASURED
SHAPE_IDS = ["-".join(map(str, s)) for s in E.SHAPES]


def _engine(c):
  return _lib.Engine("NODE_CARTPOLE", "SHOOTING", c["I"], c["T"], controls_per_interval=c["cpi"], integration_method=c["method"], max_batch=max(64, c["B"]))


def _exgd(eng, c, tight=False, nsteps=E.NSTEPS, rows=None, z=None, lam=None, params=None):
  rows = slice(None) if rows is None else list(rows)
  z = c["z"][rows] if z is None else z
  lam = np.ones((z.shape[0], c["m"])) if lam is None else lam
  lb, ub = E.clip_bounds(c, tight)
  return eng.exgd(z, lam, lb, ub, E.ETA_X, E.ETA_V, nsteps, params=E.weights()[1] if params is None else params)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return E.build_twin(tmp_path_factory.mktemp("node_shoot_products_twin"))


@pytest.fixture(scope="module")
def device():
  """{shape: dict(gl, jt, jv, z, lam, zt, lamt)}: one engine and one set of calls per shape, shared by the comparisons"""
  out = {}
  for sh in E.SHAPES:
    c = E.case(*sh)
    eng = _engine(c)
    p = E.weights()[1]
    r = dict(gl=eng.vjp(c["z"], c["lam"], params=p, add_gradf=True), jt=eng.vjp(c["z"], c["lam"], params=p, add_gradf=False),
             jv=eng.jvp(c["z"], c["v"], params=p))
    r["z"], r["lam"] = _exgd(eng, c)
    r["zt"], r["lamt"] = _exgd(eng, c, tight=True)
    eng.close()
    out[sh] = r
  return out


@pytest.mark.parametrize("sh", E.SHAPES, ids=SHAPE_IDS)
def test_products_match_oracle_autodiff(device, sh):
  c, d, ref = E.case(*sh), device[sh], E.ref_products(*sh)
  for b in E.checked(sh[0]):
    gl, jt, jv = ref[b]
    sc = max(1.0, np.abs(gl).max())
    print(sh, b, "gradL", E.rel(d["gl"][b], gl), "JTlam", E.rel(d["jt"][b], jt), "Jv", E.rel(d["jv"][b], jv))
    np.testing.assert_allclose(d["gl"][b], gl, rtol=1e-10, atol=1e-12 * sc)
    np.testing.assert_allclose(d["jt"][b], jt, rtol=1e-9, atol=1e-11 * sc)
    np.testing.assert_allclose(d["jv"][b], jv, rtol=1e-10, atol=1e-12 * max(1.0, np.abs(jv).max()))
  # <J v, lam> == <v, J^T lam> for every instance of the batch
  for b in range(sh[0]):
    lhs, rhs = d["jv"][b] @ c["lam"][b], c["v"][b] @ d["jt"][b]
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs), (b, lhs, rhs)


@pytest.mark.parametrize("sh", E.SHAPES, ids=SHAPE_IDS)
def test_ten_extragradient_steps_match_the_oracle(device, sh):
  d, ref = device[sh], E.ref_exgd(*sh)
  for b in E.checked(sh[0]):
    x, lm = ref[b]
    print(sh, b, "z", E.rel(d["z"][b], x), "lam", E.rel(d["lam"][b], lm))
    np.testing.assert_allclose(d["z"][b], x, rtol=1e-9, atol=1e-10 * max(1.0, np.abs(x).max()))
    np.testing.assert_allclose(d["lam"][b], lm, rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("sh", E.SHAPES, ids=SHAPE_IDS)
def test_device_matches_the_host_twin(device, twin, sh):
  c, d = E.case(*sh), device[sh]
  tz, tl = E.twin_exgd(twin, c)
  pairs = (("gl", E.twin_vjp(twin, c, True)), ("jt", E.twin_vjp(twin, c, False)), ("jv", E.twin_jvp(twin, c)), ("z", tz), ("lam", tl))
  err = {k: E.rel(d[k], t) for k, t in pairs}
  print(sh, "device - twin:", err)
  assert max(err.values()) <= TWIN_TOL, err


@pytest.mark.parametrize("sh", E.SHAPES[:4], ids=SHAPE_IDS[:4])
def test_matrix_core_form_matches_the_lane_form(monkeypatch, device, sh):
  c, d = E.case(*sh), device[sh]
  monkeypatch.setenv("MYRIAD_PROD_MODE", "lane")
  eng = _engine(c)                                           # (the handle reads the switch at creation)
  p = E.weights()[1]
  gl, jt, jv = eng.vjp(c["z"], c["lam"], params=p, add_gradf=True), eng.vjp(c["z"], c["lam"], params=p, add_gradf=False), eng.jvp(c["z"], c["v"], params=p)
  z, lam = _exgd(eng, c)
  eng.close()
  for a, b in ((d["gl"], gl), (d["jt"], jt), (d["jv"], jv), (d["z"], z), (d["lam"], lam)):
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("sh", E.SHAPES[:4], ids=SHAPE_IDS[:4])
def test_vjp_is_the_transpose_of_the_jacobian_blocks_of_eval(device, sh):
  B, I, cpi, method = sh
  c = E.case(*sh)
  M = 2 if method == "RK4" else 1
  W, NS, NU = M * cpi + 1, E.NS, E.NU
  eng = _engine(c)
  jblk = eng.eval(c["z"], params=E.weights()[1], want=("jblk",))["jblk"].reshape(B, I, -1)
  eng.close()
  ref = np.zeros((B, c["n"]))
  for b in range(B):
    for k in range(I):
      lk = c["lam"][b, k * NS:(k + 1) * NS]
      Jx, Ju = jblk[b, k, :NS * NS].reshape(NS, NS), jblk[b, k, NS * NS:].reshape(NS, W * NU)
      ref[b, k * NS:(k + 1) * NS] += Jx.T @ lk
      ref[b, (k + 1) * NS:(k + 2) * NS] -= lk
      u0 = (I + 1) * NS + M * k * cpi * NU
      ref[b, u0:u0 + W * NU] += Ju.T @ lk
  np.testing.assert_allclose(device[sh]["jt"], ref, rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("sh", E.SHAPES[:4], ids=SHAPE_IDS[:4])
def test_active_clip(device, sh):
  """control bounds at +-0.1: the oracle's own iterate has free variables exactly on a bound and strictly inside, and the device has the same ones there"""
  c, d, ref = E.case(*sh), device[sh], E.ref_exgd(*sh, True)
  lb, ub = E.clip_bounds(c, True)
  free = lb < ub
  for b in E.checked(sh[0]):
    x, lm = ref[b]
    on = ((x == lb) | (x == ub)) & free
    assert on.any() and ((x > lb) & (x < ub) & free).any(), sh
    assert ((d["zt"][b] == lb) == (x == lb)).all() and ((d["zt"][b] == ub) == (x == ub)).all()
    np.testing.assert_allclose(d["zt"][b], x, rtol=1e-9, atol=1e-10 * max(1.0, np.abs(x).max()))
    np.testing.assert_allclose(d["lamt"][b], lm, rtol=1e-9, atol=1e-10)


def test_exactness(device):
  sh = E.SHAPES[4]                                           # B = 37
  c, d = E.case(*sh), device[sh]
  p = E.weights()[1]
  eng = _engine(c)
  # two calls
  assert eng.vjp(c["z"], c["lam"], params=p, add_gradf=True).tobytes() == d["gl"].tobytes()
  assert eng.jvp(c["z"], c["v"], params=p).tobytes() == d["jv"].tobytes()
  z10, l10 = _exgd(eng, c)
  assert z10.tobytes() == d["z"].tobytes() and l10.tobytes() == d["lam"].tobytes()
  # 10 steps = 9 + 1
  z9, l9 = _exgd(eng, c, nsteps=9)
  z91, l91 = _exgd(eng, c, nsteps=1, z=z9, lam=l9)
  assert z91.tobytes() == z10.tobytes() and l91.tobytes() == l10.tobytes()
  # an instance alone has the bits it has inside the batch
  for b in (0, 21, 36):
    assert eng.vjp(c["z"][b], c["lam"][b], params=p, add_gradf=True)[0].tobytes() == d["gl"][b].tobytes()
    assert eng.vjp(c["z"][b], c["lam"][b], params=p, add_gradf=False)[0].tobytes() == d["jt"][b].tobytes()
    assert eng.jvp(c["z"][b], c["v"][b], params=p)[0].tobytes() == d["jv"][b].tobytes()
    zb, lb_ = _exgd(eng, c, rows=[b])
    assert zb[0].tobytes() == z10[b].tobytes() and lb_[0].tobytes() == l10[b].tobytes()
  # a weight row per instance, all the same: the bits of the shared set
  tiled = np.tile(p, (sh[0], 1))
  assert eng.vjp(c["z"], c["lam"], params=tiled, add_gradf=True).tobytes() == d["gl"].tobytes()
  assert eng.jvp(c["z"], c["v"], params=tiled).tobytes() == d["jv"].tobytes()
  zt, lt = _exgd(eng, c, params=tiled)
  assert zt.tobytes() == z10.tobytes() and lt.tobytes() == l10.tobytes()
  # device arrays
  dev = "cuda:0"
  t = {k: torch.tensor(c[k], device=dev) for k in ("z", "lam", "v")}
  tp = torch.tensor(p, device=dev)
  g, jv = torch.empty_like(t["z"]), torch.empty_like(t["lam"])
  eng.products_device("vjp", sh[0], t["z"], t["lam"], g, params=tp, params_stride=0, add_gradf=1)
  eng.products_device("jvp", sh[0], t["z"], t["v"], jv, params=tp, params_stride=0)
  lb, ub = (torch.tensor(np.ascontiguousarray(np.broadcast_to(a, c["z"].shape)), device=dev) for a in E.clip_bounds(c))
  zz, ll = t["z"].clone(), torch.ones_like(t["lam"])
  rc = eng.lib.myr_exgd(eng._h, sh[0], zz.data_ptr(), ll.data_ptr(), lb.data_ptr(), ub.data_ptr(), tp.data_ptr(), 0, E.ETA_X, E.ETA_V, E.NSTEPS, _lib.MEM_DEVICE)
  torch.cuda.synchronize()
  assert rc == 0
  assert g.cpu().numpy().tobytes() == d["gl"].tobytes() and jv.cpu().numpy().tobytes() == d["jv"].tobytes()
  assert zz.cpu().numpy().tobytes() == z10.tobytes() and ll.cpu().numpy().tobytes() == l10.tobytes()
  eng.close()


def test_inherited_state_does_not_reach_the_result(monkeypatch, device):
  sh = E.SHAPES[1]                                           # RK4: the kernel with the larger private segment
  c, d = E.case(*sh), device[sh]
  want = d["gl"].tobytes() + d["jv"].tobytes() + d["z"].tobytes() + d["lam"].tobytes()
  for env in (dict(MYRIAD_REG_FILL="zero", MYRIAD_STACK_FILL="zero"), dict(MYRIAD_REG_FILL="nan", MYRIAD_STACK_FILL="nan"),
              dict(MYRIAD_REG_FILL="random", MYRIAD_STACK_FILL="random"), dict(MYRIAD_POISON="random")):
    for k in ("MYRIAD_REG_FILL", "MYRIAD_STACK_FILL", "MYRIAD_POISON"):
      monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
      monkeypatch.setenv(k, v)
    eng = _engine(c)                                         # (the handle reads the fills at creation)
    p = E.weights()[1]
    z, lam = _exgd(eng, c)
    got = eng.vjp(c["z"], c["lam"], params=p, add_gradf=True).tobytes() + eng.jvp(c["z"], c["v"], params=p).tobytes() + z.tobytes() + lam.tobytes()
    eng.close()
    assert got == want, env


def test_errors_and_degenerate_calls():
  sh = E.SHAPES[0]
  c = E.case(*sh)
  p = E.weights()[1]
  eng = _engine(c)
  z, lam = np.ascontiguousarray(c["z"]), np.ascontiguousarray(c["lam"])
  out = np.full_like(z, 7.0)
  # null params
  assert eng.lib.myr_vjp(eng._h, sh[0], z.ctypes.data, lam.ctypes.data, None, 0, out.ctypes.data, 1, _lib.MEM_HOST) == -1
  assert b"weights" in eng.lib.myr_last_error() and (out == 7.0).all()
  with pytest.raises(ValueError):
    eng.jvp(c["z"], c["v"])
  # an empty batch writes nothing
  assert eng.lib.myr_vjp(eng._h, 0, z.ctypes.data, lam.ctypes.data, p.ctypes.data, 0, out.ctypes.data, 1, _lib.MEM_HOST) == 0 and (out == 7.0).all()
  # no steps: the inputs
  z0, l0 = _exgd(eng, c, nsteps=0)
  assert z0.tobytes() == z.tobytes() and (l0 == 1.0).all()
  eng.close()
  # the parametrised trapezoid of the reference is dead code: refused
  eng = _lib.Engine("NODE_CARTPOLE", "TRAPEZOIDAL", 4, c["T"])
  with pytest.raises(NotImplementedError, match="SHOOTING"):
    eng.vjp(np.zeros(eng.n), np.zeros(eng.m), params=p)
  eng.close()


def _hp(**kw):
  from myriad_amd.config import HParams, OptimizerType
  from myriad_amd.systems import SystemType
  return HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.SHOOTING, intervals=4, controls_per_interval=3, hidden_layers=(64, 64), **kw)


def test_extragradient_solver_over_a_node_system_with_a_shooting_optimizer():
  """nlp_solvers.solve(... EXTRAGRADIENT ...) as experiments/node_e2e_sysid.py:374-377 ends: 50 iterations on the reference's schedule"""
  from oracle import myriad_oracle as O
  from myriad_amd.config import Config, NLPSolverType
  from myriad_amd.systems.neural_ode import NeuralODE, NodeSystem
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp = _hp(nlpsolver=NLPSolverType.EXTRAGRADIENT, max_iter=5)
  assert hp.max_iter == 50
  node = NeuralODE.load_fitted_cartpole()
  sol = get_optimizer(hp, Config(verbose=False, plot=False), NodeSystem(node, hp.system())).solve_with_params(node.params)
  assert set(sol) == {'x', 'u', 'xs_and_us', 'cost', 'lambda'} and sol['lambda'].shape == (16,)
  tr = O.shooting(O.NodeCartPole(node.params), 4, 3, "HEUN")
  L = O.Lagrangian(tr)
  x, lm = tr.guess.copy(), np.ones(16)
  ex, ev = 1e-2 * 0.999, 1e-4 * 0.999                        # defaults.learning_rates of CARTPOLE, the decay at iteration 0
  for _ in range(50):
    x, lm = L.step(x, lm, ex, ev)
  np.testing.assert_allclose(sol['xs_and_us'], x, rtol=1e-7, atol=1e-8)
  np.testing.assert_allclose(sol['lambda'], lm, rtol=1e-7, atol=1e-8)


def test_run_node_endtoend_refuses_shooting_before_anything_is_solved(monkeypatch):
  from myriad_amd.config import Config
  from myriad_amd.experiments import node_e2e_sysid
  from myriad_amd.systems.neural_ode import NeuralODE
  from myriad_amd.trajectory_optimizers import TrajectoryOptimizer
  started = []
  monkeypatch.setattr(TrajectoryOptimizer, "solve", lambda self, *a, **k: started.append("solve"))
  monkeypatch.setattr(TrajectoryOptimizer, "solve_batch", lambda self, *a, **k: started.append("solve_batch"))
  with pytest.raises(NotImplementedError, match="HERMITE_SIMPSON"):
    node_e2e_sysid.run_node_endtoend(_hp(), Config(verbose=False, plot=False), num_epochs=1, node=NeuralODE.load_fitted_cartpole())
  with pytest.raises(NotImplementedError, match="HERMITE_SIMPSON"):
    node_e2e_sysid.run_node_endtoend(_hp(), Config(verbose=False, plot=False), num_epochs=1, node=NeuralODE.load_fitted_cartpole(),
                                     start_states=np.zeros((2, 4)))
  assert started == []
