"""GPU tests of the reference-shaped Python API (get_optimizer(...).solve(), solve_with_params, run_trajectory_opt,
rollout) running on the HIP kernels through the C-ABI."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from myriad_amd.config import Config, HParams, IntegrationMethod, NLPSolverType, OptimizerType, QuadratureRule
from myriad_amd.systems import SystemType

CFG = Config(verbose=False, plot=False)


def _hp(N=25, **kw):
  return HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.COLLOCATION, quadrature_rule=QuadratureRule.HERMITE_SIMPSON,
                 integration_method=IntegrationMethod.RK4, intervals=N, **kw)


def test_run_trajectory_opt_returns_cost_and_defect(golden_dir):
  """useful_scripts.py:26-76 contract: (integrated cost of the true-dynamics RK4 rollout under the solved controls,
  terminal defect); pinned by the oracle's restatement of utils.py:258-324 on the golden solution."""
  from myriad_amd.useful_scripts import run_trajectory_opt
  from oracle import myriad_oracle as O
  c, defect = run_trajectory_opt(_hp(25), CFG)
  d = np.load(os.path.join(golden_dir, "solve_hs_cartpole_N25.npz"))
  s = O.CartPole()
  u_gold = d["z"][0][51 * 4:].reshape(51, 1)
  xs, c_or = O.get_state_trajectory_and_cost(s, 25, "RK4", s.x_0, u_gold)
  assert c == pytest.approx(c_or, rel=1e-6)
  np.testing.assert_allclose(defect, O.get_defect(s, xs), atol=1e-5)
  assert defect.shape == (4,) and np.abs(defect).max() < 1.0       # open-loop RK4 re-integration of an unstable swing-up


def test_optimizer_solve_result_keys_and_shapes():
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp = _hp(10)
  opt = get_optimizer(hp, CFG, hp.system())
  sol = opt.solve()
  assert set(sol) == {'x', 'u', 'xs_and_us', 'cost', 'lambda'}           # nlp_solvers/__init__.py:90-96
  assert sol['x'].shape == (21, 4) and sol['u'].shape == (21, 1) and sol['xs_and_us'].shape == (105,) and sol['lambda'].shape == (80,)
  assert sol['cost'] == pytest.approx(85.80432338009395, rel=1e-9)        # golden N=10
  assert np.abs(opt.constraints(sol['xs_and_us'])).max() <= 1e-8
  assert opt.objective(sol['xs_and_us']) == pytest.approx(sol['cost'], rel=1e-12)
  # warm start from the solution (base.py:81-93 solve_with_params(params, guess))
  sol2 = opt.solve_with_params({'g': 9.81, 'm1': 1.0, 'm2': 0.3, 'length': 0.5}, guess=sol['xs_and_us'])
  assert sol2['cost'] == pytest.approx(sol['cost'], rel=1e-7)
  # a different model: heavier pole needs more effort
  sol3 = opt.solve_with_params({'g': 9.81, 'm1': 1.0, 'm2': 0.6, 'length': 0.5})
  assert sol3['cost'] > sol['cost'] * 1.05


def test_scipy_branch_on_gpu_callbacks_agrees_with_sqp():
  """The reference's NLPSolverType.SLSQP branch (nlp_solvers/__init__.py:50-52) fed by the HIP eval kernel."""
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp = _hp(5, nlpsolver=NLPSolverType.SLSQP)
  opt = get_optimizer(hp, CFG, hp.system())
  sol = opt.solve()
  hp2 = _hp(5, nlpsolver=NLPSolverType.SQP)
  sol2 = get_optimizer(hp2, CFG, hp2.system()).solve()
  assert sol['cost'] == pytest.approx(sol2['cost'], rel=1e-4)
  assert 'lambda' not in sol                                              # absent for SLSQP, as in the reference


def test_solve_with_params_reaches_the_scipy_branch():
  """base.py:81-93: solve_with_params wraps parametrized_objective / parametrized_constraints, so the SLSQP branch must
  solve the NON-default model too (fun, constraints, Jacobian and gradient all at m2 = 0.6)."""
  from myriad_amd.trajectory_optimizers import get_optimizer
  heavy = {'g': 9.81, 'm1': 1.0, 'm2': 0.6, 'length': 0.5}
  hp = _hp(5, nlpsolver=NLPSolverType.SLSQP)
  opt = get_optimizer(hp, CFG, hp.system())
  hp2 = _hp(5, nlpsolver=NLPSolverType.SQP)
  opt2 = get_optimizer(hp2, CFG, hp2.system())
  sol_sqp = opt2.solve_with_params(heavy)
  sol_default = opt2.solve()
  # swing-up is non-convex (SLSQP from the straight-line guess may pick another basin), so start SLSQP at the optimum of
  # the HEAVY model: it must stay there -- it would walk away if any of its four callbacks still saw the default model
  sol_slsqp = opt.solve_with_params(heavy, guess=sol_sqp['xs_and_us'])
  assert sol_slsqp['cost'] == pytest.approx(sol_sqp['cost'], rel=1e-5)
  np.testing.assert_allclose(sol_slsqp['xs_and_us'], sol_sqp['xs_and_us'], atol=1e-3)
  assert abs(sol_slsqp['cost'] - sol_default['cost']) > 0.02 * sol_default['cost']
  assert np.abs(opt.parametrized_constraints(heavy, sol_slsqp['xs_and_us'])).max() <= 1e-6
  assert np.abs(opt.constraints(sol_slsqp['xs_and_us'])).max() > 1e-4      # NOT feasible for the default model
  # and from the reference guess it returns a point that is feasible for the heavy model, not for the default one
  sol_cold = opt.solve_with_params(heavy)
  assert np.abs(opt.parametrized_constraints(heavy, sol_cold['xs_and_us'])).max() <= 1e-6
  assert np.abs(opt.constraints(sol_cold['xs_and_us'])).max() > 1e-4


def test_solve_batch_extension_parameter_sweep():
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp = _hp(10)
  opt = get_optimizer(hp, CFG, hp.system())
  rng = np.random.default_rng(1)
  B = 33
  params = np.array([9.81, 1.0, 0.3, 0.5]) * (1 + 0.1 * rng.uniform(-1, 1, (B, 4)))
  x0s = np.clip(0.1 * rng.standard_normal((B, 4)), -1, 1)
  res = opt.solve_batch(x0s=x0s, params=params)
  assert (res['status'] == 0).all() and res['x'].shape == (B, 21, 4) and res['u'].shape == (B, 21, 1)
  assert np.array_equal(res['x'][:, 0, :], x0s)
  ev = opt.engine.eval(res['xs_and_us'], params=params, want=("c",))
  assert np.abs(ev["c"]).max() <= 1e-8


@pytest.mark.parametrize("method", ["EULER", "HEUN", "MIDPOINT", "RK4"])
def test_rollout_kernel_matches_oracle(method):
  from myriad_amd import _lib
  from oracle import myriad_oracle as O
  rng = np.random.default_rng(2)
  for name in ("CARTPOLE", "VANDERPOL", "CANCERTREATMENT", "SIMPLECASE"):
    s = O.SYSTEMS[name]()
    S, B = 40, 5
    rows = (2 if method == "RK4" else 1) * S + 1
    us = 0.2 * rng.standard_normal((B, rows, 1))
    if name == "CANCERTREATMENT":
      us = np.abs(us)
    x0 = np.tile(s.x_0, (B, 1)) * (1 + 0.01 * rng.standard_normal((B, s.ns)))
    eng = _lib.Engine(name, "SHOOTING", 1, s.T / 8, controls_per_interval=S, integration_method=method)
    xs, cost = eng.rollout(x0, us, S)
    s.T = s.T / 8
    for b in range(B):
      oxs, oc = O.get_state_trajectory_and_cost(s, S, method, x0[b], us[b])
      np.testing.assert_allclose(xs[b], oxs, rtol=1e-12, atol=1e-13)
      assert cost[b] == pytest.approx(oc, rel=1e-12, abs=1e-14)
    eng.close()


def test_gather_solutions_over_rccl_single_rank():
  """The N>1 bench path's only collective, on the RCCL backend (a 1-rank group is all a 1-GPU box allows; the
  world-2 logic is covered on gloo in tests/test_host_api.py)."""
  import os
  import torch
  import torch.distributed as dist
  from myriad_amd.batched import gather_solutions
  os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29617")
  dist.init_process_group("nccl", rank=0, world_size=1)
  try:
    z = torch.arange(12, dtype=torch.float64, device="cuda").reshape(4, 3)
    st = torch.tensor([0, 1, 0, 3], dtype=torch.int32, device="cuda")
    out = gather_solutions({"z": z, "status": st}, [4])
    assert torch.equal(out["z"], z) and torch.equal(out["status"], st)
  finally:
    dist.destroy_process_group()


def test_solve_batch_fan_out_over_two_handles_of_one_device_matches_one_handle():
  """SURVEY.md 8(b) Threading: the batch axis fans out beneath the unchanged API -- one handle + one host thread per listed
  device.  `devices=[0, 0]` runs the two shards on one GPU (a 1-GPU box): same result, instance by instance, as one handle."""
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp = _hp(25)
  rng = np.random.default_rng(3)
  opt1 = get_optimizer(hp, CFG, hp.system()); opt1.devices = [0]
  x0s = np.clip(np.array(opt1.system.x_0)[None] + 0.1 * rng.standard_normal((48, 4)), -2, 2)
  a = opt1.solve_batch(x0s=x0s)
  opt2 = get_optimizer(hp, CFG, hp.system()); opt2.devices = [0, 0]; opt2.min_shard = 8
  assert len(opt2.engines_for(48)) == 2
  b = opt2.solve_batch(x0s=x0s)
  assert (a["status"] == 0).all() and (b["status"] == 0).all()
  for k in ("xs_and_us", "cost", "lambda", "iters", "status", "start", "attempts"):
    assert np.array_equal(a[k], b[k]), k
  # default device list: every visible device (1 here), never more shards than min_shard allows
  opt3 = get_optimizer(hp, CFG, hp.system())
  assert opt3._device_list() == list(range(_lib_device_count())) and len(opt3.engines_for(48)) == 1


def _lib_device_count():
  from myriad_amd import _lib
  return max(1, _lib.device_count())


def test_solve_plan_reports_the_launch_form_and_an_explicit_park_iter_selects_the_one_wavefront_form():
  """myr_solve_plan (round 5): the library says how it launched the last solve -- what bench.py quotes instead of restating the library's rules.  A small
  batch of a closed-form collocation problem runs two wavefronts per trajectory as whole solves; an explicit myr_solve_opts.park_iter > 0 selects the
  one-wavefront form with its two-phase launch (include/myriad_hip.h: park_iter) and returns the same bits; single shooting reports its own kernel."""
  from myriad_amd import _lib
  from myriad_amd.trajectory_optimizers import get_optimizer
  from myriad_amd.config import NLPSolverType
  hp = _hp(20, nlpsolver=NLPSolverType.SQP)
  opt = get_optimizer(hp, CFG, hp.system())
  x0 = np.clip(0.1 * np.random.default_rng(3).standard_normal((40, 4)), -2, 2)
  z0, lb, ub = opt.batch_inputs(x0)
  eng = opt.engine
  a = eng.solve(z0, lb, ub)
  p = eng.solve_plan()
  assert p["form"] == "fused" and p["waves_per_trajectory"] == 2 and p["park_iter"] == 0 and p["launches_per_solve"] == 1 and p["slots"] == 40
  o = eng.default_opts(); o.park_iter = 5
  b = eng.solve(z0, lb, ub, opts=o)
  p = eng.solve_plan()
  assert p["waves_per_trajectory"] == 1 and p["park_iter"] == 5 and p["launches_per_solve"] == 2
  assert (a["status"] == 0).all() and np.array_equal(a["status"], b["status"]) and np.array_equal(a["iters"], b["iters"])
  np.testing.assert_allclose(a["z"], b["z"], rtol=0, atol=1e-9)       # (W = 1 and W = 2 differ in the order of their merit sums only)
  hs = HParams(system=SystemType.VANDERPOL, optimizer=OptimizerType.SHOOTING, intervals=1, controls_per_interval=20, nlpsolver=NLPSolverType.SQP)
  os_ = get_optimizer(hs, CFG, hs.system())
  os_.solve_batch(x0s=np.tile(os_.system.x_0, (3, 1)))
  assert os_.engine.solve_plan()["form"] == "shooting_wave"


# ---- the C-ABI as it is: both memory kinds, and the argument checks ------------------------------------------------------------
_ORDER = {
  "myr_eval": ("B", "z", "params", "stride", "f", "g", "c", "j", "mem"),
  "myr_vjp": ("B", "z", "w", "params", "stride", "out", "add_gradf", "mem"),
  "myr_jvp": ("B", "z", "w", "params", "stride", "out", "mem"),
  "myr_exgd": ("B", "z", "lam", "lb", "ub", "params", "stride", "eta_x", "eta_v", "nsteps", "mem"),
  "myr_rollout": ("B", "num_steps", "u_rows", "x0", "us", "params", "stride", "xs", "cost", "mem"),
  "myr_solve": ("B", "z", "lb", "ub", "params", "stride", "opts", "lam", "cost", "status", "iters", "kkt", "mem"),
  "myr_solve_x0": ("B", "x0s", "g0", "g1", "lb", "ub", "params", "stride", "opts", "z", "lam", "cost", "status", "iters", "kkt", "mem"),
  "myr_fit_grad": ("B", "num_steps", "u_rows", "xs_obs", "us", "wt", "params", "stride", "loss", "grad", "grad_stride", "mem"),
  "myr_fbsm": ("B", "N", "x0", "adj_T", "params", "stride", "clip_lo", "clip_hi", "bang", "delta", "max_sweeps", "xs", "us", "adjs", "sweeps", "mem"),
}
_OUTPUTS = {"myr_eval": ("f", "g", "c", "j"), "myr_vjp": ("out",), "myr_jvp": ("out",), "myr_exgd": ("z", "lam"), "myr_rollout": ("xs", "cost"),
            "myr_solve": ("z", "lam", "cost", "status", "iters", "kkt"), "myr_solve_x0": ("z", "lam", "cost", "status", "iters", "kkt"),
            "myr_fit_grad": ("loss", "grad"), "myr_fbsm": ("xs", "us", "adjs", "sweeps")}


def _abi_call(ep, eng, a, handle=True):
  """One call of entry point `ep` with the named arguments `a`: numpy arrays for MYR_MEM_HOST, torch device tensors for MYR_MEM_DEVICE (copies of the
  arrays; the device is synchronised around the call, which runs on the handle's own stream).  Returns (rc, {output name: numpy array})."""
  import ctypes as C
  from myriad_amd import _lib
  dev = a["mem"] == _lib.MEM_DEVICE
  if dev:
    import torch
  held, args = {}, [eng._h if handle else None]
  for k in _ORDER[ep]:
    v = a[k]
    if isinstance(v, np.ndarray):
      v = np.ascontiguousarray(v).copy()
      if dev:
        v = torch.as_tensor(v, device="cuda:0")
      held[k] = v
      args.append(_lib._addr(v))
    elif isinstance(v, _lib.SolveOpts):
      held[k] = v
      args.append(C.byref(v))
    else:
      args.append(v)
  if dev:
    torch.cuda.synchronize()
  rc = getattr(eng.lib, ep)(*args)
  if dev:
    torch.cuda.synchronize()
  return rc, {k: (held[k].cpu().numpy() if dev else held[k]) for k in _OUTPUTS[ep] if k in held}


def _same_bits(ep, eng, make_engine, a, must_converge=False):
  """`ep` with host arrays on `eng` and with device arrays on a fresh handle: every output equal, bit for bit"""
  from myriad_amd import _lib
  rc, host = _abi_call(ep, eng, dict(a, mem=_lib.MEM_HOST))
  assert rc == 0, (ep, eng.lib.myr_last_error().decode())
  fresh = make_engine()
  try:
    rc, dev = _abi_call(ep, fresh, dict(a, mem=_lib.MEM_DEVICE))
    assert rc == 0, (ep, fresh.lib.myr_last_error().decode())
  finally:
    fresh.close()
  assert set(host) == set(dev) and host
  for k in host:
    assert host[k].dtype == dev[k].dtype and host[k].tobytes() == dev[k].tobytes(), (ep, k)
  if must_converge:      # (two equal failures would compare equal too)
    assert (host["status"] == 0).all(), host["status"]
  return host


def _params_forms(default, B):
  """params None, shared [np], per instance [B, np]"""
  d = np.asarray(default, dtype=np.float64)
  return [(None, 0), (d, 0), (np.tile(d, (B, 1)) * (1.0 + 0.01 * np.arange(B))[:, None], d.size)]


def _nan(*shape):
  return np.full(shape, np.nan)


def test_host_and_device_arrays_give_the_same_bits():
  """Every output of a MYR_MEM_HOST call equals, bit for bit, that of the same call with device arrays and MYR_MEM_DEVICE on a fresh handle: the
  staging of a host call (csrc/host_stage.h) adds copies and nothing else.  Odd sizes: n = 35, m = 24, B = 1 and 3, every optional array present and absent."""
  from myriad_amd import _lib
  from oracle import myriad_oracle as O
  rng = np.random.default_rng(11)
  cart = lambda N: (lambda: _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", N, 2.0))
  vdp = lambda: _lib.Engine("VANDERPOL", "SHOOTING", 2, 10.0, controls_per_interval=3, integration_method="HEUN")
  for make, default in ((cart(3), [9.81, 1.0, 0.3, 0.5]), (vdp, None)):
    eng = make()
    n, m, ns, nu = eng.n, eng.m, eng.ns, eng.nu
    if default is None:
      default = np.ones(eng.np)
    colloc = eng.desc.transcription != _lib.TR_IDS["SHOOTING"]
    assert not colloc or (n, m) == (35, 24)
    for B in (1, 3):
      z = 0.3 * rng.standard_normal((B, n)); lam = rng.standard_normal((B, m)); v = rng.standard_normal((B, n))
      S = 5
      x0 = 0.1 * rng.standard_normal((B, ns)); us = 0.2 * rng.standard_normal((B, S + 1, nu))
      for p, ps in _params_forms(default, B):
        common = dict(B=B, params=p, stride=ps)
        _same_bits("myr_eval", eng, make, dict(common, z=z, f=_nan(B), g=_nan(B, eng.ngrad), c=_nan(B, m), j=_nan(B, eng.jblk)))
        _same_bits("myr_eval", eng, make, dict(common, z=z, f=None, g=None, c=_nan(B, m), j=None))
        _same_bits("myr_vjp", eng, make, dict(common, z=z, w=lam, out=_nan(B, n), add_gradf=1))
        _same_bits("myr_jvp", eng, make, dict(common, z=z, w=v, out=_nan(B, m)))
        _same_bits("myr_rollout", eng, make, dict(common, num_steps=S, u_rows=S + 1, x0=x0, us=us, xs=_nan(B, S + 1, ns), cost=_nan(B)))
        _same_bits("myr_rollout", eng, make, dict(common, num_steps=S, u_rows=S + 1, x0=x0, us=us, xs=None, cost=_nan(B)))
        if colloc:
          _same_bits("myr_exgd", eng, make, dict(common, z=z, lam=lam, lb=np.full((B, n), -5.0), ub=np.full((B, n), 5.0), eta_x=1e-3, eta_v=1e-3, nsteps=3))
    eng.close()
  # the two solves: the first three instances of smoke()'s batch, which smoke() asserts to converge
  N = 10
  sysm = O.CartPole()
  tr = O.hermite_simpson(sysm, N)
  x0_all = O.random_x0(sysm, 8, seed=1)
  rows = 2 * N + 1
  lin = np.linspace(0.0, 1.0, rows)
  g0 = np.zeros(tr.guess.size); g1 = np.zeros(tr.guess.size)
  g0[:rows * 4] = (sysm.x_T[None, :] * lin[:, None]).ravel(); g1[:rows * 4] = np.repeat(1 - lin, 4)
  eng = cart(N)()
  n, m = eng.n, eng.m
  for B in (1, 3):
    x0 = x0_all[:B]
    Z0 = np.stack([np.concatenate([np.linspace(x0[b], sysm.x_T, rows).ravel(), np.zeros(rows)]) for b in range(B)])
    lb = np.tile(tr.bounds[:, 0], (B, 1)); ub = np.tile(tr.bounds[:, 1], (B, 1))
    lb[:, :4] = x0; ub[:, :4] = x0
    d = np.array([9.81, 1.0, 0.3, 0.5])
    for p, ps in ((None, 0), (d, 0), (np.tile(d, (B, 1)), 4)):
      for full in (True, False):
        res = dict(lam=_nan(B, m) if full else None, cost=_nan(B), status=np.full(B, -7, np.int32), iters=np.full(B, -7, np.int32),
                   kkt=_nan(B, 3) if full else None)
        common = dict(B=B, params=p, stride=ps, opts=eng.default_opts(), **res)
        _same_bits("myr_solve", eng, cart(N), dict(common, z=Z0, lb=lb, ub=ub), must_converge=True)
        _same_bits("myr_solve_x0", eng, cart(N), dict(common, x0s=x0, g0=g0, g1=g1, lb=tr.bounds[:, 0].copy(), ub=tr.bounds[:, 1].copy(), z=_nan(B, n)),
                   must_converge=True)
  eng.close()


def _abi_defaults(ep, eng, B):
  """valid arguments of `ep` for a batch of B on `eng` (host arrays; outputs hold a sentinel; arrays have room for one instance even when B = 0)"""
  n, m, ns, nu, R = eng.n, eng.m, eng.ns, eng.nu, max(B, 1)
  s = lambda *shape: np.full(shape, -7.25)
  i32 = lambda *shape: np.full(shape, -7, np.int32)
  a = dict(B=B, params=None, stride=0, mem=0)
  if ep == "myr_eval":
    a.update(z=np.zeros((R, n)), f=s(R), g=s(R, eng.ngrad), c=s(R, m), j=s(R, eng.jblk))
  elif ep in ("myr_vjp", "myr_jvp"):
    a.update(z=np.zeros((R, n)), w=np.zeros((R, m if ep == "myr_vjp" else n)), out=s(R, n if ep == "myr_vjp" else m), add_gradf=0)
  elif ep == "myr_exgd":
    a.update(z=s(R, n), lam=s(R, m), lb=np.full((R, n), -10.0), ub=np.full((R, n), 10.0), eta_x=1e-3, eta_v=1e-3, nsteps=1)
  elif ep == "myr_rollout":
    a.update(num_steps=4, u_rows=5, x0=np.zeros((R, ns)), us=np.zeros((R, 5, nu)), xs=s(R, 5, ns), cost=s(R))
  elif ep == "myr_solve":
    a.update(z=s(R, n), lb=np.full((R, n), -10.0), ub=np.full((R, n), 10.0), opts=eng.default_opts(), lam=s(R, m), cost=s(R), status=i32(R), iters=i32(R), kkt=s(R, 3))
  elif ep == "myr_solve_x0":
    a.update(x0s=np.zeros((R, ns)), g0=np.zeros(n), g1=np.zeros(n), lb=np.full(n, -10.0), ub=np.full(n, 10.0), opts=eng.default_opts(), z=s(R, n), lam=s(R, m),
             cost=s(R), status=i32(R), iters=i32(R), kkt=s(R, 3))
  elif ep == "myr_fit_grad":
    a.update(num_steps=4, u_rows=5, xs_obs=np.zeros((R, 5, ns)), us=np.zeros((R, 5, nu)), wt=None, loss=s(R), grad=s(R, max(eng.np, 1)), grad_stride=eng.np)
  elif ep == "myr_fbsm":
    a.update(N=4, x0=np.ones((R, ns)), adj_T=None, clip_lo=np.zeros(nu), clip_hi=np.ones(nu), bang=0.0, delta=1e-3, max_sweeps=5,
             xs=s(R, 5, ns), us=s(R, 5, nu), adjs=s(R, 5, ns), sweeps=i32(R))
  return a


def _bad_opts(eng, **kw):
  o = eng.default_opts()
  for k, v in kw.items():
    setattr(o, k, v)
  return o


def test_argument_errors_keep_their_codes_and_texts():
  """(entry point, fault) -> (return code, text of myr_last_error), one call per row, as the entry points answer today -- the order of their checks included:
  myr_eval and myr_rollout return MYR_OK for an empty batch before they look at the stride, the products and myr_fit_grad look first.  No row reaches a kernel."""
  from myriad_amd import _lib
  ARG, UNSUP = -1, -2
  engines = {"cart": _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", 3, 2.0), "node": _lib.Engine("NODE_CARTPOLE", "HERMITE_SIMPSON", 3, 2.0),
             "plant": _lib.Engine("INVASIVEPLANT", "HERMITE_SIMPSON", 3, 2.0), "twin": _lib.Engine("CARTPOLE_ELASTIC", "HERMITE_SIMPSON", 3, 2.0)}
  P = lambda eng, B=2: np.ones((B, eng.np))      # a set of parameters per instance
  direct = ("myr_eval", "myr_vjp", "myr_jvp", "myr_exgd", "myr_rollout", "myr_solve", "myr_solve_x0", "myr_fit_grad")
  nulls = {"myr_eval": ("z", "null handle or z"), "myr_vjp": ("out", "null handle or array"), "myr_jvp": ("w", "null handle or array"),
           "myr_exgd": ("lam", "null handle or array"), "myr_rollout": ("us", "null handle, x0 or us"), "myr_solve": ("ub", "null handle, z, lb or ub"),
           "myr_solve_x0": ("g1", "null handle, x0s, g0, g1, lb, ub or z"), "myr_fit_grad": ("grad", "null handle, xs_obs, us or grad"),
           "myr_fbsm": ("clip_hi", "null handle or array")}
  # (entry point, handle, B, changed arguments or a function of the engine that gives them, null handle?, code, text)
  rows = []
  for ep, (name, text) in nulls.items():
    eng = "plant" if ep == "myr_fbsm" else "cart"
    rows.append((ep, eng, 2, {name: None}, False, ARG, f"{ep}: {text}"))
    rows.append((ep, eng, 2, {}, True, ARG, f"{ep}: {text}"))
  for ep in direct:
    rows.append((ep, "plant", 2, {}, False, UNSUP, f"{ep}: INVASIVEPLANT is a discrete-time system; only myr_fbsm is available for it"))
    rows.append((ep, "cart", 2, lambda e: dict(params=P(e), stride=3), False, ARG, f"{ep}: params_stride must be 0 (shared) or np"))
    rows.append((ep, "cart", 2, {"mem": 2}, False, ARG, f"{ep}: bad mem kind"))
    rows.append((ep, "node", 2, {}, False, ARG, f"{ep}: a NODE system needs its weights in `params`"))
    rows.append((ep, "cart", 0, {}, False, 0, ""))
  for ep in ("myr_eval", "myr_vjp", "myr_jvp", "myr_exgd", "myr_solve", "myr_solve_x0"):
    rows.append((ep, "cart", -1, {}, False, ARG, f"{ep}: negative batch"))
  for ep in ("myr_eval", "myr_rollout"):      # an empty batch returns before the stride is looked at ...
    rows.append((ep, "cart", 0, lambda e: dict(params=P(e, 1), stride=3), False, 0, ""))
  for ep in ("myr_vjp", "myr_fit_grad"):      # ... here the stride comes first
    rows.append((ep, "cart", 0, lambda e: dict(params=P(e, 1), stride=3), False, ARG, f"{ep}: params_stride must be 0 (shared) or np"))
  rows += [
    ("myr_exgd", "cart", 2, {"ub": None}, False, ARG, "myr_exgd: null ub"),
    ("myr_exgd", "cart", 2, {"nsteps": -1}, False, ARG, "myr_exgd: negative nsteps"),
    ("myr_exgd", "cart", 2, {"nsteps": 0}, False, 0, ""),
    ("myr_rollout", "cart", -1, {}, False, ARG, "myr_rollout: bad sizes"),
    ("myr_rollout", "cart", 2, {"num_steps": 0}, False, ARG, "myr_rollout: bad sizes"),
    ("myr_rollout", "cart", 2, {"u_rows": 0}, False, ARG, "myr_rollout: bad sizes"),
    ("myr_fit_grad", "cart", -1, {}, False, ARG, "myr_fit_grad: bad sizes"),
    ("myr_fit_grad", "cart", 2, {"num_steps": 0}, False, ARG, "myr_fit_grad: bad sizes"),
    ("myr_fit_grad", "cart", 2, {"u_rows": 0}, False, ARG, "myr_fit_grad: bad sizes"),
    ("myr_fit_grad", "cart", 2, {"grad_stride": 3}, False, ARG, "myr_fit_grad: grad_stride must be 0 (one row: the sum over the batch) or np (a row per trajectory)"),
    ("myr_fit_grad", "twin", 2, {}, False, UNSUP, "myr_fit_grad: an elastic twin has no model of its own to fit; use the handle of its system"),
    ("myr_fit_grad", "node", 2, lambda e: dict(params=P(e), stride=e.np), False, UNSUP, "myr_fit_grad: a NODE system takes one shared set of weights (params_stride 0)"),
    ("myr_fbsm", "plant", -1, {}, False, ARG, "myr_fbsm: bad sizes"),
    ("myr_fbsm", "plant", 2, {"N": 0}, False, ARG, "myr_fbsm: bad sizes"),
    ("myr_fbsm", "plant", 2, {"max_sweeps": 0}, False, ARG, "myr_fbsm: bad sizes"),
    ("myr_fbsm", "plant", 2, {"mem": 1}, False, ARG, "myr_fbsm: host arrays only"),
    ("myr_fbsm", "plant", 2, {"mem": 2}, False, ARG, "myr_fbsm: host arrays only"),
    ("myr_fbsm", "plant", 2, lambda e: dict(params=P(e), stride=e.np + 1), False, ARG, "myr_fbsm: params_stride must be 0 (shared) or np"),
    ("myr_fbsm", "plant", 2, {}, False, ARG, "myr_fbsm: a discrete system needs `params`"),
    ("myr_fbsm", "plant", 0, {}, False, 0, ""),
  ]
  for ep in ("myr_solve", "myr_solve_x0"):
    for kw in (dict(max_iter=-1), dict(tol_feas=0.0), dict(tol_stat=-1.0), dict(tol_compl=0.0), dict(mu_init=0.0)):
      rows.append((ep, "cart", 2, lambda e, kw=kw: dict(opts=_bad_opts(e, **kw)), False, ARG, f"{ep}: bad options"))
  try:
    for ep, which, B, change, null_handle, code, text in rows:
      eng = engines[which]
      a = _abi_defaults(ep, eng, B)
      a.update(change(eng) if callable(change) else change)
      before = {k: a[k].copy() for k in _OUTPUTS[ep] if isinstance(a[k], np.ndarray)}
      rc, out = _abi_call(ep, eng, a, handle=not null_handle)
      msg = eng.lib.myr_last_error().decode()
      assert rc == code, (ep, which, B, change if not callable(change) else "...", rc, msg)
      if code != 0:
        assert text in msg, (ep, which, B, msg)
      else:      # nothing to do: nothing is written
        for k in before:
          assert out[k].tobytes() == before[k].tobytes(), (ep, k)
  finally:
    for e in engines.values():
      e.close()
