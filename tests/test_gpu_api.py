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
# the derivative family: the sets calls take E, R where the others take B
_EXGD_GRAD_TAIL = ("eta_x", "eta_v", "nsteps", "seed_z", "seed_lam", "grad", "grad_stride", "dz0", "dlam0", "mem")
_HVP_TAIL = ("with_cost", "out_z", "out_p", "p_stride", "mem")
_ORDER.update({
  "myr_exgd_grad": ("B", "z", "lam", "lb", "ub", "params", "stride") + _EXGD_GRAD_TAIL,
  "myr_exgd_grad_shoot": ("B", "z", "lam", "lb", "ub", "params", "stride") + _EXGD_GRAD_TAIL,
  "myr_exgd_grad_node": ("B", "z", "lam", "lb", "ub", "params") + _EXGD_GRAD_TAIL,
  "myr_exgd_grad_node_shoot": ("B", "z", "lam", "lb", "ub", "params") + _EXGD_GRAD_TAIL,
  "myr_exgd_grad_node_sets": ("E", "R", "z", "lam", "lb", "ub", "params") + _EXGD_GRAD_TAIL,
  "myr_hvp": ("B", "z", "lam", "v", "params", "stride") + _HVP_TAIL,
  "myr_hvp_node": ("B", "z", "lam", "v", "params") + _HVP_TAIL,
  "myr_hvp_node_sets": ("E", "R", "z", "lam", "v", "params") + _HVP_TAIL,
  "myr_fit_grad_sets": ("E", "R", "num_steps", "u_rows", "xs_obs", "us", "data_shared", "wt", "params", "loss", "grad", "grad_stride", "mem"),
  "myr_fit_gn": ("B", "num_steps", "u_rows", "xs_obs", "us", "wt", "params", "stride", "loss", "grad", "gn", "out_stride", "mem"),
  "myr_fit_gn_sets": ("E", "R", "num_steps", "u_rows", "xs_obs", "us", "data_shared", "wt", "params", "loss", "grad", "gn", "out_stride", "mem"),
})
_EXGD_GRAD_EPS = ("myr_exgd_grad", "myr_exgd_grad_shoot", "myr_exgd_grad_node", "myr_exgd_grad_node_shoot", "myr_exgd_grad_node_sets")
_HVP_EPS = ("myr_hvp", "myr_hvp_node", "myr_hvp_node_sets")
_SETS_EPS = ("myr_exgd_grad_node_sets", "myr_hvp_node_sets", "myr_fit_grad_sets", "myr_fit_gn_sets")
_FIT_EPS = ("myr_fit_grad", "myr_fit_grad_sets", "myr_fit_gn", "myr_fit_gn_sets")
_OUTPUTS = {"myr_eval": ("f", "g", "c", "j"), "myr_vjp": ("out",), "myr_jvp": ("out",), "myr_exgd": ("z", "lam"), "myr_rollout": ("xs", "cost"),
            "myr_solve": ("z", "lam", "cost", "status", "iters", "kkt"), "myr_solve_x0": ("z", "lam", "cost", "status", "iters", "kkt"),
            "myr_fit_grad": ("loss", "grad"), "myr_fbsm": ("xs", "us", "adjs", "sweeps"), "myr_fit_grad_sets": ("loss", "grad")}
_OUTPUTS.update({ep: ("grad", "dz0", "dlam0") for ep in _EXGD_GRAD_EPS})
_OUTPUTS.update({ep: ("out_z", "out_p") for ep in _HVP_EPS})
_OUTPUTS.update({"myr_fit_gn": ("loss", "grad", "gn"), "myr_fit_gn_sets": ("loss", "grad", "gn")})


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
  # the derivative family at the smallest shapes that go through every staging item: B = 1 and 3 (E = 2 sets of R = 2), two extragradient steps, the row
  # stride 0 and np, every optional array present and absent, the three params forms where the entry point has a stride
  node = lambda: _lib.Engine("NODE_CARTPOLE", "HERMITE_SIMPSON", 3, 2.0)
  node_sh = lambda: _lib.Engine("NODE_CARTPOLE", "SHOOTING", 2, 2.0, controls_per_interval=2)
  for make, default, grads, hvps in ((cart(3), [9.81, 1.0, 0.3, 0.5], ("myr_exgd_grad",), ("myr_hvp",)), (vdp, None, ("myr_exgd_grad_shoot",), ("myr_hvp",)),
                                     (node, None, ("myr_exgd_grad_node", "myr_exgd_grad_node_sets"), ("myr_hvp_node", "myr_hvp_node_sets")),
                                     (node_sh, None, ("myr_exgd_grad_node_shoot", "myr_exgd_grad_node_sets"), ("myr_hvp_node", "myr_hvp_node_sets"))):
    eng = make()
    n, m, ns, nu, npar = eng.n, eng.m, eng.ns, eng.nu, eng.np
    is_node = eng.desc.system_id == _lib.SYS_IDS["NODE_CARTPOLE"]
    if default is None:
      default = 0.1 * rng.standard_normal(npar) if is_node else np.ones(npar)
    for ep in grads + hvps + ("myr_fit_grad_sets",):
      sets = ep in _SETS_EPS
      for lead in (((2, 2),) if sets else ((1,), (3,))):
        B = int(np.prod(lead))
        arr = lambda w, scale=1.0: scale * rng.standard_normal(lead + (w,))
        if sets:
          sizes, forms = dict(E=2, R=2), [(np.stack([np.asarray(default, dtype=np.float64) * (1.0 + 0.01 * e) for e in range(2)]), 0)]
        else:
          sizes, forms = dict(B=B), ([(np.asarray(default, dtype=np.float64), 0)] if is_node else _params_forms(default, B))
        for p, ps in forms:
          for stride in (0, npar):
            rows = (lead if stride else lead[:-1]) + (npar,)
            common = dict(sizes, params=p, stride=ps)
            if ep in grads:
              for full in (True, False):
                _same_bits(ep, eng, make, dict(common, z=arr(n, 0.3), lam=arr(m), lb=np.full(lead + (n,), -5.0), ub=np.full(lead + (n,), 5.0), eta_x=1e-3,
                                               eta_v=1e-3, nsteps=2, seed_z=arr(n), seed_lam=arr(m) if full else None, grad=_nan(*rows), grad_stride=stride,
                                               dz0=_nan(*lead, n) if full else None, dlam0=_nan(*lead, m) if full else None))
            elif ep in hvps:
              for with_lam, with_z, with_p, with_cost in ((True, True, True, 1), (False, False, True, 1), (True, True, False, 0)):
                _same_bits(ep, eng, make, dict(common, z=arr(n, 0.3), lam=arr(m) if with_lam else None, v=arr(n), with_cost=with_cost,
                                               out_z=_nan(*lead, n) if with_z else None, out_p=_nan(*rows) if with_p else None, p_stride=stride))
            elif eng.desc.transcription != _lib.TR_IDS["SHOOTING"]:      # (a rollout: the transcription plays no part, one handle per system is enough)
              S = 4
              for with_wt, with_loss, with_grad, shared in ((True, True, True, 0), (False, False, True, 1), (False, True, False, 0)):
                dlead = lead[1:] if shared else lead
                xs_obs = 0.1 * rng.standard_normal(dlead + (S + 1, ns)); us = 0.2 * rng.standard_normal(dlead + (S + 1, nu))
                _same_bits(ep, eng, make, dict(common, num_steps=S, u_rows=S + 1, xs_obs=xs_obs, us=us, data_shared=shared,
                                               wt=np.linspace(0.5, 1.5, S + 1) if with_wt else None, loss=_nan(*lead) if with_loss else None,
                                               grad=_nan(*rows) if with_grad else None, grad_stride=stride))
    eng.close()
  # the fit family, two steps: B = 1 and 3 (E = 2 sets of R = 2), the row stride 0 and np, loss and grad present and null, data per set and shared, the
  # three params forms of the single-set calls; closed form under RK4 (two control rows a step), the network under HEUN (the gradient calls only:
  # myr_fit_gn* refuse it)
  S = 2
  cart_rk4 = lambda: _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", 3, 2.0, integration_method="RK4")
  node_heun = lambda: _lib.Engine("NODE_CARTPOLE", "HERMITE_SIMPSON", 3, 2.0, integration_method="HEUN")
  for make, default, u_rows, eps in ((cart_rk4, np.array([9.81, 1.0, 0.3, 0.5]), 2 * S + 1, _FIT_EPS), (node_heun, None, S + 1, _FIT_EPS[:2])):
    eng = make()
    ns, nu, npar = eng.ns, eng.nu, eng.np
    is_node = default is None
    if is_node:
      default = 0.1 * rng.standard_normal(npar)
    for ep in eps:
      sets, gn = ep in _SETS_EPS, "_gn" in ep
      for lead in (((2, 2),) if sets else ((1,), (3,))):
        B = int(np.prod(lead))
        if sets:
          sizes, forms = dict(E=2, R=2), [(np.stack([default * (1.0 + 0.01 * e) for e in range(2)]), None)]
        else:
          sizes, forms = dict(B=B), ([(default, 0)] if is_node else _params_forms(default, B))
        for p, ps in forms:
          for stride in (0, npar):
            rows = (lead if stride else lead[:-1]) + (npar,)
            for shared in ((0, 1) if sets else (None,)):
              dlead = lead[1:] if shared else lead
              for with_loss, with_grad in ((True, True), (False, True), (True, False), (False, False)):
                if not with_grad and ep == "myr_fit_grad" or not (with_loss or with_grad or gn):      # (myr_fit_grad needs grad, its sets form one of the two)
                  continue
                a = dict(sizes, params=p, num_steps=S, u_rows=u_rows, xs_obs=0.1 * rng.standard_normal(dlead + (S + 1, ns)),
                         us=0.2 * rng.standard_normal(dlead + (u_rows, nu)), wt=np.linspace(0.5, 1.5, S + 1) if with_loss else None,
                         loss=_nan(*lead) if with_loss else None, grad=_nan(*rows) if with_grad else None)
                a.update({} if sets else dict(stride=ps), **({"data_shared": shared} if sets else {}))
                a.update(dict(gn=_nan(*rows, npar), out_stride=stride) if gn else dict(grad_stride=stride))
                out = _same_bits(ep, eng, make, a)
                assert all(np.isfinite(v).all() for v in out.values()), ep      # every array that was handed over has been written
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
  elif ep == "myr_fit_gn":      # (the network system is refused: its gn is a token array, not 4 804 x 4 804 doubles)
    npar = max(eng.np, 1)
    a.update(num_steps=4, u_rows=5, xs_obs=np.zeros((R, 5, ns)), us=np.zeros((R, 5, nu)), wt=None, loss=s(R), grad=s(R, npar),
             gn=s(R, npar, npar) if npar <= 64 else s(R, 1), out_stride=eng.np)
  elif ep == "myr_fbsm":
    a.update(N=4, x0=np.ones((R, ns)), adj_T=None, clip_lo=np.zeros(nu), clip_hi=np.ones(nu), bang=0.0, delta=1e-3, max_sweeps=5,
             xs=s(R, 5, ns), us=s(R, 5, nu), adjs=s(R, 5, ns), sweeps=i32(R))
  elif ep in _EXGD_GRAD_EPS + _HVP_EPS + ("myr_fit_grad_sets", "myr_fit_gn_sets"):      # (a sets call: B is its E, of two instances each)
    sets, npar = ep in _SETS_EPS, max(eng.np, 1)
    lead = (R, 2) if sets else (R,)
    a.update(E=B, R=2)
    if "_node" in ep:
      a.update(params=np.zeros((R, npar) if sets else npar))
    if ep in _EXGD_GRAD_EPS:
      a.update(z=np.zeros(lead + (n,)), lam=np.zeros(lead + (m,)), lb=np.full(lead + (n,), -10.0), ub=np.full(lead + (n,), 10.0), eta_x=1e-3, eta_v=1e-3,
               nsteps=1, seed_z=np.ones(lead + (n,)), seed_lam=None, grad=s(*lead, npar), grad_stride=eng.np, dz0=s(*lead, n), dlam0=s(*lead, m))
    elif ep in _HVP_EPS:
      a.update(z=np.zeros(lead + (n,)), lam=np.zeros(lead + (m,)), v=np.ones(lead + (n,)), with_cost=1, out_z=s(*lead, n), out_p=s(*lead, npar), p_stride=eng.np)
    else:
      a.update(num_steps=4, u_rows=5, xs_obs=np.zeros(lead + (5, ns)), us=np.zeros(lead + (5, nu)), data_shared=0, wt=None, params=np.ones((R, npar)),
               loss=s(*lead), grad=s(*lead, npar), grad_stride=eng.np)
      if ep == "myr_fit_gn_sets":      # (out_stride where its sibling has grad_stride; the network system's gn: as for myr_fit_gn)
        del a["grad_stride"]
        a.update(gn=s(*lead, npar, npar) if npar <= 64 else s(*lead, 1), out_stride=eng.np)
  return a


def _bad_opts(eng, **kw):
  o = eng.default_opts()
  for k, v in kw.items():
    setattr(o, k, v)
  return o


def _derivative_rows():
  """The rows of the derivative family (myr_exgd_grad*, myr_hvp*, myr_fit_grad_sets), written check by check from the entry points: every refusal they
  can give with its full text, the empty call, and two faults at once wherever two siblings look in a different order.  For a sets call the
  batch column is E (R = 2)."""
  ARG, UNSUP, CAP = -1, -2, -4
  home = {"myr_exgd_grad": "cart", "myr_exgd_grad_shoot": "vdp_sh", "myr_exgd_grad_node": "node", "myr_exgd_grad_node_shoot": "node_sh",
          "myr_exgd_grad_node_sets": "node", "myr_hvp": "cart", "myr_hvp_node": "node", "myr_hvp_node_sets": "node_sh", "myr_fit_grad_sets": "cart"}
  off = lambda key: (lambda e: {key: e.np + 1})      # a row stride that is neither 0 nor np
  weights = lambda e: dict(params=np.zeros(e.np))
  plant_text = "INVASIVEPLANT is a discrete-time system; only myr_fbsm is available for it"
  twin_text = "an elastic twin has no model of its own to differentiate; use the handle of its system"
  row_batch = "must be 0 (one row: the sum over the batch) or np (a row per instance)"
  row_sets = "must be 0 (a row per set: the sum over its instances) or np (a row per instance)"
  sizes_text = "bad sizes (E >= 0 sets of R >= 1 instances, E * R an int)"
  tz_text = "TRAPEZOIDAL is not built for the network system; HERMITE_SIMPSON and SHOOTING only"
  lds_hs = "intervals too large for the LDS-resident reverse sweep beside the weight copy"
  lds_sh = "intervals x controls_per_interval too large for the LDS-resident sweep beside the weight copy"
  lds_pairs = "intervals x controls_per_interval too large for the LDS-resident pair records beside the weight copy"
  rows = []
  add = lambda ep, which, B, change, code, text, null_handle=False: rows.append((ep, which, B, change, null_handle, code, f"{ep}: {text}" if text else ""))
  for ep in _EXGD_GRAD_EPS:
    h = home[ep]
    add(ep, h, 2, {}, ARG, "null handle or array", null_handle=True)
    for k in ("z", "lam", "lb"):
      add(ep, h, 2, {k: None}, ARG, "null handle or array")
    add(ep, h, 2, {"ub": None}, ARG, "null ub")
    add(ep, h, 2, {"nsteps": -1}, ARG, "negative nsteps")
    add(ep, h, 2, {"seed_z": None}, ARG, "null seed_z or grad")
    add(ep, h, 2, {"grad": None}, ARG, "null seed_z or grad")
    add(ep, h, 2, off("grad_stride"), ARG, "grad_stride " + (row_sets if ep in _SETS_EPS else row_batch))
    add(ep, h, 2, {"mem": 2}, ARG, "bad mem kind")
    add(ep, h, 0, {}, 0, "")
    add(ep, h, 2, {"ub": None, "nsteps": -1, "seed_z": None}, ARG, "null ub")      # the run ub, nsteps, seed_z or grad: in this order everywhere
    add(ep, h, 2, {"nsteps": -1, "grad": None}, ARG, "negative nsteps")
  for ep in ("myr_exgd_grad", "myr_exgd_grad_shoot"):
    add(ep, "plant", 2, {}, UNSUP, plant_text)
    add(ep, "plant", -1, {}, UNSUP, plant_text)
    add(ep, home[ep], -1, {}, ARG, "negative batch")
    add(ep, home[ep], 2, lambda e: dict(params=np.ones((2, e.np)), stride=e.np + 2), ARG, "params_stride must be 0 (shared) or np")
    add(ep, "node", 2, {}, ARG, "a NODE system needs its weights in `params`")
    add(ep, "twin", 2, {}, UNSUP, twin_text)
    add(ep, "twin", 2, off("grad_stride"), ARG, "grad_stride " + row_batch)      # the stride is looked at before the kind of system
    add(ep, "twin", 2, {"mem": 2}, UNSUP, twin_text)
  add("myr_exgd_grad", "node", 2, weights, UNSUP, "the network system is not built (second derivatives in 4 804 weights)")
  add("myr_exgd_grad", "vdp_sh", 2, {}, UNSUP, "SHOOTING is not built (it needs the second-order adjoint of the rollout); use a collocation transcription")
  add("myr_exgd_grad", "vdp_sh", 2, {"mem": 2}, UNSUP, "SHOOTING is not built (it needs the second-order adjoint of the rollout); use a collocation transcription")
  add("myr_exgd_grad_shoot", "node", 2, weights, UNSUP, "the network system is not built (second derivatives in 4 804 weights); myr_exgd_grad_node has HERMITE_SIMPSON")
  add("myr_exgd_grad_shoot", "cart", 2, {}, UNSUP, "this handle's transcription is not SHOOTING; use myr_exgd_grad")
  add("myr_exgd_grad_shoot", "cart", 0, {}, UNSUP, "this handle's transcription is not SHOOTING; use myr_exgd_grad")
  for ep, use in (("myr_exgd_grad_node", "myr_exgd_grad"), ("myr_exgd_grad_node_shoot", "myr_exgd_grad_shoot"),
                  ("myr_exgd_grad_node_sets", "myr_exgd_grad or myr_exgd_grad_shoot"), ("myr_hvp_node", "myr_hvp"), ("myr_hvp_node_sets", "myr_hvp")):
    for B in (2, 0):
      add(ep, "cart", B, {}, UNSUP, f"this handle's system is not the network system; use {use}")
    add(ep, "cart", 2, {"mem": 2}, UNSUP, f"this handle's system is not the network system; use {use}")
    key = "grad_stride" if ep in _EXGD_GRAD_EPS else "p_stride"
    add(ep, "cart", 2, off(key), UNSUP, f"this handle's system is not the network system; use {use}")      # (a stride that is wrong for it too)
    if ep in ("myr_exgd_grad_node_sets", "myr_hvp_node", "myr_hvp_node_sets"):
      add(ep, "node_tz", 2, off(key), UNSUP, tz_text)
    if ep in _SETS_EPS:
      add(ep, home[ep], 2, {"params": None}, ARG, "null params (the [E][np] weight sets)")
      for change in ({"R": 0}, {"E": 65536, "R": 65536}):
        add(ep, home[ep], 2, change, ARG, sizes_text)
      add(ep, home[ep], -1, {}, ARG, sizes_text)
      add(ep, home[ep], 2, lambda e, key=key: {"R": 0, key: e.np + 1, "mem": 2}, ARG, sizes_text)
    else:
      add(ep, home[ep], 2, {"params": None}, ARG, "a NODE system needs its weights in `params`")
      add(ep, home[ep], -1, {}, ARG, "negative batch")
      add(ep, home[ep], -1, lambda e, key=key: {key: e.np + 1, "mem": 2}, ARG, "negative batch")
    add(ep, home[ep], 2, lambda e, key=key: {key: e.np + 1, "mem": 2}, ARG, f"{key} " + (row_sets if ep in _SETS_EPS else row_batch))
  # myr_exgd_grad_node and its siblings look at the batch before the weights, myr_hvp_node and myr_hvp_node_sets at the weights first
  add("myr_exgd_grad_node", "node", -1, {"params": None}, ARG, "negative batch")
  add("myr_exgd_grad_node_shoot", "node_sh", -1, {"params": None}, ARG, "negative batch")
  add("myr_exgd_grad_node_sets", "node", -1, {"params": None}, ARG, sizes_text)
  add("myr_hvp_node", "node", -1, {"params": None}, ARG, "a NODE system needs its weights in `params`")
  add("myr_hvp_node_sets", "node_sh", -1, {"params": None}, ARG, "null params (the [E][np] weight sets)")
  # ... and the exgd_grad calls at the sizes before the system, the hvp calls at the system first
  add("myr_exgd_grad_node", "cart", -1, {}, ARG, "negative batch")
  add("myr_exgd_grad_node_sets", "cart", -1, {}, ARG, sizes_text)
  add("myr_hvp_node", "cart", -1, {"params": None}, UNSUP, "this handle's system is not the network system; use myr_hvp")
  add("myr_hvp_node_sets", "cart", -1, {"params": None}, UNSUP, "this handle's system is not the network system; use myr_hvp")
  for ep in ("myr_hvp_node", "myr_hvp_node_sets"):      # ... whatever else is wrong with the call
    add(ep, "cart", -1, lambda e: dict(p_stride=e.np + 1, mem=2), UNSUP, "this handle's system is not the network system; use myr_hvp")
    add(ep, "node_tz", -1, lambda e: dict(p_stride=e.np + 1, mem=2), UNSUP, tz_text)
    add(ep, "node_tz", 2, {"out_z": None, "out_p": None}, ARG, "both outputs are null")
  add("myr_hvp_node", "node_sh", 0, {}, 0, "")
  # the transcriptions of the network system
  hs_only = "HERMITE_SIMPSON only, the one transcription myr_vjp / myr_exgd build for the network system"
  add("myr_exgd_grad_node", "node_sh", 2, {}, UNSUP, hs_only)
  add("myr_exgd_grad_node", "node_tz", 2, {"params": None}, UNSUP, hs_only)
  add("myr_exgd_grad_node_shoot", "node", 2, {}, UNSUP, "this handle's transcription is HERMITE_SIMPSON, not SHOOTING; use myr_exgd_grad_node")
  add("myr_exgd_grad_node_shoot", "node_tz", 2, {"params": None}, UNSUP, "TRAPEZOIDAL is not built for the network system; SHOOTING only")
  for ep in ("myr_exgd_grad_node_sets", "myr_hvp_node", "myr_hvp_node_sets"):
    add(ep, "node_tz", 2, {"params": None}, UNSUP, tz_text)
    add(ep, "node_tz", 0, {"mem": 2}, UNSUP, tz_text)
  # past the LDS bounds (an empty call is refused too: the bound belongs to the handle); the other checks come first
  for ep, which, text in (("myr_exgd_grad_node", "node_hs_big", lds_hs), ("myr_exgd_grad_node_shoot", "node_sh_big", lds_sh),
                          ("myr_exgd_grad_node_sets", "node_hs_big", lds_hs), ("myr_exgd_grad_node_sets", "node_sh_big", lds_sh),
                          ("myr_hvp_node", "node_sh_big", lds_pairs), ("myr_hvp_node_sets", "node_sh_big", lds_pairs)):
    add(ep, which, 0, {}, CAP, text)
    add(ep, which, 0, {"mem": 2}, ARG, "bad mem kind")
  for ep in ("myr_hvp_node", "myr_hvp_node_sets"):      # Hermite-Simpson has no bound here
    add(ep, "node_hs_big", 0, {}, 0, "")
  # the products
  for ep in _HVP_EPS:
    h = home[ep]
    add(ep, h, 2, {}, ARG, "null handle, z or v", null_handle=True)
    add(ep, h, 2, {"z": None}, ARG, "null handle, z or v")
    add(ep, h, 2, {"v": None}, ARG, "null handle, z or v")
    add(ep, h, 2, {"out_z": None, "out_p": None}, ARG, "both outputs are null")
    add(ep, "plant" if ep == "myr_hvp" else "cart", -1, {"out_z": None, "out_p": None, "mem": 2}, ARG, "both outputs are null")
    add(ep, h, 2, off("p_stride"), ARG, "p_stride " + (row_sets if ep in _SETS_EPS else row_batch))
    add(ep, h, 2, {"mem": 2}, ARG, "bad mem kind")
    add(ep, h, 0, {}, 0, "")
  for ep in ("myr_hvp_node", "myr_hvp_node_sets"):
    add(ep, "node", 0, {}, 0, "")
  add("myr_exgd_grad_node_sets", "node_sh", 0, {}, 0, "")
  add("myr_hvp", "plant", 2, {}, UNSUP, plant_text)
  add("myr_hvp", "plant", -1, {}, UNSUP, plant_text)      # the kind of system before the batch
  add("myr_hvp", "twin", -1, {}, UNSUP, twin_text)
  add("myr_hvp", "node", -1, weights, UNSUP, "the network system is not built (second derivatives in 4 804 weights)")
  add("myr_hvp", "node", 2, {}, UNSUP, "the network system is not built (second derivatives in 4 804 weights)")
  add("myr_hvp", "cart", -1, {}, ARG, "negative batch")
  add("myr_hvp", "cart", -1, off("p_stride"), ARG, "negative batch")
  add("myr_hvp", "cart", 2, lambda e: dict(params=np.ones((2, e.np)), stride=e.np + 2), ARG, "params_stride must be 0 (shared) or np")
  add("myr_hvp", "cart", 2, lambda e: dict(params=np.ones((2, e.np)), stride=e.np + 2, p_stride=e.np + 1), ARG, "p_stride " + row_batch)
  add("myr_hvp", "cart", 0, lambda e: dict(params=np.ones((1, e.np)), stride=e.np + 2), ARG, "params_stride must be 0 (shared) or np")
  add("myr_hvp", "cart", 2, lambda e: dict(params=np.ones((2, e.np)), stride=e.np + 2, mem=2), ARG, "params_stride must be 0 (shared) or np")
  add("myr_hvp", "cart", 0, {"mem": 2}, ARG, "bad mem kind")      # the memory kind before the empty batch returns
  add("myr_hvp", "cart", 2, {"z": None, "out_z": None, "out_p": None}, ARG, "null handle, z or v")
  add("myr_hvp", "cart", -1, {"out_z": None, "out_p": None}, ARG, "both outputs are null")
  for which, text in (("plant", plant_text), ("twin", twin_text), ("node", "the network system is not built (second derivatives in 4 804 weights)")):
    add("myr_hvp", which, 0, weights, UNSUP, text)
    add("myr_hvp", which, 2, {"out_z": None, "out_p": None}, ARG, "both outputs are null")      # ... behind the null checks
  add("myr_exgd_grad_shoot", "node_sh", 2, weights, UNSUP, "the network system is not built (second derivatives in 4 804 weights); myr_exgd_grad_node has HERMITE_SIMPSON")
  add("myr_hvp", "node_sh", 2, weights, UNSUP, "the network system is not built (second derivatives in 4 804 weights)")
  # myr_fit_grad_sets: the arguments first, the system last; a twin and a system without derivatives are answered in myr_fit_grad's name
  ep = "myr_fit_grad_sets"
  add(ep, "cart", 2, {}, ARG, "null handle, xs_obs, us or params", null_handle=True)
  for k in ("xs_obs", "us", "params"):
    add(ep, "cart", 2, {k: None}, ARG, "null handle, xs_obs, us or params")
  add(ep, "cart", 2, {"loss": None, "grad": None}, ARG, "loss and grad are both null")
  for change in ({"E": -1}, {"R": 0}, {"num_steps": 0}, {"u_rows": 0}):
    add(ep, "cart", 2, change, ARG, "bad sizes")
  add(ep, "cart", 2, off("grad_stride"), ARG, "grad_stride must be 0 (a row per set: the sum over its trajectories) or np (a row per trajectory)")
  add(ep, "cart", 2, {"data_shared": 2}, ARG, "data_shared must be 0 (data per set) or 1 (one set of data, read by every set)")
  add(ep, "cart", 2, {"data_shared": -1, "mem": 2}, ARG, "data_shared must be 0 (data per set) or 1 (one set of data, read by every set)")
  add(ep, "cart", 2, {"mem": 2}, ARG, "bad mem kind")
  add(ep, "plant", 2, {}, UNSUP, plant_text)
  add(ep, "plant", 2, {"mem": 2}, ARG, "bad mem kind")
  add(ep, "plant", 0, {}, UNSUP, plant_text)
  add(ep, "cart", 0, {}, 0, "")
  add(ep, "node", 0, {}, 0, "")
  rows.append((ep, "twin", 2, {}, False, UNSUP, "myr_fit_grad: an elastic twin has no model of its own to fit; use the handle of its system"))
  rows.append((ep, "twin", 0, {}, False, UNSUP, "myr_fit_grad: an elastic twin has no model of its own to fit; use the handle of its system"))
  return rows


def _fit_rows():
  """The rows of the fit family (myr_fit_grad, myr_fit_grad_sets, myr_fit_gn, myr_fit_gn_sets), written check by check from the entry points as
  _derivative_rows() was (which has the first rows of myr_fit_grad_sets, as the test's own list has the first of myr_fit_grad): every refusal a
  handle can reach, the empty calls, and two faults at once wherever two of the four look in a different order.  myr_fit_grad looks at the system
  before its sizes, the other three at every argument first; a twin is answered in myr_fit_grad's name by all four."""
  ARG, UNSUP = -1, -2
  plant_text = "INVASIVEPLANT is a discrete-time system; only myr_fbsm is available for it"
  twin = "myr_fit_grad: an elastic twin has no model of its own to fit; use the handle of its system"
  node_gn = "the network system's 4 804 x 4 804 Gauss-Newton matrix is not formed; use myr_fit_grad for its loss and gradient"
  node_stride = "a NODE system takes one shared set of weights (params_stride 0)"
  row = lambda key, sets: (f"{key} must be 0 (a row per set: the sum over its trajectories) or np (a row per trajectory)" if sets else
                           f"{key} must be 0 (one row: the sum over the batch) or np (a row per trajectory)")
  shared_text = "data_shared must be 0 (data per set) or 1 (one set of data, read by every set)"
  pstride_text = "params_stride must be 0 (shared) or np"
  nulls = {"myr_fit_grad": (("xs_obs", "us", "grad"), "null handle, xs_obs, us or grad"),
           "myr_fit_grad_sets": (("xs_obs", "us", "params"), "null handle, xs_obs, us or params"),
           "myr_fit_gn": (("xs_obs", "us", "gn"), "null handle, xs_obs, us or gn"),
           "myr_fit_gn_sets": (("xs_obs", "us", "gn", "params"), "null handle, xs_obs, us, gn or params")}
  rows = []
  def add(ep, which, B, change, code, text, null_handle=False):
    rows.append((ep, which, B, change, null_handle, code, text if not text or text.startswith("myr_fit_grad: ") else f"{ep}: {text}"))
  bad_pstride = lambda e: dict(params=np.ones((2, e.np)), stride=e.np + 2)
  weights = lambda e: dict(params=np.zeros(e.np))
  for ep in _FIT_EPS:
    sets, gn = ep in _SETS_EPS, "_gn" in ep
    key = "out_stride" if gn else "grad_stride"
    off = lambda e, key=key: {key: e.np + 1}
    batch = "E" if sets else "B"
    names, null_text = nulls[ep]
    # the null checks come first everywhere, whatever the handle is of
    add(ep, "cart", 2, {}, ARG, null_text, null_handle=True)
    add(ep, "cart", -1, {"num_steps": 0, "mem": 2}, ARG, null_text, null_handle=True)
    for k in names:
      add(ep, "cart", 2, {k: None}, ARG, null_text)
      add(ep, "plant", -1, {k: None, "mem": 2}, ARG, null_text)
      add(ep, "twin", -1, lambda e, k=k, key=key: {k: None, key: e.np + 1}, ARG, null_text)
    # the sizes, one at a time and in front of the row stride, the params stride, data_shared and the memory kind
    for change in ({batch: -1}, {"num_steps": 0}, {"u_rows": 0}) + (({"R": 0},) if sets else ()):
      add(ep, "cart", 2, change, ARG, "bad sizes")
    add(ep, "cart", -1, lambda e, key=key: {key: e.np + 1, "mem": 2, "u_rows": 0}, ARG, "bad sizes")
    add(ep, "cart", 2, off, ARG, row(key, sets))
    add(ep, "cart", 0, lambda e, key=key: {key: e.np + 1, "mem": 2}, ARG, row(key, sets))      # ... the row stride in front of the memory kind and the empty call
    add(ep, "cart", 2, {"mem": 2}, ARG, "bad mem kind")
    add(ep, "cart", 0, {"mem": 2}, ARG, "bad mem kind")      # the memory kind before the empty call returns
    add(ep, "cart", 0, {}, 0, "")
    add(ep, "cart", 0, {"loss": None}, 0, "")
    if sets:
      add(ep, "cart", 2, {"data_shared": 2}, ARG, shared_text)
      add(ep, "cart", 0, {"data_shared": -1, "mem": 2}, ARG, shared_text)      # data_shared behind the row stride, in front of the memory kind
      add(ep, "cart", 2, lambda e, key=key: {key: e.np + 1, "data_shared": 2}, ARG, row(key, sets))
      add(ep, "cart", 0, {"data_shared": 1}, 0, "")
      add(ep, "cart", 2, {"num_steps": 0, "data_shared": 2}, ARG, "bad sizes")      # the sizes in front of data_shared
    else:
      add(ep, "cart", 2, bad_pstride, ARG, pstride_text)
      add(ep, "cart", 0, lambda e: dict(params=np.ones((1, e.np)), stride=e.np + 2, mem=2), ARG, pstride_text)      # the params stride in front of the memory kind
      add(ep, "cart", 2, lambda e, key=key: dict(bad_pstride(e), **{key: e.np + 1}), ARG, row(key, sets))      # ... and behind the row stride
      add(ep, "cart", 2, lambda e: dict(bad_pstride(e), u_rows=0), ARG, "bad sizes")      # ... and behind the sizes
      add(ep, "cart", 0, lambda e: dict(params=np.ones(e.np)), 0, "")
      add(ep, "cart", 0, lambda e: dict(params=np.ones((1, e.np)), stride=e.np), 0, "")
    # the kind of system: myr_fit_grad in front of its sizes, the others behind every argument check and in front of the empty call
    for which, text in (("plant", plant_text), ("twin", twin)):
      add(ep, which, 2, {}, UNSUP, text)
      add(ep, which, 0, {}, UNSUP, text)
      first = ep == "myr_fit_grad"
      add(ep, which, -1, {}, *((UNSUP, text) if first else (ARG, "bad sizes")))
      add(ep, which, 2, {"num_steps": 0, "mem": 2}, *((UNSUP, text) if first else (ARG, "bad sizes")))
      add(ep, which, 2, off, *((UNSUP, text) if first else (ARG, row(key, sets))))
      add(ep, which, 0, {"mem": 2}, *((UNSUP, text) if first else (ARG, "bad mem kind")))
      if sets:
        add(ep, which, 2, {"data_shared": 2}, ARG, shared_text)
  # myr_fit_grad on the network handle: the weights, then their stride, then the memory kind; the empty call with weights returns 0
  ep = "myr_fit_grad"
  add(ep, "node", 2, {"mem": 2}, ARG, "a NODE system needs its weights in `params`")
  add(ep, "node", 2, lambda e: dict(params=np.ones((2, e.np)), stride=e.np, mem=2), UNSUP, node_stride)
  add(ep, "node", 0, lambda e: dict(params=np.ones((1, e.np)), stride=e.np, mem=2), UNSUP, node_stride)
  add(ep, "node", 2, lambda e: dict(params=np.ones((2, e.np)), stride=e.np + 2), ARG, pstride_text)
  add(ep, "node", 2, lambda e: dict(weights(e), mem=2), ARG, "bad mem kind")
  add(ep, "node", -1, {}, ARG, "bad sizes")      # (the network system is neither refused kind: the sizes come first)
  add(ep, "node", 2, lambda e: dict(grad_stride=e.np + 1), ARG, row("grad_stride", False))
  add(ep, "node", 0, weights, 0, "")
  # myr_fit_grad_sets: loss and grad both null, behind the null checks and in front of the sizes; the network system is served
  ep = "myr_fit_grad_sets"
  add(ep, "cart", -1, {"loss": None, "grad": None, "R": 0}, ARG, "loss and grad are both null")
  add(ep, "plant", 2, {"loss": None, "grad": None}, ARG, "loss and grad are both null")
  add(ep, "cart", 2, {"loss": None, "grad": None, "us": None}, ARG, "null handle, xs_obs, us or params")
  add(ep, "cart", 0, {"grad": None}, 0, "")
  add(ep, "node", 2, {"mem": 2}, ARG, "bad mem kind")
  add(ep, "node", 2, {"data_shared": 2}, ARG, shared_text)
  # myr_fit_gn*: the network refusal behind the argument checks and in front of the empty call; loss and grad may both be null
  for ep in ("myr_fit_gn", "myr_fit_gn_sets"):
    sets = ep in _SETS_EPS
    for B in (2, 0):
      add(ep, "node", B, {}, UNSUP, node_gn)
      add(ep, "node", B, {"loss": None, "grad": None}, UNSUP, node_gn)
    add(ep, "node", 0, lambda e: dict(out_stride=e.np + 1), ARG, row("out_stride", sets))
    add(ep, "node", 0, {"mem": 2}, ARG, "bad mem kind")
    add(ep, "node", -1, {}, ARG, "bad sizes")
    add(ep, "node", 2, {"gn": None}, ARG, nulls[ep][1])
    add(ep, "cart", 0, {"loss": None, "grad": None}, 0, "")
  add("myr_fit_gn", "node", 2, weights, UNSUP, node_gn)      # (no weights check of its own: the system is refused with its weights and, above, without)
  add("myr_fit_gn", "node", 0, lambda e: dict(params=np.ones((1, e.np)), stride=e.np + 2), ARG, pstride_text)
  add("myr_fit_gn_sets", "node", 2, {"data_shared": 2}, ARG, shared_text)
  # myr_fit_gn_sets bounds E * R (an int: the lanes of one launch); no array is read.  (myr_fit_grad_sets has no such bound, and no row: it would launch.)
  add("myr_fit_gn_sets", "cart", 2, {"E": 65536, "R": 65536}, ARG, "bad sizes")
  add("myr_fit_gn_sets", "cart", 2, {"E": 65536, "R": 65536, "out_stride": 1, "data_shared": 2, "mem": 2}, ARG, "bad sizes")
  add("myr_fit_gn_sets", "node", 2, {"E": 65536, "R": 65536}, ARG, "bad sizes")
  return rows


def test_argument_errors_keep_their_codes_and_texts():
  """(entry point, fault) -> (return code, text of myr_last_error), one call per row, as the entry points answer today -- the order of their checks included:
  myr_eval and myr_rollout return MYR_OK for an empty batch before they look at the stride, the products and myr_fit_grad look first.  No row reaches a kernel."""
  from myriad_amd import _lib
  ARG, UNSUP = -1, -2
  engines = {"cart": _lib.Engine("CARTPOLE", "HERMITE_SIMPSON", 3, 2.0), "node": _lib.Engine("NODE_CARTPOLE", "HERMITE_SIMPSON", 3, 2.0),
             "plant": _lib.Engine("INVASIVEPLANT", "HERMITE_SIMPSON", 3, 2.0), "twin": _lib.Engine("CARTPOLE_ELASTIC", "HERMITE_SIMPSON", 3, 2.0),
             # the derivative family's: the network system under its other transcriptions, a closed-form SHOOTING handle, and two past the LDS bounds
             "node_sh": _lib.Engine("NODE_CARTPOLE", "SHOOTING", 2, 2.0, controls_per_interval=2), "node_tz": _lib.Engine("NODE_CARTPOLE", "TRAPEZOIDAL", 3, 2.0),
             "vdp_sh": _lib.Engine("VANDERPOL", "SHOOTING", 2, 10.0, controls_per_interval=3, integration_method="HEUN"),
             "node_sh_big": _lib.Engine("NODE_CARTPOLE", "SHOOTING", 1, 2.0, controls_per_interval=2000, integration_method="HEUN"),
             "node_hs_big": _lib.Engine("NODE_CARTPOLE", "HERMITE_SIMPSON", 400, 2.0)}
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
  rows += _derivative_rows() + _fit_rows()
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
