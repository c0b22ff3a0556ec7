"""myr_fit_gn and myr_fit_gn_sets on the device (csrc/fit_gn.h: fit_gn_lane_kernel; csrc/myriad_hip.hip: dispatch_fit).

Device against twin: the twin (tests/hostsim/fit_gn_twin.cpp) is the same FitGnLane<Sys> compiled with g++; the device contracts multiply-adds
and has its own libm, so the comparison carries the bound of test_fit_gn_host_twin.py (the twin against the oracle, measured x 10):
|dgn| / max|gn| <= 1.1e-14, |dgrad| / max|grad| <= 1.2e-12, and |dloss| / loss <= 2.7e-12 (test_fit_host_twin.py's).
Measured on an MI355X over the 28 comparisons below: dloss 5.0e-14, dgrad 1.6e-13, dgn 1.7e-15 at worst.
The two wide systems run with steps of 0.05 (T = 0.05 S, the rule of fit_cases.horizon for the autograd systems).  fit_cases.horizon gives
HIVTREATMENT T = 10 -- kept long for its central-difference references --, which at S = 3 is a step of 3.3: outside the stability range of the
explicit rules (the states reach 1.7e5 and turn negative), and three such steps amplify the rounding differences between contracted and separate
multiply-adds.  Measured on the MI355X with T = 10: dloss 3.1e-14, dgrad 1.0e-12, dgn 1.95e-12 against the twin; the twin compiled with
-mfma -ffp-contract=fast differs from the plain twin by the same amounts on the host (dgrad 9.3e-13, dgn 1.8e-12), and by 4.6e-16 with steps of 0.05.

Everything else is bit equality: rows against single calls, sets against single calls, chunked against unchunked, host against device arrays,
a call against its repetition; and the refusals, with their messages, in the order include/myriad_hip.h states."""
import functools
import math

import numpy as np
import pytest
import torch

import fit_cases as F
import fit_gn_cases as G
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL, GN_TOL = 2.7e-12, 1.2e-12, 1.1e-14


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return G.build_twin(tmp_path_factory.mktemp("fit_gn_twin"))


def _engine(name, method, S, T=None):
  return _lib.Engine(name, "SHOOTING", 1, F.horizon(name, S) if T is None else T, controls_per_interval=S, integration_method=method)


def _bits(out):
  return b"".join(out[k].tobytes() for k in ("loss", "grad", "gn"))


def _check_against_twin(twin, eng, name, method, S, xs_obs, us, params, wt, T=None):
  out = eng.fit_gn(xs_obs, us, params=params, wt=wt)
  loss, grad, gn = G.twin_fit_gn(twin, name, method, F.horizon(name, S) if T is None else T, xs_obs, us, params, wt)
  assert out["gn"].tobytes() == np.ascontiguousarray(out["gn"].transpose(0, 2, 1)).tobytes()
  el = float((np.abs(out["loss"] - loss) / loss).max())
  eg, en = G.rel_errors(out["grad"], out["gn"], grad, gn)
  print(f"{name} {method} S={S} B={xs_obs.shape[0]} params {params.shape}: dloss {el:.2e} dgrad {eg:.2e} dgn {en:.2e}")
  assert el <= LOSS_TOL and eg <= GRAD_TOL and en <= GN_TOL, (el, eg, en)
  return out


# ---- device against twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 7])
@pytest.mark.parametrize("batch", [1, 63, 65, 130])
def test_device_equals_twin_over_awkward_shapes(twin, batch, S):
  """a partial wavefront, the wavefront edge, several workgroups; shared and per-trajectory parameters, weighted and not"""
  eng = _engine("CARTPOLE", "RK4", S)
  for per_instance in (False, True):
    xs_obs, us, params = F.inputs("CARTPOLE", "RK4", False, batch, S, per_instance)
    _check_against_twin(twin, eng, "CARTPOLE", "RK4", S, xs_obs, us, params, F.decaying_wt(S) if per_instance else None)
  eng.close()


@pytest.mark.parametrize("name,method,S,batch", [("HIVTREATMENT", "HEUN", 3, 65), ("ROCKETLANDING", "RK4", 2, 5)])
def test_device_equals_twin_on_the_wide_systems(twin, name, method, S, batch):
  """HIVTREATMENT: np = 9, the widest sensitivity block; ROCKETLANDING: ns = 6, nu = 2.  Steps of 0.05 for both: see the module docstring"""
  T = 0.05 * S
  eng = _engine(name, method, S, T)
  xs_obs, us, params = F.inputs(name, method, False, batch, S, True)
  _check_against_twin(twin, eng, name, method, S, xs_obs, us, params, None, T)
  xs_obs, us, params = F.inputs(name, method, False, batch, S, False)
  out = _check_against_twin(twin, eng, name, method, S, xs_obs, us, params, F.decaying_wt(S), T)
  if name == "HIVTREATMENT":                                      # A enters the running cost only
    i = F.O.SYSTEMS[name].param_names.index("A")
    assert (out["grad"][:, i] == 0.0).all() and (out["gn"][:, i, :] == 0.0).all() and (out["gn"][:, :, i] == 0.0).all()
  eng.close()


# ---- rows against singles --------------------------------------------------------------------------------------------------------------------
def test_rows_are_the_single_calls():
  S, batch = 2, 65
  xs_obs, us, params = F.inputs("CARTPOLE", "RK4", False, batch, S, True)
  eng = _engine("CARTPOLE", "RK4", S)
  wt = F.decaying_wt(S)
  out = eng.fit_gn(xs_obs, us, params=params, wt=wt)
  for b in (0, 1, 31, 63, 64):
    one = eng.fit_gn(xs_obs[b:b + 1], us[b:b + 1], params=params[b], wt=wt)
    red = eng.fit_gn(xs_obs[b:b + 1], us[b:b + 1], params=params[b:b + 1], wt=wt, reduce=True)
    for k in ("loss", "grad", "gn"):
      assert one[k].tobytes() == out[k][b:b + 1].tobytes(), (b, k)
    assert red["grad"].tobytes() == out["grad"][b].tobytes() and red["gn"].tobytes() == out["gn"][b].tobytes(), b
  eng.close()


# ---- sets ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sets_case(E, R, S):
  xs_obs, us, params = F.inputs("CARTPOLE", "RK4", False, E * R, S, True)
  out = (np.ascontiguousarray(params[::R][:E]), xs_obs.reshape(E, R, S + 1, 4), us.reshape(E, R, S + 1, 1))
  for a in out:
    a.setflags(write=False)
  return out


def _assert_sets_equal_single_calls(eng, P, xs_obs, us, wt):
  """xs_obs, us [E][R]...: data per set, or [R]...: shared"""
  rows = eng.fit_gn_sets(xs_obs, us, P, wt=wt)
  sums = eng.fit_gn_sets(xs_obs, us, P, wt=wt, reduce=True)
  E, R = P.shape[0], xs_obs.shape[-3]
  assert rows["loss"].shape == (E, R) and rows["grad"].shape == (E, R, eng.np) and rows["gn"].shape == (E, R, eng.np, eng.np)
  assert sums["loss"].shape == (E, R) and sums["grad"].shape == (E, eng.np) and sums["gn"].shape == (E, eng.np, eng.np)
  assert np.isfinite(rows["gn"]).all() and np.abs(rows["gn"]).max() > 0.0
  for e in range(E):
    x, u = (xs_obs, us) if xs_obs.ndim == 3 else (xs_obs[e], us[e])
    one = eng.fit_gn(x, u, params=P[e], wt=wt)
    red = eng.fit_gn(x, u, params=P[e], wt=wt, reduce=True)
    for k in ("loss", "grad", "gn"):
      assert rows[k][e].tobytes() == one[k].tobytes(), (e, k)
      assert sums[k][e].tobytes() == red[k].tobytes(), (e, k)
  return rows, sums


@pytest.mark.parametrize("E,R", [(3, 5), (2, 70)])
def test_sets_equal_single_calls(E, R, monkeypatch):
  """set edges inside one wavefront; a set across wavefronts.  Data per set and shared; one set per chunk gives the same bits"""
  S = 2
  P, xs_obs, us = _sets_case(E, R, S)
  eng = _engine("CARTPOLE", "RK4", S)
  monkeypatch.delenv("MYRIAD_FIT_ROWS_BYTES", raising=False)
  rows, sums = _assert_sets_equal_single_calls(eng, P, xs_obs, us, F.decaying_wt(S))
  shared = _assert_sets_equal_single_calls(eng, P, xs_obs[1], us[1], None)
  monkeypatch.setenv("MYRIAD_FIT_ROWS_BYTES", str(R * (eng.np + eng.np ** 2) * 8))      # the rows of one set
  assert _bits(eng.fit_gn_sets(xs_obs, us, P, wt=F.decaying_wt(S), reduce=True)) == _bits(sums)
  assert _bits(eng.fit_gn_sets(xs_obs, us, P, wt=F.decaying_wt(S))) == _bits(rows)
  assert _bits(eng.fit_gn_sets(xs_obs[1], us[1], P, reduce=True)) == _bits(shared[1])
  monkeypatch.setenv("MYRIAD_FIT_ROWS_BYTES", "1000")             # below one set: still a set per chunk
  assert _bits(eng.fit_gn_sets(xs_obs, us, P, wt=F.decaying_wt(S), reduce=True)) == _bits(sums)
  eng.close()


# ---- the reduction ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [65, 300])
def test_reduction_is_deterministic_and_exact_enough(batch):
  """300: thread t of the reduction adds more than one row"""
  S = 2
  xs_obs, us, params = F.inputs("CARTPOLE", "RK4", False, batch, S, True)
  eng = _engine("CARTPOLE", "RK4", S)
  rows = eng.fit_gn(xs_obs, us, params=params)
  sums = eng.fit_gn(xs_obs, us, params=params, reduce=True)
  assert sums["loss"].tobytes() == rows["loss"].tobytes()
  for k in ("grad", "gn"):
    flat = rows[k].reshape(batch, -1)
    for j, v in enumerate(sums[k].ravel()):
      assert abs(v - math.fsum(flat[:, j])) <= 1e-13 * np.abs(flat[:, j]).sum(), (k, j)
  assert sums["gn"].tobytes() == sums["gn"].T.copy().tobytes()
  assert _bits(eng.fit_gn(xs_obs, us, params=params, reduce=True)) == _bits(sums)
  assert _bits(eng.fit_gn(xs_obs, us, params=params)) == _bits(rows)
  eng.close()


def test_device_memory_and_null_outputs_give_the_same_bits():
  E, R, S = 3, 5, 2
  P, xs_obs, us = _sets_case(E, R, S)
  eng = _engine("CARTPOLE", "RK4", S)
  npar, wt = eng.np, F.decaying_wt(S)
  rows, sums = eng.fit_gn_sets(xs_obs, us, P, wt=wt), eng.fit_gn_sets(xs_obs, us, P, wt=wt, reduce=True)
  one_rows = eng.fit_gn(xs_obs[1], us[1], params=P[1], wt=wt)
  one_sums = eng.fit_gn(xs_obs[1], us[1], params=P[1], wt=wt, reduce=True)
  dev = torch.device("cuda:0")
  dx, du, dp, dw = (torch.tensor(np.array(a), device=dev) for a in (xs_obs, us, P, wt))      # (copies: the cached inputs are read-only)
  new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
  host = lambda t: t.cpu().numpy().tobytes()
  for rep in range(2):                                            # a second call: the same bits again
    dl, dg, dn, dgr, dnr = new(E, R), new(E, npar), new(E, npar, npar), new(E, R, npar), new(E, R, npar, npar)
    torch.cuda.synchronize()
    eng.fit_gn_sets_device(E, R, S, S + 1, dx, du, dp, dn, out_stride=0, wt=dw, loss=dl, grad=dg)
    eng.fit_gn_sets_device(E, R, S, S + 1, dx, du, dp, dnr, out_stride=npar, wt=dw, grad=dgr)
    torch.cuda.synchronize()
    assert host(dl) == sums["loss"].tobytes() and host(dg) == sums["grad"].tobytes() and host(dn) == sums["gn"].tobytes(), rep
    assert host(dgr) == rows["grad"].tobytes() and host(dnr) == rows["gn"].tobytes(), rep
    # loss and grad NULL: gn alone, the same bits, rows and sums
    dn2, dnr2 = new(E, npar, npar), new(E, R, npar, npar)
    eng.fit_gn_sets_device(E, R, S, S + 1, dx, du, dp, dn2, out_stride=0, wt=dw)
    eng.fit_gn_sets_device(E, R, S, S + 1, dx, du, dp, dnr2, out_stride=npar, wt=dw)
    # myr_fit_gn on device arrays: one set, its parameters shared
    d1l, d1g, d1n, d1s = new(R), new(R, npar), new(R, npar, npar), new(npar, npar)
    eng.fit_gn_device(R, S, S + 1, dx[1], du[1], d1n, npar, params=dp[1], wt=dw, loss=d1l, grad=d1g)
    eng.fit_gn_device(R, S, S + 1, dx[1], du[1], d1s, 0, params=dp[1], wt=dw)
    torch.cuda.synchronize()
    assert host(dn2) == sums["gn"].tobytes() and host(dnr2) == rows["gn"].tobytes(), rep
    assert host(d1l) == one_rows["loss"].tobytes() and host(d1g) == one_rows["grad"].tobytes() and host(d1n) == one_rows["gn"].tobytes(), rep
    assert host(d1s) == one_sums["gn"].tobytes(), rep
  # host arrays, loss and grad NULL
  gn = np.full((R, npar, npar), np.nan)
  args = (eng._h, R, S, S + 1, xs_obs[1].ctypes.data, us[1].ctypes.data, wt.ctypes.data, P[1].ctypes.data, 0)
  assert eng.lib.myr_fit_gn(*args, None, None, gn.ctypes.data, npar, _lib.MEM_HOST) == 0 and gn.tobytes() == one_rows["gn"].tobytes()
  gs = np.full((npar, npar), np.nan)
  assert eng.lib.myr_fit_gn(*args, None, None, gs.ctypes.data, 0, _lib.MEM_HOST) == 0 and gs.tobytes() == one_sums["gn"].tobytes()
  eng.close()


def test_what_ran_before_does_not_reach_the_result():
  """a fit_grad call (state scratch in the same buffer) and a larger fit_gn call between two calls: the same bits"""
  S = 2
  xs_obs, us, params = F.inputs("CARTPOLE", "RK4", False, 65, S, True)
  big = F.inputs("CARTPOLE", "RK4", False, 300, S, True)
  eng = _engine("CARTPOLE", "RK4", S)
  first = _bits(eng.fit_gn(xs_obs, us, params=params, reduce=True))
  eng.fit_grad(big[0], big[1], params=big[2], reduce=True)
  eng.fit_gn(big[0], big[1], params=big[2], reduce=True)
  assert _bits(eng.fit_gn(xs_obs, us, params=params, reduce=True)) == first
  eng.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order():
  S, R = 2, 5
  P, xs_obs, us = _sets_case(3, R, S)
  x, u = xs_obs[0], us[0]
  eng = _engine("CARTPOLE", "RK4", S)
  lib, H, D = eng.lib, _lib.MEM_HOST, 7
  loss, grad, gn = np.full((3, R), 7.0), np.full((3, R, 4), 7.0), np.full((3, R, 4, 4), 7.0)
  a = lambda v: None if v is None else v.ctypes.data
  ARG, UNS = -1, -2

  def one(h=eng._h, B=R, S_=S, rows=S + 1, xs=x, us_=u, params=None, ps=0, gn_=gn, stride=4, mem=H):
    return lib.myr_fit_gn(h, B, S_, rows, a(xs), a(us_), None, a(params), ps, a(loss), a(grad), a(gn_), stride, mem), lib.myr_last_error().decode()

  def sets(h=eng._h, E=3, R_=R, S_=S, rows=S + 1, xs=xs_obs, us_=us, shared=0, params=P, gn_=gn, stride=4, mem=H):
    return lib.myr_fit_gn_sets(h, E, R_, S_, rows, a(xs), a(us_), shared, None, a(params), a(loss), a(grad), a(gn_), stride, mem), lib.myr_last_error().decode()

  # (the argument checks of the two C calls, with their full texts and their order: tests/test_gpu_api.py)  A refused call writes nothing
  assert one(mem=D)[0] == ARG and sets(mem=D)[0] == ARG and one(stride=3)[0] == ARG and sets(shared=2)[0] == ARG
  assert (loss == 7.0).all() and (grad == 7.0).all() and (gn == 7.0).all()
  # B == 0 / E == 0: nothing is written; then a real call does write
  assert one(B=0)[0] == 0 and sets(E=0)[0] == 0
  assert (loss == 7.0).all() and (grad == 7.0).all() and (gn == 7.0).all()
  assert sets()[0] == 0 and (loss != 7.0).all() and np.isfinite(gn).all() and (gn != 7.0).any()
  eng.close()

  # MYR_E_UNSUPPORTED, behind every argument check: the network system first
  eng = _engine("NODE_CARTPOLE", "HEUN", S, 0.2)
  w = np.zeros((3, eng.np))
  for call, who in ((one, "myr_fit_gn:"), (sets, "myr_fit_gn_sets:")):
    rc, msg = call(h=eng._h, stride=3)
    assert rc == ARG and "out_stride" in msg, msg                  # (np = 4 804 here: 3 and 4 are both refused)
    rc, msg = call(h=eng._h, stride=0, mem=D)
    assert rc == ARG and "bad mem kind" in msg, msg
    rc, msg = call(h=eng._h, stride=0, params=w) if call is sets else call(h=eng._h, stride=0, params=w[0])
    assert rc == UNS and msg.startswith(who) and "4 804 x 4 804" in msg and "is not formed" in msg and "myr_fit_grad" in msg, msg
    rc, msg = call(h=eng._h, stride=0, params=w, **({"E": 0} if call is sets else {"B": 0}))
    assert rc == UNS, msg                                         # refused whatever the batch
  with pytest.raises(NotImplementedError, match="not formed"):
    eng.fit_gn(np.zeros((R, S + 1, 4)), np.zeros((R, S + 1, 1)), params=w[0])
  eng.close()
  # the elastic twins, INVASIVEPLANT: myr_fit_grad's wording
  eng = _lib.Engine("CARTPOLE_ELASTIC", "HERMITE_SIMPSON", 7, 1.0)
  with pytest.raises(NotImplementedError, match="myr_fit_grad: an elastic twin has no model of its own to fit"):
    eng.fit_gn(np.zeros((R, S + 1, eng.ns)), np.zeros((R, S + 1, eng.nu)))
  with pytest.raises(NotImplementedError, match="myr_fit_grad: an elastic twin has no model of its own to fit"):
    eng.fit_gn_sets(np.zeros((3, R, S + 1, eng.ns)), np.zeros((3, R, S + 1, eng.nu)), np.zeros((3, eng.np)))
  rc, msg = one(h=eng._h, stride=eng.np, mem=D)                    # the argument checks come first
  assert rc == ARG and "bad mem kind" in msg, msg
  eng.close()
  eng = _lib.Engine("INVASIVEPLANT", "SHOOTING", 1, 10.0, controls_per_interval=7)
  with pytest.raises(NotImplementedError, match="myr_fit_gn: INVASIVEPLANT is a discrete-time system"):
    eng.fit_gn(np.zeros((R, S + 1, eng.ns)), np.zeros((R, S + 1, eng.nu)))
  with pytest.raises(NotImplementedError, match="myr_fit_gn_sets: INVASIVEPLANT is a discrete-time system"):
    eng.fit_gn_sets(np.zeros((3, R, S + 1, eng.ns)), np.zeros((3, R, S + 1, eng.nu)), np.zeros((3, eng.np)))
  eng.close()
  # the binding's own shape checks
  eng = _engine("CARTPOLE", "RK4", S)
  with pytest.raises(ValueError):
    eng.fit_gn_sets(xs_obs, us, P[:2])
  with pytest.raises(ValueError):
    eng.fit_gn(x, u[:, :, :0])
  eng.close()


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["VANDERPOL", "CARTPOLE"])
def test_levenberg_marquardt_on_the_device(twin, name):
  """run_mle_sysid_gn on the noise-free data of the CPU test's kind (tests/fit_gn_cases.py: driver_problem): at most 30 iterations to a loss
  <= 1e-12 x the initial one, in as many iterations as the same driver takes on the twin"""
  from myriad_amd.experiments.mle_sysid import FitLoss, run_mle_sysid_gn
  hp, cfg, datasets, truth, make_twin_fit = G.driver_problem(twin, name, 1)
  host = run_mle_sysid_gn(hp, cfg, datasets[0], fit=make_twin_fit())
  fit = FitLoss(hp, engine=_engine(name, "HEUN", hp.num_steps))
  dev = run_mle_sysid_gn(hp, cfg, datasets[0], fit=fit)
  fit.engine.close()
  print(f"{name}: device {dev['iterations']} iterations, loss {dev['train_losses'][0]:.3e} -> {dev['train_losses'][-1]:.3e}; "
        f"twin {host['iterations']} iterations -> {host['train_losses'][-1]:.3e}")
  assert dev["iterations"] <= G.LM_MAX_ITER and dev["train_losses"][-1] <= G.LM_RATIO * dev["train_losses"][0]
  assert dev["iterations"] == host["iterations"]
  names = hp.system().param_names
  for k, v in dev["last_params"].items():
    assert abs(abs(v) - truth[0, names.index(k)]) <= 1e-9 * truth[0, names.index(k)], (k, v)
  assert dev["gn"].shape == (len(dev["last_params"]),) * 2 and np.isfinite(dev["covariance"]).all()
