"""myr_fit_gnvp / myr_fit_gnvp_sets on the device: the Gauss-Newton product of the network fit, matrix-free (csrc/fit.h: node_fit_gnvp_kernel), and the
Levenberg-Marquardt / conjugate-gradient drivers on it (neural_ode/node_training.py: train_gn, train_ensemble_gn).

Oracle: `jv` against torch.func.jvp of the oracle's integrate_time_independent over O.NodeCartPole in the 4 804 weights, `out` against the vjp of
2 wt (.) jv through the same function.  Error measure: fit_cases.rel_errors' (largest |difference| of a trajectory's row over the largest |reference|
of that row).  Bounds, in the convention of NODE_LOSS_TOL / NODE_GRAD_TOL of test_gpu_fit.py: 100 x the largest error measured on an MI355X over the
matrix below (profiles/r28_fit_gnvp/README.md), and never above 1e-9:
  jv  measured 6.6e-15 -> 6.6e-13        out  measured 6.7e-15 -> 6.7e-13
The two identities that need no oracle, measured the same way over the same matrix (relative to the larger side):
  v . out = 2 sum_t wt[t] |jv[t]|^2   measured 1.9e-15 -> 1.9e-13        u . G v = v . G u   measured 4.4e-14 -> 4.4e-12
(the second is a difference of two sums of 4 804 products of either sign: its relative error is that of the cancellation in u . G v).
Everything else here is bit equality (`tobytes()`), the family's contract.
"""
import functools

import numpy as np
import pytest
import torch

import fit_cases as F
from myriad_amd import _lib
from test_gpu_fit import _node_case
from test_gpu_fit_sets import _node_case as _sets_case

pytestmark = pytest.mark.gpu

JV_TOL, OUT_TOL = 6.6e-13, 6.7e-13      # 100 x measured
DOT_TOL, SYM_TOL = 1.9e-13, 4.4e-12     # 100 x measured
assert max(JV_TOL, OUT_TOL, DOT_TOL, SYM_TOL) <= 1e-9
NP_NODE = 4804
SIZES = (5, 64, 64, 4)


def _engine(method, S, T, name="NODE_CARTPOLE"):
  return _lib.Engine(name, "SHOOTING", 1, T, controls_per_interval=S, integration_method=method)


def _direction(seed, shape=(NP_NODE,)):
  return np.random.default_rng(9000 + seed).standard_normal(shape)


def _mapping_t(p):
  """flat weights (a tensor) -> the Haiku mapping of tensors, in the order of csrc/node_system.h"""
  out, o = {}, 0
  for k, a, b in zip(("linear", "linear_1", "linear_2"), SIZES[:-1], SIZES[1:]):
    out[k] = {"w": p[o:o + a * b].reshape(a, b), "b": p[o + a * b:o + a * b + b]}
    o += a * b + b
  return out


def _oracle(flat, v, method, xs_obs, us, T, wt):
  """(jv [B,S+1,4], out [B,4804]) of the oracle: jvp of the rollout in the weights, then the vjp of 2 wt (.) jv"""
  S = xs_obs.shape[1] - 1
  w = torch.ones(S + 1, dtype=torch.float64) if wt is None else torch.as_tensor(wt)
  jvs, outs = [], []
  for b in range(xs_obs.shape[0]):
    x0, ub = torch.tensor(xs_obs[b, 0]), torch.tensor(us[b])
    f = lambda p: F.O.integrate_time_independent(F.O.NodeCartPole(_mapping_t(p)).dynamics, x0, ub, T / S, S, method)[1]
    _, jv = torch.func.jvp(f, (torch.tensor(flat),), (torch.tensor(v),))
    _, pull = torch.func.vjp(f, torch.tensor(flat))
    jvs.append(jv.numpy())
    outs.append(pull(2.0 * w[:, None] * jv)[0].numpy())
  jv, out = np.stack(jvs), np.stack(outs)
  assert np.isfinite(jv).all() and np.isfinite(out).all()
  return jv, out


def _row_error(got, ref):
  B = ref.shape[0]
  return F.rel_errors(np.ones(B), got.reshape(B, -1), np.ones(B), ref.reshape(B, -1))[1]


def _rel(a, b):
  return abs(a - b) / max(abs(a), abs(b))


# ---- parity with the oracle, and the identities that need none -------------------------------------------------------------------------
@pytest.mark.parametrize("method", F.METHODS)
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("batch", [1, 5])
def test_parity_with_the_oracle_and_identities(batch, S, method):
  node, flat, xs_obs, us, T = _node_case(batch, S, method)
  v, u = _direction(1), _direction(2)
  eng = _engine(method, S, T)
  for wt in (None, F.decaying_wt(S)):
    ref_jv, ref_out = _oracle(flat, v, method, xs_obs, us, T, wt)
    got = eng.fit_gnvp(xs_obs, us, flat, v, wt=wt, want_jv=True)
    assert got["jv"].shape == (batch, S + 1, 4) and got["out"].shape == (batch, NP_NODE)
    ej, eo = _row_error(got["jv"], ref_jv), _row_error(got["out"], ref_out)
    w = np.ones(S + 1) if wt is None else wt
    quad = 2.0 * (w[None, :, None] * got["jv"] ** 2).sum(axis=(1, 2))
    ed = max(_rel(float(v @ got["out"][b]), float(quad[b])) for b in range(batch))
    Gu = eng.fit_gnvp(xs_obs, us, flat, u, wt=wt)["out"]
    es = max(_rel(float(u @ got["out"][b]), float(v @ Gu[b])) for b in range(batch))
    print(f"GNVP {method} B={batch} S={S} u_rows={us.shape[1]} wt={'none' if wt is None else 'decaying'}: djv {ej:.2e} dout {eo:.2e} "
          f"v.Gv {ed:.2e} u.Gv {es:.2e}")
    assert ej <= JV_TOL and eo <= OUT_TOL, (ej, eo)
    assert ed <= DOT_TOL and es <= SYM_TOL, (ed, es)
    assert (got["jv"][:, 0] == 0.0).all()
    assert (quad > 0.0).all()
    zero = eng.fit_gnvp(xs_obs, us, flat, np.zeros(NP_NODE), wt=wt, want_jv=True)
    assert (zero["out"] == 0.0).all() and (zero["jv"] == 0.0).all()
  eng.close()


# ---- bit contracts -------------------------------------------------------------------------------------------------------------------------
def _bits(out):
  return out["out"].tobytes() + (out["jv"].tobytes() if "jv" in out else b"")


def _assert_sets_equal_single_calls(eng, P, V, xs_obs, us, wt):
  rows = eng.fit_gnvp_sets(xs_obs, us, P, V, wt=wt, want_jv=True)
  sums = eng.fit_gnvp_sets(xs_obs, us, P, V, wt=wt, reduce=True)
  E, R, S1 = xs_obs.shape[:3]
  assert rows["out"].shape == (E, R, NP_NODE) and rows["jv"].shape == (E, R, S1, 4) and sums["out"].shape == (E, NP_NODE)
  assert np.isfinite(rows["out"]).all() and np.abs(rows["out"]).max() > 0.0
  for e in range(E):
    one = eng.fit_gnvp(xs_obs[e], us[e], P[e], V[e], wt=wt, want_jv=True)
    red = eng.fit_gnvp(xs_obs[e], us[e], P[e], V[e], wt=wt, reduce=True)
    assert rows["out"][e].tobytes() == one["out"].tobytes(), (e, np.argwhere(rows["out"][e] != one["out"])[:1])
    assert rows["jv"][e].tobytes() == one["jv"].tobytes(), e
    assert sums["out"][e].tobytes() == red["out"].tobytes(), (e, np.argwhere(sums["out"][e] != red["out"])[:1])
    for r in range(R):                                # row b of a batched call = the call on trajectory b alone
      alone = eng.fit_gnvp(xs_obs[e, r], us[e, r], P[e], V[e], wt=wt, want_jv=True)
      assert alone["out"][0].tobytes() == one["out"][r].tobytes() and alone["jv"][0].tobytes() == one["jv"][r].tobytes(), (e, r)


@pytest.mark.parametrize("method", ["HEUN", "RK4"])
@pytest.mark.parametrize("R", [1, 4, 5])
def test_sets_equal_single_calls(R, method):
  """a lone wavefront, a full workgroup, a partial second workgroup per set; E = 3 and E = 1"""
  S = 3
  P, xs_obs, us, T = _sets_case(3, R, S, method)
  V = _direction(3, (3, NP_NODE))
  eng = _engine(method, S, T)
  for wt in (None, F.decaying_wt(S)):
    _assert_sets_equal_single_calls(eng, P, V, xs_obs, us, wt)
  _assert_sets_equal_single_calls(eng, P[1:2], V[1:2], xs_obs[1:2], us[1:2], None)
  eng.close()


def test_shared_data_equals_replicated_data():
  P, xs_obs, us, T = _sets_case(3, 5, 3, "RK4")
  V = _direction(4, (3, NP_NODE))
  eng = _engine("RK4", 3, T)
  x1, u1 = xs_obs[1], us[1]
  rep_x, rep_u = np.ascontiguousarray(np.broadcast_to(x1, (3,) + x1.shape)), np.ascontiguousarray(np.broadcast_to(u1, (3,) + u1.shape))
  for reduce in (False, True):
    shared = eng.fit_gnvp_sets(x1, u1, P, V, reduce=reduce, want_jv=True)
    assert shared["jv"].shape == (3, 5, 4, 4)
    assert _bits(shared) == _bits(eng.fit_gnvp_sets(rep_x, rep_u, P, V, reduce=reduce, want_jv=True))
  eng.close()


def _fit_reduce(rows):
  """fit_reduce_sets_kernel in numpy, for one set: thread t adds rows t, t + 256, ... in ascending order, then the 256 partial sums meet in a tree"""
  part = np.zeros((256, rows.shape[1]))
  for b in range(rows.shape[0]):
    part[b % 256] += rows[b]
  w = 128
  while w > 0:
    part[:w] += part[w:2 * w]
    w >>= 1
  return part[0]


@pytest.mark.parametrize("R,S", [(5, 3), (260, 1)])
def test_reduce_is_the_fit_reduction_of_the_rows(R, S):
  """reduce=True = the rows summed in myr_fit_grad's fixed order (restated in numpy: IEEE additions in the kernel's order); R = 260: a thread with two rows"""
  method = "HEUN"
  P, xs_obs, us, T = _sets_case(1, 5, S, method)
  xs_obs, us = np.ascontiguousarray(np.resize(xs_obs[0], (R,) + xs_obs.shape[2:])), np.ascontiguousarray(np.resize(us[0], (R,) + us.shape[2:]))
  xs_obs[:, 0] += 0.01 * _direction(5, (R, 4))      # (different start states: different rows)
  v = _direction(6)
  eng = _engine(method, S, T)
  rows = eng.fit_gnvp(xs_obs, us, P[0], v)["out"]
  red = eng.fit_gnvp(xs_obs, us, P[0], v, reduce=True)["out"]
  assert red.shape == (NP_NODE,) and red.tobytes() == _fit_reduce(rows).tobytes()
  grad = eng.fit_grad(xs_obs, us, params=P[0])["grad"]                          # ... which is the order myr_fit_grad sums its own rows in
  assert eng.fit_grad(xs_obs, us, params=P[0], reduce=True)["grad"].tobytes() == _fit_reduce(grad).tobytes()
  eng.close()


def test_chunked_equals_unchunked(monkeypatch):
  P, xs_obs, us, T = _sets_case(3, 5, 3, "HEUN")
  V = _direction(7, (3, NP_NODE))
  eng = _engine("HEUN", 3, T)
  monkeypatch.delenv("MYRIAD_FIT_ROWS_BYTES", raising=False)
  whole = eng.fit_gnvp_sets(xs_obs, us, P, V, reduce=True, want_jv=True)
  rows_whole = eng.fit_gnvp_sets(xs_obs, us, P, V, want_jv=True)
  one_set = 5 * NP_NODE * 8                                       # bytes of one set's rows
  for bound in (one_set, 2 * one_set + 8, 1000):                  # three chunks; two sets and one; below one set: still a set per chunk
    monkeypatch.setenv("MYRIAD_FIT_ROWS_BYTES", str(bound))
    assert _bits(eng.fit_gnvp_sets(xs_obs, us, P, V, reduce=True, want_jv=True)) == _bits(whole), bound
    assert _bits(eng.fit_gnvp_sets(xs_obs[0], us[0], P, V, reduce=True, want_jv=True)) == _bits(eng.fit_gnvp_sets(
        np.ascontiguousarray(np.broadcast_to(xs_obs[0], xs_obs.shape)), np.ascontiguousarray(np.broadcast_to(us[0], us.shape)), P, V, reduce=True,
        want_jv=True)), bound
    assert _bits(eng.fit_gnvp_sets(xs_obs, us, P, V, want_jv=True)) == _bits(rows_whole), bound
  eng.close()


def test_device_memory_history_and_jv_do_not_change_the_bits():
  P, xs_obs, us, T = _sets_case(3, 5, 3, "RK4")
  E, R, S1 = xs_obs.shape[:3]
  S, u_rows = S1 - 1, us.shape[2]
  V = _direction(8, (E, NP_NODE))
  wt = F.decaying_wt(S)
  eng = _engine("RK4", S, T)
  rows = eng.fit_gnvp_sets(xs_obs, us, P, V, wt=wt, want_jv=True)
  sums = eng.fit_gnvp_sets(xs_obs, us, P, V, wt=wt, reduce=True)
  one = eng.fit_gnvp(xs_obs[1], us[1], P[1], V[1], wt=wt, want_jv=True)
  # out with jv = out without; the forward tangent alone gives the same jv
  assert eng.fit_gnvp_sets(xs_obs, us, P, V, wt=wt)["out"].tobytes() == rows["out"].tobytes()
  only = eng.fit_gnvp_sets(xs_obs, us, P, V, wt=wt, want_jv=True, want_out=False)
  assert "out" not in only and only["jv"].tobytes() == rows["jv"].tobytes()
  assert eng.fit_gnvp(xs_obs[1], us[1], P[1], V[1], wt=wt)["out"].tobytes() == one["out"].tobytes()
  assert eng.fit_gnvp(xs_obs[1], us[1], P[1], V[1], wt=wt, want_jv=True, want_out=False)["jv"].tobytes() == one["jv"].tobytes()
  # an unrelated fit_grad on the handle in between: the same bits again
  eng.fit_grad(xs_obs[2], us[2], params=P[0])
  assert _bits(eng.fit_gnvp_sets(xs_obs, us, P, V, wt=wt, want_jv=True)) == _bits(rows)
  assert _bits(eng.fit_gnvp(xs_obs[1], us[1], P[1], V[1], wt=wt, want_jv=True)) == _bits(one)
  # device arrays
  dev = torch.device("cuda:0")
  dx, du, dp, dv, dw = (torch.tensor(np.array(a), device=dev) for a in (xs_obs, us, P, V, wt))      # (copies: the cached inputs are read-only)
  nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
  for rep in range(2):
    dj, do, dor = nan(E, R, S1, 4), nan(E, NP_NODE), nan(E, R, NP_NODE)
    d1j, d1o = nan(R, S1, 4), nan(R, NP_NODE)
    torch.cuda.synchronize()
    eng.fit_gnvp_sets_device(E, R, S, u_rows, dx, du, dp, dv, jv=dj, out=do, out_stride=0, wt=dw)
    eng.fit_gnvp_sets_device(E, R, S, u_rows, dx, du, dp, dv, jv=None, out=dor, out_stride=NP_NODE, wt=dw)
    eng.fit_gnvp_device(R, S, u_rows, dx[1], du[1], dp[1], dv[1], jv=d1j, out=d1o, out_stride=NP_NODE, wt=dw)
    torch.cuda.synchronize()
    assert dj.cpu().numpy().tobytes() == rows["jv"].tobytes() and do.cpu().numpy().tobytes() == sums["out"].tobytes(), rep
    assert dor.cpu().numpy().tobytes() == rows["out"].tobytes(), rep
    assert d1j.cpu().numpy().tobytes() == one["jv"].tobytes() and d1o.cpu().numpy().tobytes() == one["out"].tobytes(), rep
  eng.close()


def test_fit_grad_sets_keeps_its_bits_around_a_product():
  """myr_fit_grad_sets before and after a myr_fit_gnvp_sets call on the handle = the plain call on a fresh handle"""
  P, xs_obs, us, T = _sets_case(3, 5, 3, "RK4")
  V = _direction(9, (3, NP_NODE))
  bits = lambda o: o["loss"].tobytes() + o["grad"].tobytes()
  fresh = _engine("RK4", 3, T)
  plain = [bits(fresh.fit_grad_sets(xs_obs, us, P, reduce=reduce)) for reduce in (False, True)]
  fresh.close()
  eng = _engine("RK4", 3, T)
  before = [bits(eng.fit_grad_sets(xs_obs, us, P, reduce=reduce)) for reduce in (False, True)]
  eng.kernel_time_reset()
  eng.fit_gnvp_sets(xs_obs, us, P, V, reduce=True, want_jv=True)
  ms, n = eng.kernel_time(_lib.K_FIT)                 # the product is timed on the fit family's slot, once per call
  assert n == 1 and ms > 0.0
  after = [bits(eng.fit_grad_sets(xs_obs, us, P, reduce=reduce)) for reduce in (False, True)]
  eng.close()
  assert before == plain and after == plain


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order():
  P, xs_obs, us, T = _sets_case(3, 5, 3, "HEUN")
  V = _direction(10, (3, NP_NODE))
  E, R, S, u_rows = 3, 5, 3, us.shape[2]
  eng = _engine("HEUN", S, T)
  jv, out = np.full((E, R, S + 1, 4), 7.0), np.full((E, R, NP_NODE), 7.0)
  a = {"h": eng._h, "E": E, "R": R, "S": S, "u_rows": u_rows, "xs": xs_obs.ctypes.data, "us": us.ctypes.data, "shared": 0, "p": P.ctypes.data,
       "v": V.ctypes.data, "jv": jv.ctypes.data, "out": out.ctypes.data, "stride": NP_NODE, "mem": _lib.MEM_HOST}

  def sets(**kw):
    k = dict(a, **kw)
    rc = eng.lib.myr_fit_gnvp_sets(k["h"], k["E"], k["R"], k["S"], k["u_rows"], k["xs"], k["us"], k["shared"], None, k["p"], k["v"], k["jv"], k["out"],
                                   k["stride"], k["mem"])
    return rc, eng.lib.myr_last_error().decode()

  def single(**kw):
    k = dict(a, E=R)
    k.update(kw)
    rc = eng.lib.myr_fit_gnvp(k["h"], k["E"], k["S"], k["u_rows"], k["xs"], k["us"], None, k["p"], k["v"], k["jv"], k["out"], k["stride"], k["mem"])
    return rc, eng.lib.myr_last_error().decode()

  cart = _engine("RK4", S, T, name="CARTPOLE")
  for call, who in ((sets, "myr_fit_gnvp_sets"), (single, "myr_fit_gnvp")):
    # every fault with all the later ones beside it: the first in the order is the one reported
    later = {"jv": None, "out": None, "S": 0, "stride": 3, "mem": 9, "h": cart._h}
    if call is sets:
      later["shared"] = 2
    for null in ("h", "xs", "us", "p", "v"):
      assert call(**dict(later, **{null: None})) == (-1, f"{who}: null handle, xs_obs, us, params or v"), null
    later["h"] = cart._h
    assert call(**later) == (-1, f"{who}: jv and out are both null")
    del later["jv"], later["out"]
    for bad in ({"S": 0}, {"u_rows": 0}, {"E": -1}) + (({"R": 0}, {"E": 1 << 20, "R": 1 << 20}) if call is sets else ()):
      assert call(**dict(later, **bad)) == (-1, f"{who}: bad sizes"), bad
    del later["S"]
    rc, msg = call(**later)
    assert rc == -1 and msg.startswith(f"{who}: out_stride must be 0 (") and msg.endswith("or np (a row per trajectory)"), msg
    later["stride"] = 0                              # (np of the other handle is not this one's)
    if call is sets:
      assert call(**later) == (-1, f"{who}: data_shared must be 0 (data per set) or 1 (one set of data, read by every set)")
      del later["shared"]
    assert call(**later) == (-1, f"{who}: bad mem kind")
    del later["mem"]
    rc, msg = call(E=0, **later)                      # another system is refused before the empty call is looked at
    assert rc == -2 and msg.startswith(f"{who}: the network system only") and "myr_fit_gn" in msg and "multiply" in msg, msg
    # the empty call: nothing is written
    assert call(E=0)[0] == 0 and (jv == 7.0).all() and (out == 7.0).all()
    # one output alone is enough
    assert call(jv=None)[0] == 0 and np.isfinite(out).all() and (out[0] != 7.0).all() and (jv == 7.0).all()
    out[:] = 7.0
    assert call(out=None)[0] == 0 and (out == 7.0).all() and (jv[0, 0, 0] == 0.0).all()
    jv[:] = 7.0
  # the binding raises what the family raises
  with pytest.raises(NotImplementedError, match="network system only"):
    cart.fit_gnvp(xs_obs[0], us[0], np.zeros(cart.np), np.zeros(cart.np))
  with pytest.raises(ValueError):
    eng.fit_gnvp_sets(xs_obs, us, P, V[:2])                       # a direction per set
  with pytest.raises(NotImplementedError, match="Gauss-Newton matrix is not formed"):      # myr_fit_gn keeps its own refusal of the network system
    eng.fit_gn(xs_obs[0], us[0], params=P[0])
  cart.close()
  eng.close()


# ---- the drivers -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _training_case():
  from myriad_amd.config import Config, HParams, OptimizerType
  from myriad_amd.systems import SystemType
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping
  from myriad_amd.utils import generate_dataset
  hp = HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.SHOOTING, intervals=1, controls_per_interval=3, train_size=6, val_size=2,
               test_size=2, minibatch_size=3, num_epochs=6, loss_recording_frequency=1, early_stop_check_frequency=1)
  data = generate_dataset(hp, Config(verbose=False, plot=False))
  assert data.shape == (10, 4, 5)
  flat = flat_from_mapping(NeuralODE.load_fitted_cartpole().params)
  P0 = flat[None] + 0.05 * np.random.default_rng(12).standard_normal((2, NP_NODE))
  return hp, SystemType.CARTPOLE().T, data, P0


def test_train_gn_three_outer_steps():
  from myriad_amd.neural_ode import node_training
  from myriad_amd.systems.neural_ode import flat_from_mapping, mapping_from_flat
  hp, T, data, P0 = _training_case()
  train, val = data[:6], data[6:8]
  fit = node_training.NodeFitLoss(hp, T)
  # gn_product is one myr_fit_gnvp call with the weights of the loss
  v = _direction(13)
  wt = np.full(4, 1.0 / (6 * 4 * 4))
  ref = fit.engine.fit_gnvp(train[:, :, :4], train[:, :, 4:], P0[0], v, wt=wt, reduce=True)["out"]
  assert fit.gn_product(mapping_from_flat(P0[0]), v, train).tobytes() == ref.tobytes()
  assert fit.gn_products(P0, np.stack([v, v]), train)[0].tobytes() == ref.tobytes()
  history = []
  cg_iters, cg_tol = 8, 1e-2
  best, last, record = node_training.train_gn(hp, T, mapping_from_flat(P0[0]), train, val, max_iter=3, cg_iters=cg_iters, cg_tol=cg_tol, fit=fit,
                                              history=history)
  assert len(history) == 3 and last == 3 and [r[0] for r in record] == [0, 1, 2, 3]
  assert any(s["accepted"] for s in history)
  loss = record[0][1]
  for i, s in enumerate(history):
    assert s["loss"] == loss and 1 <= s["cg_products"] <= cg_iters
    if s["accepted"]:                                 # every accepted step lowers the training loss; a rejected one leaves the point and raises lam
      assert s["trial_loss"] < loss
      loss = s["trial_loss"]
    elif i + 1 < len(history):
      assert history[i + 1]["lam"] == 4.0 * s["lam"] and history[i + 1]["params"].tobytes() == s["params"].tobytes()
    assert record[i + 1][1] == loss
    # the step's own residual test, with (G + lam I) d + g recomputed by an independent call
    res = fit.gn_product(s["params"], s["d"], train) + s["lam"] * s["d"] + s["grad"]
    rel = float(np.linalg.norm(res) / np.linalg.norm(s["grad"]))
    print(f"step {i}: lam {s['lam']:.2e} products {s['cg_products']} residual {rel:.3e} (recurrence {s['cg_residual']:.3e}) "
          f"loss {s['loss']:.6e} -> {s['trial_loss']:.6e} {'accepted' if s['accepted'] else 'rejected'}")
    assert abs(rel - s["cg_residual"]) <= 1e-8 * max(1.0, rel)
    assert rel <= cg_tol or s["cg_products"] == cg_iters
    assert s["grad"].tobytes() == flat_from_mapping(fit.value_and_grad(mapping_from_flat(s["params"]), train)[1]).tobytes()
  assert best is not None and min(r[2] for r in record) == fit(best, val)
  fit.engine.close()


def test_train_ensemble_gn_equals_its_train_gn_runs():
  from myriad_amd.neural_ode import node_training
  from myriad_amd.systems.neural_ode import flat_from_mapping
  hp, T, data, P0 = _training_case()
  fit = node_training.NodeFitLoss(hp, T)
  trains, vals = np.stack([data[:6], data[2:8]]), np.stack([data[6:8], data[8:10]])      # data per model
  kw = dict(max_iter=3, cg_iters=8, cg_tol=1e-2)
  hists = [[], []]
  both = node_training.train_ensemble_gn(hp, T, P0, trains, vals, fit=fit, histories=hists, **kw)
  for e in range(2):
    hist = []
    best, last, record = node_training.train_gn(hp, T, P0[e], trains[e], vals[e], fit=fit, history=hist, **kw)
    assert (last, record) == both[e][1:]
    assert flat_from_mapping(best).tobytes() == flat_from_mapping(both[e][0]).tobytes()
    assert len(hist) == len(hists[e]) == 3
    for s, t in zip(hist, hists[e]):                  # the weights, the steps and the dampings of every trial point, to the bit
      assert s["params"].tobytes() == t["params"].tobytes() and s["d"].tobytes() == t["d"].tobytes()
      assert (s["lam"], s["cg_products"], s["trial_loss"], s["accepted"]) == (t["lam"], t["cg_products"], t["trial_loss"], t["accepted"])
  shared = node_training.train_ensemble_gn(hp, T, P0[:1], data[:6], data[6:8], fit=fit, **kw)      # one set of data, read by every model
  assert shared[0][1:] == both[0][1:]
  fit.engine.close()
