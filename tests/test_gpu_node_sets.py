"""myr_exgd_grad_node_sets and myr_hvp_node_sets on the device: E weight sets of R instances each in one call against the single-set entry points
(myr_exgd_grad_node, myr_exgd_grad_node_shoot, myr_hvp_node) run on every set alone -- equal BYTES, rows and per-set sums, dz0 and dlam0 --, across
the workgroup widths, the forms of the call, chunks of the history that begin and end inside a set, host and device arrays; one comparison with the
torch oracle per transcription on a set other than set 0; and run_node_endtoend_sets against run_node_endtoend on every network alone.

The weight sets are the committed weights plus 5 % noise per set (tests/node_sets_cases.py), every set different from set 0 in bits: a kernel that
read set 0 for every instance, or the wrong set for a chunk that starts inside a set, would fail the byte comparisons.  The shapes are the smallest
at which the set mapping can fail.  The oracle tolerances are those of the single-set suites (test_gpu_node_exgd_grad.py,
test_gpu_node_shoot_exgd_grad.py, test_gpu_node_hvp.py: 100 x the error measured there); they apply because the bits are the single-set call's.
"""
import numpy as np
import pytest
import torch

import node_sets_cases as NS_
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

HS_ORACLE_TOL = 100.0 * 3.9e-15        # test_gpu_node_exgd_grad.ORACLE_TOL
SHOOT_ORACLE_TOL = 100.0 * 4.3e-15     # test_gpu_node_shoot_exgd_grad.ORACLE_TOL
HVP_ORACLE_TOL = 100.0 * 4.5e-15       # test_gpu_node_hvp.ORACLE_TOL
KEYS = ("grad", "dz0", "dlam0")
NP = NS_.NP
SHOOT_SHAPES = ((1, 3), (2, 2), (4, 1))      # (intervals, cpi): 1, 2 and 4 wavefronts per instance (node_shoot_exgd_grad_wpi)


def _hs_engine(N):
  return _lib.Engine("NODE_CARTPOLE", "HERMITE_SIMPSON", N, 0.1 * N)


def _shoot_engine(I, cpi, method):
  return _lib.Engine("NODE_CARTPOLE", "SHOOTING", I, 0.05 * I * cpi, controls_per_interval=cpi, integration_method=method)


def _nx(eng):
  return eng.x_rows * eng.ns


def _exgd_sets(eng, c, P, nsteps, **kw):
  a = dict(z=c["z"], lam=c["lam"], lb=c["lb"], ub=c["ub"], eta_x=c["eta_x"], eta_v=c["eta_v"], nsteps=nsteps, seed_z=c["seed_z"],
           seed_lam=c["seed_lam"], params=P)
  a.update(kw)
  return eng.exgd_grad_node_sets(**a)


def _exgd_single(eng, c, P, e, nsteps, **kw):
  """the single-set entry point of the handle's transcription on set e alone: B = R, its own weights"""
  call = eng.exgd_grad_node_shoot if eng.desc.transcription == _lib.TR_IDS["SHOOTING"] else eng.exgd_grad_node
  a = dict(z=c["z"][e], lam=c["lam"][e], lb=c["lb"][e], ub=c["ub"][e], eta_x=c["eta_x"], eta_v=c["eta_v"], nsteps=nsteps, seed_z=c["seed_z"][e],
           seed_lam=c["seed_lam"][e], params=P[e])
  if "seed_lam" in kw and kw["seed_lam"] is None:
    a["seed_lam"] = None
  a.update({k: v for k, v in kw.items() if k != "seed_lam"})
  return call(**a)


def _check_exgd_sets_equal_singles(eng, tag):
  """every (E, R), nsteps and seed_lam form on this handle: rows, per-set sums, dz0 and dlam0 of the sets call = the single-set call on each set"""
  for E, R in NS_.SETS:
    P = NS_.weight_sets(E)
    c = NS_.instances(eng.n, eng.m, E, R, seed=100 * E + R, nx=_nx(eng))
    for nsteps in (0, 1, 2):
      for kw in ({}, {"seed_lam": None}):
        rows, sums = _exgd_sets(eng, c, P, nsteps, **kw), _exgd_sets(eng, c, P, nsteps, reduce=True, **kw)
        assert rows["grad"].shape == (E, R, NP) and sums["grad"].shape == (E, NP) and rows["dz0"].shape == (E, R, eng.n)
        for e in range(E):
          one, one_sum = _exgd_single(eng, c, P, e, nsteps, **kw), _exgd_single(eng, c, P, e, nsteps, reduce=True, **kw)
          where = (tag, E, R, nsteps, sorted(kw), e)
          for k in KEYS:
            assert rows[k][e].tobytes() == one[k].tobytes(), where + (k,)
          assert sums["grad"][e].tobytes() == one_sum["grad"].tobytes(), where
          assert sums["dz0"][e].tobytes() == one["dz0"].tobytes() and sums["dlam0"][e].tobytes() == one["dlam0"].tobytes(), where
        if nsteps:
          assert np.abs(rows["grad"]).max() > 0
          if E > 1:      # the inputs of set 0 under the weights of set 1 give other bits: the weights take part
            swapped = _exgd_single(eng, c, P[[1] + list(range(1, E))], 0, nsteps, **kw)
            assert swapped["grad"].tobytes() != rows["grad"][0].tobytes()


# ---- bit equality with the single-set calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wpi", [1, 2, 4])
@pytest.mark.parametrize("N", [1, 3])       # 3 points: fewer than the 4 wavefronts; 7 points: a partial second round
def test_exgd_grad_sets_equal_single_calls_hermite_simpson(monkeypatch, N, wpi):
  monkeypatch.setenv("MYRIAD_NODE_EXGD_WPI", str(wpi))      # (the handle reads it at creation)
  eng = _hs_engine(N)
  _check_exgd_sets_equal_singles(eng, ("HS", N, wpi))
  eng.close()


@pytest.mark.parametrize("method", ["HEUN", "RK4"])
@pytest.mark.parametrize("I,cpi", SHOOT_SHAPES)
def test_exgd_grad_sets_equal_single_calls_shooting(I, cpi, method):
  eng = _shoot_engine(I, cpi, method)
  _check_exgd_sets_equal_singles(eng, ("SHOOTING", I, cpi, method))
  eng.close()


def _hvp_engines():
  return [("HS-1", lambda: _hs_engine(1)), ("HS-3", lambda: _hs_engine(3))] + \
         [(f"SHOOTING-{I}x{cpi}-{method}", lambda I=I, cpi=cpi, method=method: _shoot_engine(I, cpi, method))
          for (I, cpi), method in zip(SHOOT_SHAPES, ("HEUN", "RK4", "HEUN"))]


@pytest.mark.parametrize("name,make", _hvp_engines(), ids=[n for n, _ in _hvp_engines()])
def test_hvp_sets_equal_single_calls(name, make):
  eng = make()
  for E, R in NS_.SETS:
    P = NS_.weight_sets(E)
    c = NS_.instances(eng.n, eng.m, E, R, seed=300 * E + R, nx=_nx(eng))
    for wc in (True, False):
      for lam in (c["lam"], None):
        for want in (dict(want_z=True, want_p=False), dict(want_z=False, want_p=True), dict(want_z=True, want_p=True)):
          rows = eng.hvp_node_sets(c["z"], lam, c["v"], P, with_cost=wc, **want)
          sums = eng.hvp_node_sets(c["z"], lam, c["v"], P, with_cost=wc, reduce=True, **want) if want["want_p"] else None
          for e in range(E):
            le = None if lam is None else lam[e]
            one = eng.hvp_node(c["z"][e], le, c["v"][e], P[e], with_cost=wc, **want)
            where = (name, E, R, wc, lam is None, sorted(k for k, v in want.items() if v), e)
            assert set(one) == set(rows)
            for k in one:
              assert rows[k][e].tobytes() == one[k].tobytes(), where + (k,)
            if sums is not None:
              one_sum = eng.hvp_node(c["z"][e], le, c["v"][e], P[e], with_cost=wc, reduce=True, **want)
              assert sums["hp"][e].tobytes() == one_sum["hp"].tobytes(), where
              if want["want_z"]:
                assert sums["hz"][e].tobytes() == one["hz"].tobytes(), where
    if E > 1:
      a = eng.hvp_node(c["z"][0], c["lam"][0], c["v"][0], P[1], want_p=True)
      b = eng.hvp_node(c["z"][0], c["lam"][0], c["v"][0], P[0], want_p=True)
      assert a["hz"].tobytes() != b["hz"].tobytes() and a["hp"].tobytes() != b["hp"].tobytes()      # the weights take part
  eng.close()


# ---- chunks of the history that begin and end inside a set ------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda: _hs_engine(3), lambda: _shoot_engine(2, 2, "HEUN"), lambda: _shoot_engine(4, 1, "RK4")],
                         ids=["HS-3", "SHOOTING-2x2-HEUN", "SHOOTING-4x1-RK4"])
def test_chunks_that_straddle_sets_give_the_unchunked_bits(monkeypatch, make):
  E, R, nsteps = 3, 2, 2
  eng = make()
  P = NS_.weight_sets(E)
  c = NS_.instances(eng.n, eng.m, E, R, seed=77, nx=_nx(eng))
  monkeypatch.delenv("MYRIAD_EXGD_GRAD_HIST_BYTES", raising=False)
  rows, sums = _exgd_sets(eng, c, P, nsteps), _exgd_sets(eng, c, P, nsteps, reduce=True)
  per = (nsteps * (2 * eng.n + eng.m) + eng.n) * 8              # bytes of one instance's history (exgd_grad_chunk)
  for chunk in (R + 1, 1):                                      # 3 instances: set 0 and half of set 1, then the rest; 1: every instance its own launch
    monkeypatch.setenv("MYRIAD_EXGD_GRAD_HIST_BYTES", str(chunk * per))      # (read at every call)
    ch, chs = _exgd_sets(eng, c, P, nsteps), _exgd_sets(eng, c, P, nsteps, reduce=True)
    for k in KEYS:
      assert ch[k].tobytes() == rows[k].tobytes(), (chunk, k)
    assert chs["grad"].tobytes() == sums["grad"].tobytes(), chunk
    for e in range(E):                                          # ... and the single-set call, itself chunked
      one = _exgd_single(eng, c, P, e, nsteps)
      assert one["grad"].tobytes() == rows["grad"][e].tobytes(), (chunk, e)
  eng.close()


# ---- host and device arrays; what ran before -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda: _hs_engine(3), lambda: _shoot_engine(2, 2, "HEUN")], ids=["HS-3", "SHOOTING-2x2-HEUN"])
def test_device_arrays_and_a_used_handle_give_the_same_bits(make):
  E, R, nsteps = 3, 2, 2
  eng = make()
  P = NS_.weight_sets(E)
  c = NS_.instances(eng.n, eng.m, E, R, seed=78, nx=_nx(eng))
  rows, sums = _exgd_sets(eng, c, P, nsteps), _exgd_sets(eng, c, P, nsteps, reduce=True)
  hv = eng.hvp_node_sets(c["z"], c["lam"], c["v"], P, want_p=True)
  hvs = eng.hvp_node_sets(c["z"], c["lam"], c["v"], P, want_p=True, reduce=True)
  dev = "cuda:0"
  t = {k: torch.tensor(np.ascontiguousarray(c[k]), device=dev) for k in ("z", "lam", "lb", "ub", "seed_z", "seed_lam", "v")}
  tp = torch.tensor(P, device=dev)
  new = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)
  g, gs, dz, dl = new(E, R, NP), new(E, NP), new(E, R, eng.n), new(E, R, eng.m)
  eng.exgd_grad_node_sets_device(E, R, t["z"], t["lam"], t["lb"], t["ub"], c["eta_x"], c["eta_v"], nsteps, t["seed_z"], g, NP, tp,
                                 seed_lam=t["seed_lam"], dz0=dz, dlam0=dl)
  eng.exgd_grad_node_sets_device(E, R, t["z"], t["lam"], t["lb"], t["ub"], c["eta_x"], c["eta_v"], nsteps, t["seed_z"], gs, 0, tp,
                                 seed_lam=t["seed_lam"])
  hz, hp, hps = new(E, R, eng.n), new(E, R, NP), new(E, NP)
  eng.hvp_node_sets_device(E, R, t["z"], t["lam"], t["v"], tp, out_z=hz, out_p=hp, p_stride=NP)
  eng.hvp_node_sets_device(E, R, t["z"], t["lam"], t["v"], tp, out_p=hps, p_stride=0)
  torch.cuda.synchronize()
  b = lambda x: x.cpu().numpy().tobytes()
  assert b(g) == rows["grad"].tobytes() and b(gs) == sums["grad"].tobytes() and b(dz) == rows["dz0"].tobytes() and b(dl) == rows["dlam0"].tobytes()
  assert b(hz) == hv["hz"].tobytes() and b(hp) == hv["hp"].tobytes() and b(hps) == hvs["hp"].tobytes()
  assert b(t["z"]) == c["z"].tobytes() and b(tp) == P.tobytes()                   # inputs are not modified
  # unrelated calls on the handle, then the same calls again: the same bits
  eng.exgd(c["z"][0], c["lam"][0], c["lb"][0], c["ub"][0], c["eta_x"], c["eta_v"], 1, params=P[2])
  eng.vjp(c["z"][1], c["lam"][1], params=P[1])
  again, again_hv = _exgd_sets(eng, c, P, nsteps), eng.hvp_node_sets(c["z"], c["lam"], c["v"], P, want_p=True)
  assert all(again[k].tobytes() == rows[k].tobytes() for k in KEYS)
  assert again_hv["hz"].tobytes() == hv["hz"].tobytes() and again_hv["hp"].tobytes() == hv["hp"].tobytes()
  eng.close()


# ---- E == 0 and the refusals ---------------------------------------------------------------------------------------------------------------
def _raw_calls(eng, c, P, grad, hz):
  ptr = {k: c[k].ctypes.data for k in ("z", "lam", "lb", "ub", "seed_z", "v")}
  ptr.update(params=P.ctypes.data, grad=grad.ctypes.data, out_z=hz.ctypes.data)

  def exgd(E=2, R=1, nsteps=1, grad_stride=NP, mem=_lib.MEM_HOST, **null):
    a = dict(ptr); a.update(null)
    return eng.lib.myr_exgd_grad_node_sets(eng._h, E, R, a["z"], a["lam"], a["lb"], a["ub"], a["params"], c["eta_x"], c["eta_v"], nsteps, a["seed_z"], None,
                                           a["grad"], grad_stride, None, None, mem)

  def hvp(E=2, R=1, p_stride=NP, mem=_lib.MEM_HOST, out_p=None, **null):
    a = dict(ptr); a.update(null)
    return eng.lib.myr_hvp_node_sets(eng._h, E, R, a["z"], a["lam"], a["v"], a["params"], 1, a["out_z"], out_p, p_stride, mem)

  return exgd, hvp


@pytest.mark.parametrize("scheme", ["HERMITE_SIMPSON", "SHOOTING"])
def test_no_sets_and_the_refusals(scheme):
  make = lambda system="NODE_CARTPOLE", tr=scheme: _lib.Engine(system, tr, 3, 0.3)
  eng = make()
  E, R = 2, 1
  P = NS_.weight_sets(E)
  c = {k: np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v for k, v in NS_.instances(eng.n, eng.m, E, R, seed=79, nx=_nx(eng)).items()}
  grad, hz = np.full((E, R, NP), 7.0), np.full((E, R, eng.n), 7.0)
  exgd, hvp = _raw_calls(eng, c, P, grad, hz)
  # E == 0: MYR_OK, nothing written
  assert exgd(E=0) == 0 and hvp(E=0) == 0 and (grad == 7.0).all() and (hz == 7.0).all()
  eng.exgd_grad_node_sets_probe(); eng.hvp_node_sets_probe()
  assert exgd() == 0 and hvp() == 0 and not (grad == 7.0).any() and not (hz == 7.0).any()
  assert hvp(lam=None) == 0                                                       # lam may be null
  eng.close()
  # (MYR_E_ARG and MYR_E_UNSUPPORTED -- another system, TRAPEZOIDAL -- with their full texts and the order of the checks: tests/test_gpu_api.py)


def test_capacity_bounds_are_those_of_the_single_set_calls():
  P = NS_.weight_sets(1)
  eng = _hs_engine(400)                                          # (5 064 + 54 N + 19) doubles = 213 KB: myr_exgd_grad_node refuses it too
  z = np.zeros((1, 1, eng.n))
  with pytest.raises(_lib.MyriadHipError, match="myr_exgd_grad_node_sets: intervals too large for the LDS"):
    eng.exgd_grad_node_sets(z, np.zeros((1, 1, eng.m)), -np.ones(eng.n), np.ones(eng.n), 0.01, 0.01, 1, z, P)
  assert eng.hvp_node_sets(z, None, z, P)["hz"].shape == (1, 1, eng.n)      # the Hermite-Simpson product refuses no horizon
  eng.close()
  eng = _lib.Engine("NODE_CARTPOLE", "SHOOTING", 1, 2.0, controls_per_interval=2000)
  z = np.zeros((1, 1, eng.n))
  with pytest.raises(_lib.MyriadHipError, match="myr_exgd_grad_node_sets: intervals x controls_per_interval too large"):
    eng.exgd_grad_node_sets(z, np.zeros((1, 1, eng.m)), -np.ones(eng.n), np.ones(eng.n), 0.01, 0.01, 1, z, P)
  with pytest.raises(_lib.MyriadHipError, match="myr_hvp_node_sets: intervals x controls_per_interval too large"):
    eng.hvp_node_sets(z, None, z, P)
  eng.close()


# ---- one oracle comparison per transcription, on a set other than set 0 ------------------------------------------------------------------------
def _as_sets(case, E, e, keys):
  """the case's arrays [R, ...] as set e of E sets; the other sets get the same inputs (they run under their own weights)"""
  return {k: np.ascontiguousarray(np.broadcast_to(np.asarray(case[k]), (E,) + np.shape(case[k]))) for k in keys}


def test_exgd_grad_oracle_hermite_simpson():
  from node_exgd_grad_cases import rel_error
  E, e = 3, 2
  P = NS_.weight_sets(E)
  case, *ref = NS_.hs_reference(P[e], 3, 3, 2)
  assert case["params"].tobytes() == P[e].tobytes()
  a = _as_sets(case, E, e, ("z", "lam", "lb", "ub", "seed_z", "seed_lam"))
  eng = _hs_engine(3)
  out = eng.exgd_grad_node_sets(a["z"], a["lam"], a["lb"], a["ub"], case["eta_x"], case["eta_v"], case["nsteps"], a["seed_z"], P, seed_lam=a["seed_lam"])
  eng.close()
  errs = tuple(rel_error(out[k][e], r) for k, r in zip(KEYS, ref))
  print("HS sets: device-oracle on set", e, errs)
  assert max(errs) <= HS_ORACLE_TOL, errs
  assert rel_error(out["grad"][0], ref[0]) > 1e-6                # set 0 has other weights: it does not meet this reference


def test_exgd_grad_oracle_shooting():
  from node_shoot_exgd_grad_cases import rel_error
  E, e = 3, 1
  P = NS_.weight_sets(E)
  case, *ref = NS_.shoot_reference(P[e], 3, 2, "HEUN", 3, 2)
  a = _as_sets(case, E, e, ("z", "lam", "lb", "ub", "seed_z", "seed_lam"))
  eng = _shoot_engine(3, 2, "HEUN")
  out = eng.exgd_grad_node_sets(a["z"], a["lam"], a["lb"], a["ub"], case["eta_x"], case["eta_v"], case["nsteps"], a["seed_z"], P, seed_lam=a["seed_lam"])
  eng.close()
  rows = case["rows"]
  errs = tuple(rel_error(out[k][e][rows], r[rows]) for k, r in zip(KEYS, ref))
  print("SHOOTING sets: device-oracle on set", e, errs)
  assert max(errs) <= SHOOT_ORACLE_TOL, errs
  assert rel_error(out["grad"][0][rows], ref[0][rows]) > 1e-6


@pytest.mark.parametrize("cs", [("HERMITE_SIMPSON", 3, 1, "HEUN", 2), ("SHOOTING", 3, 2, "HEUN", 2)], ids=["HS", "SHOOTING"])
def test_hvp_oracle(cs):
  from node_hvp_cases import rel_error
  tr, I, cpi, method, batch = cs
  E, e = 3, 2
  P = NS_.weight_sets(E)
  case, ref = NS_.hvp_reference(P[e], *cs)
  a = _as_sets(case, E, e, ("z", "lam", "v"))
  eng = _lib.Engine("NODE_CARTPOLE", tr, I, case["T"], controls_per_interval=cpi, integration_method=method)
  for wc in (1, 0):
    out = eng.hvp_node_sets(a["z"], a["lam"], a["v"], P, with_cost=bool(wc), want_p=True)
    rows = case["rows"]
    errs = (rel_error(out["hz"][e][rows], ref[wc][0][rows]), rel_error(out["hp"][e][rows], ref[wc][1][rows]))
    print(tr, "sets: device-oracle on set", e, "with_cost", wc, errs)
    assert max(errs) <= HVP_ORACLE_TOL, errs
    assert rel_error(out["hp"][0][rows], ref[wc][1][rows]) > 1e-6
  eng.close()


# ---- the optimizer's methods and the driver --------------------------------------------------------------------------------------------------
def _hp(shooting):
  from myriad_amd.config import HParams, OptimizerType, QuadratureRule
  from myriad_amd.systems import SystemType
  if shooting:
    return HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.SHOOTING, intervals=2, controls_per_interval=2, hidden_layers=(64, 64),
                   num_unrolled=2)
  return HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.COLLOCATION, quadrature_rule=QuadratureRule.HERMITE_SIMPSON, intervals=3,
                 num_unrolled=2)


@pytest.mark.parametrize("shooting", [False, True], ids=["HS", "SHOOTING"])
def test_optimizer_methods_route_weight_rows_to_the_sets_calls(shooting):
  from myriad_amd.config import Config
  from myriad_amd.systems.neural_ode import NeuralODE, NodeSystem
  from myriad_amd.trajectory_optimizers import get_optimizer
  hp = _hp(shooting)
  opt = get_optimizer(hp, Config(verbose=False, plot=False), NodeSystem(NeuralODE.load_fitted_cartpole(), hp.system()))
  eng = opt.engine
  E, R = 2, 2
  P = NS_.weight_sets(E)
  c = NS_.instances(eng.n, eng.m, E, R, seed=80, nx=_nx(eng))
  g = opt.unrolled_grad(c["z"], c["lam"], P, c["seed_z"], 2, eta_x=c["eta_x"], eta_v=c["eta_v"], lb=c["lb"], ub=c["ub"])
  gs = opt.unrolled_grad(c["z"], c["lam"], P, c["seed_z"], 2, eta_x=c["eta_x"], eta_v=c["eta_v"], lb=c["lb"], ub=c["ub"], reduce=True)
  ref = _exgd_sets(eng, c, P, 2, seed_lam=None)
  assert g.shape == (E, R, NP) and g.tobytes() == ref["grad"].tobytes()
  assert gs.shape == (E, NP) and gs.tobytes() == _exgd_sets(eng, c, P, 2, seed_lam=None, reduce=True)["grad"].tobytes()
  hz = opt.lagrangian_hessp(c["z"], c["lam"], c["v"], params=P)
  assert hz.shape == (E, R, eng.n) and hz.tobytes() == eng.hvp_node_sets(c["z"], c["lam"], c["v"], P)["hz"].tobytes()


@pytest.mark.parametrize("batched", [False, True], ids=["single", "start_states"])
@pytest.mark.parametrize("shooting", [False, True], ids=["HS", "SHOOTING"])
def test_driver_equals_a_run_per_network(shooting, batched):
  """three epochs of run_node_endtoend_sets on two networks of different seeds, a reset at epoch 2: every array of entry e = run_node_endtoend on
  network e alone, to the bit"""
  from myriad_amd.config import Config
  from myriad_amd.experiments import node_e2e_sysid as D
  from myriad_amd.systems.neural_ode import flat_from_mapping
  hp, cfg = _hp(shooting), Config(verbose=False, plot=False)
  x0s = np.asarray(hp.system().x_0, dtype=np.float64)[None] + np.array([[0.0, 0.0, 0.0, 0.0], [0.05, -0.05, 0.02, 0.0]]) if batched else None
  seeds = (11, 12)
  runs = D.run_node_endtoend_sets(hp, cfg, [D.initial_node(s) for s in seeds], num_epochs=3, start_states=x0s, save_and_reset_time=2, shooting=shooting)
  assert len(runs) == 2
  for e, s in enumerate(seeds):
    one = D.run_node_endtoend(hp, cfg, num_epochs=3, node=D.initial_node(s), start_states=x0s, save_and_reset_time=2, shooting=shooting)
    got = runs[e]
    assert set(got) == set(one) and got["ts"] == one["ts"] == [0, 1, 2]
    assert got["imitation_losses"] == one["imitation_losses"]      # equal floats
    assert np.asarray(got["true_opt_us"]).tobytes() == np.asarray(one["true_opt_us"]).tobytes()
    for k in ("primal_guesses", "dual_guesses"):
      assert len(got[k]) == len(one[k]) and all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got[k], one[k])), (e, k)
    assert sorted(got["saved_params"]) == sorted(one["saved_params"]) == [0, 2, 3]
    for ep in one["saved_params"]:
      assert flat_from_mapping(got["saved_params"][ep]).tobytes() == flat_from_mapping(one["saved_params"][ep]).tobytes(), (e, ep)
    assert flat_from_mapping(got["params"]).tobytes() == flat_from_mapping(one["params"]).tobytes()
  assert flat_from_mapping(runs[0]["params"]).tobytes() != flat_from_mapping(runs[1]["params"]).tobytes()
