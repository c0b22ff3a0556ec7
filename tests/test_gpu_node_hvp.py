"""myr_hvp_node on the device (myriad_amd/csrc/node_hvp.h: node_hvp_colloc_kernel, node_hvp_shoot_kernel) against the oracle, its host twin, central
differences of myr_vjp on the same handle (under SHOOTING K14's matrix-core passes, under collocation the Hermite-Simpson node kernel: independent
implementations), and itself across the forms of the call; TrajectoryOptimizer.lagrangian_hessp over a NodeSystem.

Cases (transcription, I, cpi, method, B) of tests/node_hvp_cases.py, the committed weights, with_cost 1 and 0.  Tolerances: 100 x the largest
rel_error of out_z and out_p measured on an MI355X with the cases as they stand (profiles/r23_node_hvp/README.md); a row is a sum of a few thousand
fp64 products, so a figure above 1e-11 would be a bug.  Central differences: 1e-6 of the row's largest entry, the family's figure.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import node_hvp_cases as H
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

ORACLE_MEASURED = 4.5e-15      # device against torch: lagrangian_hessp at 1 x 100 HEUN 4.48e-15, (SHOOTING, 1, 12, MIDPOINT, 1) without the cost 4.18e-15; the others 4.4e-16 ... 3.2e-15
TWIN_MEASURED = 4.5e-15        # device against the host twin: all 37 instances of (HERMITE_SIMPSON, 3, 1, HEUN, 37) without the cost 4.43e-15; the others 3.2e-16 ... 3.9e-15
ORACLE_TOL = 100.0 * ORACLE_MEASURED
TWIN_TOL = 100.0 * TWIN_MEASURED
assert max(ORACLE_TOL, TWIN_TOL) <= 1e-11
HS_BATCH, SHOOT_BATCH = H.HS_CASES[2], H.SHOOT_CASES[5]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return H.build_twin(tmp_path_factory.mktemp("node_hvp_twin_gpu"))


def _engine(c, system="NODE_CARTPOLE", tr=None):
  tr = c["tr"] if tr is None else tr
  if tr == "SHOOTING":
    return _lib.Engine(system, tr, c["I"], c["T"], controls_per_interval=c["cpi"], integration_method=c["method"])
  return _lib.Engine(system, tr, c["I"], c["T"])


def _device(eng, c, rows=None, **kw):
  r = slice(None) if rows is None else list(rows)
  a = dict(z=c["z"][r], lam=c["lam"][r], v=c["v"][r], params=c["params"], want_p=True)
  a.update(kw)
  return eng.hvp_node(**a)


# ---- parity with the oracle and the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", H.CASES, ids=H.IDS)
def test_parity_with_the_oracle_and_the_twin(twin, cs):
  case, ref = H.reference(*cs)
  rows = case["rows"]
  z_in, lam_in, v_in = case["z"].copy(), case["lam"].copy(), case["v"].copy()
  eng = _engine(case)
  worst_o = worst_t = 0.0
  for wc in (1, 0):
    out = _device(eng, case, with_cost=wc)
    tz, tp = H.twin_of_case(twin, case, wc)
    eo = max(H.rel_error(out["hz"][rows], ref[wc][0][rows]), H.rel_error(out["hp"][rows], ref[wc][1][rows]))
    et = max(H.rel_error(out["hz"], tz), H.rel_error(out["hp"], tp))
    print(f"NODE {cs} with_cost {wc}: device-oracle {eo:.2e} device-twin {et:.2e}")
    worst_o, worst_t = max(worst_o, eo), max(worst_t, et)
  eng.close()
  assert (case["z"] == z_in).all() and (case["lam"] == lam_in).all() and (case["v"] == v_in).all()
  assert worst_o <= ORACLE_TOL, worst_o
  assert worst_t <= TWIN_TOL, worst_t


# ---- independent of the oracle and the twin ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,I,cpi,method", (("HERMITE_SIMPSON", 3, 1, "HEUN"), ("SHOOTING", 3, 2, "HEUN"), ("SHOOTING", 2, 2, "RK4")))
@pytest.mark.parametrize("wc", (1, 0))
def test_central_differences_of_myr_vjp(tr, I, cpi, method, wc):
  """g = grad_z L from myr_vjp (add_gradf = with_cost): (g(z + e v) - g(z - e v)) / 2 e against out_z; <g(z; p + d) - g(z; p - d), v> / 2 against
  out_p . (|p| o r), d = 1e-6 |p| o r with r uniform in [-1, 1]"""
  c = H.inputs(tr, I, cpi, method, 2)
  p = c["params"]
  eng = _engine(c)
  out = _device(eng, c, with_cost=wc)
  g = lambda z, pp: eng.vjp(z, c["lam"], params=pp, add_gradf=bool(wc))
  eps = 1e-6 * (1.0 + np.abs(c["z"]).max())
  fz = (g(c["z"] + eps * c["v"], p) - g(c["z"] - eps * c["v"], p)) / (2.0 * eps)
  ez = H.rel_error(out["hz"], fz)
  print(f"NODE {tr} {I}x{cpi} {method} with_cost {wc}: out_z against central differences {ez:.2e}")
  assert np.abs(fz).max() > 0 and ez <= 1e-6
  rng = np.random.default_rng(11)
  for _ in range(3):
    delta = np.abs(p) * rng.uniform(-1.0, 1.0, p.size)
    fd = ((g(c["z"], p + 1e-6 * delta) - g(c["z"], p - 1e-6 * delta)) * c["v"]).sum(axis=1) / 2e-6
    an = out["hp"] @ delta
    print("  out_p . delta", an, "central differences", fd)
    np.testing.assert_allclose(an, fd, rtol=1e-6)
  eng.close()


# ---- forms of the call -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", (HS_BATCH, SHOOT_BATCH, H.SHOOT_CASES[2]), ids=lambda c: "-".join(map(str, c)))
def test_forms_of_the_call(cs):
  c, _ = H.reference(*cs)
  B = c["z"].shape[0]
  eng = _engine(c)
  rows, again = _device(eng, c), _device(eng, c)
  assert rows["hz"].tobytes() == again["hz"].tobytes() and rows["hp"].tobytes() == again["hp"].tobytes()      # two calls: the same bits
  # out_z with and without out_p; out_p alone
  only_z, only_p = _device(eng, c, want_p=False), _device(eng, c, want_z=False)
  assert set(only_z) == {"hz"} and set(only_p) == {"hp"}
  assert only_z["hz"].tobytes() == rows["hz"].tobytes() and only_p["hp"].tobytes() == rows["hp"].tobytes()
  # a null lam is a zero lam, and not the case's
  a, b = _device(eng, c, lam=None), _device(eng, c, lam=np.zeros_like(c["lam"]))
  assert a["hz"].tobytes() == b["hz"].tobytes() and a["hp"].tobytes() == b["hp"].tobytes() and a["hz"].tobytes() != rows["hz"].tobytes()
  # the batch sum: the row sum within the twin tolerance, the same bits on every call
  s1, s2 = _device(eng, c, reduce=True), _device(eng, c, reduce=True)
  exact = np.array([float(sum(Fraction(float(x)) for x in rows["hp"][:, k])) for k in range(eng.np)])
  assert H.rel_error(s1["hp"][None], exact[None]) <= TWIN_TOL
  assert s1["hp"].tobytes() == s2["hp"].tobytes() and s1["hz"].tobytes() == rows["hz"].tobytes()
  # a call of another shape and flag on the same handle in between
  _device(eng, c, rows=[0], with_cost=0, lam=None)
  after = _device(eng, c)
  assert after["hz"].tobytes() == rows["hz"].tobytes() and after["hp"].tobytes() == rows["hp"].tobytes()
  # device arrays: the same bits as host arrays, inputs untouched
  t = {k: torch.tensor(np.array(c[k]), device="cuda:0") for k in ("z", "lam", "v", "params")}
  hz = torch.empty_like(t["z"]); hp = torch.empty((B, eng.np), dtype=torch.float64, device="cuda:0")
  hs = torch.empty(eng.np, dtype=torch.float64, device="cuda:0")
  eng.hvp_node_device(B, t["z"], t["lam"], t["v"], t["params"], out_z=hz, out_p=hp, p_stride=eng.np)
  eng.hvp_node_device(B, t["z"], t["lam"], t["v"], t["params"], out_p=hs, p_stride=0)
  torch.cuda.synchronize()
  assert hz.cpu().numpy().tobytes() == rows["hz"].tobytes() and hp.cpu().numpy().tobytes() == rows["hp"].tobytes()
  assert hs.cpu().numpy().tobytes() == s1["hp"].tobytes()
  for k in ("z", "lam", "v", "params"):
    assert (t[k].cpu().numpy() == c[k]).all()
  eng.close()


@pytest.mark.parametrize("cs", (HS_BATCH, SHOOT_BATCH), ids=lambda c: "-".join(map(str, c)))
def test_an_instance_alone_gives_the_bits_it_gives_inside_the_batch(cs):
  c, _ = H.reference(*cs)
  eng = _engine(c)
  whole, alone = _device(eng, c), _device(eng, c, rows=[21])
  eng.close()
  assert np.isfinite(whole["hz"]).all() and np.isfinite(whole["hp"]).all()
  assert whole["hz"][21].tobytes() == alone["hz"][0].tobytes() and whole["hp"][21].tobytes() == alone["hp"][0].tobytes()


def test_a_handle_that_ran_other_calls_gives_the_same_bits():
  """a fresh handle against one that has run myr_vjp, myr_exgd_grad_node_shoot and a product of another flag before"""
  c, _ = H.reference(*H.SHOOT_CASES[1])
  eng = _engine(c)
  fresh = _device(eng, c)
  eng.close()
  eng = _engine(c)
  eng.vjp(c["z"], c["lam"], params=c["params"], add_gradf=True)
  eng.exgd_grad_node_shoot(c["z"], c["lam"], -10.0 * np.ones(c["n"]), 10.0 * np.ones(c["n"]), 0.01, 0.5, 1, c["v"], c["params"])
  _device(eng, c, with_cost=0, rows=[1])
  used = _device(eng, c)
  eng.close()
  assert fresh["hz"].tobytes() == used["hz"].tobytes() and fresh["hp"].tobytes() == used["hp"].tobytes()


def test_inherited_registers_do_not_reach_the_result(monkeypatch):
  bits = {}
  for pat in ("zero", "nan", "random"):
    monkeypatch.setenv("MYRIAD_REG_FILL", pat)
    monkeypatch.setenv("MYRIAD_STACK_FILL", pat)
    bits[pat] = b""
    for cs in (H.HS_CASES[1], H.SHOOT_CASES[4]):
      c, _ = H.reference(*cs)
      eng = _engine(c)                                           # (the handle reads the fill at creation)
      out, red = _device(eng, c), _device(eng, c, reduce=True)
      eng.close()
      assert np.isfinite(out["hz"]).all() and np.isfinite(out["hp"]).all()
      bits[pat] += out["hz"].tobytes() + out["hp"].tobytes() + red["hp"].tobytes()
  assert bits["zero"] == bits["nan"] == bits["random"]


# ---- a long horizon ----------------------------------------------------------------------------------------------------------------------
def test_the_horizon_myr_exgd_grad_node_refuses(twin):
  c = H.inputs("HERMITE_SIMPSON", 400, 1, "HEUN", 1)
  eng = _engine(c)
  with pytest.raises(_lib.MyriadHipError, match="too large for the LDS"):
    eng.exgd_grad_node(c["z"], c["lam"], -np.ones(c["n"]), np.ones(c["n"]), 0.01, 0.01, 1, c["v"], c["params"])
  out = _device(eng, c)
  eng.close()
  tz, tp = H.twin_of_case(twin, c)
  ez, ep = H.rel_error(out["hz"], tz), H.rel_error(out["hp"], tp)
  print(f"NODE HERMITE_SIMPSON N = 400: device-twin out_z {ez:.2e} out_p {ep:.2e}")
  assert np.abs(tz).max() > 0 and np.abs(tp).max() > 0 and max(ez, ep) <= TWIN_TOL


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors():
  c = H.inputs("SHOOTING", 3, 2, "HEUN", 2)
  p = np.array(c["params"])
  hz, hp = np.full((2, c["n"]), 7.0), np.full((2, 4804), 7.0)
  d = np.zeros(4804)

  def call(eng, B=2, z=c["z"].ctypes.data, lam=c["lam"].ctypes.data, v=c["v"].ctypes.data, params=p.ctypes.data, oz=hz.ctypes.data,
           op=hp.ctypes.data, p_stride=4804, mem=_lib.MEM_HOST):
    rc = eng.lib.myr_hvp_node(eng._h, B, z, lam, v, params, 1, oz, op, p_stride, mem)
    return rc, eng.lib.myr_last_error()

  # (the argument checks of the C call, the handles it refuses and myr_hvp's refusal of the network system, with their full texts and their
  # order: tests/test_gpu_api.py)
  eng = _engine(c)
  assert call(eng)[0] == 0 and np.isfinite(hz).all() and (hz != 7.0).any() and (hp != 7.0).any()
  hz[:], hp[:] = 7.0, 7.0
  assert call(eng, B=0)[0] == 0 and (hz == 7.0).all() and (hp == 7.0).all()      # B == 0: nothing is written
  assert call(eng, oz=None)[0] == 0 and call(eng, op=None)[0] == 0 and call(eng, lam=None)[0] == 0
  eng.hvp_node_probe()
  eng.close()
  # beyond the LDS formula: 5 064 + 13 + 9 x 2 000 doubles = 185 KB; 1 x 1 711 HEUN is the last that fits, 1 x 1 712 the first that does not
  eng = _lib.Engine("NODE_CARTPOLE", "SHOOTING", 1, 2.0, controls_per_interval=2000, integration_method="HEUN")
  with pytest.raises(_lib.MyriadHipError, match="too large for the LDS") as e:
    eng.hvp_node_probe()
  assert e.value.args and "myr_hvp_node" in str(e.value)
  eng.close()
  for cpi, fits in ((1711, True), (1712, False)):
    eng = _lib.Engine("NODE_CARTPOLE", "SHOOTING", 1, 2.0, controls_per_interval=cpi, integration_method="HEUN")
    rc = eng.lib.myr_hvp_node(eng._h, 0, d.ctypes.data, None, d.ctypes.data, d.ctypes.data, 1, d.ctypes.data, None, 0, _lib.MEM_HOST)
    assert rc == (0 if fits else -4), (cpi, rc)
    eng.close()


# ---- the optimizer's method ------------------------------------------------------------------------------------------------------------
def test_lagrangian_hessp_over_a_node_system():
  from myriad_amd.config import Config, HParams, OptimizerType, QuadratureRule
  from myriad_amd.systems import SystemType
  from myriad_amd.systems.neural_ode import NeuralODE, NodeSystem, flat_from_mapping
  from myriad_amd.trajectory_optimizers import get_optimizer
  node = NeuralODE.load_fitted_cartpole()
  for hp, tr in ((HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.COLLOCATION, quadrature_rule=QuadratureRule.HERMITE_SIMPSON, intervals=5,
                          hidden_layers=(64, 64)), "HERMITE_SIMPSON"),
                 (HParams(system=SystemType.CARTPOLE, hidden_layers=(64, 64)), "SHOOTING")):      # the reference's default hyperparameters: shooting
    opt = get_optimizer(hp, Config(verbose=False, plot=False), NodeSystem(node, hp.system()))
    eng = opt.engine
    assert opt.transcription == tr
    rng = np.random.default_rng(3)
    nx = 4 * (2 * hp.intervals + 1 if tr == "HERMITE_SIMPSON" else hp.intervals + 1)
    z = np.concatenate([0.5 * rng.standard_normal(nx), rng.uniform(-5.0, 5.0, eng.n - nx)])
    lam, v = 0.1 * rng.standard_normal(eng.m), rng.standard_normal(eng.n)
    flat = flat_from_mapping(node.params)
    moved = {k: {f: 1.01 * np.asarray(a) for f, a in layer.items()} for k, layer in node.params.items()}      # another Haiku mapping
    for wc in (True, False):
      hv = opt.lagrangian_hessp(z, lam, v, with_cost=wc)
      assert hv.shape == (eng.n,)
      assert hv.tobytes() == eng.hvp_node(z, lam, v, flat, with_cost=wc)["hz"][0].tobytes()
      assert hv.tobytes() == opt.lagrangian_hessp(z, lam, v, params=node.params, with_cost=wc).tobytes()
      hm = opt.lagrangian_hessp(z, lam, v, params=moved, with_cost=wc)
      assert hm.tobytes() == eng.hvp_node(z, lam, v, flat_from_mapping(moved), with_cost=wc)["hz"][0].tobytes() and hm.tobytes() != hv.tobytes()
      ref = H.oracle_hvp(tr, hp.intervals, hp.controls_per_interval, hp.integration_method.name, float(opt.system.T), z, lam, v, int(wc))[0]
      e = H.rel_error(hv[None], ref[None])
      print(f"NODE {tr} with_cost={wc}: lagrangian_hessp against the oracle {e:.2e}")
      assert np.abs(ref).max() > 0 and e <= ORACLE_TOL
