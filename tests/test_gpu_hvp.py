"""myr_hvp on the device (myriad_amd/csrc/colloc_hvp.h: colloc_hvp_kernel; shoot_hvp.h: shoot_hvp_kernel, shoot_hvp_gather_kernel) against its host
twin, the oracle, central differences of myr_vjp, and itself across the forms of the call.

Tolerances (profiles/r17_hvp/README.md; the figures are the largest |d| / max|row| over out_z and out_p, measured on an MI355X with the cases as
they stand):
  device against twin     parity cases (B = 3): 10 x 4.1e-15 (VANDERPOL Hermite-Simpson); shape cases: 10 x 2.3e-14 (out_p of CARTPOLE shooting 20 x 5 RK4,
                          B = 130; Hermite-Simpson N = 33 8.7e-15, 1 x 65 Euler 1.4e-14).  The two run the same algebra and differ
                          by the compiler's FMA contraction and, under the collocation schemes, the order of the parameter sum (butterfly / ascending).
  device against oracle   10 x the host twin's asserted bound against the oracle (tests/test_hvp_host_twin.py): 1e-11 for out_z, 2.7e-11 for out_p
                          (measured 8.0e-16 and 3.6e-15 at worst)
  central differences     1e-6 of the row's largest entry (the project's figure for such differences)
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import hvp_cases as H
import test_hvp_host_twin as T
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

PARITY_TWIN_MEASURED = 4.1e-15   # the parity cases: VANDERPOL Hermite-Simpson with the cost (the others 5e-17 ... 1.8e-15)
SHAPE_TWIN_MEASURED = 2.3e-14    # the shape cases: out_p of shooting 20 x 5 RK4, B = 130 (the others 1e-16 ... 1.4e-14)
PARITY_TWIN_TOL = 10.0 * PARITY_TWIN_MEASURED
SHAPE_TWIN_TOL = 10.0 * SHAPE_TWIN_MEASURED
ORACLE_Z_TOL, ORACLE_P_TOL = 10.0 * T.Z_TOL, 10.0 * T.P_TOL
PARITY = ("CARTPOLE", "VANDERPOL", "CANCERTREATMENT", "BACTERIA", "TIMBERHARVEST", "BEARPOPULATIONS", "ROCKETLANDING", "PREDATORPREY")
PARITY_SHAPES = tuple(s for s in H.HOST_SHAPES if s[1] == 3)      # the two collocation schemes at N = 3, shooting 3 x 2 under the four integrators


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return H.build_twin(tmp_path_factory.mktemp("hvp_twin_gpu"))


def _engine(c):
  return _lib.Engine(c["name"], c["tr"], c["N"], c["T"], controls_per_interval=c["cpi"], integration_method=c["method"])


def _device(eng, c, with_cost=True, **kw):
  a = dict(z=c["z"], lam=c["lam"], v=c["v"], params=c["params"], with_cost=with_cost, want_z=True, want_p=True)
  a.update(kw)
  return eng.hvp(**a)


# ---- parity with the oracle and the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY)
def test_parity_with_the_oracle_and_the_twin(twin, name):
  worst_t, worst_o = 0.0, 0.0
  for tr, N, cpi, method in PARITY_SHAPES:
    for wc in (1, 0):
      case, ref_z, ref_p = H.reference(name, tr, N, cpi, method, 3, wc)
      eng = _engine(case)
      out = _device(eng, case, wc)
      eng.close()
      tz, tp = H.twin_of_case(twin, case, wc)
      et = max(H.rel_error(out["hz"], tz), H.rel_error(out["hp"], tp))
      eoz, eop = H.rel_error(out["hz"], ref_z), H.rel_error(out["hp"], ref_p)
      print(f"{name} {tr} {N}x{cpi} {method} with_cost={wc}: device-twin {et:.2e} device-oracle z {eoz:.2e} p {eop:.2e}")
      worst_t, worst_o = max(worst_t, et), max(worst_o, eoz, eop)
      assert np.isfinite(out["hz"]).all() and np.isfinite(out["hp"]).all()
      assert et <= PARITY_TWIN_TOL, (tr, method, wc, et)
      assert eoz <= ORACLE_Z_TOL and eop <= ORACLE_P_TOL, (tr, method, wc, eoz, eop)
  print(f"{name}: device-twin {worst_t:.2e} device-oracle {worst_o:.2e}")


# ---- shapes where the kernels can go wrong, against the twin ---------------------------------------------------------------------------
SHAPES = ([("HERMITE_SIMPSON", N, 1, "HEUN") for N in (1, 31, 32, 33)] + [("TRAPEZOIDAL", N, 1, "HEUN") for N in (63, 64, 65)] +
          [("SHOOTING", I, cpi, m) for I, cpi in ((1, 1), (1, 65), (43, 1), (20, 5)) for m in ("RK4", "EULER")])


@pytest.mark.parametrize("tr,N,cpi,method", SHAPES)
def test_awkward_shapes_against_the_twin(twin, tr, N, cpi, method):
  """K = 2 N + 1 and N + 1 straddle 64 points; B I = 129 and 130 pairs straddle a wavefront; cpi = 1 makes every control row a shared row"""
  worst = 0.0
  eng = _engine(H.inputs("CARTPOLE", tr, N, cpi, method, 1))
  for B in (1, 3, 130):
    c = H.inputs("CARTPOLE", tr, N, cpi, method, B)
    out = _device(eng, c)
    tz, tp = H.twin_of_case(twin, c)
    ez, ep = H.rel_error(out["hz"], tz), H.rel_error(out["hp"], tp)
    worst = max(worst, ez, ep)
    assert np.abs(tz).max() > 0 and np.abs(tp).max() > 0
    assert max(ez, ep) <= SHAPE_TWIN_TOL, (B, ez, ep)
  eng.close()
  print(f"{tr} {N}x{cpi} {method}: device-twin {worst:.2e}")


# ---- independent of the oracle and the twin ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("CARTPOLE", "VANDERPOL"))
@pytest.mark.parametrize("tr,N,cpi,method", (("HERMITE_SIMPSON", 10, 1, "HEUN"), ("SHOOTING", 4, 5, "RK4")))
def test_central_differences_of_myr_vjp(name, tr, N, cpi, method):
  """g = grad_z L from myr_vjp (add_gradf = 1): (g(z + eps v) - g(z - eps v)) / 2 eps against out_z, v^T (g(p + d) - g(p - d)) / 2 d against out_p"""
  c = H.inputs(name, tr, N, cpi, method, 2)
  eng = _engine(c)
  out = _device(eng, c)
  g = lambda z, p: eng.vjp(z, c["lam"], params=p, add_gradf=True)
  eps = 1e-6 * (1.0 + np.abs(c["z"]).max())
  fz = (g(c["z"] + eps * c["v"], c["params"]) - g(c["z"] - eps * c["v"], c["params"])) / (2.0 * eps)
  fp = np.empty_like(out["hp"])
  for k in range(eng.np):
    d = 1e-6 * np.abs(c["params"][:, k])
    pp, pm = c["params"].copy(), c["params"].copy()
    pp[:, k] += d; pm[:, k] -= d
    fp[:, k] = ((g(c["z"], pp) - g(c["z"], pm)) * c["v"]).sum(axis=1) / (2.0 * d)
  eng.close()
  ez, ep = H.rel_error(out["hz"], fz), H.rel_error(out["hp"], fp)
  print(f"{name} {tr} {method}: out_z against central differences {ez:.2e}, out_p {ep:.2e}")
  assert ez <= 1e-6 and ep <= 1e-6


# ---- forms of the call -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,N,cpi,method", (("HERMITE_SIMPSON", 5, 1, "HEUN"), ("TRAPEZOIDAL", 5, 1, "HEUN"), ("SHOOTING", 4, 3, "RK4"), ("SHOOTING", 4, 3, "HEUN")))
def test_forms_of_the_call(tr, N, cpi, method):
  B = 70
  c = H.inputs("CARTPOLE", tr, N, cpi, method, B)
  eng = _engine(c)
  z_in, lam_in, v_in, p_in = (c[k].copy() for k in ("z", "lam", "v", "params"))
  rows = _device(eng, c)
  # shared parameters = the same row for every instance
  shared = _device(eng, c, params=c["params"][0])
  tiled = _device(eng, c, params=np.tile(c["params"][0], (B, 1)))
  assert shared["hz"].tobytes() == tiled["hz"].tobytes() and shared["hp"].tobytes() == tiled["hp"].tobytes()
  # a null lam is a zero lam
  a, b = _device(eng, c, lam=None), _device(eng, c, lam=np.zeros_like(c["lam"]))
  assert a["hz"].tobytes() == b["hz"].tobytes() and a["hp"].tobytes() == b["hp"].tobytes() and a["hz"].tobytes() != rows["hz"].tobytes()
  # one output alone
  only_z, only_p = _device(eng, c, want_p=False), _device(eng, c, want_z=False)
  assert set(only_z) == {"hz"} and set(only_p) == {"hp"}
  assert only_z["hz"].tobytes() == rows["hz"].tobytes() and only_p["hp"].tobytes() == rows["hp"].tobytes()
  # the batch sum: within 1e-13 scale of the exact row sum, the same bits on every call
  s1, s2 = _device(eng, c, reduce=True), _device(eng, c, reduce=True)
  exact = np.array([float(sum(Fraction(float(x)) for x in rows["hp"][:, k])) for k in range(eng.np)])
  assert (np.abs(s1["hp"] - exact) <= 1e-13 * np.abs(rows["hp"]).sum(axis=0)).all()
  assert s1["hp"].tobytes() == s2["hp"].tobytes() and s1["hz"].tobytes() == rows["hz"].tobytes()
  # device arrays: the same bits as host arrays
  t = {k: torch.tensor(c[k], device="cuda:0") for k in ("z", "lam", "v", "params")}
  hz = torch.empty_like(t["z"]); hp = torch.empty((B, eng.np), dtype=torch.float64, device="cuda:0"); hs = torch.empty(eng.np, dtype=torch.float64, device="cuda:0")
  eng.hvp_device(B, t["z"], t["lam"], t["v"], out_z=hz, out_p=hp, p_stride=eng.np, params=t["params"], params_stride=eng.np)
  eng.hvp_device(B, t["z"], t["lam"], t["v"], out_p=hs, p_stride=0, params=t["params"], params_stride=eng.np)
  torch.cuda.synchronize()
  assert hz.cpu().numpy().tobytes() == rows["hz"].tobytes() and hp.cpu().numpy().tobytes() == rows["hp"].tobytes()
  assert hs.cpu().numpy().tobytes() == s1["hp"].tobytes()
  # inputs untouched, on the host and on the device
  for k, ref in (("z", z_in), ("lam", lam_in), ("v", v_in), ("params", p_in)):
    assert (c[k] == ref).all() and (t[k].cpu().numpy() == ref).all()
  # B == 0 does nothing
  eng.hvp_device(0, t["z"], t["lam"], t["v"], out_z=hz, out_p=hp, p_stride=eng.np)
  torch.cuda.synchronize()
  assert hz.cpu().numpy().tobytes() == rows["hz"].tobytes()
  eng.close()


@pytest.mark.parametrize("name,tr,N,cpi,method", (("CARTPOLE", "HERMITE_SIMPSON", 40, 1, "HEUN"), ("CARTPOLE", "TRAPEZOIDAL", 40, 1, "HEUN"),
                                                  ("CARTPOLE", "SHOOTING", 7, 3, "RK4"), ("BACTERIA", "SHOOTING", 7, 3, "RK4"), ("BACTERIA", "TRAPEZOIDAL", 40, 1, "HEUN")))
def test_inherited_registers_do_not_reach_the_result(monkeypatch, name, tr, N, cpi, method):
  """(BACTERIA: the terminal cost is the one branch of the shooting kernel that depends on the lane -- only the pairs of the last interval take it)"""
  c = H.inputs(name, tr, N, cpi, method, 65)            # a partial last wavefront of points / pairs
  bits = {}
  for pat in ("zero", "nan", "random"):
    monkeypatch.setenv("MYRIAD_REG_FILL", pat)
    monkeypatch.setenv("MYRIAD_STACK_FILL", pat)
    eng = _engine(c)                                      # (the handle reads the fill at creation)
    out, red = _device(eng, c), _device(eng, c, reduce=True)
    eng.close()
    assert np.isfinite(out["hz"]).all() and np.isfinite(out["hp"]).all() and np.isfinite(red["hp"]).all()
    bits[pat] = out["hz"].tobytes() + out["hp"].tobytes() + red["hp"].tobytes()
  assert bits["zero"] == bits["nan"] == bits["random"]


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors():
  c = H.inputs("CARTPOLE", "SHOOTING", 3, 2, "HEUN", 2)
  hz, hp = np.full((2, c["n"]), 7.0), np.full((2, 4), 7.0)

  def call(eng, B=2, z=c["z"].ctypes.data, v=c["v"].ctypes.data, oz=hz.ctypes.data, op=hp.ctypes.data, p=c["params"].ctypes.data, pstride=4,
           p_stride=4, mem=_lib.MEM_HOST):
    rc = eng.lib.myr_hvp(eng._h, B, z, c["lam"].ctypes.data, v, p, pstride, 1, oz, op, p_stride, mem)
    return rc, eng.lib.myr_last_error()

  # (the argument checks of the C call and the systems it is not built for, with their full texts and their order: tests/test_gpu_api.py)
  eng = _engine(c)
  assert call(eng)[0] == 0 and (hz != 7.0).any() and (hp != 7.0).any()
  hz[:], hp[:] = 7.0, 7.0
  assert call(eng, B=0)[0] == 0 and (hz == 7.0).all() and (hp == 7.0).all()      # B == 0: nothing is written
  assert call(eng, oz=None)[0] == 0 and call(eng, op=None)[0] == 0
  eng.close()


# ---- the optimizer's method ------------------------------------------------------------------------------------------------------------
def test_lagrangian_hessp():
  from myriad_amd.config import Config, HParams, OptimizerType, QuadratureRule
  from myriad_amd.systems import SystemType
  from myriad_amd.trajectory_optimizers import get_optimizer
  for hp, tr in ((HParams(system=SystemType.VANDERPOL, optimizer=OptimizerType.COLLOCATION, quadrature_rule=QuadratureRule.TRAPEZOIDAL, intervals=5), "TRAPEZOIDAL"),
                 (HParams(system=SystemType.VANDERPOL), "SHOOTING")):      # the reference's default hyperparameters: shooting
    opt = get_optimizer(hp, Config(verbose=False, plot=False), hp.system())
    eng = opt.engine
    assert opt.transcription == tr
    rng = np.random.default_rng(3)
    z = 0.5 + 0.1 * rng.standard_normal(eng.n)
    lam, v = 0.1 * rng.standard_normal(eng.m), rng.standard_normal(eng.n)
    p = opt.system.device_params()
    for wc in (True, False):
      hv = opt.lagrangian_hessp(z, lam, v, with_cost=wc)
      assert hv.shape == (eng.n,)
      assert hv.tobytes() == eng.hvp(z, lam, v, params=p, with_cost=wc)["hz"][0].tobytes()
      s, zt = H.psi("VANDERPOL", tr, hp.intervals, hp.controls_per_interval, hp.integration_method.name, float(opt.system.T), z, lam, v,
                    [float(x) for x in np.atleast_1d(p)], int(wc))
      ref = torch.autograd.grad(s, zt)[0].numpy()
      e = H.rel_error(hv[None], ref[None])
      print(f"{tr} with_cost={wc}: lagrangian_hessp against the oracle {e:.2e}")
      assert np.abs(ref).max() > 0 and e <= ORACLE_Z_TOL


def test_scipy_callbacks_of_the_integration_document(monkeypatch):
  """INTEGRATION.md's hip_hessians as written, on a handle the stub's own declarations create: the objective's hessp and the constraints' hess(x, v)"""
  import ctypes as C
  import os
  import re
  import test_integration_stub as S
  monkeypatch.setenv("MYRIAD_HIP_LIB", S.LIB)
  txt = open(os.path.join(H.ROOT, "INTEGRATION.md")).read()
  blk = [b for b in re.findall(r"```python\n(.*?)```", txt, re.S) if "def hip_hessians" in b]
  ns = {}
  exec(compile(S._blocks()[0], "INTEGRATION.md:hip_sqp", "exec"), ns)
  exec(compile(blk[0], "INTEGRATION.md:hip_hessians", "exec"), ns)
  c = H.inputs("VANDERPOL", "SHOOTING", 4, 5, "RK4", 1)
  d = ns["Desc"](ns["SYS"]["VANDERPOL"], 2, 3, 4, 5, 0, 1, 0, c["T"])
  h = C.c_void_p()
  assert ns["lib"].myr_create(C.byref(d), C.byref(h)) == 0
  dims = ns["Dims"](); ns["lib"].myr_get_dims(h, C.byref(dims))
  hessp, hess = ns["hip_hessians"](h, dims)
  eng = _engine(c)
  f = eng.hvp(c["z"], None, c["v"])["hz"][0]
  g = eng.hvp(c["z"], c["lam"], c["v"], with_cost=False)["hz"][0]
  eng.close()
  assert hessp(c["z"][0], c["v"][0]).tobytes() == f.tobytes() and np.abs(f).max() > 0
  op = hess(c["z"][0], c["lam"][0])
  assert op.shape == (c["n"], c["n"]) and op.matvec(c["v"][0]).tobytes() == g.tobytes() and np.abs(g).max() > 0
  ns["lib"].myr_destroy(h)
