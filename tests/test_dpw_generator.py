"""The generated mixed derivatives (myriad_amd/csrc/systems_dpw_gen.h) are what tools/gen_systems.py --dpw writes today, cover the 20
closed-form systems and no twin, and equal sympy's own mixed derivative of the systems' definitions, evaluated numerically at three random
points per system.  The generator needs sympy, as tools/gen_systems.py always has: without it these tests fail, they do not skip.
(systems_gen.h and systems_dp_gen.h are pinned by tests/test_fit_generator.py; --dpw writes neither.)"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import exgd_grad_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "myriad_amd", "csrc")


def _generator():
  spec = importlib.util.spec_from_file_location("gen_systems", os.path.join(ROOT, "tools", "gen_systems.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


GEN = _generator()
CLOSED = [S for S in GEN.systems() if not S["name"].endswith("_ELASTIC")]


def test_dpw_header_is_reproduced_byte_for_byte(tmp_path):
  gen = _generator()
  gen.OUT_DPW = str(tmp_path / "systems_dpw_gen.h")
  gen.OUT_DP = str(tmp_path / "systems_dp_gen.h")      # (never written by --dpw; kept away from the tree all the same)
  gen.OUT = str(tmp_path / "systems_gen.h")
  gen.main_dpw()
  assert not os.path.exists(gen.OUT) and not os.path.exists(gen.OUT_DP)
  with open(gen.OUT_DPW, "rb") as a, open(os.path.join(CSRC, "systems_dpw_gen.h"), "rb") as b:
    assert a.read() == b.read()


def test_dpw_header_covers_the_twenty_systems_and_no_twin():
  txt = open(os.path.join(CSRC, "systems_dpw_gen.h")).read()
  names = [S["name"] for S in GEN.systems()]
  for n in names:
    assert (f"struct SysDpw<Sys{n}>" in txt) == (not n.endswith("_ELASTIC")), n
  assert sum(not n.endswith("_ELASTIC") for n in names) == 20
  assert "INVASIVEPLANT" not in txt
  for S in CLOSED:                                     # a second function exactly where the system has a terminal cost
    body = txt.split(f"struct SysDpw<Sys{S['name']}>")[1].split("template <>")[0]
    assert ("term_vjp_p_dir" in body) == ("gT" in S), S["name"]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  lib = E.build_twin(tmp_path_factory.mktemp("dpw_twin"))
  vp = C.c_void_p
  lib.dpw_point.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_double, vp, C.c_double, vp, vp]
  lib.dpw_point.restype = C.c_int
  return lib


def _plain(expr, sp):
  """the definitions' gym helpers as sympy's own functions: clip as a Piecewise, angle_normalize as the identity (the points keep |theta| < pi)"""
  expr = expr.replace(GEN.clipf, lambda x, lo, hi: sp.Piecewise((lo, x < lo), (hi, x > hi), (x, True)))
  return expr.replace(GEN.angnormf, lambda x: x)


@pytest.mark.parametrize("S", CLOSED, ids=[S["name"] for S in CLOSED])
def test_vjp_p_dir_is_sympys_mixed_derivative(twin, S):
  import sympy as sp
  x, u, p = list(S["x"]), list(S["u"]), list(S["p"])
  w = x + u
  ns, nu, npar = len(x), len(u), len(p)
  tt = sp.Symbol("tt", nonnegative=True)
  mu = sp.symbols(f"mu0:{ns}", real=True)
  d = sp.symbols(f"d0:{ns + nu}", real=True)
  wg = sp.Symbol("wg", real=True)
  lag = _plain(wg * sp.sympify(S["g"]) + sum(mu[i] * sp.sympify(S["f"][i]) for i in range(ns)), sp)
  phi = sum(d[i] * sp.diff(lag, w[i]) for i in range(ns + nu))
  gp = [sp.diff(phi, pk) for pk in p]
  gT = _plain(sp.sympify(S.get("gT", 0)), sp)
  gpT = [sp.diff(sum(d[i] * sp.diff(gT, w[i]) for i in range(ns + nu)), pk) for pk in p]
  rng = np.random.default_rng(S["id"])
  from myriad_amd._lib import SYS_IDS
  for _ in range(3):
    xv, uv = rng.uniform(0.2, 1.5, ns), rng.uniform(0.2, 2.6, nu)      # positive states (logarithms), controls on both sides of the gym clips
    pv = np.array(S["pdefault"], dtype=np.float64) * (1.0 + 0.1 * (2.0 * rng.random(npar) - 1.0))
    tv, wgv = float(rng.uniform(0.0, 2.0)), float(rng.uniform(0.1, 1.0))
    muv, dv = rng.standard_normal(ns), rng.standard_normal(ns + nu)
    vals = dict(zip(x, xv)) | dict(zip(u, uv)) | dict(zip(p, pv)) | dict(zip(mu, muv)) | dict(zip(d, dv)) | {wg: wgv, tt: tv}
    for which, exprs in ((0, gp), (1, gpT)):
      out = np.full(npar, np.nan)
      rc = twin.dpw_point(SYS_IDS[S["name"]], which, xv.ctypes.data, uv.ctypes.data, pv.ctypes.data, tv, muv.ctypes.data, wgv, dv.ctypes.data,
                          out.ctypes.data)
      if which == 1 and "gT" not in S:
        assert rc == -1
        continue
      assert rc == 0
      ref = np.array([float(sp.N(e.subs(vals), 30)) for e in exprs])
      scale = max(np.abs(ref).max(), 1e-300)
      assert np.abs(out - ref).max() <= 1e-12 * scale, (S["name"], which, out, ref)
      assert which == 1 or np.abs(ref).max() > 0
