"""Inputs and oracle references shared by the tests of the Lagrangian Hessian-vector product (test_hvp_host_twin.py, test_gpu_hvp.py).

A case is (system, transcription, N, cpi, integrator, batch).  Its inputs are drawn from a fixed seed the way exgd_grad_cases.py and fit_cases.py
draw theirs: states at x_0 (1 + 0.05 N(0,1)) (plus 0.05 N(0,1) where x_0 has zeros), controls from fit_cases._controls, a parameter row per
instance (the defaults moved by up to 5 %), lam = 0.1 N(0,1), v = N(0,1), steps of at most 0.05: T = min(system.T, 0.05 I cpi).

With L(z, lam, p) = with_cost f(z, p) + lam^T c(z, p) and psi = <grad_z L, v>, the reference is torch.autograd.grad(psi, [z, p...]) with
create_graph=True through `oracle.make_transcription`, the parameters as tensors (fit_cases.make_system; BEARPOPULATIONS and PREDATORPREY with
the two fix-ups of exgd_grad_cases._transcription).  HIVTREATMENT, SEIR and TUMOUR, whose constructors convert their arguments, take out_p from
central differences of psi with step 1e-6 |p|; HIVTREATMENT and SEIR are then drawn at states and parameters of order one, where such a difference
resolves seven digits.  Their out_z is autograd like everybody's.

PENDULUM and MOUNTAINCAR: the oracle's dynamics are wrapped so that every point they are evaluated at -- every stage point of every step -- is
recorded, and a draw with a point within 1e-3 of a kink of the field (|u| = 2, |x1| = 8, theta = pi mod 2 pi; |u| = 1) is not taken.
"""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import fit_cases as F  # noqa: E402
from oracle import myriad_oracle as O  # noqa: E402

TRANSCRIPTIONS = ("HERMITE_SIMPSON", "TRAPEZOIDAL", "SHOOTING")
METHODS = F.METHODS
SYSTEMS = F.SYSTEMS
FD_SYSTEMS = F.FD_SYSTEMS
FD_RTOL = F.FD_RTOL
KINK = 1e-3
# (transcription, N, cpi, method) of the host matrix: the two collocation schemes at N = 3, shooting 3 x 2 under each integrator, single shooting 1 x 4 RK4
HOST_SHAPES = (("HERMITE_SIMPSON", 3, 1, "HEUN"), ("TRAPEZOIDAL", 3, 1, "HEUN"), ("SHOOTING", 3, 2, "EULER"), ("SHOOTING", 3, 2, "HEUN"),
               ("SHOOTING", 3, 2, "MIDPOINT"), ("SHOOTING", 3, 2, "RK4"), ("SHOOTING", 1, 4, "RK4"))


def horizon(name, tr, N, cpi):
  return min(float(O.SYSTEMS[name]().T), 0.05 * N * (cpi if tr == "SHOOTING" else 1))


def dims(name, tr, N, cpi, method):
  """(x rows, u rows, n, m)"""
  s = O.SYSTEMS[name]()
  if tr == "SHOOTING":
    xr, ur, m = N + 1, (2 if method == "RK4" else 1) * N * cpi + 1, N * s.ns
  else:
    xr = ur = 2 * N + 1 if tr == "HERMITE_SIMPSON" else N + 1
    m = (2 if tr == "HERMITE_SIMPSON" else 1) * N * s.ns
  return xr, ur, xr * s.ns + ur * s.nu, m


def _transcription(name, tr, N, cpi, method, T, prow, visited=None):
  sysm = F.make_system(name, prow)
  sysm.T = T
  if name == "BEARPOPULATIONS":                        # the constructor takes float(c_p), float(c_f): set them, so that autograd sees the cost's parameters
    sysm.c_p, sysm.c_f = prow[4], prow[5]
  if name == "PREDATORPREY":                           # x_T = [None, None, B] only shapes the guess and the bounds, which the cases do not take from here
    sysm.x_T = None
  with torch.no_grad():                                # (the guesses roll the system out; nothing of them is used here)
    if tr == "SHOOTING":
      t = O.make_transcription(sysm, "SHOOTING", N, cpi, integration_method=method)
    else:
      t = O.make_transcription(sysm, "COLLOCATION", N, quadrature_rule=tr)
  if visited is not None:                              # from here on every evaluation of the field is recorded
    dyn = sysm.dynamics
    def recording(x, u, *a):
      visited.append((x.detach().numpy().reshape(-1, sysm.ns), u.detach().numpy().reshape(-1, sysm.nu)))
      return dyn(x, u, *a)
    sysm.dynamics = recording
  return sysm, t


def _kink_distance(name, visited):
  if name not in ("PENDULUM", "MOUNTAINCAR"):
    return np.inf
  d = np.inf
  for xs, us in visited:
    if name == "PENDULUM":
      d = min(d, np.abs(np.abs(us) - 2.0).min(), np.abs(np.abs(xs[:, 1]) - 8.0).min(), np.abs(np.mod(xs[:, 0], 2 * np.pi) - np.pi).min())
    else:
      d = min(d, np.abs(np.abs(us) - 1.0).min())
  return float(d)


def psi(name, tr, N, cpi, method, T, z, lam, v, prow, with_cost, visited=None):
  """psi = <grad_z L, v> of one instance as a torch scalar, and its leaves (parameter tensors or floats, z)"""
  _, t = _transcription(name, tr, N, cpi, method, T, prow, visited)
  zt = torch.tensor(np.asarray(z), dtype=torch.float64, requires_grad=True)
  L = torch.tensor(np.asarray(lam)) @ t.constraints(zt)
  if with_cost:
    L = L + t.objective(zt)
  g = torch.autograd.grad(L, zt, create_graph=True)[0]
  return (g * torch.tensor(np.asarray(v))).sum(), zt


def _draw(name, tr, N, cpi, method, batch, seed, order_one):
  sysm = O.SYSTEMS[name]()
  xr, ur, n, m = dims(name, tr, N, cpi, method)
  rng = np.random.default_rng(100000 * seed + 1000 * SYSTEMS.index(name) + 100 * TRANSCRIPTIONS.index(tr) + 10 * N + cpi + 3 * METHODS.index(method) + 7 * batch)
  us = F._controls(sysm, rng, batch, ur)
  x0 = np.tile(sysm.x_0, (batch, xr, 1)).astype(np.float64)
  if order_one:
    x0 = np.ones_like(x0)
  xs = x0 * (1.0 + 0.05 * rng.standard_normal(x0.shape)) + 0.05 * rng.standard_normal(x0.shape) * (0.0 if name in F.LENHART or name == "TUMOUR" else 1.0)
  z = np.concatenate([xs.reshape(batch, -1), us.reshape(batch, -1)], axis=1)
  lam = 0.1 * rng.standard_normal((batch, m))
  v = rng.standard_normal((batch, n))
  p0 = sysm.params()
  params = p0 * (1.0 + 0.05 * (2.0 * rng.random((batch, p0.size)) - 1.0))
  if order_one:
    params = 0.5 + rng.random((batch, p0.size))
  return dict(name=name, tr=tr, N=N, cpi=cpi, method=method, T=horizon(name, tr, N, cpi), z=z, lam=lam, v=v, params=params, n=n, m=m,
              ns=sysm.ns, nu=sysm.nu)


def oracle_hvp(case, with_cost, want_p=True):
  """(out_z [B][n], out_p [B][np], kink distance) of the oracle"""
  c = case
  batch, npar = c["z"].shape[0], c["params"].shape[1]
  oz, op, kink = np.empty((batch, c["n"])), np.zeros((batch, npar)), np.inf
  fd = c["name"] in FD_SYSTEMS
  args = (c["name"], c["tr"], c["N"], c["cpi"], c["method"], c["T"])
  for b in range(batch):
    visited = []
    pt = [float(x) for x in c["params"][b]] if fd else [torch.tensor(float(x), dtype=torch.float64, requires_grad=True) for x in c["params"][b]]
    s, zt = psi(*args, c["z"][b], c["lam"][b], c["v"][b], pt, with_cost, visited)
    gs = torch.autograd.grad(s, [zt] + ([] if fd else pt), allow_unused=True)
    oz[b] = 0.0 if gs[0] is None else gs[0].numpy()
    kink = min(kink, _kink_distance(c["name"], visited))
    if not want_p:
      continue
    if fd:
      for k in range(npar):
        d = 1e-6 * abs(c["params"][b, k])
        pp, pm = c["params"][b].copy(), c["params"][b].copy()
        pp[k] += d; pm[k] -= d
        sp = psi(*args, c["z"][b], c["lam"][b], c["v"][b], [float(x) for x in pp], with_cost)[0]
        sm = psi(*args, c["z"][b], c["lam"][b], c["v"][b], [float(x) for x in pm], with_cost)[0]
        op[b, k] = (float(sp.detach()) - float(sm.detach())) / (2.0 * d)
    else:
      op[b] = [0.0 if g is None else float(g) for g in gs[1:]]
  return oz, op, kink


@functools.lru_cache(maxsize=None)
def reference(name, tr, N, cpi, method, batch=2, with_cost=1, order_one=None):
  """(case, out_z, out_p): the first draw of the seeds 0 .. 19 whose oracle run is finite and stays KINK away from the kinks; asserts there is one.
  order_one (default: HIVTREATMENT and SEIR) draws states and parameters of order one, for the central differences in p."""
  if order_one is None:
    order_one = name in ("HIVTREATMENT", "SEIR")
  last = None
  for seed in range(20):
    case = _draw(name, tr, N, cpi, method, batch, seed, order_one)
    oz, op, kink = oracle_hvp(case, with_cost)
    last = (seed, kink)
    if np.isfinite(oz).all() and np.isfinite(op).all() and kink > KINK:
      for a in list(case.values()) + [oz, op]:
        if isinstance(a, np.ndarray):
          a.setflags(write=False)
      return case, oz, op
  raise AssertionError(f"{name} {tr} {N}x{cpi} {method}: no finite draw away from the kinks (last: seed, kink = {last})")


@functools.lru_cache(maxsize=None)
def inputs(name, tr, N, cpi, method, batch):
  """a draw without a reference (shapes the oracle would take long for): seed 0, read-only"""
  case = _draw(name, tr, N, cpi, method, batch, 0, False)
  for a in case.values():
    if isinstance(a, np.ndarray):
      a.setflags(write=False)
  return case


def rel_error(a, ref):
  """largest |a - ref| / max|ref| of the row over the instances of a case"""
  den = np.abs(ref).max(axis=-1)
  return float((np.abs(a - ref).max(axis=-1) / np.where(den > 0, den, 1.0)).max())


def build_twin(tmp_dir):
  """tests/hostsim/hvp_twin.cpp -> tmp_dir/libhvp_twin.so (g++ -O2 -std=c++17), loaded with ctypes"""
  import ctypes as C
  import subprocess
  out = os.path.join(str(tmp_dir), "libhvp_twin.so")
  subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "hostsim", "hvp_twin.cpp"), "-o", out], check=True)
  lib = C.CDLL(out)
  vp = C.c_void_p
  lib.hvp_twin.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
  lib.hvp_twin.restype = C.c_int
  lib.hvp_step_two_ways.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]
  lib.hvp_step_two_ways.restype = C.c_int
  return lib


def twin_hvp(lib, name, tr, N, cpi, method, T, z, lam, v, params, with_cost=1):
  """the device algebra on the host over the batch: (out_z [B][n], out_p [B][np]); lam may be None; params [np] or [B][np]"""
  from myriad_amd._lib import INT_IDS, SYS_IDS, TR_IDS
  z, v, params = (np.ascontiguousarray(a, dtype=np.float64) for a in (z, v, params))
  lam = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64)
  batch, npar = z.shape[0], params.shape[-1]
  oz, op = np.empty(z.shape), np.empty((batch, npar))
  rc = lib.hvp_twin(SYS_IDS[name], TR_IDS[tr], INT_IDS[method], batch, int(N), int(cpi), float(T), z.ctypes.data,
                    None if lam is None else lam.ctypes.data, v.ctypes.data, params.ctypes.data, 0 if params.ndim == 1 else npar, int(with_cost),
                    oz.ctypes.data, op.ctypes.data)
  assert rc == 0, f"hvp_twin: no specialisation for {name} {tr}"
  return oz, op


def twin_of_case(lib, case, with_cost=1, v=None, lam="case"):
  c = case
  return twin_hvp(lib, c["name"], c["tr"], c["N"], c["cpi"], c["method"], c["T"], c["z"], c["lam"] if isinstance(lam, str) else lam,
                  c["v"] if v is None else v, c["params"], with_cost)
