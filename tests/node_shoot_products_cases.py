"""Inputs, oracle references and the host twin shared by the tests of the Lagrangian products and extragradient steps of the network system under
SHOOTING (test_node_shoot_products_host_twin.py, test_gpu_node_shoot_products.py).

A shape is (B, I, cpi, method); the weights are the committed (64, 64) set (NeuralODE.load_fitted_cartpole), shared by the batch.  Points:
z = tr.guess + 0.2 N(0, 1), lam and v standard normal, all from default_rng(1).  References: the oracle's autodiff through
O.shooting(O.NodeCartPole(params), I, cpi, method) -- O.Lagrangian.grad_x / jvp, and the extragradient loop written with explicit lb / ub from
grad_x / grad_lmbda.  Every reference is computed once (lru_cache) and handed out read-only.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from oracle import myriad_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, NU, NP = 4, 1, 4804
METHODS = {"EULER": 0, "HEUN": 1, "MIDPOINT": 2, "RK4": 3}
# (B, I, cpi, method): 12 pairs, one partial tile | exactly one tile, two control rows per step | a tile boundary inside one instance, one step per
# interval | single shooting, no row shared by two intervals | 111 pairs: more than one wavefront's worth, last group partial | an instance wider
# than 64 pairs
SHAPES = ((3, 4, 3, "HEUN"), (4, 4, 2, "RK4"), (1, 17, 1, "EULER"), (5, 1, 10, "MIDPOINT"), (37, 3, 2, "HEUN"), (2, 70, 1, "HEUN"))
ETA_X, ETA_V, NSTEPS = 1e-2, 1e-3, 10


def checked(B):
  """the instances of a batch that are checked against the oracle: all, or 0, 21 and 36 of the batch of 37"""
  return (0, 21, 36) if B == 37 else tuple(range(B))


@functools.lru_cache(maxsize=None)
def weights():
  """(Haiku mapping, flat device vector) of the committed weight set"""
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping
  node = NeuralODE.load_fitted_cartpole()
  flat = np.ascontiguousarray(flat_from_mapping(node.params), dtype=np.float64)
  flat.setflags(write=False)
  return node.params, flat


@functools.lru_cache(maxsize=None)
def transcription(I, cpi, method):
  return O.shooting(O.NodeCartPole(weights()[0]), I, cpi, method)


def _ro(*arrays):
  for a in arrays:
    a.setflags(write=False)
  return arrays


@functools.lru_cache(maxsize=None)
def case(B, I, cpi, method):
  """dict(tr, T, n, m, z [B,n], lam [B,m], v [B,n], lb, ub [n])"""
  tr = transcription(I, cpi, method)
  n, m = tr.guess.size, I * NS
  rng = np.random.default_rng(1)
  z = tr.guess[None] + 0.2 * rng.standard_normal((B, n))
  lam = rng.standard_normal((B, m))
  v = rng.standard_normal((B, n))
  lb, ub = tr.bounds[:, 0].copy(), tr.bounds[:, 1].copy()
  _ro(z, lam, v, lb, ub)
  return dict(tr=tr, T=float(O.NodeCartPole(weights()[0]).T), n=n, m=m, B=B, I=I, cpi=cpi, method=method, z=z, lam=lam, v=v, lb=lb, ub=ub)


@functools.lru_cache(maxsize=None)
def ref_products(B, I, cpi, method):
  """{b: (grad L, J^T lam, J v)} of the checked instances by the oracle's autodiff"""
  c = case(B, I, cpi, method)
  L, cb = O.Lagrangian(c["tr"]), O.Callbacks(c["tr"])
  out = {}
  for b in checked(B):
    gl = L.grad_x(c["z"][b], c["lam"][b])
    out[b] = _ro(gl, gl - cb.grad(c["z"][b]), L.jvp(c["z"][b], c["v"][b]))
  return out


def clip_bounds(c, tight=False):
  """the call's lb, ub [n]; tight: the control bounds at +-0.1"""
  lb, ub = c["lb"].copy(), c["ub"].copy()
  if tight:
    lb[(c["I"] + 1) * NS:] = -0.1; ub[(c["I"] + 1) * NS:] = 0.1
  return lb, ub


@functools.lru_cache(maxsize=None)
def ref_exgd(B, I, cpi, method, tight=False, nsteps=NSTEPS):
  """{b: (z, lam)} of the checked instances after `nsteps` extragradient steps from (z_b, 1) by the oracle (extra_gradient.py:25-33 with explicit bounds)"""
  c = case(B, I, cpi, method)
  L = O.Lagrangian(c["tr"])
  lb, ub = clip_bounds(c, tight)
  out = {}
  for b in checked(B):
    x, lm = c["z"][b].copy(), np.ones(c["m"])
    for _ in range(nsteps):
      xb = np.clip(x - ETA_X * L.grad_x(x, lm), lb, ub)
      x = np.clip(x - ETA_X * L.grad_x(xb, lm), lb, ub)
      lm = lm + ETA_V * L.grad_lmbda(x, lm)
    assert np.isfinite(x).all() and np.isfinite(lm).all()
    out[b] = _ro(x, lm)
  return out


def rel(a, ref):
  """largest |a - ref| over max(1, largest |ref|)"""
  return float(np.abs(np.asarray(a) - np.asarray(ref)).max() / max(1.0, np.abs(ref).max()))


# ---- the host twin ------------------------------------------------------------------------------------------------------------------------------
def build_twin(tmp_dir):
  """tests/hostsim/node_shoot_products_twin.cpp -> tmp_dir/libnode_shoot_products_twin.so (g++ -O2 -std=c++17), loaded with ctypes"""
  out = os.path.join(str(tmp_dir), "libnode_shoot_products_twin.so")
  subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "hostsim", "node_shoot_products_twin.cpp"), "-o", out], check=True)
  lib = C.CDLL(out)
  vp, i, d = C.c_void_p, C.c_int, C.c_double
  lib.node_shoot_vjp_twin.argtypes = [i, i, i, i, d, vp, vp, vp, i, i, vp]
  lib.node_shoot_jvp_twin.argtypes = [i, i, i, i, d, vp, vp, vp, i, vp]
  lib.node_shoot_exgd_twin.argtypes = [i, i, i, i, d, vp, vp, vp, vp, vp, i, d, d, i]
  for f in (lib.node_shoot_vjp_twin, lib.node_shoot_jvp_twin, lib.node_shoot_exgd_twin):
    f.restype = C.c_int
  return lib


def _c(a):
  return np.ascontiguousarray(a, dtype=np.float64)


def twin_vjp(lib, c, add_gradf, rows=None):
  rows = list(range(c["B"])) if rows is None else list(rows)
  z, lam, p = _c(c["z"][rows]), _c(c["lam"][rows]), weights()[1]
  out = np.empty_like(z)
  assert lib.node_shoot_vjp_twin(METHODS[c["method"]], len(rows), c["I"], c["cpi"], c["T"], z.ctypes.data, lam.ctypes.data, p.ctypes.data, 0, int(add_gradf),
                                 out.ctypes.data) == 0
  return out


def twin_jvp(lib, c, rows=None):
  rows = list(range(c["B"])) if rows is None else list(rows)
  z, v, p = _c(c["z"][rows]), _c(c["v"][rows]), weights()[1]
  out = np.empty((len(rows), c["m"]))
  assert lib.node_shoot_jvp_twin(METHODS[c["method"]], len(rows), c["I"], c["cpi"], c["T"], z.ctypes.data, v.ctypes.data, p.ctypes.data, 0, out.ctypes.data) == 0
  return out


def twin_exgd(lib, c, tight=False, nsteps=NSTEPS, rows=None):
  rows = list(range(c["B"])) if rows is None else list(rows)
  z, lam, p = _c(c["z"][rows]).copy(), np.ones((len(rows), c["m"])), weights()[1]
  lb, ub = (np.ascontiguousarray(np.broadcast_to(a, z.shape)) for a in clip_bounds(c, tight))
  assert lib.node_shoot_exgd_twin(METHODS[c["method"]], len(rows), c["I"], c["cpi"], c["T"], z.ctypes.data, lam.ctypes.data, lb.ctypes.data, ub.ctypes.data,
                                  p.ctypes.data, 0, ETA_X, ETA_V, int(nsteps)) == 0
  return z, lam
