"""Inputs and oracle references shared by the tests of the Lagrangian Hessian-vector product of the network system (test_node_hvp_host_twin.py,
test_gpu_node_hvp.py), in the manner of node_shoot_exgd_grad_cases.py.

A case is (transcription, I, cpi, method, batch); the weights are the committed (64, 64) set, shared by the batch.  A draw: T = 0.05 I cpi (cpi = 1
under collocation), states 0.5 N(0, 1), controls U(-5, 5), lam = 0.1 N(0, 1), v = N(0, 1).  With L = with_cost f + lam^T c and
psi = <grad_z L, v> the reference is torch.autograd.grad(psi, [z, weight leaves]) with create_graph=True through
`O.make_transcription(O.NodeCartPole(leaves), ...)`, as hvp_cases.psi does for the closed-form systems.  A case is accepted on the reference alone:
finite, max|out_z| > 0 and max|out_p| > 0 for both values of with_cost, and the two references differ in out_z by more than 1e-6 relative (the
flag is then tested); the first of the seeds 0 ... 19 that meets this, and a case without one fails.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import torch

import node_shoot_exgd_grad_cases as S
from hvp_cases import ROOT, O, rel_error  # noqa: F401

NS, NU, NP = 4, 1, 4804
KEYS = S.KEYS
METHODS = S.METHODS
TR_CODE = {"HERMITE_SIMPSON": 0, "SHOOTING": 2}
FLAG_DIFFERENCE = 1e-6
# (transcription, I, cpi, method, batch).  Hermite-Simpson: fewer points than wavefronts | a ragged second round | a batch.  SHOOTING: the smallest | -- |
# two control rows a step | single shooting | more intervals than lanes and wavefront rounds | a batch
HS_CASES = (("HERMITE_SIMPSON", 1, 1, "HEUN", 1), ("HERMITE_SIMPSON", 3, 1, "HEUN", 2), ("HERMITE_SIMPSON", 3, 1, "HEUN", 37))
SHOOT_CASES = (("SHOOTING", 1, 1, "EULER", 1), ("SHOOTING", 3, 2, "HEUN", 2), ("SHOOTING", 2, 2, "RK4", 2), ("SHOOTING", 1, 12, "MIDPOINT", 1),
               ("SHOOTING", 70, 1, "HEUN", 1), ("SHOOTING", 4, 3, "HEUN", 37))
CASES = HS_CASES + SHOOT_CASES
IDS = ["-".join(map(str, c)) for c in CASES]
checked = S.checked                                          # the instances compared with the oracle: all, or 0, 21 and 36 of the batch of 37
weights = S.weights


def dims(tr, I, cpi, method):
  """(n, m, number of state entries)"""
  if tr == "SHOOTING":
    n, m = S.dims(I, cpi, method)
    return n, m, (I + 1) * NS
  K = 2 * I + 1
  return K * (NS + NU), 2 * I * NS, K * NS


def _transcription(tr, I, cpi, method, T, tp):
  sysm = O.NodeCartPole(tp)
  sysm.T = T
  with torch.no_grad():
    if tr == "SHOOTING":
      return O.make_transcription(sysm, "SHOOTING", I, cpi, integration_method=method)
    return O.make_transcription(sysm, "COLLOCATION", I, quadrature_rule="HERMITE_SIMPSON")


def oracle_hvp(tr, I, cpi, method, T, z, lam, v, with_cost):
  """(out_z [n], out_p [4804] in the device order) of one instance"""
  tp = S._leaves(True)
  t = _transcription(tr, I, cpi, method, T, tp)
  zt = torch.tensor(np.asarray(z), dtype=torch.float64, requires_grad=True)
  L = torch.tensor(np.asarray(lam)) @ t.constraints(zt)
  if with_cost:
    L = L + t.objective(zt)
  g = torch.autograd.grad(L, zt, create_graph=True)[0]
  psi = (g * torch.tensor(np.asarray(v))).sum()
  leaves = [tp[k][f] for k in KEYS for f in ("w", "b")]
  gs = torch.autograd.grad(psi, [zt] + leaves, allow_unused=True)
  gs = [torch.zeros_like(x) if gi is None else gi for gi, x in zip(gs, [zt] + leaves)]
  return gs[0].numpy(), np.concatenate([gi.numpy().ravel() for gi in gs[1:]])


def _draw(tr, I, cpi, method, batch, seed):
  n, m, nx = dims(tr, I, cpi, method)
  rng = np.random.default_rng(100000 * seed + 23000 + 1000 * TR_CODE[tr] + 100 * I + 10 * cpi + METHODS[method] + 7 * batch)
  z = np.concatenate([0.5 * rng.standard_normal((batch, nx)), rng.uniform(-5.0, 5.0, (batch, n - nx))], axis=1)
  return dict(tr=tr, I=I, cpi=cpi, method=method, T=0.05 * I * cpi, z=z, lam=0.1 * rng.standard_normal((batch, m)), v=rng.standard_normal((batch, n)),
              params=weights()[1], n=n, m=m)


@functools.lru_cache(maxsize=None)
def reference(tr, I, cpi, method, batch):
  """(case, {1: (out_z, out_p), 0: (out_z, out_p)}): the rows of checked(batch) hold the oracle, the others NaN.  case["rows"]: those rows."""
  rows = list(checked(batch))
  last = None
  for seed in range(20):
    c = _draw(tr, I, cpi, method, batch, seed)
    ref = {}
    for wc in (1, 0):
      oz, op = np.full((batch, c["n"]), np.nan), np.full((batch, NP), np.nan)
      for b in rows:
        oz[b], op[b] = oracle_hvp(tr, I, cpi, method, c["T"], c["z"][b], c["lam"][b], c["v"][b], wc)
      ref[wc] = (oz, op)
    finite = all(np.isfinite(a[rows]).all() for wc in ref for a in ref[wc])
    nonzero = all(np.abs(a[b]).max() > 0 for wc in ref for a in ref[wc] for b in rows)
    flag = min(np.abs(ref[1][0][b] - ref[0][0][b]).max() / np.abs(ref[1][0][b]).max() for b in rows) if finite and nonzero else 0.0
    last = (seed, finite, nonzero, flag)
    if finite and nonzero and flag > FLAG_DIFFERENCE:
      for a in list(c.values()) + [x for wc in ref for x in ref[wc]]:
        if isinstance(a, np.ndarray):
          a.setflags(write=False)
      c.update(seed=seed, rows=rows, flag=flag)
      return c, ref
  raise AssertionError(f"NODE {tr} {I}x{cpi} {method}: no accepted draw (last: seed, finite, nonzero, with_cost difference = {last})")


@functools.lru_cache(maxsize=None)
def inputs(tr, I, cpi, method, batch):
  """a draw without a reference (seed 0, read-only): the long horizon and the central differences"""
  c = _draw(tr, I, cpi, method, batch, 0)
  for a in c.values():
    if isinstance(a, np.ndarray):
      a.setflags(write=False)
  return c


# ---- the host twin ------------------------------------------------------------------------------------------------------------------------------
def build_twin(tmp_dir):
  """tests/hostsim/node_hvp_twin.cpp -> tmp_dir/libnode_hvp_twin.so (g++ -O2 -std=c++17), loaded with ctypes"""
  out = os.path.join(str(tmp_dir), "libnode_hvp_twin.so")
  subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "hostsim", "node_hvp_twin.cpp"), "-o", out], check=True)
  lib = C.CDLL(out)
  vp, i, d = C.c_void_p, C.c_int, C.c_double
  lib.node_hvp_twin.argtypes = [i, i, i, i, i, d, vp, vp, vp, vp, i, vp, vp]
  lib.node_hvp_twin.restype = C.c_int
  lib.node_hvp_point_two_ways.argtypes = [vp, vp, vp, d, vp, vp, vp]
  lib.node_hvp_point_two_ways.restype = None
  return lib


def twin_hvp(lib, tr, I, cpi, method, T, z, lam, v, params, with_cost=1, want_p=True):
  """node_hvp_host over the batch: (out_z [B][n], out_p [B][4804] or None); lam may be None"""
  z, v, params = (np.ascontiguousarray(a, dtype=np.float64) for a in (z, v, params))
  lam = None if lam is None else np.ascontiguousarray(lam, dtype=np.float64)
  oz, op = np.empty(z.shape), (np.empty((z.shape[0], NP)) if want_p else None)
  rc = lib.node_hvp_twin(TR_CODE[tr], METHODS[method], z.shape[0], int(I), int(cpi), float(T), z.ctypes.data, None if lam is None else lam.ctypes.data,
                         v.ctypes.data, params.ctypes.data, int(with_cost), oz.ctypes.data, None if op is None else op.ctypes.data)
  assert rc == 0
  return oz, op


def twin_of_case(lib, c, with_cost=1, **kw):
  c = dict(c); c.update(kw)
  return twin_hvp(lib, c["tr"], c["I"], c["cpi"], c["method"], c["T"], c["z"], c["lam"], c["v"], c["params"], with_cost)
