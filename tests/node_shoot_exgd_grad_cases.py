"""Inputs and oracle references shared by the tests of the unrolled-extragradient derivative in the network weights under SHOOTING
(test_node_shoot_exgd_grad_host_twin.py, test_gpu_node_shoot_exgd_grad.py), in the manner of node_exgd_grad_cases.py.

A case is (I, cpi, method, nsteps, batch); the weights are the committed (64, 64) set, shared by the batch.  A draw: T = 0.05 I cpi, states
0.5 N(0, 1), controls U(-5, 5), lam = 0.1 N(0, 1), eta_x = 0.2 / |grad^2_zz L| (ten rounds of the power iteration on exact Hessian-vector
products -- a double backward -- of the first instance), eta_v = 0.5; the first node is pinned, 30 % of the other variables of every instance
get a box of 0.3 |eta_x g_i| around z_i, about half of the rest finite bounds far away.  The reference is torch autograd through
`O.make_transcription(O.NodeCartPole(leaves), "SHOOTING", I, cpi, integration_method=method)` (the weights as tensors that require a gradient)
and the step restated with `torch.clamp`.  The acceptance conditions are exgd_grad_cases' and look at the reference alone: no unclipped value
within TIE of a bound, no clipped one equal to its bound, at least MIN_CLIPPED of the free variables of every instance clipped in some
half-step; the first of the seeds 0 ... 19 that meets them, and a case without one fails.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import torch

import exgd_grad_cases as E
from exgd_grad_cases import MIN_CLIPPED, ROOT, TIE, O, rel_error  # noqa: F401

NS, NU, NP = 4, 1, 4804
KEYS = ("linear", "linear_1", "linear_2")
METHODS = {"EULER": 0, "HEUN": 1, "MIDPOINT": 2, "RK4": 3}
# (I, cpi, method, nsteps, batch): the smallest | -- | no steps | single shooting | more intervals than lanes or wavefront rounds | a batch
CASES = ((1, 1, "EULER", 1, 1), (3, 2, "HEUN", 3, 2), (2, 2, "RK4", 0, 2), (1, 12, "MIDPOINT", 2, 1), (70, 1, "HEUN", 2, 1), (4, 3, "HEUN", 2, 37))
CHUNKED = (5, 2, "RK4", 2, 3)                                # under a history bound small enough for chunks of one instance
CHUNKED_HIST_BYTES = 4096                                    # one instance's history is 2 (2 n + m) + n = 2 (90 + 20) + 45 = 265 doubles: chunks of one


def checked(batch):
  """the instances of a batch that are compared with the oracle: all, or 0, 21 and 36 of the batch of 37"""
  return (0, 21, 36) if batch == 37 else tuple(range(batch))


def dims(I, cpi, method):
  M = 2 if method == "RK4" else 1
  return (I + 1) * NS + (M * I * cpi + 1) * NU, I * NS


@functools.lru_cache(maxsize=None)
def weights():
  """(Haiku mapping, flat device vector) of the committed weight set"""
  from myriad_amd.systems.neural_ode import NeuralODE, flat_from_mapping
  node = NeuralODE.load_fitted_cartpole()
  flat = flat_from_mapping(node.params)
  flat.setflags(write=False)
  return node.params, flat


def _leaves(grad):
  params, _ = weights()
  return {k: {f: torch.tensor(np.asarray(params[k][f], dtype=np.float64), requires_grad=grad) for f in ("w", "b")} for k in KEYS}


def _transcription(I, cpi, method, T, tp):
  sysm = O.NodeCartPole(tp)
  sysm.T = T
  with torch.no_grad():
    return O.make_transcription(sysm, "SHOOTING", I, cpi, integration_method=method)


def oracle_run(I, cpi, method, T, z, lam, lb, ub, eta_x, eta_v, nsteps, grad_params=True):
  """One instance through `nsteps` steps in torch: (z_n, lam_n, (weight leaves in the device order, z0, lam0), values in front of every clamp)"""
  tp = _leaves(grad_params)
  tr = _transcription(I, cpi, method, T, tp)
  z0, lam0 = E.start_leaves(z, lam)
  x, lm, pre, _ = E.unrolled_steps(tr, z0, lam0, lb, ub, eta_x, eta_v, nsteps)
  return x, lm, ([tp[k][f] for k in KEYS for f in ("w", "b")], z0, lam0), pre


def _draw(I, cpi, method, nsteps, batch, seed):
  n, m = dims(I, cpi, method)
  T = 0.05 * I * cpi
  rng = np.random.default_rng(100000 * seed + 9000 + 100 * I + 10 * cpi + METHODS[method] + 3 * nsteps + 7 * batch)
  xs = 0.5 * rng.standard_normal((batch, I + 1, NS))
  us = rng.uniform(-5.0, 5.0, (batch, n - (I + 1) * NS))
  z = np.concatenate([xs.reshape(batch, -1), us], axis=1)
  lam = 0.1 * rng.standard_normal((batch, m))
  seed_z = rng.standard_normal((batch, n))
  seed_lam = rng.standard_normal((batch, m))
  tr = _transcription(I, cpi, method, T, _leaves(False))
  L = lambda xx, ll: tr.objective(xx) + ll @ tr.constraints(xx)

  def grad_x(zz, ll, create_graph=False):
    xi = torch.tensor(zz, dtype=torch.float64, requires_grad=True)
    return xi, torch.autograd.grad(L(xi, torch.as_tensor(ll)), xi, create_graph=create_graph)[0]

  g0 = np.stack([grad_x(z[b], lam[b])[1].numpy() for b in range(batch)])
  v, lip = rng.standard_normal(n), 0.0
  for _ in range(10):                                               # |grad^2_zz L| of the first instance: exact products by a double backward
    xi, g = grad_x(z[0], lam[0], create_graph=True)
    hv = torch.autograd.grad(g @ torch.tensor(v / np.linalg.norm(v)), xi)[0].numpy()
    lip, v = np.linalg.norm(hv), hv
  eta_x, eta_v = 0.2 / max(lip, 1e-12), 0.5
  delta = eta_x * np.abs(g0)
  lb, ub = E.draw_boxes(rng, z, delta, NS)
  return dict(I=I, cpi=cpi, method=method, T=T, nsteps=nsteps, z=z, lam=lam, lb=lb, ub=ub, params=weights()[1], eta_x=float(eta_x),
              eta_v=float(eta_v), seed_z=seed_z, seed_lam=seed_lam, n=n, m=m, ns=NS, nu=NU)


def _oracle(c):
  """(grad, dz0, dlam0 -- the rows of checked(batch), the others NaN --, tie distance, clipped fraction); the conditions look at every instance"""
  batch = c["z"].shape[0]
  grad, dz0, dlam0 = np.full((batch, NP), np.nan), np.full((batch, c["n"]), np.nan), np.full((batch, c["m"]), np.nan)
  tie, clipped = np.inf, np.zeros((batch, c["n"]), dtype=bool)
  rows = checked(batch)
  for b in range(batch):
    xn, ln, (pt, z0, lam0), pre = oracle_run(c["I"], c["cpi"], c["method"], c["T"], c["z"][b], c["lam"][b], c["lb"][b], c["ub"][b], c["eta_x"],
                                             c["eta_v"], c["nsteps"], grad_params=b in rows)
    if b in rows:
      out = (torch.tensor(c["seed_z"][b]) * xn).sum() + (torch.tensor(c["seed_lam"][b]) * ln).sum()
      gs = torch.autograd.grad(out, pt + [z0, lam0], allow_unused=True)
      gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, pt + [z0, lam0])]
      grad[b] = np.concatenate([g.numpy().ravel() for g in gs[:-2]])
      dz0[b], dlam0[b] = gs[-2].numpy(), gs[-1].numpy()
    t, outside = E.clamp_conditions(pre, c["lb"][b], c["ub"][b])
    tie, clipped[b] = min(tie, t), outside
  return grad, dz0, dlam0, tie, E.clipped_fraction(clipped, c["lb"], c["ub"])


@functools.lru_cache(maxsize=None)
def reference(I, cpi, method, nsteps, batch):
  """(case, grad, dz0, dlam0): the first draw whose oracle run is finite and meets the tie and clip conditions; asserts that there is one.
  case["rows"]: the instances the reference holds (the others are NaN)."""
  last = None
  for seed in range(20):
    case = _draw(I, cpi, method, nsteps, batch, seed)
    grad, dz0, dlam0, tie, frac = _oracle(case)
    rows = list(checked(batch))
    last = (seed, tie, frac)
    finite = np.isfinite(grad[rows]).all() and np.isfinite(dz0[rows]).all() and np.isfinite(dlam0[rows]).all()
    if finite and (nsteps == 0 or (tie > TIE and frac >= MIN_CLIPPED)):
      for a in list(case.values()) + [grad, dz0, dlam0]:
        if isinstance(a, np.ndarray):
          a.setflags(write=False)
      case.update(seed=seed, tie=tie, clipped=frac, rows=rows)
      return case, grad, dz0, dlam0
  raise AssertionError(f"NODE {I}x{cpi} {method} nsteps={nsteps}: no draw meets the tie and clip conditions (last: seed, tie, clipped = {last})")


def shape_case(I, cpi, method, nsteps, B):
  """inputs without an oracle run (shoot_exgd_grad_cases.shape_case for the network): a third of the variables in a box of 1e-3 that the steps
  leave, the first node pinned"""
  n, m = dims(I, cpi, method)
  rng = np.random.default_rng(11 + 1000 * I + 100 * cpi + 10 * nsteps + B + METHODS[method])
  z = np.concatenate([0.5 * rng.standard_normal((B, (I + 1) * NS)), rng.uniform(-5.0, 5.0, (B, n - (I + 1) * NS))], axis=1)
  box = rng.random((B, n)) < 1.0 / 3.0
  lb, ub = np.where(box, z - 1e-3, -np.inf), np.where(box, z + 1e-3, np.inf)
  lb[:, :NS] = z[:, :NS]; ub[:, :NS] = z[:, :NS]
  return dict(I=I, cpi=cpi, method=method, T=0.05 * I * cpi, nsteps=nsteps, z=z, lam=0.1 * rng.standard_normal((B, m)), lb=lb, ub=ub,
              params=weights()[1], eta_x=0.05, eta_v=0.5, seed_z=rng.standard_normal((B, n)), seed_lam=rng.standard_normal((B, m)), n=n, m=m)


# ---- the host twin ------------------------------------------------------------------------------------------------------------------------------
def build_twin(tmp_dir):
  """tests/hostsim/node_shoot_exgd_grad_twin.cpp -> tmp_dir/libnode_shoot_exgd_grad_twin.so (g++ -O2 -std=c++17), loaded with ctypes"""
  out = os.path.join(str(tmp_dir), "libnode_shoot_exgd_grad_twin.so")
  subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "hostsim", "node_shoot_exgd_grad_twin.cpp"), "-o", out],
                 check=True)
  lib = C.CDLL(out)
  vp, i, d = C.c_void_p, C.c_int, C.c_double
  lib.node_shoot_exgd_grad_twin.argtypes = [i, i, i, i, d, vp, vp, vp, vp, vp, d, d, i, vp, vp, i, vp, vp, vp]
  lib.node_shoot_exgd_grad_twin.restype = C.c_int
  return lib


def twin_grad(lib, I, cpi, method, T, z, lam, lb, ub, params, eta_x, eta_v, nsteps, seed_z, seed_lam=None, fused=True):
  """node_shoot_exgd_grad_host over the batch: (grad [B][4804], dz0 [B][n], dlam0 [B][m]); fused=False: items 1 .. 5 as three passes a step"""
  z, lam, lb, ub, params, seed_z = (np.ascontiguousarray(a, dtype=np.float64) for a in (z, lam, lb, ub, params, seed_z))
  seed_lam = None if seed_lam is None else np.ascontiguousarray(seed_lam, dtype=np.float64)
  grad, dz0, dlam0 = np.empty((z.shape[0], NP)), np.empty(z.shape), np.empty(lam.shape)
  rc = lib.node_shoot_exgd_grad_twin(METHODS[method], z.shape[0], int(I), int(cpi), float(T), z.ctypes.data, lam.ctypes.data, lb.ctypes.data,
                                     ub.ctypes.data, params.ctypes.data, float(eta_x), float(eta_v), int(nsteps), seed_z.ctypes.data,
                                     None if seed_lam is None else seed_lam.ctypes.data, 1 if fused else 0, grad.ctypes.data, dz0.ctypes.data,
                                     dlam0.ctypes.data)
  assert rc == NP
  return grad, dz0, dlam0


def twin_of_case(lib, c, fused=True, **kw):
  c = dict(c); c.update(kw)
  return twin_grad(lib, c["I"], c["cpi"], c["method"], c["T"], c["z"], c["lam"], c["lb"], c["ub"], c["params"], c["eta_x"], c["eta_v"], c["nsteps"],
                   c["seed_z"], c["seed_lam"], fused)
