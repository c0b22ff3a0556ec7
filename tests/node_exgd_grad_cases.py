"""Inputs and oracle references shared by the tests of the unrolled-extragradient derivative in the network weights
(test_node_exgd_grad_host_twin.py, test_gpu_node_exgd_grad.py), in the manner of exgd_grad_cases.py.

A case is (N, nsteps, batch), Hermite-Simpson throughout; the weights are the committed (64, 64) set, shared by the batch.  A draw: states
0.5 N(0, 1), controls U(-5, 5), lam = 0.1 N(0, 1), T = 0.1 N, eta_x = 0.2 / |grad^2_zz L| (ten rounds of the power iteration on exact
Hessian-vector products of the first instance), eta_v = 0.5; the state of the first point is pinned, 30 % of the other variables of every
instance get a box of 0.3 |eta_x g_i| around z_i, about half of the rest finite bounds far away.  The reference is torch autograd through
`oracle.NodeCartPole` (the weights as tensors that require a gradient) and exgd_grad_cases.oracle_run's restatement of the step.  The acceptance
conditions are that module's: no unclipped value within TIE of a bound, none equal to its bound, at least MIN_CLIPPED of the free variables of
every instance clipped in some half-step, the first of the seeds 0 ... 19 that meets them.
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
CASES = ((1, 1, 1), (3, 3, 2), (2, 0, 2), (33, 2, 1))      # (N, nsteps, batch)
CHUNKED = (7, 2, 3)                                          # with a 4 KB history bound: the chunked path
CHUNKED_HIST_BYTES = 4096


def dims(N):
  K = 2 * N + 1
  return K, K * (NS + NU), 2 * N * NS


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


def _transcription(N, T, tp):
  sysm = O.NodeCartPole(tp)
  sysm.T = T
  with torch.no_grad():
    return O.make_transcription(sysm, "COLLOCATION", N, quadrature_rule="HERMITE_SIMPSON")


def oracle_run(N, T, z, lam, lb, ub, eta_x, eta_v, nsteps, grad_params=True):
  """exgd_grad_cases.oracle_run for the network system: (z_n, lam_n, (weight leaves in the device order, z0, lam0), values in front of every clamp)"""
  tp = _leaves(grad_params)
  tr = _transcription(N, T, tp)
  z0, lam0 = E.start_leaves(z, lam)
  x, lm, pre, _ = E.unrolled_steps(tr, z0, lam0, lb, ub, eta_x, eta_v, nsteps)
  return x, lm, ([tp[k][f] for k in KEYS for f in ("w", "b")], z0, lam0), pre


def _draw(N, nsteps, batch, seed):
  K, n, m = dims(N)
  T = 0.1 * N
  rng = np.random.default_rng(100000 * seed + 4000 + 10 * N + nsteps + 7 * batch)
  xs = 0.5 * rng.standard_normal((batch, K, NS))
  us = rng.uniform(-5.0, 5.0, (batch, K, NU))
  z = np.concatenate([xs.reshape(batch, -1), us.reshape(batch, -1)], axis=1)
  lam = 0.1 * rng.standard_normal((batch, m))
  seed_z = rng.standard_normal((batch, n))
  seed_lam = rng.standard_normal((batch, m))
  tr = _transcription(N, T, _leaves(False))
  L = lambda xx, ll: tr.objective(xx) + ll @ tr.constraints(xx)

  def grad_x(zz, ll, create_graph=False):
    xi = torch.tensor(zz, dtype=torch.float64, requires_grad=True) if not torch.is_tensor(zz) else zz
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
  return dict(N=N, T=T, nsteps=nsteps, z=z, lam=lam, lb=lb, ub=ub, params=weights()[1], eta_x=float(eta_x), eta_v=float(eta_v), seed_z=seed_z,
              seed_lam=seed_lam, K=K, n=n, m=m, ns=NS, nu=NU)


def _oracle(c):
  batch = c["z"].shape[0]
  grad, dz0, dlam0 = np.empty((batch, NP)), np.empty((batch, c["n"])), np.empty((batch, c["m"]))
  tie, clipped = np.inf, np.zeros((batch, c["n"]), dtype=bool)
  for b in range(batch):
    xn, ln, (pt, z0, lam0), pre = oracle_run(c["N"], c["T"], c["z"][b], c["lam"][b], c["lb"][b], c["ub"][b], c["eta_x"], c["eta_v"], c["nsteps"])
    out = (torch.tensor(c["seed_z"][b]) * xn).sum() + (torch.tensor(c["seed_lam"][b]) * ln).sum()
    gs = torch.autograd.grad(out, pt + [z0, lam0], allow_unused=True)
    gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, pt + [z0, lam0])]
    grad[b] = np.concatenate([g.numpy().ravel() for g in gs[:-2]])
    dz0[b], dlam0[b] = gs[-2].numpy(), gs[-1].numpy()
    t, outside = E.clamp_conditions(pre, c["lb"][b], c["ub"][b])
    tie, clipped[b] = min(tie, t), outside
  return grad, dz0, dlam0, tie, E.clipped_fraction(clipped, c["lb"], c["ub"])


@functools.lru_cache(maxsize=None)
def reference(N, nsteps, batch):
  """(case, grad, dz0, dlam0): the first draw whose oracle run is finite and meets the tie and clip conditions; asserts that there is one"""
  last = None
  for seed in range(20):
    case = _draw(N, nsteps, batch, seed)
    grad, dz0, dlam0, tie, frac = _oracle(case)
    last = (seed, tie, frac)
    finite = np.isfinite(grad).all() and np.isfinite(dz0).all() and np.isfinite(dlam0).all()
    if finite and (nsteps == 0 or (tie > TIE and frac >= MIN_CLIPPED)):
      for a in list(case.values()) + [grad, dz0, dlam0]:
        if isinstance(a, np.ndarray):
          a.setflags(write=False)
      case["clipped"] = frac
      return case, grad, dz0, dlam0
  raise AssertionError(f"NODE N={N} nsteps={nsteps}: no draw meets the tie and clip conditions (last: seed, tie, clipped = {last})")


def build_twin(tmp_dir):
  """tests/hostsim/node_exgd_grad_twin.cpp -> tmp_dir/libnode_exgd_grad_twin.so (g++ -O2 -std=c++17), loaded with ctypes"""
  out = os.path.join(str(tmp_dir), "libnode_exgd_grad_twin.so")
  subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "hostsim", "node_exgd_grad_twin.cpp"), "-o", out], check=True)
  lib = C.CDLL(out)
  vp = C.c_void_p
  lib.node_exgd_grad_twin.argtypes = [C.c_int, C.c_int, C.c_double, vp, vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, vp, vp, vp, vp]
  lib.node_exgd_grad_twin.restype = C.c_int
  return lib


def twin_grad(lib, N, T, z, lam, lb, ub, params, eta_x, eta_v, nsteps, seed_z, seed_lam=None):
  """node_exgd_grad_host over the batch: (grad [B][4804], dz0 [B][n], dlam0 [B][m])"""
  z, lam, lb, ub, params, seed_z = (np.ascontiguousarray(a, dtype=np.float64) for a in (z, lam, lb, ub, params, seed_z))
  seed_lam = None if seed_lam is None else np.ascontiguousarray(seed_lam, dtype=np.float64)
  grad, dz0, dlam0 = np.empty((z.shape[0], NP)), np.empty(z.shape), np.empty(lam.shape)
  rc = lib.node_exgd_grad_twin(z.shape[0], N, float(T), z.ctypes.data, lam.ctypes.data, lb.ctypes.data, ub.ctypes.data, params.ctypes.data,
                               float(eta_x), float(eta_v), int(nsteps), seed_z.ctypes.data, None if seed_lam is None else seed_lam.ctypes.data,
                               grad.ctypes.data, dz0.ctypes.data, dlam0.ctypes.data)
  assert rc == NP
  return grad, dz0, dlam0


def twin_of_case(lib, c):
  return twin_grad(lib, c["N"], c["T"], c["z"], c["lam"], c["lb"], c["ub"], c["params"], c["eta_x"], c["eta_v"], c["nsteps"], c["seed_z"], c["seed_lam"])
