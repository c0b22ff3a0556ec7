"""Inputs shared by the tests of the weight-set calls of the network system (test_gpu_node_sets.py, test_node_sets_host.py): E weight sets -- the
committed (64, 64) weights plus 5 % noise per set --, random instances without an oracle run for the bit comparisons, and the oracle references of
the single-set case modules (node_exgd_grad_cases, node_shoot_exgd_grad_cases, node_hvp_cases) taken under ANOTHER weight set: those modules read
their weights through their `weights()` functions, which `weights_as` replaces for the length of a `with` block; their cached `reference`
functions are called through `__wrapped__`, so nothing of this enters their caches.
"""
import contextlib

import numpy as np

import node_exgd_grad_cases as X
import node_hvp_cases as H
import node_shoot_exgd_grad_cases as S

NS, NU, NP = 4, 1, 4804
NOISE = 0.05
SETS = ((3, 1), (3, 2), (1, 3), (2, 5))                      # (E, R)


def weight_sets(E, seed=5):
  """[E, 4804]: row e = the committed weights times (1 + 0.05 N(0, 1)) entry by entry, a draw per set; every row differs from row 0 in bits"""
  rng = np.random.default_rng(seed)
  flat = X.weights()[1]
  rows = np.stack([flat * (1.0 + NOISE * rng.standard_normal(NP)) for _ in range(E)])
  assert all(rows[e].tobytes() != rows[0].tobytes() for e in range(1, E))
  return rows


@contextlib.contextmanager
def weights_as(flat):
  """the three case modules draw, step and differentiate under the weight vector `flat` inside the block"""
  from myriad_amd.systems.neural_ode import mapping_from_flat
  flat = np.array(flat, dtype=np.float64)
  flat.setflags(write=False)
  fn = lambda: (mapping_from_flat(flat), flat)
  saved = [(mod, mod.weights) for mod in (X, S, H)]
  for mod, _ in saved:
    mod.weights = fn
  try:
    yield
  finally:
    for mod, old in saved:
      mod.weights = old


def hs_reference(flat, N, nsteps, batch):
  """node_exgd_grad_cases.reference under the weights `flat`: (case, grad, dz0, dlam0), its acceptance conditions included"""
  with weights_as(flat):
    return X.reference.__wrapped__(N, nsteps, batch)


def shoot_reference(flat, I, cpi, method, nsteps, batch):
  with weights_as(flat):
    return S.reference.__wrapped__(I, cpi, method, nsteps, batch)


def hvp_reference(flat, tr, I, cpi, method, batch):
  with weights_as(flat):
    return H.reference.__wrapped__(tr, I, cpi, method, batch)


def instances(n, m, E, R, seed, nx):
  """E R random instances [E, R, ...] without an oracle run (the shape_case of the single-set modules): states 0.5 N(0, 1) in the first nx entries,
  controls U(-5, 5), a third of the variables in a box of 1e-3 that the steps leave, the first state pinned"""
  rng = np.random.default_rng(seed)
  z = np.concatenate([0.5 * rng.standard_normal((E, R, nx)), rng.uniform(-5.0, 5.0, (E, R, n - nx))], axis=2)
  box = rng.random((E, R, n)) < 1.0 / 3.0
  lb, ub = np.where(box, z - 1e-3, -np.inf), np.where(box, z + 1e-3, np.inf)
  lb[..., :NS] = z[..., :NS]; ub[..., :NS] = z[..., :NS]
  return dict(z=z, lam=0.1 * rng.standard_normal((E, R, m)), lb=lb, ub=ub, seed_z=rng.standard_normal((E, R, n)),
              seed_lam=rng.standard_normal((E, R, m)), v=rng.standard_normal((E, R, n)), eta_x=0.05, eta_v=0.5)
