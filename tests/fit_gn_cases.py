"""Shared by the Gauss-Newton fit tests (test_fit_gn_host_twin.py, test_gpu_fit_gn.py): the host twin of csrc/fit_gn.h, the oracle's
references, noise-free fitting problems, and a stand-in for the device engine that runs the twin.

The inputs are fit_cases'.  The reference of a case is J = d xh / d p of the oracle's own rollout -- forward-mode autograd, one pass per
parameter; central differences of the rollout with step 1e-6 |p| for fit_cases.FD_SYSTEMS -- from which grad = 2 sum_t wt[t] J_t^T r_t and
gn = 2 sum_t wt[t] J_t^T J_t are formed in numpy.  Everything is cached: a reference is computed once per session and never modified."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import torch

import fit_cases as F
from myriad_amd._lib import INT_IDS, SYS_IDS

GN_SYSTEMS = ("CARTPOLE", "VANDERPOL", "CANCERTREATMENT", "PENDULUM", "HIVTREATMENT", "ROCKETLANDING", "HARVEST")
LM_SYSTEMS = ("CARTPOLE", "VANDERPOL", "PENDULUM", "MOUNTAINCAR", "CANCERTREATMENT", "GLUCOSE")      # the candidates the issue names
LM_MAX_ITER, LM_RATIO = 30, 1e-12


# ---- the twin ----------------------------------------------------------------------------------------------------------------------------
def build_twin(tmp_dir):
  """tests/hostsim/fit_gn_twin.cpp -> tmp_dir/libfit_gn_twin.so (g++ -O2 -std=c++17), loaded with ctypes"""
  out = os.path.join(str(tmp_dir), "libfit_gn_twin.so")
  subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", os.path.join(F.ROOT, "tests", "hostsim", "fit_gn_twin.cpp"), "-o", out], check=True)
  lib = C.CDLL(out)
  vp = C.c_void_p
  lib.fit_gn_twin.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp]
  lib.fit_gn_twin.restype = C.c_int
  lib.fit_gn_twin_rollout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, vp, C.c_int, vp]
  lib.fit_gn_twin_rollout.restype = C.c_int
  return lib


def _c(a):
  return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def twin_fit_gn(lib, name, method, T, xs_obs, us, params=None, wt=None, want_grad=True):
  """FitGnLane<Sys> on the host over the batch: (loss [batch], grad [batch][np] or None, gn [batch][np][np]); params [np], [batch][np] or None"""
  xs_obs, us, params, wt = _c(xs_obs), _c(us), _c(params), _c(wt)
  batch, npar = xs_obs.shape[0], len(F.O.SYSTEMS[name].param_names)
  loss, grad, gn = np.empty(batch), (np.empty((batch, npar)) if want_grad else None), np.empty((batch, npar, npar))
  rc = lib.fit_gn_twin(SYS_IDS[name], INT_IDS[method], batch, xs_obs.shape[1] - 1, float(T), us.shape[1], xs_obs.ctypes.data, us.ctypes.data,
                       None if wt is None else wt.ctypes.data, None if params is None else params.ctypes.data,
                       0 if params is None or params.ndim == 1 else npar, loss.ctypes.data, None if grad is None else grad.ctypes.data, gn.ctypes.data)
  assert rc == 0, f"fit_gn_twin: no specialisation for {name}"
  return loss, grad, gn


def twin_rollout(lib, name, method, T, x0, us, params=None):
  """Rollout<Sys>::run on the host: xs [batch][S+1][ns] with u_rows = S + 1"""
  x0, us, params = _c(x0), _c(us), _c(params)
  batch, S = x0.shape[0], us.shape[1] - 1
  xs = np.empty((batch, S + 1, x0.shape[1]))
  rc = lib.fit_gn_twin_rollout(SYS_IDS[name], INT_IDS[method], batch, S, float(T), us.shape[1], x0.ctypes.data, us.ctypes.data,
                               None if params is None else params.ctypes.data, 0, xs.ctypes.data)
  assert rc == 0, f"fit_gn_twin_rollout: no specialisation for {name}"
  return xs


# ---- the oracle's references -------------------------------------------------------------------------------------------------------------
def _oracle_states(name, method, x0, us, prow, h, S):
  sysm = F.make_system(name, prow)
  return F.O.integrate_time_independent(sysm.dynamics, torch.tensor(x0), torch.tensor(us), h, S, method)[1]


def oracle_jacobian(name, method, xs_obs, us, prow):
  """(xh [S+1][ns], J [S+1][ns][np]) of the oracle's rollout of ONE trajectory at the parameters prow [np]"""
  import torch.autograd.forward_ad as fwad
  S, npar = xs_obs.shape[0] - 1, prow.shape[0]
  h = F.horizon(name, S) / S
  J = np.zeros((S + 1, xs_obs.shape[1], npar))
  if name in F.FD_SYSTEMS:
    xh = _oracle_states(name, method, xs_obs[0], us, [float(v) for v in prow], h, S).numpy()
    for k in range(npar):
      d = 1e-6 * abs(prow[k])
      pp, pm = prow.copy(), prow.copy()
      pp[k] += d
      pm[k] -= d
      J[:, :, k] = (_oracle_states(name, method, xs_obs[0], us, [float(v) for v in pp], h, S).numpy()
                    - _oracle_states(name, method, xs_obs[0], us, [float(v) for v in pm], h, S).numpy()) / (2.0 * d)
    return xh, J
  xh = None
  for k in range(npar):
    with fwad.dual_level():
      pt = [fwad.make_dual(torch.tensor(float(v), dtype=torch.float64), torch.tensor(1.0 if i == k else 0.0, dtype=torch.float64))
            for i, v in enumerate(prow)]
      primal, tangent = fwad.unpack_dual(_oracle_states(name, method, xs_obs[0], us, pt, h, S))
      xh = primal.detach().numpy().copy()
      if tangent is not None:
        J[:, :, k] = tangent.numpy()
  return xh, J


def grad_gn_from_jacobian(xh, J, xs_obs, wt=None):
  """(loss, grad [np], gn [np][np]) of one trajectory from its states and their sensitivities"""
  w = np.ones(xh.shape[0]) if wt is None else np.asarray(wt)
  r = xh - xs_obs
  loss = float((w * (r * r).sum(-1)).sum())
  grad = 2.0 * np.einsum("t,tik,ti->k", w, J, r)
  gn = 2.0 * np.einsum("t,tik,til->kl", w, J, J)
  return loss, grad, gn


@functools.lru_cache(maxsize=None)
def _jacobians(name, method, long_u=False, batch=F.B, S=None, per_instance=False):
  xs_obs, us, params = F.inputs(name, method, long_u, batch, S, per_instance)
  prow = np.broadcast_to(params, (xs_obs.shape[0], params.shape[-1]))
  return [oracle_jacobian(name, method, xs_obs[b], us[b], prow[b].copy()) for b in range(xs_obs.shape[0])]


@functools.lru_cache(maxsize=None)
def reference(name, method, long_u=False, weighted=False, batch=F.B, S=None, per_instance=False):
  """(loss [batch], grad [batch][np], gn [batch][np][np]) of the oracle for fit_cases.inputs' case"""
  xs_obs = F.inputs(name, method, long_u, batch, S, per_instance)[0]
  wt = F.decaying_wt(xs_obs.shape[1] - 1) if weighted else None
  rows = [grad_gn_from_jacobian(xh, J, xs_obs[b], wt) for b, (xh, J) in enumerate(_jacobians(name, method, long_u, batch, S, per_instance))]
  out = tuple(np.array([r[i] for r in rows]) for i in range(3))
  for a in out:
    assert np.isfinite(a).all(), f"the oracle's own reference is not finite for {name} {method}"
    a.setflags(write=False)
  return out


def rel_errors(grad, gn, ref_grad, ref_gn):
  """(largest |dgrad| / max|grad|, largest |dgn| / max|gn|) of a trajectory, over the trajectories of a case"""
  eg = np.abs(grad - ref_grad).max(axis=-1) / np.abs(ref_grad).max(axis=-1)
  en = np.abs(gn - ref_gn).max(axis=(-2, -1)) / np.abs(ref_gn).max(axis=(-2, -1))
  return float(eg.max()), float(en.max())


# ---- a stand-in for _lib.Engine that runs the twin (the `fit=` of the drivers: FitLoss(hp, engine=TwinEngine(...))) -----------------------
class TwinEngine:
  """fit_gn, fit_gn_sets, fit_grad and fit_grad_sets of _lib.Engine (reduce=True forms included) on the host twin; sums in row order"""

  def __init__(self, lib, name, method, T):
    self.lib, self.name, self.method, self.T = lib, name, method, T
    self.np = len(F.O.SYSTEMS[name].param_names)
    self.calls = []                                               # (entry point, number of sets) of every call

  def _one(self, xs_obs, us, params, wt, reduce):
    loss, grad, gn = twin_fit_gn(self.lib, self.name, self.method, self.T, xs_obs, us, params, wt)
    if reduce:
      g, G = np.zeros(self.np), np.zeros((self.np, self.np))
      for b in range(loss.shape[0]):                              # a fixed order, so that a set's sums do not depend on the sets beside it
        g, G = g + grad[b], G + gn[b]
      grad, gn = g, G
    return {"loss": loss, "grad": grad, "gn": gn}

  def fit_gn(self, xs_obs, us, params=None, wt=None, reduce=False):
    self.calls.append(("fit_gn", 1))
    return self._one(xs_obs, us, params, wt, reduce)

  def fit_gn_sets(self, xs_obs, us, params, wt=None, reduce=False):
    params = np.asarray(params)
    self.calls.append(("fit_gn_sets", params.shape[0]))
    xs_obs, us = np.asarray(xs_obs), np.asarray(us)
    rows = [self._one(xs_obs if xs_obs.ndim == 3 else xs_obs[e], us if us.ndim == 3 else us[e], params[e], wt, reduce) for e in range(params.shape[0])]
    return {k: np.stack([r[k] for r in rows]) for k in ("loss", "grad", "gn")}

  def fit_grad(self, xs_obs, us, params=None, wt=None, reduce=False):
    out = self._one(xs_obs, us, params, wt, reduce)
    return {"loss": out["loss"], "grad": out["grad"]}

  def fit_grad_sets(self, xs_obs, us, params, wt=None, reduce=False, want_grad=True):
    params = np.asarray(params)
    self.calls.append(("fit_grad_sets", params.shape[0]))
    xs_obs, us = np.asarray(xs_obs), np.asarray(us)
    rows = [self._one(xs_obs if xs_obs.ndim == 3 else xs_obs[e], us if us.ndim == 3 else us[e], params[e], wt, reduce) for e in range(params.shape[0])]
    return {k: np.stack([r[k] for r in rows]) for k in (("loss", "grad") if want_grad else ("loss",))}

  def close(self):
    pass


# ---- noise-free fitting problems -----------------------------------------------------------------------------------------------------------
LM_B = 8


@functools.lru_cache(maxsize=None)
def lm_inputs(name):
  """(x0 [8][ns], us [8][S+1][nu], start [np]) of the Levenberg-Marquardt problem of a system: the start states and controls of
  fit_cases.inputs(name, "HEUN", batch=8), and its parameters -- the defaults moved by up to 5 % -- as the start point.  The data are the
  rollout at the DEFAULT parameters, without noise: lm_data."""
  xs_obs, us, start = F.inputs(name, "HEUN", batch=LM_B)
  return xs_obs[:, 0].copy(), us, start


def lm_data(lib, name):
  """xs_obs [8][S+1][ns]: the twin's own rollout at the default parameters (HEUN)"""
  x0, us, _ = lm_inputs(name)
  return twin_rollout(lib, name, "HEUN", F.horizon(name), x0, us)


def lm_run(fit_gn, start, max_iter=LM_MAX_ITER):
  """Levenberg-Marquardt in ALL np parameters from `start` [np]; fit_gn(p [np]) -> (loss, grad [np], gn [np][np]), summed over the batch.
  Returns the LevenbergMarquardt object (params, loss, loss0, iterations, gn)."""
  from myriad_amd.experiments.mle_sysid import LevenbergMarquardt
  keys = [str(k) for k in range(start.shape[0])]
  vec = lambda m: np.array([m[k] for k in keys])
  ev = lambda m: (lambda l, g, G: (l, dict(zip(keys, g)), G))(*fit_gn(vec(m)))
  lm = LevenbergMarquardt(dict(zip(keys, (float(v) for v in start))), max_iter=max_iter)
  lm.begin(*ev(lm.params))
  while not lm.done:
    lm.end(*ev(lm.trial()))
  lm.vector = vec(lm.params)
  return lm


def driver_problem(lib, name, E, S=7):
  """A small fitting problem for the drivers of experiments/mle_sysid.py: hyperparameters of test_fit_sets_host._setup's kind (train 5, val 2,
  test 2 trajectories of S steps), E noise-free datasets [E][9][S+1][ns+nu] -- the twin's rollouts (HEUN) at the default parameters scaled by
  1, 1.02, 1.04, ... per set, on fit_cases.horizon's horizon --, those parameters [E][np], and a factory of FitLoss objects on the twin stand-in.
  On the device the same problem runs on _lib.Engine(name, "SHOOTING", 1, horizon, controls_per_interval=S, integration_method="HEUN")."""
  from myriad_amd.config import Config, HParams, OptimizerType
  from myriad_amd.experiments.mle_sysid import FitLoss
  from myriad_amd.systems import SystemType
  hp = HParams(system=SystemType[name], optimizer=OptimizerType.SHOOTING, intervals=1, controls_per_interval=S, train_size=5, val_size=2, test_size=2,
               seed=7)
  total, T = hp.train_size + hp.val_size + hp.test_size, F.horizon(name, S)
  xs_obs, us, _ = F.inputs(name, "HEUN", batch=E * total, S=S)
  truth = F.O.SYSTEMS[name]().params()[None] * (1.0 + 0.02 * np.arange(E))[:, None]
  us = us.reshape(E, total, S + 1, -1)
  xs = np.stack([twin_rollout(lib, name, "HEUN", T, xs_obs[e * total:(e + 1) * total, 0], us[e], truth[e]) for e in range(E)])
  datasets = np.concatenate([xs, us], axis=-1)
  return hp, Config(verbose=False), datasets, truth, lambda: FitLoss(hp, engine=TwinEngine(lib, name, "HEUN", T))
