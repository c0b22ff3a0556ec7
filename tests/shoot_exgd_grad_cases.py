"""Inputs and oracle references shared by the tests of the unrolled-extragradient derivative under SHOOTING (test_shoot_exgd_grad_host_twin.py,
test_gpu_shoot_exgd_grad.py).

A case is (system, I, cpi, integrator, nsteps, batch).  z, lam and the parameter row per instance are hvp_cases._draw's with tr = "SHOOTING"
(HIVTREATMENT and SEIR at states and parameters of order one, for the central differences, as hvp_cases.reference draws them); the seeds come from a generator of their own.  Step
sizes, boxes and conditions are exgd_grad_cases': eta_x L = 0.2 and eta_x eta_v |J|^2 = 0.2 from ten rounds of the power iteration on the first
instance; the state of the first node pinned (lb == ub); of the other, free variables 30 % per instance in a box of 0.3 |eta_x g_i| around z_i, which
the first half-step leaves, about half of the rest with finite bounds far away.  The reference is torch autograd through
`oracle.make_transcription(..., "SHOOTING", ...)` and the formulas of `Lagrangian.step` restated with `torch.clamp`; HIVTREATMENT, SEIR and TUMOUR
take the parameter gradient from central differences with step 1e-6 |p| (dz0 and dlam0 are autograd for them too).

Conditions of a draw (the first of the seeds 0 .. 19 that meets them is taken; a case without one fails): the run is finite; no unclipped value in
front of a clamp lies within TIE = 1e-6 of a bound and no clipped one equals its bound (`torch.clamp` passes the cotangent where lb <= v <= ub, the
device where lb < clip(v) < ub); at least MIN_CLIPPED = 15 % of the free variables of every instance clip in at least one half-step; and no point
the field of PENDULUM / MOUNTAINCAR is evaluated at -- every stage point of every step of every rollout, recorded as hvp_cases does -- lies within
KINK = 1e-3 of a kink.

One more condition, for the three central-difference systems only, on the REFERENCE alone (the code under test is not looked at): the difference
quotient must resolve the tolerance it is compared under.  Its rounding noise is eps |out| / (1e-6 |p|); TUMOUR runs at states of 9 000 and a
parameter of 0.009 (drawn at order one its Lagrangian's gradient is below the 1e-5 the boxes need: no draw clips), and at seed 0 of 1 x 4 RK4 the
quotient with step 1e-6 |p| is 1.5e-6 max|grad| away from the twin while the one with step 1e-5 |p| is 4e-9 away.  So a draw is taken only if the
quotients with steps 1e-6 |p| and 2e-6 |p| -- whose truncation errors are negligible and whose rounding errors are independent, the second half
the first -- agree within FD_SELF = FD_RTOL / 4 of max|grad|.  The reference stays the quotient with step 1e-6 |p|, the tolerance FD_RTOL.
"""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import exgd_grad_cases as E  # noqa: E402
import hvp_cases as H  # noqa: E402
from oracle import myriad_oracle as O  # noqa: E402

SYSTEMS = H.SYSTEMS
METHODS = H.METHODS
FD_SYSTEMS = H.FD_SYSTEMS
FD_RTOL = H.FD_RTOL
TIE = E.TIE
KINK = E.KINK
MIN_CLIPPED = E.MIN_CLIPPED
FD_SELF = 0.25 * FD_RTOL          # |quotient(1e-6 |p|) - quotient(2e-6 |p|)| / max|grad| of a draw of a central-difference system
# (I, cpi, method) of the host matrix: 3 x 2 under each integrator, single shooting 1 x 4 RK4
HOST_SHAPES = ((3, 2, "EULER"), (3, 2, "HEUN"), (3, 2, "MIDPOINT"), (3, 2, "RK4"), (1, 4, "RK4"))
rel_error = E.rel_error


def oracle_run(name, I, cpi, method, T, z, lam, lb, ub, prow, eta_x, eta_v, nsteps, grad_params=True, visited=None):
  """One instance through `nsteps` steps in torch.  Returns (z_n, lam_n, leaves, pre): the leaf tensors (parameters, z0, lam0) and the values in
  front of every clamp; `visited` collects every point the field is evaluated at."""
  pt = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in prow] if grad_params else [float(v) for v in prow]
  _, tr = H._transcription(name, "SHOOTING", I, cpi, method, T, pt, visited)
  z0, lam0 = E.start_leaves(z, lam)
  x, lm, pre, _ = E.unrolled_steps(tr, z0, lam0, lb, ub, eta_x, eta_v, nsteps)
  return x, lm, (pt, z0, lam0), pre


def _draw(name, I, cpi, method, nsteps, batch, seed):
  base = H._draw(name, "SHOOTING", I, cpi, method, batch, seed, name in ("HIVTREATMENT", "SEIR"))
  z, lam, params, n, m, ns, T = base["z"], base["lam"], base["params"], base["n"], base["m"], base["ns"], base["T"]
  rng = np.random.default_rng(7919 + 100000 * seed + 1000 * SYSTEMS.index(name) + 10 * I + cpi + 3 * METHODS.index(method) + 7 * batch + 31 * nsteps)
  seed_z = rng.standard_normal((batch, n))
  seed_lam = rng.standard_normal((batch, m))
  tr_of = lambda b: H._transcription(name, "SHOOTING", I, cpi, method, T, [float(v) for v in params[b]])[1]
  lag = O.Lagrangian(tr_of(0))
  g0 = np.stack([O.Lagrangian(tr_of(b)).grad_x(z[b], lam[b]) for b in range(batch)])
  gz = lag.grad_x(z[0], 0.0 * lam[0])
  v, w, lip, jn = rng.standard_normal(n), rng.standard_normal(n), 0.0, 0.0
  for _ in range(10):                                                # (exgd_grad_cases._draw)
    eps = 1e-6 * (1.0 + np.abs(z[0]).max())
    hv = (lag.grad_x(z[0] + eps * v / np.linalg.norm(v), lam[0]) - g0[0]) / eps
    lip, v = np.linalg.norm(hv), hv
    jw = lag.jvp(z[0], w / np.linalg.norm(w))
    jtjw = lag.grad_x(z[0], jw) - gz                                 # J^T (J w): grad_x L is affine in lam
    jn, w = np.linalg.norm(jtjw), jtjw
  eta_x = 0.2 / max(lip, 1e-12)
  eta_v = 0.2 / max(eta_x * jn, 1e-12)
  delta = eta_x * np.abs(g0)
  lb, ub = E.draw_boxes(rng, z, delta, ns)
  return dict(name=name, I=I, cpi=cpi, method=method, T=T, nsteps=nsteps, z=z, lam=lam, lb=lb, ub=ub, params=params, eta_x=float(eta_x),
              eta_v=float(eta_v), seed_z=seed_z, seed_lam=seed_lam, n=n, m=m, ns=ns, nu=base["nu"])


def _oracle(case):
  """(grad [B][np], dz0 [B][n], dlam0 [B][m], tie distance, kink distance, clipped fraction, central-difference self-check): exgd_grad_cases._oracle
  over the shooting run"""
  c = case
  batch, npar = c["z"].shape[0], c["params"].shape[1]
  grad, dz0, dlam0 = np.empty((batch, npar)), np.empty((batch, c["n"])), np.empty((batch, c["m"]))
  tie, kink, clipped = np.inf, np.inf, np.zeros((batch, c["n"]), dtype=bool)
  fd = c["name"] in FD_SYSTEMS
  grad2 = np.empty((batch, npar))                      # the quotient with twice the step (FD_SELF)

  def out_of(b, prow, grad_params, visited=None):
    xn, ln, leaves, pre = oracle_run(c["name"], c["I"], c["cpi"], c["method"], c["T"], c["z"][b], c["lam"][b], c["lb"][b], c["ub"][b], prow,
                                     c["eta_x"], c["eta_v"], c["nsteps"], grad_params, visited)
    return (torch.tensor(c["seed_z"][b]) * xn).sum() + (torch.tensor(c["seed_lam"][b]) * ln).sum(), leaves, pre

  for b in range(batch):
    visited = []
    out, (pt, z0, lam0), pre = out_of(b, c["params"][b], not fd, visited)
    gs = torch.autograd.grad(out, ([] if fd else pt) + [z0, lam0], allow_unused=True)
    gs = [torch.zeros(()) if g is None else g for g in gs]
    dz0[b], dlam0[b] = gs[-2].numpy(), gs[-1].numpy()
    if fd:
      for k in range(npar):
        d = 1e-6 * abs(c["params"][b, k])
        pp, pm = c["params"][b].copy(), c["params"][b].copy()
        pp[k] += d; pm[k] -= d
        grad[b, k] = (float(out_of(b, pp, False)[0].detach()) - float(out_of(b, pm, False)[0].detach())) / (2.0 * d)
        pp[k] += d; pm[k] -= d
        grad2[b, k] = (float(out_of(b, pp, False)[0].detach()) - float(out_of(b, pm, False)[0].detach())) / (4.0 * d)
    else:
      grad[b] = [float(g) for g in gs[:npar]]
    t, outside = E.clamp_conditions(pre, c["lb"][b], c["ub"][b])
    tie, clipped[b] = min(tie, t), outside
    kink = min(kink, H._kink_distance(c["name"], visited))
  with np.errstate(invalid="ignore"):
    self_check = rel_error(grad2, grad) if fd else 0.0
  return grad, dz0, dlam0, tie, kink, E.clipped_fraction(clipped, c["lb"], c["ub"]), self_check


@functools.lru_cache(maxsize=None)
def reference(name, I, cpi, method, nsteps=3, batch=2):
  """(case, grad, dz0, dlam0) of the first draw that meets the conditions; asserts that there is one.  case["seed"], ["tie"], ["kink"], ["clipped"]
  say which draw it is and by how much it meets them."""
  last = None
  for seed in range(20):
    case = _draw(name, I, cpi, method, nsteps, batch, seed)
    grad, dz0, dlam0, tie, kink, frac, fd_self = _oracle(case)
    last = (seed, tie, kink, frac, fd_self)
    finite = np.isfinite(grad).all() and np.isfinite(dz0).all() and np.isfinite(dlam0).all()
    if finite and (nsteps == 0 or (tie > TIE and kink > KINK and frac >= MIN_CLIPPED and fd_self <= FD_SELF)):
      for a in list(case.values()) + [grad, dz0, dlam0]:
        if isinstance(a, np.ndarray):
          a.setflags(write=False)
      case.update(seed=seed, tie=tie, kink=kink, clipped=frac, fd_self=fd_self)
      return case, grad, dz0, dlam0
  raise AssertionError(f"{name} {I}x{cpi} {method} nsteps={nsteps}: no draw meets the conditions (last: seed, tie, kink, clipped, fd self-check = {last})")


def build_twin(tmp_dir):
  """tests/hostsim/shoot_exgd_grad_twin.cpp -> tmp_dir/libshoot_exgd_grad_twin.so (g++ -O2 -std=c++17), loaded with ctypes"""
  import ctypes as C
  import subprocess
  out = os.path.join(str(tmp_dir), "libshoot_exgd_grad_twin.so")
  subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "hostsim", "shoot_exgd_grad_twin.cpp"), "-o", out], check=True)
  lib = C.CDLL(out)
  vp = C.c_void_p
  lib.shoot_exgd_grad_twin.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp, vp, C.c_int, C.c_double, C.c_double,
                                       C.c_int, vp, vp, C.c_int, vp, vp, vp]
  lib.shoot_exgd_grad_twin.restype = C.c_int
  return lib


def twin_grad(lib, name, I, cpi, method, T, z, lam, lb, ub, params, eta_x, eta_v, nsteps, seed_z, seed_lam=None, fused=True):
  """ShootExgdGrad on the host over the batch: (grad [B][np], dz0 [B][n], dlam0 [B][m]); fused=False: items 1 .. 5 as three passes a step"""
  from myriad_amd._lib import INT_IDS, SYS_IDS
  z, lam, params, seed_z = (np.ascontiguousarray(a, dtype=np.float64) for a in (z, lam, params, seed_z))
  lb = np.ascontiguousarray(np.broadcast_to(np.asarray(lb, dtype=np.float64), z.shape))
  ub = np.ascontiguousarray(np.broadcast_to(np.asarray(ub, dtype=np.float64), z.shape))
  seed_lam = None if seed_lam is None else np.ascontiguousarray(seed_lam, dtype=np.float64)
  batch, npar = z.shape[0], params.shape[-1]
  grad, dz0, dlam0 = np.empty((batch, npar)), np.empty(z.shape), np.empty(lam.shape)
  rc = lib.shoot_exgd_grad_twin(SYS_IDS[name], INT_IDS[method], batch, int(I), int(cpi), float(T), z.ctypes.data, lam.ctypes.data, lb.ctypes.data,
                                ub.ctypes.data, params.ctypes.data, 0 if params.ndim == 1 else npar, float(eta_x), float(eta_v), int(nsteps),
                                seed_z.ctypes.data, None if seed_lam is None else seed_lam.ctypes.data, 1 if fused else 0, grad.ctypes.data,
                                dz0.ctypes.data, dlam0.ctypes.data)
  assert rc == 0, f"shoot_exgd_grad_twin: no specialisation for {name} {method}"
  return grad, dz0, dlam0


def twin_of_case(lib, case, fused=True, **kw):
  c = dict(case); c.update(kw)
  return twin_grad(lib, c["name"], c["I"], c["cpi"], c["method"], c["T"], c["z"], c["lam"], c["lb"], c["ub"], c["params"], c["eta_x"], c["eta_v"],
                   c["nsteps"], c["seed_z"], c["seed_lam"], fused)


def shape_case(I, cpi, method, nsteps, B, name="CARTPOLE"):
  """inputs without an oracle run (test_gpu_exgd_grad.shape_case over a shooting problem): states around x_0, a third of the variables in a box of
  1e-3 that the steps leave, the first node pinned, steps of 0.05"""
  sysm = O.SYSTEMS[name]()
  xr, ur, n, m = H.dims(name, "SHOOTING", I, cpi, method)
  rng = np.random.default_rng(7 + 1000 * I + 100 * cpi + 10 * nsteps + B + METHODS.index(method))
  xs = np.tile(sysm.x_0, (B, xr, 1)) + 0.2 * rng.standard_normal((B, xr, sysm.ns))
  us = rng.uniform(-1.0, 1.0, (B, ur, sysm.nu))
  z = np.concatenate([xs.reshape(B, -1), us.reshape(B, -1)], axis=1)
  box = rng.random((B, n)) < 0.3
  lb = np.where(box, z - 1e-3, -np.inf)
  ub = np.where(box, z + 1e-3, np.inf)
  lb[:, :sysm.ns] = z[:, :sysm.ns]; ub[:, :sysm.ns] = z[:, :sysm.ns]
  params = sysm.params() * (1.0 + 0.05 * (2.0 * rng.random((B, sysm.params().size)) - 1.0))
  return dict(name=name, I=I, cpi=cpi, method=method, T=0.05 * I * cpi, nsteps=nsteps, z=z, lam=0.1 * rng.standard_normal((B, m)), lb=lb, ub=ub,
              params=params, eta_x=0.02, eta_v=0.02, seed_z=rng.standard_normal((B, n)), seed_lam=rng.standard_normal((B, m)), n=n, m=m, ns=sysm.ns,
              nu=sysm.nu)
