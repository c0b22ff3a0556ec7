"""Inputs and oracle references shared by the tests of the unrolled-extragradient derivative (test_exgd_grad_host_twin.py,
test_gpu_exgd_grad.py).

A case is (system, scheme, N, nsteps, batch).  Its inputs -- z, lam, the seeds, a parameter row per instance, bounds -- are drawn from a fixed
seed.  The state of the first point is pinned (lb == ub).  Of the other, free variables 30 % per instance get a box of 0.3 |eta_x g_i| around z_i,
which the first half-step leaves; the rest is wide or unbounded.  `clipped` of a case is the fraction of the FREE variables that clip in at least
one half-step, the smallest over the instances; a draw with less than 15 % is not taken.  The reference is torch autograd through
`oracle.make_transcription` and the formulas of `Lagrangian.step` restated with `torch.clamp`, the parameters as tensors (fit_cases.make_system);
HIVTREATMENT, SEIR and TUMOUR, whose constructors convert their arguments, take the parameter gradient from central differences with step
1e-6 |p| (dz0 and dlam0 are autograd for them too).  A central difference resolves eps |x| / (1e-6 |p|): HIVTREATMENT and SEIR are drawn at states
and parameters of order one, where that is seven digits (at their x_0 of 800 / 1000 and k = 2.4e-5, c = 1e-4 it is three).

Tie condition: `torch.clamp` passes the cotangent where lb <= v <= ub, the device where lb < clip(v) < ub; the two agree unless an iterate meets a
bound exactly.  The oracle's run records every value in front of its clamp, and `reference` asserts that no unclipped one (lb < v < ub) lies within
1e-6 of a bound, that no clipped one equals its bound, and that no point PENDULUM / MOUNTAINCAR visit lies within 1e-3 of a kink of their fields
(|u| = 2, |x1| = 8, theta = pi mod 2 pi; |u| = 1).  The draw of a case is the first of the seeds 0, 1, ... 19 whose run satisfies this and stays
finite and clips enough; a case without one fails.
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

SCHEMES = ("HERMITE_SIMPSON", "TRAPEZOIDAL")
SYSTEMS = F.SYSTEMS
FD_SYSTEMS = F.FD_SYSTEMS
FD_RTOL = F.FD_RTOL
TIE = 1e-6
KINK = 1e-3
MIN_CLIPPED = 0.15      # of the free variables of every instance, in at least one half-step


def horizon(name, N):
  """T of a case: intervals of at most 0.1 (the systems' own horizons over three intervals are far outside the range where a step is a small move)."""
  return min(float(O.SYSTEMS[name]().T), 0.1 * N)


def dims(name, scheme, N):
  s = O.SYSTEMS[name]()
  K = 2 * N + 1 if scheme == "HERMITE_SIMPSON" else N + 1
  return K, K * (s.ns + s.nu), (2 if scheme == "HERMITE_SIMPSON" else 1) * N * s.ns


def _transcription(name, scheme, N, T, prow):
  sysm = F.make_system(name, prow)
  sysm.T = T
  if name == "BEARPOPULATIONS":                        # the constructor takes float(c_p), float(c_f): set them, so that autograd sees the cost's parameters
    sysm.c_p, sysm.c_f = prow[4], prow[5]
  if name == "PREDATORPREY":                           # x_T = [None, None, B] only shapes the guess and the bounds, which the cases do not take from here
    sysm.x_T = None
  with torch.no_grad():                                # (the trapezoidal guess rolls the system out; nothing of it is used here)
    return sysm, O.make_transcription(sysm, "COLLOCATION", N, quadrature_rule=scheme)


def start_leaves(z, lam):
  """(z0, lam0): the starting point of a run as leaf tensors"""
  return (torch.tensor(np.asarray(z), dtype=torch.float64, requires_grad=True),
          torch.tensor(np.asarray(lam), dtype=torch.float64, requires_grad=True))


def unrolled_steps(tr, x, lm, lo, hi, eta_x, eta_v, nsteps):
  """`nsteps` steps of `Lagrangian.step` (extra_gradient.py:25-33) over the transcription `tr`, restated with `torch.clamp`, from the tensors
  (x, lm) between the bounds (lo, hi).  Returns (x_n, lam_n, pre, pts): the values in front of every clamp and every point the run evaluated the
  Lagrangian's gradient at.  The one statement of the step for the four case modules of the family."""
  lo, hi = torch.tensor(np.asarray(lo)), torch.tensor(np.asarray(hi))
  L = lambda xx, ll: tr.objective(xx) + ll @ tr.constraints(xx)      # extra_gradient.py:21-23

  def gx(xx, ll):                                                   # the PARTIAL gradient in x: lam_s is itself a function of x_s, so the
    xi = xx * 1.0                                                    # derivative is taken in a copy that lam_s does not hang on
    return torch.autograd.grad(L(xi, ll), xi, create_graph=True)[0]

  pre, pts = [], []
  for _ in range(nsteps):
    pts.append(x)
    v = x - eta_x * gx(x, lm)
    pre.append(v)
    xb = torch.clamp(v, lo, hi)
    pts.append(xb)
    v = x - eta_x * gx(xb, lm)
    pre.append(v)
    x = torch.clamp(v, lo, hi)
    pts.append(x)
    lm = lm + eta_v * tr.constraints(x)
  return x, lm, pre, pts


def draw_boxes(rng, z, delta, ns):
  """(lb, ub) around z [B][n] for first half-steps of length delta: the first point's state (the first ns entries) pinned; a box of 0.3 delta,
  which the first half-step leaves, around 30 % of the other, FREE variables of every instance, taken from those whose half-step is longer than
  1e-5; of the rest about half get finite bounds far away.  Draws from rng one permutation per instance, then one random((B, n))."""
  batch, n = z.shape
  lb = np.full((batch, n), -np.inf)
  ub = np.full((batch, n), np.inf)
  clipv = np.zeros((batch, n), dtype=bool)
  for b in range(batch):
    cand = ns + np.flatnonzero(delta[b, ns:] > 1e-5)
    clipv[b, rng.permutation(cand)[:int(round(0.3 * (n - ns)))]] = True
  wide = ~clipv & (rng.random((batch, n)) < 0.5)
  lb[clipv] = (z - 0.3 * delta)[clipv]; ub[clipv] = (z + 0.3 * delta)[clipv]
  lb[wide] = (z - 1.0 - 100.0 * delta)[wide]; ub[wide] = (z + 1.0 + 100.0 * delta)[wide]
  lb[:, :ns] = z[:, :ns]; ub[:, :ns] = z[:, :ns]
  return lb, ub


def clamp_conditions(pre, lo, hi):
  """(tie, outside) of one instance from the values in front of its clamps: the smallest distance of an unclipped value (lo < v < hi) to a
  bound -- 0 where a clipped one meets its bound exactly: clamp passes it, the mask does not --, and which variables clipped in some half-step"""
  tie, outside = np.inf, np.zeros(np.shape(lo), dtype=bool)
  for v in pre:
    v = v.detach().numpy()
    out = (v <= lo) | (v >= hi)
    with np.errstate(invalid="ignore"):
      dist = np.minimum(np.abs(v - lo), np.abs(v - hi))
    tie = min(tie, float(dist[~out].min()) if (~out).any() else np.inf)
    if (dist[out] == 0.0).any():
      tie = 0.0
    outside |= out
  return tie, outside


def clipped_fraction(clipped, lb, ub):
  """of the FREE variables (lb < ub; a pinned one is clipped by construction) the fraction that clipped, the smallest over the instances"""
  free = lb < ub
  return float(min((clipped[b] & free[b]).sum() / free[b].sum() for b in range(len(lb))))


def oracle_run(name, scheme, N, T, z, lam, lb, ub, prow, eta_x, eta_v, nsteps, grad_params=True):
  """One instance through `nsteps` steps in torch.  Returns (z_n, lam_n, leaves, pre, pts): the leaf tensors (parameters, z0, lam0), the values in
  front of every clamp and every point the run evaluated the Lagrangian's gradient at."""
  pt = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in prow] if grad_params else [float(v) for v in prow]
  z0, lam0 = start_leaves(z, lam)
  x, lm, pre, pts = unrolled_steps(_transcription(name, scheme, N, T, pt)[1], z0, lam0, lb, ub, eta_x, eta_v, nsteps)
  return x, lm, (pt, z0, lam0), pre, pts


def _kink_distance(name, K, ns, nu, pts):
  """smallest distance of the visited points to a kink of the system's field (inf for a smooth system)"""
  if name not in ("PENDULUM", "MOUNTAINCAR") or not pts:
    return np.inf
  d = np.inf
  for p in pts:
    p = p.detach().numpy()
    xs, us = p[:K * ns].reshape(K, ns), p[K * ns:].reshape(K, nu)
    if name == "PENDULUM":
      d = min(d, np.abs(np.abs(us) - 2.0).min(), np.abs(np.abs(xs[:, 1]) - 8.0).min(), np.abs(np.mod(xs[:, 0], 2 * np.pi) - np.pi).min())
    else:
      d = min(d, np.abs(np.abs(us) - 1.0).min())
  return float(d)


def _draw(name, scheme, N, nsteps, batch, seed):
  sysm = O.SYSTEMS[name]()
  ns, nu = sysm.ns, sysm.nu
  K, n, m = dims(name, scheme, N)
  T = horizon(name, N)
  rng = np.random.default_rng(100000 * seed + 1000 * SYSTEMS.index(name) + 100 * SCHEMES.index(scheme) + 10 * N + nsteps + 7 * batch)
  us = F._controls(sysm, rng, batch, K)
  if name == "PENDULUM":
    us = rng.uniform(-3.0, 3.0, us.shape)              # both sides of the torque clip
  if name == "MOUNTAINCAR":
    us = rng.uniform(-1.5, 1.5, us.shape)
  x0 = np.tile(sysm.x_0, (batch, K, 1)).astype(np.float64)
  if name in ("HIVTREATMENT", "SEIR"):                 # central differences in p resolve eps |x| / (1e-6 |p|): four digits at their x_0 of 800 / 1000,
    x0 = np.ones_like(x0)                              # seven at states of order one
  xs = x0 * (1.0 + 0.05 * rng.standard_normal(x0.shape)) + 0.05 * rng.standard_normal(x0.shape) * (0.0 if name in F.LENHART or name == "TUMOUR" else 1.0)
  z = np.concatenate([xs.reshape(batch, -1), us.reshape(batch, -1)], axis=1)
  lam = 0.1 * rng.standard_normal((batch, m))
  seed_z = rng.standard_normal((batch, n))
  seed_lam = rng.standard_normal((batch, m))
  p0 = sysm.params()
  params = p0 * (1.0 + 0.05 * (2.0 * rng.random((batch, p0.size)) - 1.0))
  if name in ("HIVTREATMENT", "SEIR"):                 # ... and parameters of order one: a step of 1e-6 |p| in k = 2.4e-5 or c = 1e-4 leaves eps |out| / 1e-11
    params = 0.5 + rng.random((batch, p0.size))
  # step sizes from the first instance: eta_x L = 0.2 and eta_x eta_v |J|^2 = 0.2, with L = |grad^2_zz L| and |J| from ten rounds of the power
  # iteration on difference quotients of grad_x L and on J^T J -- three steps of a stable iteration, whatever the units of the system
  _, tr = _transcription(name, scheme, N, T, [float(v) for v in params[0]])
  lag = O.Lagrangian(tr)
  g0 = np.stack([O.Lagrangian(_transcription(name, scheme, N, T, [float(v) for v in params[b]])[1]).grad_x(z[b], lam[b]) for b in range(batch)])
  gz = lag.grad_x(z[0], 0.0 * lam[0])
  v, w, lip, jn = rng.standard_normal(n), rng.standard_normal(n), 0.0, 0.0
  for _ in range(10):
    eps = 1e-6 * (1.0 + np.abs(z[0]).max())
    hv = (lag.grad_x(z[0] + eps * v / np.linalg.norm(v), lam[0]) - g0[0]) / eps
    lip, v = np.linalg.norm(hv), hv
    jw = lag.jvp(z[0], w / np.linalg.norm(w))
    jtjw = lag.grad_x(z[0], jw) - gz                     # J^T (J w): grad_x L is affine in lam
    jn, w = np.linalg.norm(jtjw), jtjw
  eta_x = 0.2 / max(lip, 1e-12)
  eta_v = 0.2 / max(eta_x * jn, 1e-12)
  delta = eta_x * np.abs(g0)
  lb, ub = draw_boxes(rng, z, delta, ns)
  return dict(name=name, scheme=scheme, N=N, T=T, nsteps=nsteps, z=z, lam=lam, lb=lb, ub=ub, params=params, eta_x=float(eta_x), eta_v=float(eta_v),
              seed_z=seed_z, seed_lam=seed_lam, K=K, n=n, m=m, ns=ns, nu=nu)


def _oracle(case):
  """(grad [B][np], dz0 [B][n], dlam0 [B][m], tie distance, kink distance, clipped fraction) of a draw; the fraction is that of the FREE
  variables (lb < ub) that clip in at least one half-step, the smallest over the instances"""
  c = case
  batch, npar = c["z"].shape[0], c["params"].shape[1]
  grad, dz0, dlam0 = np.empty((batch, npar)), np.empty((batch, c["n"])), np.empty((batch, c["m"]))
  tie, kink, clipped = np.inf, np.inf, np.zeros((batch, c["n"]), dtype=bool)
  fd = c["name"] in FD_SYSTEMS

  def out_of(b, prow, grad_params):
    xn, ln, leaves, pre, pts = oracle_run(c["name"], c["scheme"], c["N"], c["T"], c["z"][b], c["lam"][b], c["lb"][b], c["ub"][b], prow, c["eta_x"],
                                          c["eta_v"], c["nsteps"], grad_params)
    return (torch.tensor(c["seed_z"][b]) * xn).sum() + (torch.tensor(c["seed_lam"][b]) * ln).sum(), leaves, pre, pts

  for b in range(batch):
    out, (pt, z0, lam0), pre, pts = out_of(b, c["params"][b], not fd)
    gs = torch.autograd.grad(out, ([] if fd else pt) + [z0, lam0], allow_unused=True)
    gs = [torch.zeros(()) if g is None else g for g in gs]
    dz0[b], dlam0[b] = gs[-2].numpy(), gs[-1].numpy()
    if fd:
      for k in range(npar):
        d = 1e-6 * abs(c["params"][b, k])
        pp, pm = c["params"][b].copy(), c["params"][b].copy()
        pp[k] += d; pm[k] -= d
        grad[b, k] = (float(out_of(b, pp, False)[0].detach()) - float(out_of(b, pm, False)[0].detach())) / (2.0 * d)
    else:
      grad[b] = [float(g) for g in gs[:npar]]
    t, out = clamp_conditions(pre, c["lb"][b], c["ub"][b])
    tie, clipped[b] = min(tie, t), out
    kink = min(kink, _kink_distance(c["name"], c["K"], c["ns"], c["nu"], pts))
  return grad, dz0, dlam0, tie, kink, clipped_fraction(clipped, c["lb"], c["ub"])


@functools.lru_cache(maxsize=None)
def reference(name, scheme, N=3, nsteps=3, batch=2):
  """(case, grad, dz0, dlam0): the first draw whose oracle run is finite, meets the tie condition and clips at least MIN_CLIPPED of the free
  variables of every instance; asserts that there is one."""
  last = None
  for seed in range(20):
    case = _draw(name, scheme, N, nsteps, batch, seed)
    grad, dz0, dlam0, tie, kink, frac = _oracle(case)
    last = (seed, tie, kink, frac)
    finite = np.isfinite(grad).all() and np.isfinite(dz0).all() and np.isfinite(dlam0).all()
    if finite and (nsteps == 0 or (tie > TIE and kink > KINK and frac >= MIN_CLIPPED)):
      for a in list(case.values()) + [grad, dz0, dlam0]:
        if isinstance(a, np.ndarray):
          a.setflags(write=False)
      case["clipped"] = frac
      return case, grad, dz0, dlam0
  raise AssertionError(f"{name} {scheme} N={N} nsteps={nsteps}: no draw meets the tie and clip conditions (last: seed, tie, kink, clipped = {last})")


def rel_error(a, ref):
  """largest |a - ref| / max|ref| of the row over the instances of a case"""
  den = np.abs(ref).max(axis=-1)
  return float((np.abs(a - ref).max(axis=-1) / np.where(den > 0, den, 1.0)).max())


def build_twin(tmp_dir):
  """tests/hostsim/exgd_grad_twin.cpp -> tmp_dir/libexgd_grad_twin.so (g++ -O2 -std=c++17), loaded with ctypes"""
  import ctypes as C
  import subprocess
  out = os.path.join(str(tmp_dir), "libexgd_grad_twin.so")
  subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "hostsim", "exgd_grad_twin.cpp"), "-o", out], check=True)
  lib = C.CDLL(out)
  vp = C.c_void_p
  lib.exgd_grad_twin.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_int,
                                 vp, vp, vp, vp, vp]
  lib.exgd_grad_twin.restype = C.c_int
  return lib


def twin_grad(lib, name, scheme, N, T, z, lam, lb, ub, params, eta_x, eta_v, nsteps, seed_z, seed_lam=None):
  """ExgdGradPoint on the host over the batch: (grad [B][np], dz0 [B][n], dlam0 [B][m])"""
  from myriad_amd._lib import SYS_IDS
  z, lam, lb, ub, params, seed_z = (np.ascontiguousarray(a, dtype=np.float64) for a in (z, lam, lb, ub, params, seed_z))
  seed_lam = None if seed_lam is None else np.ascontiguousarray(seed_lam, dtype=np.float64)
  batch, npar = z.shape[0], params.shape[-1]
  grad, dz0, dlam0 = np.empty((batch, npar)), np.empty(z.shape), np.empty(lam.shape)
  rc = lib.exgd_grad_twin(SYS_IDS[name], SCHEMES.index(scheme), batch, N, float(T), z.ctypes.data, lam.ctypes.data, lb.ctypes.data, ub.ctypes.data,
                          params.ctypes.data, 0 if params.ndim == 1 else npar, float(eta_x), float(eta_v), int(nsteps), seed_z.ctypes.data,
                          None if seed_lam is None else seed_lam.ctypes.data, grad.ctypes.data, dz0.ctypes.data, dlam0.ctypes.data)
  assert rc == 0, f"exgd_grad_twin: no specialisation for {name} {scheme}"
  return grad, dz0, dlam0


def twin_of_case(lib, case):
  c = case
  return twin_grad(lib, c["name"], c["scheme"], c["N"], c["T"], c["z"], c["lam"], c["lb"], c["ub"], c["params"], c["eta_x"], c["eta_v"], c["nsteps"],
                   c["seed_z"], c["seed_lam"])
