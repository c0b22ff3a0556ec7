"""Reference Jacobians and the host twin shared by the tests of the forward-mode Jacobian of the unrolled extragradient steps
(test_exgd_jac_host_twin.py, test_gpu_exgd_jac.py).

A case is K10's (tests/exgd_grad_cases.py: `reference` -- the same draws, so its tie, kink and clipped-fraction conditions are asserted there).
The reference Jacobian is torch autograd through `oracle_run`, one backward pass per entry of (z_n, lam_n); for HIVTREATMENT, SEIR and TUMOUR,
whose constructors convert their arguments, central differences of the whole (z_n, lam_n) in each parameter.

The step of those differences is FD_STEP |p| = 3e-4 |p|, not K10's 1e-6 |p|: K10 differences ONE number, the seeded sum; here every entry of a
row must be resolved against the row's largest.  A central difference carries rounding noise eps |x| / (step |p|) and truncation of order
(step |p|)^2: TUMOUR's states are of order 1e4 beside derivative rows of order one, so that 1e-6 |p| leaves 4e-5 of noise, while at 3e-4 |p| both
parts stay below 3e-7 for the three systems (measured against the twin at steps 1e-6 ... 1e-3: the error falls as 1 / step down to 1e-4 and
rises as step^2 from 1e-3).  The bound stays FD_RTOL = 1e-6.
"""
import functools
import os

import numpy as np
import torch

import exgd_grad_cases as E

ROOT = E.ROOT
SCHEMES = E.SCHEMES
SYSTEMS = E.SYSTEMS
FD_SYSTEMS = E.FD_SYSTEMS
FD_RTOL = E.FD_RTOL
FD_STEP = 3e-4


def _run(c, b, prow, grad_params):
  return E.oracle_run(c["name"], c["scheme"], c["N"], c["T"], c["z"][b], c["lam"][b], c["lb"][b], c["ub"][b], prow, c["eta_x"], c["eta_v"], c["nsteps"],
                      grad_params)


@functools.lru_cache(maxsize=None)
def reference_jac(name, scheme, N=3, nsteps=3, batch=2):
  """(case, jz [B][np][n], jlam [B][np][m], zn [B][n], lamn [B][m]) of K10's draw of the case"""
  c = E.reference(name, scheme, N, nsteps, batch)[0]
  npar = c["params"].shape[1]
  jz, jlam = np.zeros((batch, npar, c["n"])), np.zeros((batch, npar, c["m"]))
  zn, lamn = np.empty((batch, c["n"])), np.empty((batch, c["m"]))
  for b in range(batch):
    if name in FD_SYSTEMS:
      xn, ln = _run(c, b, c["params"][b], False)[:2]
      zn[b], lamn[b] = xn.detach().numpy(), ln.detach().numpy()
      for k in range(npar):
        d = FD_STEP * abs(c["params"][b, k])
        side = []
        for sgn in (1.0, -1.0):
          p = c["params"][b].copy()
          p[k] += sgn * d
          xs, ls = _run(c, b, p, False)[:2]
          side.append((xs.detach().numpy(), ls.detach().numpy()))
        jz[b, k] = (side[0][0] - side[1][0]) / (2.0 * d)
        jlam[b, k] = (side[0][1] - side[1][1]) / (2.0 * d)
    else:
      xn, ln, (pt, _, _) = _run(c, b, c["params"][b], True)[:3]
      zn[b], lamn[b] = xn.detach().numpy(), ln.detach().numpy()
      for out, dst in ((xn, jz), (ln, jlam)):
        for i in range(out.numel()):
          if not out[i].requires_grad:                 # (an entry no parameter reaches: a pinned variable after zero steps)
            continue
          gs = torch.autograd.grad(out[i], pt, retain_graph=True, allow_unused=True)
          dst[b, :, i] = [0.0 if g is None else float(g) for g in gs]
  for a in (jz, jlam, zn, lamn):
    a.setflags(write=False)
  return c, jz, jlam, zn, lamn


def rel_error_rows(a, ref):
  """largest |a - ref| / max|ref| of a row [.., row], over the instances and the parameters; a zero reference row must be met exactly"""
  den = np.abs(ref).max(axis=-1)
  return float((np.abs(a - ref).max(axis=-1) / np.where(den > 0, den, 1.0)).max())


def build_twin(tmp_dir):
  """tests/hostsim/exgd_jac_twin.cpp -> tmp_dir/libexgd_jac_twin.so (g++ -O2 -std=c++17), loaded with ctypes"""
  import ctypes as C
  import subprocess
  out = os.path.join(str(tmp_dir), "libexgd_jac_twin.so")
  subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tests", "hostsim", "exgd_jac_twin.cpp"), "-o", out], check=True)
  lib = C.CDLL(out)
  vp = C.c_void_p
  lib.exgd_jac_twin.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, vp, vp,
                                C.c_int, vp, vp, vp, vp]
  lib.exgd_jac_twin.restype = C.c_int
  return lib


def twin_jac(lib, name, scheme, N, T, z, lam, lb, ub, params, eta_x, eta_v, nsteps, jz0=None, jlam0=None, gcols=0):
  """ExgdJacPoint on the host over the batch: {"zn", "lamn", "jz" [B][np][n], "jlam" [B][np][m]}; gcols: columns to a group (0: all at once)"""
  from myriad_amd._lib import SYS_IDS
  z, lam, lb, ub, params = (np.ascontiguousarray(a, dtype=np.float64) for a in (z, lam, lb, ub, params))
  jz0, jlam0 = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (jz0, jlam0))
  batch, npar = z.shape[0], params.shape[-1]
  out = dict(zn=np.empty(z.shape), lamn=np.empty(lam.shape), jz=np.empty((batch, npar, z.shape[1])), jlam=np.empty((batch, npar, lam.shape[1])))
  rc = lib.exgd_jac_twin(SYS_IDS[name], SCHEMES.index(scheme), batch, N, float(T), z.ctypes.data, lam.ctypes.data, lb.ctypes.data, ub.ctypes.data,
                         params.ctypes.data, 0 if params.ndim == 1 else npar, float(eta_x), float(eta_v), int(nsteps),
                         None if jz0 is None else jz0.ctypes.data, None if jlam0 is None else jlam0.ctypes.data, int(gcols),
                         out["zn"].ctypes.data, out["lamn"].ctypes.data, out["jz"].ctypes.data, out["jlam"].ctypes.data)
  assert rc == 0, f"exgd_jac_twin: no specialisation for {name} {scheme}"
  return out


def twin_of_case(lib, case, **kw):
  c = case
  a = dict(nsteps=c["nsteps"])
  a.update(kw)
  return twin_jac(lib, c["name"], c["scheme"], c["N"], c["T"], c["z"], c["lam"], c["lb"], c["ub"], c["params"], c["eta_x"], c["eta_v"], **a)


def seeded(case, out):
  """seed_z . jz[k] + seed_lam . jlam[k]: what K10's grad[k] is, [B][np]"""
  return np.einsum("bi,bki->bk", case["seed_z"], out["jz"]) + np.einsum("bi,bki->bk", case["seed_lam"], out["jlam"])


# ---- the Levenberg-Marquardt driver's case (myriad_amd/experiments/e2e_sysid.py: run_endtoend_gn) -------------------------------------------
DRIVER = dict(system="CANCERTREATMENT", scheme="TRAPEZOIDAL", N=10, nsteps=10)
DRIVER_COND = 1.97           # cond(J) at p*, measured with the twin (J: sqrt(w) o d u_n / d (r, delta), 11 x 2)
DRIVER_RTOL = 1e-10 * DRIVER_COND


def driver_case():
  """(hp, inputs) of the zero-residual problem: the optimizer's guess, bounds and step sizes from the oracle's transcription, the fitted keys
  (param_guesses), the system's true values of them and the start, param_guesses perturbed by 5 %"""
  from myriad_amd.config import HParams, OptimizerType, QuadratureRule
  from myriad_amd.defaults import learning_rates, param_guesses
  from myriad_amd.systems import SystemType
  d = DRIVER
  st = getattr(SystemType, d["system"])
  hp = HParams(system=st, optimizer=OptimizerType.COLLOCATION, quadrature_rule=getattr(QuadratureRule, d["scheme"]), intervals=d["N"])
  system = hp.system()
  sysm = E.O.SYSTEMS[d["system"]]()
  tr = E.O.make_transcription(sysm, "COLLOCATION", d["N"], quadrature_rule=d["scheme"])
  lr = learning_rates.get(st, {})
  names = tuple(system.param_names)
  keys = list(param_guesses[st])
  return hp, dict(system=system, names=names, keys=keys, T=float(sysm.T), rows=d["N"] + 1, nu=sysm.nu,
                  z0=tr.guess[None].copy(), lb=tr.bounds[None, :, 0].copy(), ub=tr.bounds[None, :, 1].copy(), lam0=np.zeros((1, d["N"] * sysm.ns)),
                  eta_x=float(lr.get("eta_x", hp.eta_x)), eta_v=float(lr.get("eta_v", hp.eta_lmbda)),
                  true={k: float(system.device_params()[names.index(k)]) for k in keys},
                  start={k: 1.05 * float(v) for k, v in param_guesses[st].items()})


def twin_driver_run(lib, case, params):
  """one evaluation of the driver's residual on the twin: {"zn", "jz"} with split_params' names and signs, as TrajectoryOptimizer.unrolled_jacobian"""
  from myriad_amd.experiments.mle_sysid import split_params
  c, d = case, DRIVER
  p, sign = split_params(c["system"], params)
  out = twin_jac(lib, d["system"], d["scheme"], d["N"], c["T"], c["z0"], c["lam0"], c["lb"], c["ub"], p, c["eta_x"], c["eta_v"], d["nsteps"])
  out["jz"] = out["jz"] * np.asarray(sign)[None, :, None]
  return out
