"""ctypes binding of libmyriad_hip.so (C-ABI: include/myriad_hip.h).

The product path has no CPU fallback: if the HIP library is missing or no MI355X is visible, the
calls raise -- they never route to the oracle or to any host implementation.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MYRIAD_HIP_LIB") or os.path.join(_HERE, "libmyriad_hip.so")   # override: development builds

SYS_IDS = {"CARTPOLE": 0, "VANDERPOL": 1, "CANCERTREATMENT": 2, "SIMPLECASE": 3, "NODE_CARTPOLE": 4, "BIOREACTOR": 5,
           "GLUCOSE": 6, "MOULDFUNGICIDE": 7, "SIMPLECASEWITHBOUNDS": 8, "HIVTREATMENT": 9, "EPIDEMICSEIRN": 10, "SEIR": 11,
           "BEARPOPULATIONS": 12, "PENDULUM": 13, "MOUNTAINCAR": 14, "ROCKETLANDING": 15,
           "BACTERIA": 16, "TUMOUR": 17, "HARVEST": 18, "TIMBERHARVEST": 19, "PREDATORPREY": 20,
           "INVASIVEPLANT": 21,   # INVASIVEPLANT: discrete-time, myr_fbsm only
           "PENDULUM_ELASTIC": 113, "ROCKETLANDING_ELASTIC": 115, "CARTPOLE_ELASTIC": 100, "VANDERPOL_ELASTIC": 101, "MOUNTAINCAR_ELASTIC": 114}   # elastic twins (slack controls on the dynamics), see include/myriad_hip.h
TR_IDS = {"HERMITE_SIMPSON": 0, "TRAPEZOIDAL": 1, "SHOOTING": 2}
INT_IDS = {"EULER": 0, "HEUN": 1, "MIDPOINT": 2, "RK4": 3}
MEM_HOST, MEM_DEVICE = 0, 1
K_EVAL, K_SOLVE, K_ROLLOUT, K_RESID, K_PROD, K_FBSM, K_FIT, K_HVP_NODE, K_HVP_NODE_SHOOT = 0, 1, 2, 3, 4, 5, 6, 7, 8
STATUS_NAMES = {0: "CONVERGED", 1: "MAXITER", 2: "NAN", 3: "STALLED", 4: "INFEASIBLE"}
STATUS_INFEASIBLE = 4   # assigned by the library's restoration phase inside myr_solve (csrc/myriad_hip.hip: solve_restored), never by a kernel


class ProblemDesc(C.Structure):
  _fields_ = [("system_id", C.c_int32), ("transcription", C.c_int32), ("integration_method", C.c_int32),
              ("intervals", C.c_int32), ("controls_per_interval", C.c_int32), ("device", C.c_int32),
              ("max_batch", C.c_int32), ("reserved", C.c_int32), ("T", C.c_double)]


class Dims(C.Structure):
  _fields_ = [("n", C.c_int32), ("m", C.c_int32), ("ns", C.c_int32), ("nu", C.c_int32), ("np", C.c_int32),
              ("x_rows", C.c_int32), ("u_rows", C.c_int32), ("jblk", C.c_int32), ("ngrad", C.c_int32),
              ("reserved", C.c_int32)]


class SolveOpts(C.Structure):
  _fields_ = [("max_iter", C.c_int32), ("restarts", C.c_int32), ("tol_feas", C.c_double),
              ("tol_stat", C.c_double), ("tol_compl", C.c_double), ("mu_init", C.c_double),
              ("restoration", C.c_int32), ("park_iter", C.c_int32)]


class MyriadHipError(RuntimeError):
  pass


# The C-ABI (include/myriad_hip.h): exported function -> (argument types, return type).  load() declares every function from this table, and
# __graft_entry__.build() checks the built library against its names (EXPORTS).
_i, _f, _p = C.c_int32, C.c_double, C.c_void_p      # _p: the handle, and raw addresses (host numpy or device pointers)
_opts = C.POINTER(SolveOpts)
_EXGD_GRAD_TAIL = [_f, _f, _i, _p, _p, _p, _i, _p, _p, _i]      # eta_x, eta_v, nsteps, seed_z, seed_lam, grad, grad_stride, dz0, dlam0, mem
_HVP_TAIL = [_i, _p, _p, _i, _i]                                # with_cost, out_z, out_p, p_stride, mem
_SIGNATURES = {
  "myr_create": ([C.POINTER(ProblemDesc), C.POINTER(C.c_void_p)], C.c_int),
  "myr_destroy": ([_p], C.c_int),
  "myr_get_dims": ([_p, C.POINTER(Dims)], C.c_int),
  "myr_default_solve_opts": ([_opts], None),
  "myr_device_count": ([], C.c_int),
  "myr_eval": ([_p, _i, _p, _p, _i, _p, _p, _p, _p, _i], C.c_int),
  "myr_solve": ([_p, _i, _p, _p, _p, _p, _i, _opts, _p, _p, _p, _p, _p, _i], C.c_int),
  "myr_solve_x0": ([_p, _i, _p, _p, _p, _p, _p, _p, _i, _opts, _p, _p, _p, _p, _p, _p, _i], C.c_int),
  "myr_solve_info": ([_p, _i, _p, _p, _p], C.c_int),
  "myr_solve_plan": ([_p, _p], C.c_int),
  "myr_rollout": ([_p, _i, _i, _i, _p, _p, _p, _i, _p, _p, _i], C.c_int),
  "myr_fit_grad": ([_p, _i, _i, _i, _p, _p, _p, _p, _i, _p, _p, _i, _i], C.c_int),
  "myr_fit_grad_sets": ([_p, _i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _i, _i], C.c_int),
  "myr_fit_gn": ([_p, _i, _i, _i, _p, _p, _p, _p, _i, _p, _p, _p, _i, _i], C.c_int),
  "myr_fit_gn_sets": ([_p, _i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i, _i], C.c_int),
  "myr_fit_gnvp": ([_p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _i, _i], C.c_int),
  "myr_fit_gnvp_sets": ([_p, _i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i, _i], C.c_int),
  "myr_set_var_scale": ([_p, _p], C.c_int),
  "myr_vjp": ([_p, _i, _p, _p, _p, _i, _p, _i, _i], C.c_int),
  "myr_jvp": ([_p, _i, _p, _p, _p, _i, _p, _i], C.c_int),
  "myr_exgd": ([_p, _i, _p, _p, _p, _p, _p, _i, _f, _f, _i, _i], C.c_int),
  "myr_exgd_grad": ([_p, _i, _p, _p, _p, _p, _p, _i] + _EXGD_GRAD_TAIL, C.c_int),
  "myr_exgd_grad_shoot": ([_p, _i, _p, _p, _p, _p, _p, _i] + _EXGD_GRAD_TAIL, C.c_int),
  "myr_exgd_grad_node": ([_p, _i, _p, _p, _p, _p, _p] + _EXGD_GRAD_TAIL, C.c_int),
  "myr_exgd_grad_node_shoot": ([_p, _i, _p, _p, _p, _p, _p] + _EXGD_GRAD_TAIL, C.c_int),
  "myr_exgd_grad_node_sets": ([_p, _i, _i, _p, _p, _p, _p, _p] + _EXGD_GRAD_TAIL, C.c_int),
  "myr_exgd_jac": ([_p, _i, _p, _p, _p, _p, _p, _i, _f, _f, _i, _p, _p, _p, _p, _p, _p, _i], C.c_int),
  "myr_hvp": ([_p, _i, _p, _p, _p, _p, _i] + _HVP_TAIL, C.c_int),
  "myr_hvp_node": ([_p, _i, _p, _p, _p, _p] + _HVP_TAIL, C.c_int),
  "myr_hvp_node_sets": ([_p, _i, _i, _p, _p, _p, _p] + _HVP_TAIL, C.c_int),
  "myr_fbsm": ([_p, _i, _i, _p, _p, _p, _i, _p, _p, _f, _f, _i, _p, _p, _p, _p, _i], C.c_int),
  "myr_kernel_time": ([_p, _i, C.POINTER(C.c_double), C.POINTER(C.c_int32)], C.c_int),
  "myr_kernel_time_reset": ([_p], C.c_int),
  "myr_last_error": ([], C.c_char_p),
  "myr_version": ([], C.c_char_p),
  "myr_abi_sizeof": ([_i], C.c_int32),
}
EXPORTS = list(_SIGNATURES)


_lib = None


def load() -> C.CDLL:
  """Load the HIP library; raise loudly when it has not been built (python __graft_entry__.py build)."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise MyriadHipError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
                         "There is no CPU fallback.")
  # PyTorch-ROCm ships its own HIP runtime.  If this library brought the system runtime in first, a later torch.cuda
  # initialisation in the same process reports "No HIP GPUs are available"; loading torch's libraries first makes one
  # runtime serve both (torch is optional: nothing else here uses it).
  if "torch" not in sys.modules and os.environ.get("MYRIAD_NO_TORCH_PRELOAD") is None:
    try:
      import torch  # noqa: F401
    except Exception:
      pass
  lib = C.CDLL(LIB_PATH)
  # ABI guard: the structs have no size field; a library built from another header would read past (or short of) ours
  lib.myr_version.restype = C.c_char_p
  if not hasattr(lib, "myr_abi_sizeof"):
    raise MyriadHipError(f"{LIB_PATH} ({lib.myr_version().decode()}) predates myr_abi_sizeof: rebuild it (python __graft_entry__.py build)")
  for name, (argtypes, restype) in _SIGNATURES.items():
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = argtypes, restype
  for which, st in ((0, SolveOpts), (1, ProblemDesc), (2, Dims)):
    if lib.myr_abi_sizeof(which) != C.sizeof(st):
      raise MyriadHipError(f"{LIB_PATH} ({lib.myr_version().decode()}): {st.__name__} is {lib.myr_abi_sizeof(which)} bytes in the library, "
                           f"{C.sizeof(st)} in this binding -- library and binding come from different headers")
  _lib = lib
  return lib


def _chk(rc: int, what: str):
  if rc != 0:
    msg = load().myr_last_error().decode()
    if rc == -2:
      raise NotImplementedError(f"{what}: {msg}")
    if rc == -1:
      raise ValueError(f"{what}: {msg}")
    raise MyriadHipError(f"{what} failed ({rc}): {msg}")


def _addr(a) -> Optional[int]:
  """Address of a numpy array (host) or of anything exposing data_ptr() (torch device tensor); None -> NULL."""
  if a is None:
    return None
  if isinstance(a, np.ndarray):
    return a.ctypes.data
  if hasattr(a, "data_ptr"):
    return a.data_ptr()
  if isinstance(a, int):
    return a
  raise TypeError(type(a))


def _f64(a, shape=None):
  a = np.ascontiguousarray(a, dtype=np.float64)
  if shape is not None and tuple(a.shape) != tuple(shape):
    raise ValueError(f"expected shape {shape}, got {a.shape}")
  return a


def device_count() -> int:
  """Devices the library can create handles on (0 without a GPU)."""
  return int(load().myr_device_count())


class Engine:
  """One handle = one (system, transcription, sizes, device) problem family; owns device scratch and a stream."""

  def __init__(self, system: str, transcription: str, intervals: int, T: float, controls_per_interval: int = 1,
               integration_method: str = "HEUN", device: int = 0, max_batch: int = 4096):
    self.lib = load()
    d = ProblemDesc(SYS_IDS[system], TR_IDS[transcription], INT_IDS[integration_method], int(intervals),
                    int(controls_per_interval), int(device), int(max_batch), 0, float(T))
    self._h = C.c_void_p()
    _chk(self.lib.myr_create(C.byref(d), C.byref(self._h)), "myr_create")
    dm = Dims()
    _chk(self.lib.myr_get_dims(self._h, C.byref(dm)), "myr_get_dims")
    self.dims = dm
    self.desc = d
    for k in ("n", "m", "ns", "nu", "np", "x_rows", "u_rows", "jblk", "ngrad"):
      setattr(self, k, int(getattr(dm, k)))

  def close(self):
    if getattr(self, "_h", None) and self._h.value:
      self.lib.myr_destroy(self._h)
      self._h = C.c_void_p()

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  # ---- host (numpy) entry points -------------------------------------------------------------
  def _params(self, params, B):
    if params is None:
      return None, 0
    p = _f64(params)
    if p.ndim == 1:
      if p.shape[0] != self.np:
        raise ValueError("params must have np entries")
      return p, 0
    if p.shape != (B, self.np):
      raise ValueError(f"params must be [B,{self.np}]")
    return p, self.np

  def eval(self, z, params=None, want=("f", "gradf", "c", "jblk")):
    z = _f64(z)
    if z.ndim == 1:
      z = z[None]
    B = z.shape[0]
    if z.shape[1] != self.n:
      raise ValueError(f"z must be [B,{self.n}]")
    p, ps = self._params(params, B)
    out = {"f": np.empty(B) if "f" in want else None,
           "gradf": np.empty((B, self.ngrad)) if "gradf" in want else None,
           "c": np.empty((B, self.m)) if "c" in want else None,
           "jblk": np.empty((B, self.jblk)) if "jblk" in want else None}
    _chk(self.lib.myr_eval(self._h, B, _addr(z), _addr(p), ps, _addr(out["f"]), _addr(out["gradf"]),
                           _addr(out["c"]), _addr(out["jblk"]), MEM_HOST), "myr_eval")
    return {k: v for k, v in out.items() if v is not None}

  def eval_device(self, B, z, params=None, params_stride=0, f=None, gradf=None, c=None, jblk=None):
    """Zero-copy variant: every argument is a device tensor (anything with data_ptr()) on this handle's device."""
    _chk(self.lib.myr_eval(self._h, int(B), _addr(z), _addr(params), int(params_stride), _addr(f), _addr(gradf),
                           _addr(c), _addr(jblk), MEM_DEVICE), "myr_eval")

  def default_opts(self) -> SolveOpts:
    o = SolveOpts()
    self.lib.myr_default_solve_opts(C.byref(o))
    return o

  def set_var_scale(self, scale=None):
    """Variable scales [ns+nu] of the solve path (None = unscaled); see include/myriad_hip.h, myr_set_var_scale."""
    if scale is None:
      _chk(self.lib.myr_set_var_scale(self._h, None), "myr_set_var_scale")
      return
    s = _f64(scale)
    if s.shape != (self.ns + self.nu,):
      raise ValueError(f"scale must have ns+nu = {self.ns + self.nu} entries")
    _chk(self.lib.myr_set_var_scale(self._h, _addr(s)), "myr_set_var_scale")

  # Result arrays of solve / solve_x0: fresh numpy arrays per call by default.  A caller that solves batch after batch sets
  # `result_buffers` to a dict of its own arrays ("z" [B,n], "lam" [B,m], "cost" [B], "status" int32 [B], "iters" int32 [B],
  # "kkt" [B,3] -- e.g. views of pinned memory); a call whose batch size matches writes its results there (no allocation, no
  # page faults) and returns views of them, valid until the next call.
  result_buffers = None

  def _results(self, B, z=None):
    rb = self.result_buffers
    if rb is not None and rb["cost"].shape[0] == B:
      if z is not None:
        rb["z"][...] = z
      return rb["z"], rb["lam"], rb["cost"], rb["status"], rb["iters"], rb["kkt"]
    return (np.empty((B, self.n)) if z is None else z, np.empty((B, self.m)), np.empty(B), np.empty(B, dtype=np.int32),
            np.empty(B, dtype=np.int32), np.empty((B, 3)))

  def solve(self, z0, lb, ub, params=None, opts: Optional[SolveOpts] = None):
    z = _f64(z0)
    if z.ndim == 1:
      z = z[None]
    B = z.shape[0]
    if not (self.result_buffers is not None and self.result_buffers["cost"].shape[0] == B):
      z = z.copy()
    lb = np.ascontiguousarray(np.broadcast_to(_f64(lb), z.shape))
    ub = np.ascontiguousarray(np.broadcast_to(_f64(ub), z.shape))
    p, ps = self._params(params, B)
    o = opts or self.default_opts()
    z, lam, cost, status, iters, kkt = self._results(B, z)
    _chk(self.lib.myr_solve(self._h, B, _addr(z), _addr(lb), _addr(ub), _addr(p), ps, C.byref(o), _addr(lam),
                            _addr(cost), _addr(status), _addr(iters), _addr(kkt), MEM_HOST), "myr_solve")
    return self._with_info({"z": z, "lam": lam, "cost": cost, "status": status, "iters": iters, "kkt": kkt}, B)

  def _with_info(self, res, B):
    """myr_solve_info: which start produced each instance (restoration inside the library, include/myriad_hip.h)"""
    start = np.empty(B, dtype=np.int32); attempts = np.empty(B, dtype=np.int32); restored = np.empty(B, dtype=np.int32)
    _chk(self.lib.myr_solve_info(self._h, B, _addr(start), _addr(attempts), _addr(restored)), "myr_solve_info")
    res["start"] = start; res["attempts"] = attempts; res["restored"] = restored
    return res

  def solve_x0(self, x0s, g0, g1, lb, ub, params=None, opts: Optional[SolveOpts] = None):
    """myr_solve_x0: the instances differ in their start state only; guess and bounds are expanded on the device
    (z0[b] = g0 + g1 * tile(x0s[b]) on the state rows, lb/ub [n] with the first point pinned to x0s[b])."""
    x0s = np.ascontiguousarray(_f64(x0s))
    if x0s.ndim == 1:
      x0s = x0s[None]
    B = x0s.shape[0]
    if x0s.shape[1] != self.ns:
      raise ValueError(f"x0s must be [B,{self.ns}]")
    tpl = [np.ascontiguousarray(_f64(a)).reshape(-1) for a in (g0, g1, lb, ub)]
    if any(a.shape[0] != self.n for a in tpl):
      raise ValueError(f"g0, g1, lb, ub must have {self.n} entries")
    p, ps = self._params(params, B)
    o = opts or self.default_opts()
    z, lam, cost, status, iters, kkt = self._results(B)
    _chk(self.lib.myr_solve_x0(self._h, B, _addr(x0s), _addr(tpl[0]), _addr(tpl[1]), _addr(tpl[2]), _addr(tpl[3]), _addr(p), ps,
                               C.byref(o), _addr(z), _addr(lam), _addr(cost), _addr(status), _addr(iters), _addr(kkt), MEM_HOST), "myr_solve_x0")
    return self._with_info({"z": z, "lam": lam, "cost": cost, "status": status, "iters": iters, "kkt": kkt}, B)

  def solve_device(self, B, z, lb, ub, params, params_stride, opts, lam, cost, status, iters, kkt=None):
    _chk(self.lib.myr_solve(self._h, int(B), _addr(z), _addr(lb), _addr(ub), _addr(params), int(params_stride),
                            C.byref(opts), _addr(lam), _addr(cost), _addr(status), _addr(iters), _addr(kkt),
                            MEM_DEVICE), "myr_solve")

  def rollout(self, x0, us, num_steps, params=None, want_xs=True):
    x0 = _f64(x0)
    us = _f64(us)
    if x0.ndim == 1:
      x0 = x0[None]
    if us.ndim == 2:
      us = us[None]
    B = x0.shape[0]
    p, ps = self._params(params, B)
    xs = np.empty((B, num_steps + 1, self.ns)) if want_xs else None
    cost = np.empty(B)
    _chk(self.lib.myr_rollout(self._h, B, int(num_steps), int(us.shape[1]), _addr(x0), _addr(us), _addr(p), ps,
                              _addr(xs), _addr(cost), MEM_HOST), "myr_rollout")
    return xs, cost

  # ---- trajectory-matching fit: myr_fit_grad, myr_fit_gn and their _sets forms ------------------------------------
  def _fit_call(self, call, mem, B, num_steps, u_rows, xs_obs, us, wt, params, params_stride, outs, row_stride):
    """the C call of the single-set pair: `outs` is (loss, grad) for myr_fit_grad, (loss, grad, gn) for myr_fit_gn; the arrays are host or device
    ones, as `mem` says"""
    _chk(getattr(self.lib, call)(self._h, int(B), int(num_steps), int(u_rows), _addr(xs_obs), _addr(us), _addr(wt), _addr(params), int(params_stride),
                                 *map(_addr, outs), int(row_stride), mem), call)

  def _fit_sets_call(self, call, mem, E, R, num_steps, u_rows, xs_obs, us, data_shared, wt, params, outs, row_stride):
    """... and of the sets pair (myr_fit_grad_sets, myr_fit_gn_sets)"""
    _chk(getattr(self.lib, call)(self._h, int(E), int(R), int(num_steps), int(u_rows), _addr(xs_obs), _addr(us), int(data_shared), _addr(wt),
                                 _addr(params), *map(_addr, outs), int(row_stride), mem), call)

  def _fit_data(self, xs_obs, us):
    """the data of a single-set fit call: (xs_obs [B,S+1,ns], us [B,u_rows,nu], B, S); one trajectory may come without its batch axis"""
    xs_obs, us = _f64(xs_obs), _f64(us)
    if xs_obs.ndim == 2:
      xs_obs = xs_obs[None]
    if us.ndim == 2:
      us = us[None]
    B, S = xs_obs.shape[0], xs_obs.shape[1] - 1
    if xs_obs.ndim != 3 or xs_obs.shape[2] != self.ns or S < 1:
      raise ValueError(f"xs_obs must be [B,S+1,{self.ns}] with S >= 1")
    if us.ndim != 3 or us.shape[0] != B or us.shape[2] != self.nu:
      raise ValueError(f"us must be [B,u_rows,{self.nu}]")
    return xs_obs, us, B, S

  def _fit_sets_data(self, xs_obs, us, params):
    """... and of a sets call: (xs_obs, us, params [E,np], E, R, S, shared) -- the data [E,R,...], or [R,...] read by every set"""
    xs_obs, us, params = _f64(xs_obs), _f64(us), _f64(params)
    if params.ndim != 2 or params.shape[1] != self.np:
      raise ValueError(f"params must be [E,{self.np}]")
    E = params.shape[0]
    if xs_obs.ndim not in (3, 4) or us.ndim != xs_obs.ndim:
      raise ValueError("xs_obs and us must both be [E,R,...] (data per set) or both [R,...] (data shared by the sets)")
    shared = xs_obs.ndim == 3
    lead = () if shared else (E,)
    R, S = xs_obs.shape[-3], xs_obs.shape[-2] - 1
    if xs_obs.shape[:-3] != lead or xs_obs.shape[-1] != self.ns or S < 1 or R < 1:
      raise ValueError(f"xs_obs must be [{'' if shared else 'E,'}R,S+1,{self.ns}] with R >= 1, S >= 1 and E = {E} as in params")
    if us.shape[:-2] != lead + (R,) or us.shape[-1] != self.nu or us.shape[-2] < 1:
      raise ValueError(f"us must be [{'' if shared else 'E,'}R,u_rows,{self.nu}]")
    return xs_obs, us, params, E, R, S, shared

  def _fit(self, call, with_gn, xs_obs, us, params, wt, reduce):
    """fit_grad and fit_gn: the shape rules they share, the result arrays and the call"""
    xs_obs, us, B, S = self._fit_data(xs_obs, us)
    p, ps = self._params(params, B)
    w = None if wt is None else _f64(wt, (S + 1,))
    lead = () if reduce else (B,)
    loss, grad = np.empty(B), np.empty(lead + (self.np,))
    gn = np.empty(lead + (self.np, self.np)) if with_gn else None
    self._fit_call(call, MEM_HOST, B, S, us.shape[1], xs_obs, us, w, p, ps, (loss, grad, gn)[:3 if with_gn else 2], 0 if reduce else self.np)
    return self._present(loss=loss, grad=grad, gn=gn)

  def _fit_sets(self, call, with_gn, xs_obs, us, params, wt, reduce, want_grad):
    """fit_grad_sets and fit_gn_sets: the same for E parameter sets"""
    xs_obs, us, params, E, R, S, shared = self._fit_sets_data(xs_obs, us, params)
    w = None if wt is None else _f64(wt, (S + 1,))
    out = (E,) if reduce else (E, R)
    loss = np.empty((E, R))
    grad = np.empty(out + (self.np,)) if want_grad else None
    gn = np.empty(out + (self.np, self.np)) if with_gn else None
    self._fit_sets_call(call, MEM_HOST, E, R, S, us.shape[-2], xs_obs, us, shared, w, params, (loss, grad, gn)[:3 if with_gn else 2],
                        0 if reduce else self.np)
    return self._present(loss=loss, grad=grad, gn=gn)

  def fit_grad(self, xs_obs, us, params=None, wt=None, reduce=False):
    """myr_fit_grad: trajectory-matching loss and its gradient in the model parameters.  xs_obs [B,S+1,ns] (recorded states; the
    rollout starts from xs_obs[:,0]), us [B,u_rows,nu], params [np] (shared) or [B,np] (None: the system's defaults), wt [S+1]
    (None: 1).  Returns {"loss" [B], "grad" [B,np], or [np] = the sum over the batch with reduce=True}."""
    return self._fit("myr_fit_grad", False, xs_obs, us, params, wt, reduce)

  def fit_grad_device(self, B, num_steps, u_rows, xs_obs, us, grad, grad_stride, params=None, params_stride=0, wt=None, loss=None):
    """Zero-copy variant of fit_grad: every array is a device tensor on this handle's device."""
    self._fit_call("myr_fit_grad", MEM_DEVICE, B, num_steps, u_rows, xs_obs, us, wt, params, params_stride, (loss, grad), grad_stride)

  def fit_grad_sets(self, xs_obs, us, params, wt=None, reduce=False, want_grad=True):
    """myr_fit_grad_sets: fit_grad for E independent parameter sets of R trajectories each in one call.  params [E,np]; xs_obs [E,R,S+1,ns] and
    us [E,R,u_rows,nu], or [R,S+1,ns] and [R,u_rows,nu]: one set of data that every parameter set reads; wt [S+1] (None: 1), shared by all sets.
    Returns {"loss" [E,R], "grad" [E,R,np], or [E,np] = per set the sum over its trajectories with reduce=True}; want_grad=False: the loss only
    (no reverse sweep, no "grad").  Set e has the bits of fit_grad on that set alone."""
    return self._fit_sets("myr_fit_grad_sets", False, xs_obs, us, params, wt, reduce, want_grad)

  def fit_grad_sets_device(self, E, R, num_steps, u_rows, xs_obs, us, params, grad=None, grad_stride=0, data_shared=False, wt=None, loss=None):
    """Zero-copy variant of fit_grad_sets: every array is a device tensor on this handle's device; grad=None: the loss only."""
    self._fit_sets_call("myr_fit_grad_sets", MEM_DEVICE, E, R, num_steps, u_rows, xs_obs, us, data_shared, wt, params, (loss, grad), grad_stride)

  def fit_gn(self, xs_obs, us, params=None, wt=None, reduce=False):
    """myr_fit_gn: fit_grad's loss and gradient with the Gauss-Newton matrix gn = 2 J^T W J of the fit (J: the sensitivity of the rolled-out
    states in the parameters), by one forward pass.  Arguments as fit_grad.  Returns {"loss" [B], "grad" [B,np], "gn" [B,np,np]}; with
    reduce=True "grad" [np] and "gn" [np,np] are the sums over the batch."""
    return self._fit("myr_fit_gn", True, xs_obs, us, params, wt, reduce)

  def fit_gn_device(self, B, num_steps, u_rows, xs_obs, us, gn, out_stride, params=None, params_stride=0, wt=None, loss=None, grad=None):
    """Zero-copy variant of fit_gn: every array is a device tensor on this handle's device (loss, grad may be None)."""
    self._fit_call("myr_fit_gn", MEM_DEVICE, B, num_steps, u_rows, xs_obs, us, wt, params, params_stride, (loss, grad, gn), out_stride)

  def fit_gn_sets(self, xs_obs, us, params, wt=None, reduce=False):
    """myr_fit_gn_sets: fit_gn for E independent parameter sets of R trajectories each in one call; arguments as fit_grad_sets.  Returns
    {"loss" [E,R], "grad" [E,R,np], "gn" [E,R,np,np]}; with reduce=True "grad" [E,np] and "gn" [E,np,np] are, per set, the sums over its
    trajectories.  Set e has the bits of fit_gn on that set alone."""
    return self._fit_sets("myr_fit_gn_sets", True, xs_obs, us, params, wt, reduce, True)

  def fit_gn_sets_device(self, E, R, num_steps, u_rows, xs_obs, us, params, gn, out_stride=0, data_shared=False, wt=None, loss=None, grad=None):
    """Zero-copy variant of fit_gn_sets: every array is a device tensor on this handle's device (loss, grad may be None)."""
    self._fit_sets_call("myr_fit_gn_sets", MEM_DEVICE, E, R, num_steps, u_rows, xs_obs, us, data_shared, wt, params, (loss, grad, gn), out_stride)

  # ---- the Gauss-Newton product of the network fit: myr_fit_gnvp and its _sets form ------------------------------------------------
  def fit_gnvp(self, xs_obs, us, params, v, wt=None, reduce=False, want_jv=False, want_out=True):
    """myr_fit_gnvp: the Gauss-Newton matrix of the network fit times a direction, without the matrix.  xs_obs [B,S+1,ns] (only the start states
    xs_obs[:,0] are read), us [B,u_rows,nu], params [np], v [np], wt [S+1] (None: 1).  Returns {"out" [B,np] = fit_gn's gn[b] @ v, or [np] = the
    sum over the batch with reduce=True}; want_jv=True adds "jv" [B,S+1,ns], the tangent of the rolled-out states along v; want_out=False: the
    forward tangent only (no "out")."""
    xs_obs, us, B, S = self._fit_data(xs_obs, us)
    params, v = _f64(params, (self.np,)), _f64(v, (self.np,))
    w = None if wt is None else _f64(wt, (S + 1,))
    jv = np.empty((B, S + 1, self.ns)) if want_jv else None
    out = np.empty((() if reduce else (B,)) + (self.np,)) if want_out else None
    self.fit_gnvp_device(B, S, us.shape[1], xs_obs, us, params, v, jv=jv, out=out, out_stride=0 if reduce else self.np, wt=w, mem=MEM_HOST)
    return self._present(out=out, jv=jv)

  def fit_gnvp_device(self, B, num_steps, u_rows, xs_obs, us, params, v, jv=None, out=None, out_stride=0, wt=None, mem=MEM_DEVICE):
    """Zero-copy variant of fit_gnvp: every array is a device tensor on this handle's device (jv or out may be None, not both)."""
    _chk(self.lib.myr_fit_gnvp(self._h, int(B), int(num_steps), int(u_rows), _addr(xs_obs), _addr(us), _addr(wt), _addr(params), _addr(v), _addr(jv),
                               _addr(out), int(out_stride), mem), "myr_fit_gnvp")

  def fit_gnvp_sets(self, xs_obs, us, params, v, wt=None, reduce=False, want_jv=False, want_out=True):
    """myr_fit_gnvp_sets: fit_gnvp for E weight sets of R trajectories each in one call.  params [E,np], v [E,np] (a direction per set); xs_obs, us
    as in fit_grad_sets ([E,R,...], or [R,...] read by every set).  Returns {"out" [E,R,np], or [E,np] with reduce=True; "jv" [E,R,S+1,ns] with
    want_jv=True}.  Set e has the bits of fit_gnvp on that set alone."""
    xs_obs, us, params, E, R, S, shared = self._fit_sets_data(xs_obs, us, params)
    v = _f64(v, (E, self.np))
    w = None if wt is None else _f64(wt, (S + 1,))
    jv = np.empty((E, R, S + 1, self.ns)) if want_jv else None
    out = np.empty(((E,) if reduce else (E, R)) + (self.np,)) if want_out else None
    self.fit_gnvp_sets_device(E, R, S, us.shape[-2], xs_obs, us, params, v, jv=jv, out=out, out_stride=0 if reduce else self.np, data_shared=shared,
                              wt=w, mem=MEM_HOST)
    return self._present(out=out, jv=jv)

  def fit_gnvp_sets_device(self, E, R, num_steps, u_rows, xs_obs, us, params, v, jv=None, out=None, out_stride=0, data_shared=False, wt=None,
                           mem=MEM_DEVICE):
    """Zero-copy variant of fit_gnvp_sets: every array is a device tensor on this handle's device (jv or out may be None, not both)."""
    _chk(self.lib.myr_fit_gnvp_sets(self._h, int(E), int(R), int(num_steps), int(u_rows), _addr(xs_obs), _addr(us), int(data_shared), _addr(wt),
                                    _addr(params), _addr(v), _addr(jv), _addr(out), int(out_stride), mem), "myr_fit_gnvp_sets")

  # ---- Lagrangian products / extragradient (collocation transcriptions) ------------------------
  def _batch2(self, a, width, name):
    a = _f64(a)
    if a.ndim == 1:
      a = a[None]
    if a.shape[1] != width:
      raise ValueError(f"{name} must be [B,{width}]")
    return a

  def vjp(self, z, lam, params=None, add_gradf=False):
    """J(z)^T lam (+ grad f(z) when add_gradf: the gradient of the Lagrangian in z), [B,n]."""
    z = self._batch2(z, self.n, "z"); lam = self._batch2(lam, self.m, "lam")
    B = z.shape[0]
    if lam.shape[0] != B:
      raise ValueError("z and lam must have the same batch size")
    p, ps = self._params(params, B)
    out = np.empty((B, self.n))
    _chk(self.lib.myr_vjp(self._h, B, _addr(z), _addr(lam), _addr(p), ps, _addr(out), int(bool(add_gradf)), MEM_HOST), "myr_vjp")
    return out

  def jvp(self, z, v, params=None):
    """J(z) v, [B,m]."""
    z = self._batch2(z, self.n, "z"); v = self._batch2(v, self.n, "v")
    B = z.shape[0]
    if v.shape[0] != B:
      raise ValueError("z and v must have the same batch size")
    p, ps = self._params(params, B)
    out = np.empty((B, self.m))
    _chk(self.lib.myr_jvp(self._h, B, _addr(z), _addr(v), _addr(p), ps, _addr(out), MEM_HOST), "myr_jvp")
    return out

  def exgd(self, z, lam, lb, ub, eta_x, eta_v, nsteps, params=None):
    """`nsteps` extragradient iterations; returns the new (z, lam)."""
    z = self._batch2(z, self.n, "z").copy(); lam = self._batch2(lam, self.m, "lam").copy()
    B = z.shape[0]
    lb = np.ascontiguousarray(np.broadcast_to(_f64(lb), z.shape))
    ub = np.ascontiguousarray(np.broadcast_to(_f64(ub), z.shape))
    p, ps = self._params(params, B)
    _chk(self.lib.myr_exgd(self._h, B, _addr(z), _addr(lam), _addr(lb), _addr(ub), _addr(p), ps, float(eta_x), float(eta_v),
                           int(nsteps), MEM_HOST), "myr_exgd")
    return z, lam

  # ---- the derivative family (myr_exgd_grad*, myr_hvp*): one C call, one host body, one probe for each of the two ------------------------------
  # `kind` says what `params` is: "rows" (a closed-form system: None, [np] or [B,np], passed with its stride), "shared" (the network system: its
  # 4 804 weights, no stride) or "sets" ([E,np] weight sets of R instances each: the arrays are [E,R,.] and the call takes E, R where the others take B)
  def _weights(self, params):
    p = None if params is None else np.ascontiguousarray(_f64(params))
    if p is not None and p.shape != (self.np,):
      raise ValueError(f"params must be the {self.np} shared weights")
    return p

  def _sets3(self, a, E, R, width, name):
    a = _f64(a)
    if a.shape != (E, R, width):
      raise ValueError(f"{name} must be [E = {E}, R = {R}, {width}]")
    return a

  def _weight_sets(self, params):
    p = np.ascontiguousarray(_f64(params))
    if p.ndim != 2 or p.shape[1] != self.np:
      raise ValueError(f"params must be [E,{self.np}]: a weight set per row")
    return p

  def _sets_z(self, z, E):
    z = _f64(z)
    if z.ndim != 3 or z.shape[0] != E or z.shape[1] < 1 or z.shape[2] != self.n:
      raise ValueError(f"z must be [E = {E}, R, {self.n}] with R >= 1")
    return z

  def _param_args(self, kind, params, B):
    """what the C call takes for `params`: (array, stride), or (array,) for the network calls"""
    return self._params(params, B) if kind == "rows" else (self._weights(params),)

  @staticmethod
  def _present(**arrays):
    return {k: v for k, v in arrays.items() if v is not None}

  def _exgd_grad_call(self, call, mem, sizes, z, lam, lb, ub, pargs, eta_x, eta_v, nsteps, seed_z, seed_lam, grad, grad_stride, dz0, dlam0):
    """the C call: `sizes` (B,) or (E, R), `pargs` as _param_args gives them; the arrays are host or device ones, as `mem` says"""
    _chk(getattr(self.lib, call)(self._h, *map(int, sizes), _addr(z), _addr(lam), _addr(lb), _addr(ub), _addr(pargs[0]), *map(int, pargs[1:]), float(eta_x),
                                 float(eta_v), int(nsteps), _addr(seed_z), _addr(seed_lam), _addr(grad), int(grad_stride), _addr(dz0), _addr(dlam0), mem), call)

  def _exgd_grad(self, call, kind, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, seed_lam, params, reduce, want_start):
    if kind == "sets":
      pargs = (self._weight_sets(params),)
      z = self._sets_z(z, pargs[0].shape[0])
      lead = z.shape[:2]
      lam = self._sets3(lam, *lead, self.m, "lam")
    else:
      z = self._batch2(z, self.n, "z"); lam = self._batch2(lam, self.m, "lam")
      lead = z.shape[:1]
      if lam.shape[0] != lead[0]:
        raise ValueError("z and lam must have the same batch size")
    lb, ub, sz = (np.ascontiguousarray(np.broadcast_to(_f64(a), z.shape)) for a in (lb, ub, seed_z))
    sl = None if seed_lam is None else np.ascontiguousarray(np.broadcast_to(_f64(seed_lam), lam.shape))
    if kind != "sets":
      pargs = self._param_args(kind, params, lead[0])
    grad = np.empty((lead[:-1] if reduce else lead) + (self.np,))      # reduce: a row for the batch, or a row per set
    dz0 = np.empty(lead + (self.n,)) if want_start else None
    dlam0 = np.empty(lead + (self.m,)) if want_start else None
    self._exgd_grad_call(call, MEM_HOST, lead, z, lam, lb, ub, pargs, eta_x, eta_v, nsteps, sz, sl, grad, 0 if reduce else self.np, dz0, dlam0)
    return self._present(grad=grad, dz0=dz0, dlam0=dlam0)

  def _exgd_grad_probe(self, call, kind):
    """an empty batch: the library's checks run, nothing else"""
    d = np.zeros(1)
    self._exgd_grad_call(call, MEM_HOST, (0, 1) if kind == "sets" else (0,), d, d, d, d, (None, 0) if kind == "rows" else (d,), 0.0, 0.0, 0, d, None, d, 0,
                         None, None)

  def _hvp_call(self, call, mem, sizes, z, lam, v, pargs, with_cost, out_z, out_p, p_stride):
    _chk(getattr(self.lib, call)(self._h, *map(int, sizes), _addr(z), _addr(lam), _addr(v), _addr(pargs[0]), *map(int, pargs[1:]), int(bool(with_cost)),
                                 _addr(out_z), _addr(out_p), int(p_stride), mem), call)

  def _hvp(self, call, kind, z, lam, v, params, with_cost, want_z, want_p, reduce):
    if kind == "sets":
      pargs = (self._weight_sets(params),)
      z = self._sets_z(z, pargs[0].shape[0])
      lead = z.shape[:2]
      v = self._sets3(v, *lead, self.n, "v")
      lam = None if lam is None else self._sets3(lam, *lead, self.m, "lam")
    else:
      z = self._batch2(z, self.n, "z"); v = self._batch2(v, self.n, "v")
      lead = z.shape[:1]
      lam = None if lam is None else self._batch2(lam, self.m, "lam")
      if v.shape[0] != lead[0] or (lam is not None and lam.shape[0] != lead[0]):
        raise ValueError("z, lam and v must have the same batch size")
      pargs = self._param_args(kind, params, lead[0])
    hz = np.empty(lead + (self.n,)) if want_z else None
    hp = np.empty((lead[:-1] if reduce else lead) + (self.np,)) if want_p else None
    self._hvp_call(call, MEM_HOST, lead, z, lam, v, pargs, with_cost, hz, hp, 0 if reduce else self.np)
    return self._present(hz=hz, hp=hp)

  def _hvp_probe(self, call, kind):
    d = np.zeros(1)
    self._hvp_call(call, MEM_HOST, (0, 1) if kind == "sets" else (0,), d, None, d, (d,), 1, d, None, 0)

  def exgd_grad(self, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, seed_lam=None, params=None, reduce=False, want_start=True):
    """myr_exgd_grad: derivative of `nsteps` extragradient steps from (z, lam) in the model parameters, contracted with the seed.
    Returns {"grad" [B,np], or [np] = the sum over the batch with reduce=True, "dz0" [B,n], "dlam0" [B,m]} (the last two with want_start)."""
    return self._exgd_grad("myr_exgd_grad", "rows", z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, seed_lam, params, reduce, want_start)

  def exgd_grad_probe(self):
    """Raises the library's error when myr_exgd_grad is not built for this handle (an empty batch: the checks run, nothing else)."""
    self._exgd_grad_probe("myr_exgd_grad", "rows")

  def exgd_grad_device(self, B, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, grad, grad_stride, seed_lam=None, params=None, params_stride=0,
                       dz0=None, dlam0=None):
    """Zero-copy variant of exgd_grad: every array is a device tensor on this handle's device."""
    self._exgd_grad_call("myr_exgd_grad", MEM_DEVICE, (B,), z, lam, lb, ub, (params, params_stride), eta_x, eta_v, nsteps, seed_z, seed_lam, grad, grad_stride,
                         dz0, dlam0)

  # myr_exgd_jac: the Jacobian of the same steps itself, forward mode (csrc/exgd_jac.h) -- closed-form systems, the collocation transcriptions
  def exgd_jac(self, z, lam, lb, ub, eta_x, eta_v, nsteps, params=None, jz0=None, jlam0=None, want=("zn", "lamn", "jz", "jlam")):
    """myr_exgd_jac: d z_n / d params and d lam_n / d params of `nsteps` extragradient steps from (z, lam), np tangent columns in one call.
    jz0 [B,np,n], jlam0 [B,np,m] or None (= 0): the tangents of the start.  Returns the entries of `want` (at least one of "jz", "jlam"):
    {"zn" [B,n], "lamn" [B,m] (the bits of exgd), "jz" [B,np,n], "jlam" [B,np,m]}."""
    z = self._batch2(z, self.n, "z"); lam = self._batch2(lam, self.m, "lam")
    B = z.shape[0]
    if lam.shape[0] != B:
      raise ValueError("z and lam must have the same batch size")
    unknown = set(want) - {"zn", "lamn", "jz", "jlam"}
    if unknown or not {"jz", "jlam"} & set(want):
      raise ValueError(f"want: at least one of 'jz', 'jlam', beside 'zn', 'lamn' (got {tuple(want)})")
    lb, ub = (np.ascontiguousarray(np.broadcast_to(_f64(a), z.shape)) for a in (lb, ub))
    j0 = [None if a is None else np.ascontiguousarray(np.broadcast_to(_f64(a), (B, self.np, w))) for a, w in ((jz0, self.n), (jlam0, self.m))]
    shapes = dict(zn=(B, self.n), lamn=(B, self.m), jz=(B, self.np, self.n), jlam=(B, self.np, self.m))
    out = {k: np.empty(shapes[k]) if k in want else None for k in shapes}
    p, ps = self._params(params, B)
    self.exgd_jac_device(B, z, lam, lb, ub, eta_x, eta_v, nsteps, params=p, params_stride=ps, jz0=j0[0], jlam0=j0[1], mem=MEM_HOST, **out)
    return self._present(**out)

  def exgd_jac_probe(self):
    """Raises the library's error when myr_exgd_jac is not built for this handle (an empty batch: the checks run, nothing else)."""
    d = np.zeros(1)
    self.exgd_jac_device(0, d, d, d, d, 0.0, 0.0, 0, jz=d, mem=MEM_HOST)

  def exgd_jac_device(self, B, z, lam, lb, ub, eta_x, eta_v, nsteps, params=None, params_stride=0, jz0=None, jlam0=None, zn=None, lamn=None, jz=None,
                      jlam=None, mem=MEM_DEVICE):
    """Zero-copy variant of exgd_jac: every array is a device tensor on this handle's device (jz or jlam may be None, not both)."""
    _chk(self.lib.myr_exgd_jac(self._h, int(B), _addr(z), _addr(lam), _addr(lb), _addr(ub), _addr(params), int(params_stride), float(eta_x), float(eta_v),
                               int(nsteps), _addr(jz0), _addr(jlam0), _addr(zn), _addr(lamn), _addr(jz), _addr(jlam), mem), "myr_exgd_jac")

  # myr_exgd_grad_shoot: the same derivative on a SHOOTING handle (csrc/shoot_exgd_grad.h) -- the signatures, the return dict and the checks of the
  # three methods above; myr_exgd_grad itself keeps refusing SHOOTING
  def exgd_grad_shoot(self, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, seed_lam=None, params=None, reduce=False, want_start=True):
    return self._exgd_grad("myr_exgd_grad_shoot", "rows", z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, seed_lam, params, reduce, want_start)

  def exgd_grad_shoot_probe(self):
    self._exgd_grad_probe("myr_exgd_grad_shoot", "rows")

  def exgd_grad_shoot_device(self, B, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, grad, grad_stride, seed_lam=None, params=None, params_stride=0,
                             dz0=None, dlam0=None):
    self._exgd_grad_call("myr_exgd_grad_shoot", MEM_DEVICE, (B,), z, lam, lb, ub, (params, params_stride), eta_x, eta_v, nsteps, seed_z, seed_lam, grad,
                         grad_stride, dz0, dlam0)

  def exgd_grad_node(self, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, params, seed_lam=None, reduce=False, want_start=True):
    """myr_exgd_grad_node: exgd_grad in the 4 804 shared weights of the network system (`params`: the flat vector of csrc/node_system.h's order;
    Hermite-Simpson).  Returns {"grad" [B,np], or [np] = the sum over the batch with reduce=True, "dz0" [B,n], "dlam0" [B,m]}."""
    return self._exgd_grad("myr_exgd_grad_node", "shared", z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, seed_lam, params, reduce, want_start)

  def exgd_grad_node_probe(self):
    """Raises the library's error when myr_exgd_grad_node is not built for this handle (an empty batch: the checks run, nothing else)."""
    self._exgd_grad_probe("myr_exgd_grad_node", "shared")

  def exgd_grad_node_device(self, B, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, grad, grad_stride, params, seed_lam=None, dz0=None, dlam0=None):
    """Zero-copy variant of exgd_grad_node: every array is a device tensor on this handle's device."""
    self._exgd_grad_call("myr_exgd_grad_node", MEM_DEVICE, (B,), z, lam, lb, ub, (params,), eta_x, eta_v, nsteps, seed_z, seed_lam, grad, grad_stride, dz0, dlam0)

  # myr_exgd_grad_node_shoot: the same derivative in the weights on a SHOOTING handle (csrc/node_shoot_exgd_grad.h) -- the signatures, the return
  # dict and the checks of the three methods above; myr_exgd_grad_node itself keeps refusing SHOOTING
  def exgd_grad_node_shoot(self, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, params, seed_lam=None, reduce=False, want_start=True):
    return self._exgd_grad("myr_exgd_grad_node_shoot", "shared", z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, seed_lam, params, reduce, want_start)

  def exgd_grad_node_shoot_probe(self):
    self._exgd_grad_probe("myr_exgd_grad_node_shoot", "shared")

  def exgd_grad_node_shoot_device(self, B, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, grad, grad_stride, params, seed_lam=None, dz0=None,
                                  dlam0=None):
    self._exgd_grad_call("myr_exgd_grad_node_shoot", MEM_DEVICE, (B,), z, lam, lb, ub, (params,), eta_x, eta_v, nsteps, seed_z, seed_lam, grad, grad_stride,
                         dz0, dlam0)

  # ---- E weight sets of R instances each in one call (myr_exgd_grad_node_sets, myr_hvp_node_sets) --------------------------
  def exgd_grad_node_sets(self, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, params, seed_lam=None, reduce=False, want_start=True):
    """myr_exgd_grad_node_sets: exgd_grad_node (exgd_grad_node_shoot on a SHOOTING handle) for E weight sets of R instances each in one call.
    params [E,np]; z [E,R,n], lam [E,R,m]; lb, ub, seed_z broadcast to z, seed_lam (None: zero) to lam.  Returns {"grad" [E,R,np], or [E,np] =
    per set the sum over its instances with reduce=True, "dz0" [E,R,n], "dlam0" [E,R,m]} (the last two with want_start).  Set e has the bits of
    the single-set call on that set alone."""
    return self._exgd_grad("myr_exgd_grad_node_sets", "sets", z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, seed_lam, params, reduce, want_start)

  def exgd_grad_node_sets_device(self, E, R, z, lam, lb, ub, eta_x, eta_v, nsteps, seed_z, grad, grad_stride, params, seed_lam=None, dz0=None,
                                 dlam0=None):
    """Zero-copy variant of exgd_grad_node_sets: every array is a device tensor on this handle's device."""
    self._exgd_grad_call("myr_exgd_grad_node_sets", MEM_DEVICE, (E, R), z, lam, lb, ub, (params,), eta_x, eta_v, nsteps, seed_z, seed_lam, grad, grad_stride,
                         dz0, dlam0)

  def exgd_grad_node_sets_probe(self):
    """Raises the library's error when myr_exgd_grad_node_sets is not built for this handle (no sets: the checks run, nothing else)."""
    self._exgd_grad_probe("myr_exgd_grad_node_sets", "sets")

  def hvp_node_sets(self, z, lam, v, params, with_cost=True, want_z=True, want_p=False, reduce=False):
    """myr_hvp_node_sets: hvp_node for E weight sets of R instances each in one call.  params [E,np]; z, v [E,R,n]; lam [E,R,m] or None (zero
    multipliers).  Returns {"hz" [E,R,n] (with want_z), "hp" [E,R,np], or [E,np] = per set the sum over its instances with reduce=True (with
    want_p)}.  Set e has the bits of hvp_node on that set alone."""
    return self._hvp("myr_hvp_node_sets", "sets", z, lam, v, params, with_cost, want_z, want_p, reduce)

  def hvp_node_sets_device(self, E, R, z, lam, v, params, out_z=None, out_p=None, p_stride=0, with_cost=True):
    """Zero-copy variant of hvp_node_sets: every array is a device tensor on this handle's device (lam, out_z, out_p may be None)."""
    self._hvp_call("myr_hvp_node_sets", MEM_DEVICE, (E, R), z, lam, v, (params,), with_cost, out_z, out_p, p_stride)

  def hvp_node_sets_probe(self):
    """Raises the library's error when myr_hvp_node_sets is not built for this handle (no sets: the checks run, nothing else)."""
    self._hvp_probe("myr_hvp_node_sets", "sets")

  def hvp(self, z, lam, v, params=None, with_cost=True, want_z=True, want_p=False, reduce=False):
    """myr_hvp: Lagrangian Hessian-vector product.  With L = f + lam^T c (f dropped when with_cost is false) and psi = <grad_z L, v>:
    {"hz" [B,n] = grad_z psi = (d2L/dz dz) v (with want_z), "hp" [B,np] = grad_p psi = (d2L/dp dz) v, or [np] = the sum over the batch with
    reduce=True (with want_p)}.  lam None: zero multipliers."""
    return self._hvp("myr_hvp", "rows", z, lam, v, params, with_cost, want_z, want_p, reduce)

  def hvp_device(self, B, z, lam, v, out_z=None, out_p=None, p_stride=0, params=None, params_stride=0, with_cost=True):
    """Zero-copy variant of hvp: every array is a device tensor on this handle's device (lam, out_z, out_p may be None); nothing is copied."""
    self._hvp_call("myr_hvp", MEM_DEVICE, (B,), z, lam, v, (params, params_stride), with_cost, out_z, out_p, p_stride)

  def hvp_node(self, z, lam, v, params, with_cost=True, want_z=True, want_p=False, reduce=False):
    """myr_hvp_node: hvp on a handle of the network system (HERMITE_SIMPSON or SHOOTING); `params`: the 4 804 shared weights, the flat vector of
    csrc/node_system.h's order.  Returns {"hz" [B,n] (with want_z), "hp" [B,np], or [np] = the sum over the batch with reduce=True (with want_p)}."""
    return self._hvp("myr_hvp_node", "shared", z, lam, v, params, with_cost, want_z, want_p, reduce)

  def hvp_node_device(self, B, z, lam, v, params, out_z=None, out_p=None, p_stride=0, with_cost=True):
    """Zero-copy variant of hvp_node: every array is a device tensor on this handle's device (lam, out_z, out_p may be None); nothing is copied."""
    self._hvp_call("myr_hvp_node", MEM_DEVICE, (B,), z, lam, v, (params,), with_cost, out_z, out_p, p_stride)

  def hvp_node_probe(self):
    """Raises the library's error when myr_hvp_node is not built for this handle (an empty batch: the checks run, nothing else)."""
    self._hvp_probe("myr_hvp_node", "shared")

  def products_device(self, op, B, z, w, out, params=None, params_stride=0, add_gradf=0):
    """Zero-copy vjp ('vjp') / jvp ('jvp') on device tensors."""
    if op == "vjp":
      _chk(self.lib.myr_vjp(self._h, int(B), _addr(z), _addr(w), _addr(params), int(params_stride), _addr(out), int(add_gradf), MEM_DEVICE), "myr_vjp")
    else:
      _chk(self.lib.myr_jvp(self._h, int(B), _addr(z), _addr(w), _addr(params), int(params_stride), _addr(out), MEM_DEVICE), "myr_jvp")

  def fbsm(self, x0, N, clip_lo, clip_hi, params=None, adj_T=None, delta=0.001, max_sweeps=10000, bang=0.0, discrete=False):
    """Batched Forward-Backward Sweep: returns {'x' [B,N+1,ns], 'u' [B,N+1,nu], 'adj' [B,N+1,ns], 'sweeps' [B]};
    for a discrete system (`discrete=True`, INVASIVEPLANT) 'u' is [B,N,nu], one row per step."""
    x0 = _f64(x0)
    if x0.ndim == 1:
      x0 = x0[None]
    B = x0.shape[0]
    p, ps = self._params(params, B)
    aT = None if adj_T is None else _f64(adj_T)
    lo = np.ascontiguousarray(np.broadcast_to(_f64(clip_lo), (self.nu,))); hi = np.ascontiguousarray(np.broadcast_to(_f64(clip_hi), (self.nu,)))
    xs = np.empty((B, N + 1, self.ns)); us = np.empty((B, N + (0 if discrete else 1), self.nu)); adjs = np.empty((B, N + 1, self.ns))
    sw = np.empty(B, dtype=np.int32)
    _chk(self.lib.myr_fbsm(self._h, B, int(N), _addr(x0), _addr(aT), _addr(p), ps, _addr(lo), _addr(hi), float(bang), float(delta),
                           int(max_sweeps), _addr(xs), _addr(us), _addr(adjs), _addr(sw), MEM_HOST), "myr_fbsm")
    return {"x": xs, "u": us, "adj": adjs, "sweeps": sw}

  def solve_plan(self) -> dict:
    """myr_solve_plan: how the library launched the first attempt of the last solve on this handle (include/myriad_hip.h)"""
    p = np.zeros(8, dtype=np.int32)
    _chk(self.lib.myr_solve_plan(self._h, _addr(p)), "myr_solve_plan")
    return {"form": ("lane", "fused", "wave", "shooting_wave")[int(p[0])], "waves_per_trajectory": int(p[1]), "park_iter": int(p[2]),
            "launches_per_solve": int(p[3]), "slots": int(p[4]), "helpers_max": int(p[5])}

  def kernel_time(self, kernel_id: int):
    ms = C.c_double(); n = C.c_int32()
    _chk(self.lib.myr_kernel_time(self._h, kernel_id, C.byref(ms), C.byref(n)), "myr_kernel_time")
    return ms.value, n.value

  def kernel_time_reset(self):
    _chk(self.lib.myr_kernel_time_reset(self._h), "myr_kernel_time_reset")
