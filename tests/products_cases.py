"""Inputs and oracle references shared by the tests of the Lagrangian products and the extragradient steps themselves -- myr_vjp, myr_jvp, myr_exgd
(test_products_cases.py, test_gpu_products_matrix.py).

Nothing is drawn here: a case is what exgd_grad_cases._draw (collocation), shoot_exgd_grad_cases._draw (SHOOTING), node_exgd_grad_cases._draw
(the network system) and hvp_cases.inputs (shapes of the products, which need no boxes and no step sizes) return, with four keys added so that
one engine and one oracle serve all of them: tr, cpi, method and v (= seed_z, the direction of J v).

Forward values need no tie condition: clip is continuous, so a value that lands near a bound moves the result by at most its distance to it.  What
is kept is the clip fraction: a case is the first of the seeds 0 .. 19 whose oracle run is finite and in which at least exgd_grad_cases.MIN_CLIPPED
(15 %) of the free variables of every instance (of every row the oracle runs, for a shape case) clip in some half-step.

Conditioning, recorded with every case (`response`) and asserted by test_products_cases.py: the oracle runs every row a second time from z with each
entry moved by -1, 0 or +1 ulp (a fixed pattern), and the two runs must agree within MAX_RESPONSE = 1e-12, a tenth of the ceiling the device is held
to -- an iteration that amplifies one bit beyond that cannot hold a kernel to 1e-11.  Every case answers with 4e-18 ... 9e-15, but one: the step sizes of
a draw come from ten rounds of a power iteration on its first instance, which for ROCKETLANDING Hermite-Simpson N = 33 (536 variables of very
different scales) leaves a growing mode.  Row 0 of that case answers one ulp with 3.4e-11 of max|z_n| after ten steps (row 64 with 4e-14; after one
step both with 5e-15), and none of the seeds 0 .. 19 does better than 1e-10.  The case is kept as it is drawn; the GPU module holds its ten-step
comparison under a figure of its own and says so.

The reference of an instance b, with tr_b the oracle's transcription at that instance's own parameter row:
  gl = Lagrangian(tr_b).grad_x(z, lam)          gf = Callbacks(tr_b).grad(z)          jv = Lagrangian(tr_b).jvp(z, v)
  jt = gl - gf, taken as the same autograd of the Lagrangian with the cost term left out, grad_z (lam . c(z)): the subtraction itself leaves
       eps max|gl| of rounding in jt, which is 4e-12 of max|jt| where the cost is scaled far above the constraints (GLUCOSE's by 100 000,
       BEARPOPULATIONS' by c_p = 10 000).  test_products_cases.py holds the two forms together within that rounding.
  (z_n, lam_n) = the `oracle_run(..., grad_params=False)` of the case's module, detached.

TIMBERHARVEST: its default r is 0 and the draws scale parameters by 1 +- 5 %, so exp(-r t) is 1 in every ordinary case.  `discounted=True` takes
the inputs of the ordinary case and replaces that one parameter entry by 0.3.
"""
import functools

import numpy as np
import torch

import exgd_grad_cases as E
import hvp_cases as H
import shoot_exgd_grad_cases as S
from exgd_grad_cases import MIN_CLIPPED, O, rel_error  # noqa: F401

SCHEMES = E.SCHEMES
SYSTEMS = E.SYSTEMS
# SHOOTING (I, cpi, integrator): every system; 3 x 2 RK4 has control rows shared by two steps and by two intervals
SHOOT_SHAPES = ((3, 2, "HEUN"), (3, 2, "RK4"), (1, 4, "RK4"))
# ... and the eight systems of test_gpu_hvp.PARITY under the other two integrators
SHOOT_EXTRA_SHAPES = ((3, 2, "EULER"), (3, 2, "MIDPOINT"))
SHOOT_EXTRA_SYSTEMS = ("CARTPOLE", "VANDERPOL", "CANCERTREATMENT", "BACTERIA", "TIMBERHARVEST", "BEARPOPULATIONS", "ROCKETLANDING", "PREDATORPREY")
DISCOUNT_R = 0.3
DISCOUNT_SHOOT = (3, 2, "RK4")

# shapes (test_gpu_products_matrix.py, sections 3 .. 5): one draw at the largest batch; a smaller batch is its leading rows
PRODUCT_SHAPE_N = (1, 2, 51)
PRODUCT_SHAPE_B = (1, 63, 65, 257)
EXGD_SHAPES = [("HERMITE_SIMPSON", N) for N in (1, 31, 32, 33, 100)] + [("TRAPEZOIDAL", N) for N in (63, 64, 65)]      # test_gpu_exgd_grad.py's list
EXGD_SHAPE_B = (1, 130)
EXGD_SHAPE_STEPS = (1, 10)
EXGD_WIDE = (("ROCKETLANDING", "HERMITE_SIMPSON", 33, 65), ("HIVTREATMENT", "HERMITE_SIMPSON", 33, 65))      # the widest points
SHOOT_SHAPE_CASES = (("CARTPOLE", 4, 3, "RK4"), ("VANDERPOL", 1, 50, "HEUN"))
SHOOT_SHAPE_B = (1, 63, 65, 130)
SHOOT_SHAPE_STEPS = (1, 5)
MAX_RESPONSE = 1e-12  # of the oracle's own run to one bit of its input (module docstring)
ILL_CONDITIONED = ("ROCKETLANDING", "HERMITE_SIMPSON", 33, 65)      # the one case above it (module docstring)
CAPACITY_N = 568      # CARTPOLE Hermite-Simpson: the largest horizon whose iterate fits the 160 KiB of LDS (288 N + 128 bytes)


def _freeze(obj):
  for a in (obj.values() if isinstance(obj, dict) else obj):
    if isinstance(a, np.ndarray):
      a.setflags(write=False)
  return obj


def _normalised(kind, c):
  """the keys the four generators do not share: tr, N, cpi, method, v"""
  c = dict(c)
  c["kind"] = kind
  if kind == "colloc":
    c.update(tr=c["scheme"], cpi=1, method="HEUN", v=c["seed_z"])
  elif kind == "shoot":
    c.update(tr="SHOOTING", N=c["I"], v=c["seed_z"])
  elif kind == "node":
    c.update(name="NODE_CARTPOLE", tr="HERMITE_SIMPSON", cpi=1, method="HEUN", v=c["seed_z"])
  return c


def transcription(c, b):
  """the oracle's transcription of instance b, at its own parameter row"""
  if c["kind"] == "node":
    import node_exgd_grad_cases as ND
    return ND._transcription(c["N"], c["T"], ND._leaves(False))
  prow = [float(v) for v in c["params"][b]]
  if c["tr"] == "SHOOTING":
    return H._transcription(c["name"], "SHOOTING", c["N"], c["cpi"], c["method"], c["T"], prow)[1]
  return E._transcription(c["name"], c["tr"], c["N"], c["T"], prow)[1]


def _steps(c, b, nsteps):
  """(z_n, lam_n, values in front of every clamp) of the case's own oracle_run"""
  a = (c["z"][b], c["lam"][b], c["lb"][b], c["ub"][b])
  if c["kind"] == "node":
    import node_exgd_grad_cases as ND
    x, lm, _, pre = ND.oracle_run(c["N"], c["T"], *a, c["eta_x"], c["eta_v"], nsteps, grad_params=False)
  elif c["tr"] == "SHOOTING":
    x, lm, _, pre = S.oracle_run(c["name"], c["N"], c["cpi"], c["method"], c["T"], *a, c["params"][b], c["eta_x"], c["eta_v"], nsteps, grad_params=False)
  else:
    x, lm, _, pre, _ = E.oracle_run(c["name"], c["tr"], c["N"], c["T"], *a, c["params"][b], c["eta_x"], c["eta_v"], nsteps, grad_params=False)
  return x.detach().numpy(), lm.detach().numpy(), pre


def oracle_row(c, b, nsteps=0, products=True):
  """the reference of instance b: gl, gf, jt, jv and, for nsteps > 0, z_n, lam_n and `outside` (which variables clipped in some half-step)"""
  out = {}
  if products:
    tr = transcription(c, b)
    L, cb = O.Lagrangian(tr), O.Callbacks(tr)
    gl, gf = L.grad_x(c["z"][b], c["lam"][b]), cb.grad(c["z"][b])
    lam = O._t(c["lam"][b])
    jt = torch.func.grad(lambda x: lam @ tr.constraints(x))(O._t(c["z"][b])).numpy()      # = gl - gf without the cancellation (module docstring)
    out.update(gl=gl, gf=gf, jt=jt, jv=L.jvp(c["z"][b], c["v"][b]))
  if nsteps:
    zn, ln, pre = _steps(c, b, nsteps)
    out.update(z_n=zn, lam_n=ln, outside=E.clamp_conditions(pre, c["lb"][b], c["ub"][b])[1])
  return out


def dense_products(c, b):
  """(J^T lam, J v) of instance b from the oracle's dense Jacobian: independent of the autograd of the Lagrangian that `oracle_row` takes"""
  J = O.Callbacks(transcription(c, b)).jac(c["z"][b])
  return J.T @ c["lam"][b], J @ c["v"][b]


def _stack(rows):
  return _freeze({k: np.stack([r[k] for r in rows]) for k in rows[0]})


def _clipped(c, ref, rows):
  free = c["lb"][rows] < c["ub"][rows]
  return float(min((ref["outside"][i] & free[i]).sum() / free[i].sum() for i in range(len(rows))))


def response(c, ref, rows, nsteps):
  """the oracle's own answer to one bit: the largest rel_error between its run and its run from z with every entry moved by -1, 0 or +1 ulp"""
  rng = np.random.default_rng(12345)
  worst = 0.0
  for i, b in enumerate(rows):
    moved = dict(c)
    z = c["z"].copy()
    z[b] = z[b] * (1.0 + 2.0 ** -52 * rng.integers(-1, 2, z[b].shape))
    moved["z"] = z
    with np.errstate(all="ignore"):
      r = oracle_row(moved, b, nsteps, products=False)
      worst = max(worst, rel_error(r["z_n"][None], ref["z_n"][i:i + 1]), rel_error(r["lam_n"][None], ref["lam_n"][i:i + 1]))
  return worst if np.isfinite(worst) else np.inf


def _first_that_clips(draw, rows_of, nsteps, what, products=True):
  """(case, reference of `rows`) of the first seed whose run is finite and clips enough on every row the oracle runs; case["response"]: `response`"""
  last = None
  for seed in range(20):
    c = draw(seed)
    rows = list(rows_of(c))
    with np.errstate(all="ignore"):
      ref = _stack([oracle_row(c, b, nsteps, products) for b in rows])
    frac = _clipped(c, ref, rows)
    last = (seed, frac)
    if all(np.isfinite(a).all() for a in ref.values()) and frac >= MIN_CLIPPED:
      c.update(seed=seed, clipped=frac, response=response(c, ref, rows, nsteps), rows=tuple(rows))
      return _freeze(c), ref
  raise AssertionError(f"{what}: no finite draw clips {MIN_CLIPPED:.0%} of the free variables (last: seed, clipped = {last})")


def _discounted(c, ref_of):
  """the case with TIMBERHARVEST's r replaced by DISCOUNT_R, and its reference; the clip fraction is that of the new run and is asserted by the tests"""
  c = {k: v for k, v in c.items() if k != "key"}
  p = c["params"].copy()
  p[:, O.SYSTEMS["TIMBERHARVEST"].param_names.index("r")] = DISCOUNT_R
  c["params"] = p
  ref = ref_of(c)
  c["clipped"] = _clipped(c, ref, list(c["rows"]))
  return _freeze(c), ref


# ---- the parity matrix (N = 3 or 3 x 2 / 1 x 4, three steps, every instance through the oracle) ---------------------------------------
@functools.lru_cache(maxsize=None)
def _colloc(name, scheme, N, nsteps, batch, discounted):
  if discounted:
    assert name == "TIMBERHARVEST"
    return _discounted(_colloc(name, scheme, N, nsteps, batch, False)[0], lambda c: _stack([oracle_row(c, b, nsteps) for b in range(batch)]))
  return _first_that_clips(lambda seed: _normalised("colloc", E._draw(name, scheme, N, nsteps, batch, seed)), lambda c: range(batch), nsteps,
                           f"{name} {scheme} N={N}")


@functools.lru_cache(maxsize=None)
def _shoot(name, I, cpi, method, nsteps, batch, discounted):
  if discounted:
    assert name == "TIMBERHARVEST"
    return _discounted(_shoot(name, I, cpi, method, nsteps, batch, False)[0], lambda c: _stack([oracle_row(c, b, nsteps) for b in range(batch)]))
  return _first_that_clips(lambda seed: _normalised("shoot", S._draw(name, I, cpi, method, nsteps, batch, seed)), lambda c: range(batch), nsteps,
                           f"{name} {I}x{cpi} {method}")


@functools.lru_cache(maxsize=None)
def _node(N, nsteps, batch):
  import node_exgd_grad_cases as ND
  return _first_that_clips(lambda seed: _normalised("node", ND._draw(N, nsteps, batch, seed)), lambda c: range(batch), nsteps, f"NODE_CARTPOLE N={N}")


def colloc_case(name, scheme, N=3, nsteps=3, batch=3, discounted=False):
  c = _colloc(name, scheme, N, nsteps, batch, discounted)[0]
  c.setdefault("key", ("colloc", name, scheme, N, nsteps, batch, discounted))
  return c


def shoot_case(name, I, cpi, method, nsteps=3, batch=2, discounted=False):
  c = _shoot(name, I, cpi, method, nsteps, batch, discounted)[0]
  c.setdefault("key", ("shoot", name, I, cpi, method, nsteps, batch, discounted))
  return c


def node_case(N=3, nsteps=3, batch=2):
  c = _node(N, nsteps, batch)[0]
  c.setdefault("key", ("node", N, nsteps, batch))
  return c


def forward_reference(case):
  """{gl, gf, jt, jv, z_n, lam_n, outside}, each [B][.], read-only; cached with the case (functools.lru_cache on the case's key)"""
  kind, *key = case["key"]
  return {"colloc": _colloc, "shoot": _shoot, "node": _node}[kind](*key)[1]


def parity_cases():
  """every case of section 1 of the matrix, as (id, thunk)"""
  out = []
  for name in SYSTEMS:
    for scheme in SCHEMES:
      out.append((f"{name}-{scheme}", functools.partial(colloc_case, name, scheme)))
  for scheme in SCHEMES:
    out.append((f"TIMBERHARVEST-{scheme}-r0.3", functools.partial(colloc_case, "TIMBERHARVEST", scheme, discounted=True)))
  for name in SYSTEMS:
    for shape in SHOOT_SHAPES:
      out.append((f"{name}-{shape[0]}x{shape[1]}-{shape[2]}", functools.partial(shoot_case, name, *shape)))
  for name in SHOOT_EXTRA_SYSTEMS:
    for shape in SHOOT_EXTRA_SHAPES:
      out.append((f"{name}-{shape[0]}x{shape[1]}-{shape[2]}", functools.partial(shoot_case, name, *shape)))
  out.append(("TIMBERHARVEST-%dx%d-%s-r0.3" % DISCOUNT_SHOOT, functools.partial(shoot_case, "TIMBERHARVEST", *DISCOUNT_SHOOT, discounted=True)))
  return out


# ---- shapes: one draw at the largest batch, the oracle on a few rows ---------------------------------------------------------------------
def edge_rows(batches):
  """rows 0 and B - 1 of every batch size"""
  return sorted({0} | {B - 1 for B in batches})


@functools.lru_cache(maxsize=None)
def product_shape(scheme, N):
  """(case, reference of its `rows`): CARTPOLE inputs of hvp_cases.inputs at the largest batch, the products' reference on rows 0 and B - 1 of every
  batch size"""
  c = _normalised("inputs", H.inputs("CARTPOLE", scheme, N, 1, "HEUN", max(PRODUCT_SHAPE_B)))
  rows = edge_rows(PRODUCT_SHAPE_B)
  c["rows"] = tuple(rows)
  return _freeze(c), _stack([oracle_row(c, b) for b in rows])


@functools.lru_cache(maxsize=None)
def exgd_shape(name, scheme, N, batch, steps):
  """(case, {nsteps: reference of its `rows`}): exgd_grad_cases._draw at `batch` -- step sizes that keep max(steps) steps stable, boxes that the first
  half-step leaves --, the oracle on rows 0 and batch - 1 after each of `steps`.  The clip fraction is that of the longest run."""
  rows = edge_rows((batch,))
  c, ref = _first_that_clips(lambda seed: _normalised("colloc", E._draw(name, scheme, N, max(steps), batch, seed)), lambda c: rows, max(steps),
                             f"{name} {scheme} N={N} B={batch}", products=False)
  refs = {max(steps): ref}
  for k in steps:
    if k not in refs:
      refs[k] = _stack([oracle_row(c, b, k, products=False) for b in rows])
  return c, refs


@functools.lru_cache(maxsize=None)
def shoot_shape(name, I, cpi, method):
  """(case, products' reference, {nsteps: steps' reference}) of a SHOOTING shape: shoot_exgd_grad_cases._draw at the largest batch, the oracle on
  rows 0 and B - 1 of every batch size"""
  rows = edge_rows(SHOOT_SHAPE_B)
  top = max(SHOOT_SHAPE_STEPS)
  c, ref = _first_that_clips(lambda seed: _normalised("shoot", S._draw(name, I, cpi, method, top, max(SHOOT_SHAPE_B), seed)), lambda c: rows, top,
                             f"{name} {I}x{cpi} {method} B={max(SHOOT_SHAPE_B)}")
  refs = {top: ref}
  for k in SHOOT_SHAPE_STEPS:
    if k not in refs:
      refs[k] = _stack([oracle_row(c, b, k, products=False) for b in rows])
  return c, ref, refs


def head(c, B):
  """the leading B instances of a case"""
  out = dict(c)
  for k in ("z", "lam", "v", "lb", "ub", "seed_z", "seed_lam"):
    if k in c:
      out[k] = c[k][:B]
  if c["params"].ndim == 2:
    out["params"] = c["params"][:B]
  return out


def row_index(c, b):
  """where instance b stands in the case's reference arrays"""
  return c["rows"].index(b)
