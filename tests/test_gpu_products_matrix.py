"""myr_vjp, myr_jvp and myr_exgd on the device -- colloc_vjp_kernel, colloc_jvp_kernel, colloc_exgd_kernel (myriad_amd/csrc/colloc_products.h);
shoot_eval_kernel with lamin, shoot_jvp_kernel, exgd_update_kernel, axpy_kernel (shoot_eval.h) under shoot_exgd_steps (myriad_hip.hip) -- against the
oracle for every system, and against themselves across shapes, batch sizes, forms of the call and what ran before on the handle.  The cases and
their references are tests/products_cases.py's; tests/test_products_cases.py checks those references on themselves.  Everything goes through
_lib.Engine.

Tolerances.  `rel_error` is exgd_grad_cases': the largest |d| / max|ref| of a row.  MEASURED below holds, per quantity, the worst figure over every
comparison with the oracle in this module (938 of them), on an MI355X with the cases as they stand, and the case that produced it:
  gl       grad L = grad f + J^T lam       1.0e-15   VANDERPOL 1 x 50 Heun, B = 65, row 64
  jt       J^T lam                         9.8e-16   VANDERPOL 1 x 50 Heun, B = 63, row 62
  jv       J v                             3.2e-15   TUMOUR 1 x 4 RK4
  steps3   iterates after 1, 2 or 3 steps  2.6e-14   lam of ROCKETLANDING 1 x 4 RK4 (the next: 8.6e-16)
  steps10  iterates after 5 or 10 steps    4.4e-16   lam of CARTPOLE trapezoidal N = 65, B = 130, row 129, ten steps
Each is asserted at 10 x its figure -- the device contracts multiply-adds and has its own libm; 10 x is the project's margin --, under a ceiling of
1e-11, test_gpu_exgd_grad.ORACLE_TOL, which already holds the DERIVATIVE of these steps.  Bit equalities are exact.

One comparison has a figure of its own, steps10_ill: ten steps of ROCKETLANDING Hermite-Simpson N = 33, B = 65, row 0, measured 4.1e-13 (lam; z 2.7e-13;
row 64 of the same call 6.2e-15, one step 4e-16).  That is not the kernel: the ORACLE answers one ulp in z of that row with 3.4e-11 after ten steps
(products_cases.py, `response`; every other case with less than 1e-14) -- the draw's step sizes, from ten rounds of a power iteration, do not keep
ten steps of this system stable at this horizon, whatever the seed.  Held apart, it does not loosen the ten-step bound of the other cases by three
orders; it is the one comparison here that stands on an ill-conditioned reference, and it is asserted at 10 x its figure like the others.

Wall time, the whole module: 34 s on an MI355X machine (145 tests; the slowest, VANDERPOL 1 x 50 Heun at B = 130, 5 s, of which the draw of its 130
instances is 4: shoot_exgd_grad_cases._draw sends every instance through the oracle once for the boxes).  tests/test_products_cases.py: 84 s on
a host without a device (143 tests; the same draw 13 s there, the second oracle run of every steps reference, for the conditioning, 20 s).
"""
import numpy as np
import pytest

import products_cases as P
from myriad_amd import _lib

pytestmark = pytest.mark.gpu

CEILING = 1e-11
# quantity -> (worst rel_error against the oracle, the case that produced it): the module docstring
MEASURED = {
  "gl": (1.0e-15, "VANDERPOL 1x50 HEUN B=65 row 64"),
  "jt": (9.8e-16, "VANDERPOL 1x50 HEUN B=63 row 62"),
  "jv": (3.2e-15, "TUMOUR SHOOTING 1x4 RK4"),
  "steps3": (2.6e-14, "ROCKETLANDING SHOOTING 1x4 RK4 lam"),
  "steps10": (4.4e-16, "CARTPOLE TRAPEZOIDAL N=65 B=130 nsteps=10 lam row 129"),
  "steps10_ill": (4.1e-13, "ROCKETLANDING HERMITE_SIMPSON N=33 B=65 nsteps=10 lam row 0"),
}
TOL = {k: min(10.0 * v[0], CEILING) for k, v in MEASURED.items()}
GRID_CAP = 16384 * 256      # grid_for (myriad_hip.hip): above this many units a thread takes a second trip through its grid-stride loop


def _engine(c, N=None):
  return _lib.Engine(c["name"], c["tr"], c["N"] if N is None else N, c["T"], controls_per_interval=c["cpi"], integration_method=c["method"])


def _bits(*arrays):
  return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _check(quantity, out, ref, what):
  e = P.rel_error(np.asarray(out), np.asarray(ref))
  print(f"MEASURE {quantity} {e:.3e} {what}")
  assert np.isfinite(out).all(), (quantity, what)
  assert e <= TOL[quantity], (quantity, what, e, TOL[quantity])


def _steps_quantity(nsteps, ill=False):
  return "steps3" if nsteps <= 3 else ("steps10_ill" if ill else "steps10")


def _products(eng, c, params=None):
  p = c["params"] if params is None else params
  return (eng.vjp(c["z"], c["lam"], params=p, add_gradf=True), eng.vjp(c["z"], c["lam"], params=p, add_gradf=False), eng.jvp(c["z"], c["v"], params=p))


def _exgd(eng, c, nsteps, params=None, z=None, lam=None):
  return eng.exgd(c["z"] if z is None else z, c["lam"] if lam is None else lam, c["lb"], c["ub"], c["eta_x"], c["eta_v"], nsteps,
                  params=c["params"] if params is None else params)


def _row(c, b):
  """instance b alone, as a one-instance case"""
  out = dict(c)
  for k in ("z", "lam", "v", "lb", "ub"):
    if k in c:
      out[k] = c[k][b:b + 1]
  if c["params"].ndim == 2:
    out["params"] = c["params"][b:b + 1]
  return out


def _against_oracle_rows(c, B, outs, ref, quantities, what):
  """rows 0 and B - 1 of the outputs against the reference rows of the case"""
  for b in sorted({0, B - 1}):
    i = P.row_index(c, b)
    for q, out, key in zip(quantities, outs, ("gl", "jt", "jv") if len(outs) == 3 else ("z_n", "lam_n")):
      _check(q, out[b:b + 1], ref[key][i:i + 1], f"{what} row {b}")


# ---- 1. parity, every system ------------------------------------------------------------------------------------------------------------
PARITY = P.parity_cases()


def _parity(c):
  ref = P.forward_reference(c)
  what = "%s %s %dx%d %s" % (c["name"], c["tr"], c["N"], c["cpi"], c["method"]) + (" r=0.3" if c["key"][-1] is True else "")
  B = c["z"].shape[0]
  kept = {k: c[k].copy() for k in ("z", "lam", "v", "lb", "ub", "params")}
  eng = _engine(c)
  gl, jt, jv = _products(eng, c)
  _check("gl", gl, ref["gl"], what)
  _check("jt", jt, ref["jt"], what)
  _check("jv", jv, ref["jv"], what)
  z3, lam3 = _exgd(eng, c, 3)
  _check("steps3", z3, ref["z_n"], what + " z")
  _check("steps3", lam3, ref["lam_n"], what + " lam")
  assert (z3 != c["z"]).any() and (lam3 != c["lam"]).any()
  # no step: the inputs, bit for bit
  z0, lam0 = _exgd(eng, c, 0)
  assert _bits(z0, lam0) == _bits(c["z"], c["lam"])
  # three steps = two steps, then one
  z2, lam2 = _exgd(eng, c, 2)
  z21, lam21 = _exgd(eng, c, 1, z=z2, lam=lam2)
  assert _bits(z21, lam21) == _bits(z3, lam3)
  # the inputs are untouched
  for k, a in kept.items():
    assert _bits(a) == _bits(c[k]), k
  # the shared-parameter form = the same row for every instance
  if c["params"].ndim == 2:
    one, tiled = c["params"][0].copy(), np.tile(c["params"][0], (B, 1))
    assert _bits(*_products(eng, c, one)) == _bits(*_products(eng, c, tiled))
    assert _bits(*_exgd(eng, c, 3, one)) == _bits(*_exgd(eng, c, 3, tiled))
    assert _bits(*_products(eng, c, tiled)) != _bits(gl, jt, jv)      # ... and the rows of the case do differ
  eng.close()


@pytest.mark.parametrize("thunk", [t for _, t in PARITY], ids=[i for i, _ in PARITY])
def test_parity_with_the_oracle(thunk):
  _parity(thunk())


# ---- 2. the network system under Hermite-Simpson: the same three kernels with the network evaluated per lane ------------------------------
def test_node_cartpole_parity_with_the_oracle():
  _parity(P.node_case())


# ---- 3. shapes of the collocation products -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", P.PRODUCT_SHAPE_N)
@pytest.mark.parametrize("scheme", P.SCHEMES)
def test_shapes_of_the_collocation_products(scheme, N):
  """one thread per (instance, point) for J^T lam, per (instance, interval) for J v, 256 to a block: B = 63, 65, 257 put an instance's points across
  block edges and leave a ragged last block"""
  c, ref = P.product_shape(scheme, N)
  eng = _engine(c)
  alone = [_products(eng, _row(c, b)) for b in range(max(P.PRODUCT_SHAPE_B))]
  for B in P.PRODUCT_SHAPE_B:
    outs = _products(eng, P.head(c, B))
    _against_oracle_rows(c, B, outs, ref, ("gl", "jt", "jv"), f"CARTPOLE {scheme} N={N} B={B}")
    for k in range(3):
      assert outs[k].shape[0] == B
      assert _bits(outs[k]) == _bits(*[alone[b][k] for b in range(B)]), (B, k)
  eng.close()


# ---- 4. shapes of myr_exgd (collocation) -------------------------------------------------------------------------------------------------
def _exgd_shapes(name, scheme, N, batches, steps):
  c, refs = P.exgd_shape(name, scheme, N, max(batches), steps)
  eng = _engine(c)
  for nsteps in steps:
    alone = [_exgd(eng, _row(c, b), nsteps) for b in range(max(batches))]
    for B in batches:
      z, lam = _exgd(eng, P.head(c, B), nsteps)
      rows = [b for b in sorted({0, B - 1}) if b in c["rows"]]
      for b in rows:
        i = P.row_index(c, b)
        q = _steps_quantity(nsteps, (name, scheme, N, max(batches)) == P.ILL_CONDITIONED)
        _check(q, z[b:b + 1], refs[nsteps]["z_n"][i:i + 1], f"{name} {scheme} N={N} B={B} nsteps={nsteps} z row {b}")
        _check(q, lam[b:b + 1], refs[nsteps]["lam_n"][i:i + 1], f"{name} {scheme} N={N} B={B} nsteps={nsteps} lam row {b}")
      assert _bits(z) == _bits(*[alone[b][0] for b in range(B)]) and _bits(lam) == _bits(*[alone[b][1] for b in range(B)]), (B, nsteps)
  eng.close()


@pytest.mark.parametrize("scheme,N", P.EXGD_SHAPES)
def test_shapes_of_exgd(scheme, N):
  """K = 3, 63, 65, 67, 201 and 64, 65, 66 points: the `j += 64` and `k += 64` lane loops of colloc_exgd_kernel take one, two and four trips, with
  a ragged last one; B = 130 one-wavefront workgroups"""
  _exgd_shapes("CARTPOLE", scheme, N, P.EXGD_SHAPE_B, P.EXGD_SHAPE_STEPS)


@pytest.mark.parametrize("name,scheme,N,B", P.EXGD_WIDE)
def test_shapes_of_exgd_widest_points(name, scheme, N, B):
  _exgd_shapes(name, scheme, N, (B,), P.EXGD_SHAPE_STEPS)


def test_exgd_at_the_capacity_edge():
  """colloc_exgd_lds_bytes: (2 n + m + K NS) doubles + 16 bytes = 288 N + 128 for CARTPOLE Hermite-Simpson.  N = 568 (163 712 bytes) is the largest
  horizon that fits the 160 KiB; N = 569 is refused with launch_products' message and leaves z and lam as they were."""
  N = P.CAPACITY_N
  c, refs = P.exgd_shape("CARTPOLE", "HERMITE_SIMPSON", N, 2, (2,))
  assert 288 * N + 128 <= 160 * 1024 < 288 * (N + 1) + 128
  eng = _engine(c)
  z, lam = _exgd(eng, c, 2)
  eng.close()
  _check("steps3", z, refs[2]["z_n"], f"CARTPOLE HERMITE_SIMPSON N={N} z")
  _check("steps3", lam, refs[2]["lam_n"], f"CARTPOLE HERMITE_SIMPSON N={N} lam")
  eng = _engine(c, N + 1)
  rng = np.random.default_rng(569)
  z, lam = rng.standard_normal((2, eng.n)), rng.standard_normal((2, eng.m))
  lb, ub = np.full((2, eng.n), -1.0), np.full((2, eng.n), 1.0)
  z_in, lam_in = z.copy(), lam.copy()
  rc = eng.lib.myr_exgd(eng._h, 2, z.ctypes.data, lam.ctypes.data, lb.ctypes.data, ub.ctypes.data, None, 0, 0.01, 0.01, 2, _lib.MEM_HOST)
  assert rc == -4                                                                               # MYR_E_CAPACITY
  assert eng.lib.myr_last_error().decode() == "myr_exgd: intervals too large for the LDS-resident iterate"
  assert _bits(z, lam) == _bits(z_in, lam_in)
  eng.close()


# ---- 5. shapes of the SHOOTING products and steps ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,I,cpi,method", P.SHOOT_SHAPE_CASES)
def test_shapes_of_the_shooting_products_and_steps(name, I, cpi, method):
  """one lane per instance, 64 to a block: B = 63, 65, 130 are a ragged wavefront, one lane of a second, a ragged third"""
  c, ref, refs = P.shoot_shape(name, I, cpi, method)
  eng = _engine(c)
  top = max(P.SHOOT_SHAPE_B)
  alone = [_products(eng, _row(c, b)) for b in range(top)]
  alone_steps = {k: [_exgd(eng, _row(c, b), k) for b in range(top)] for k in P.SHOOT_SHAPE_STEPS}
  for B in P.SHOOT_SHAPE_B:
    what = f"{name} {I}x{cpi} {method} B={B}"
    h = P.head(c, B)
    outs = _products(eng, h)
    _against_oracle_rows(c, B, outs, ref, ("gl", "jt", "jv"), what)
    for k in range(3):
      assert _bits(outs[k]) == _bits(*[alone[b][k] for b in range(B)]), (B, k)
    for nsteps in P.SHOOT_SHAPE_STEPS:
      zl = _exgd(eng, h, nsteps)
      q = _steps_quantity(nsteps)
      _against_oracle_rows(c, B, zl, refs[nsteps], (q, q), f"{what} nsteps={nsteps}")
      assert _bits(zl[0]) == _bits(*[alone_steps[nsteps][b][0] for b in range(B)]), (B, nsteps)
      assert _bits(zl[1]) == _bits(*[alone_steps[nsteps][b][1] for b in range(B)]), (B, nsteps)
  eng.close()


# ---- 6. the grid-stride loops ----------------------------------------------------------------------------------------------------------------
GRID_B, GRID_DISTINCT = 2_200_000, 1000


def _tiled(c):
  out = dict(c)
  for k in ("z", "lam", "v", "lb", "ub", "params"):
    out[k] = np.tile(c[k], (GRID_B // GRID_DISTINCT, 1))
  return out


def _same_rows(big, small):
  return (big.reshape(GRID_B // GRID_DISTINCT, *small.shape) == small[None]).all()


def test_grid_stride_loops_of_the_collocation_kernels():
  """SIMPLECASE trapezoidal N = 2 (K = 3 points, n = 6, m = 2) at B = 2 200 000: B K = 6.6e6 and B N = 4.4e6 units, both above the 16384 x 256 =
  4 194 304 that grid_for caps a grid at, so threads of colloc_vjp_kernel and colloc_jvp_kernel take a second trip; myr_exgd runs B one-wavefront
  workgroups.  1 000 distinct instances tiled: every row must have the bits of its source row in a 1 000-instance call.
  The handle: myr_create sizes nothing by max_batch (a hint); the call's staging buffer grows to what one call moves -- 106 + 35 + 106 MB for
  myr_vjp, 3 x 106 + 35 MB for myr_exgd -- and the products need no solver workspace: under 0.4 GB of device memory in all."""
  base = P.head(P._normalised("colloc", P.E._draw("SIMPLECASE", "TRAPEZOIDAL", 2, 1, GRID_DISTINCT, 0)), GRID_DISTINCT)
  K, n, m = P.E.dims("SIMPLECASE", "TRAPEZOIDAL", 2)
  assert GRID_B * K > GRID_CAP and GRID_B * 2 > GRID_CAP and GRID_B % GRID_DISTINCT == 0
  big = _tiled(base)
  eng = _engine(base)
  small = _products(eng, base) + _exgd(eng, base, 1)
  assert all(np.isfinite(a).all() for a in small) and len({_bits(a[b]) for a in small[:1] for b in range(GRID_DISTINCT)}) == GRID_DISTINCT
  for out, ref in zip(_products(eng, big) + _exgd(eng, big, 1), small):
    assert _same_rows(out, ref)
  eng.close()


def test_grid_stride_loop_of_the_shooting_update():
  """SIMPLECASE 1 x 1 Euler (n = 4, m = 1) at B = 2 200 000: B n = 8.8e6 elements, above the cap of exgd_update_kernel's grid; shoot_eval_kernel
  runs 34 375 workgroups of 64 lanes.  One step, the same comparison.  The handle's shared scratch grows to B (2 NS + 2 n + m) doubles = 194 MB
  next to 317 MB of staged arrays."""
  base = P._normalised("shoot", P.S._draw("SIMPLECASE", 1, 1, "EULER", 1, GRID_DISTINCT, 0))
  assert GRID_B * base["n"] > GRID_CAP and base["n"] == 4
  big = _tiled(base)
  eng = _engine(base)
  small = _products(eng, base) + _exgd(eng, base, 1)
  assert all(np.isfinite(a).all() for a in small)
  for out, ref in zip(_products(eng, big) + _exgd(eng, big, 1), small):
    assert _same_rows(out, ref)
  eng.close()


# ---- 7. what ran before does not reach the result --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", ["HERMITE_SIMPSON", "SHOOTING"])
def test_what_ran_before_does_not_reach_the_result(tr):
  """the SHOOTING products live in the handle's shared scratch buffer, every call's arrays in its staging buffer: a call gives the same bits before
  and after a larger call of each kind and a solve on the same handle"""
  if tr == "SHOOTING":
    c, _, _ = P.shoot_shape("CARTPOLE", 4, 3, "RK4")
  else:
    c, _ = P.exgd_shape("CARTPOLE", "HERMITE_SIMPSON", 33, max(P.EXGD_SHAPE_B), P.EXGD_SHAPE_STEPS)
  small, large = P.head(c, 3), P.head(c, 130)
  eng = _engine(c)
  before = _bits(*_products(eng, small), *_exgd(eng, small, 2))
  big = _bits(*_products(eng, large), *_exgd(eng, large, 2))
  opts = eng.default_opts()
  opts.max_iter = 3
  wide = np.where(np.arange(c["n"]) < c["ns"], 0.0, 50.0)
  res = eng.solve(large["z"][:5], large["z"][:5] - wide, large["z"][:5] + wide, opts=opts)
  assert res["z"].shape == (5, c["n"])
  after = _bits(*_products(eng, small), *_exgd(eng, small, 2))
  assert after == before
  assert _bits(*_products(eng, large), *_exgd(eng, large, 2)) == big
  eng.close()


# ---- 8. adjoint identity and linearity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,N,cpi,method", [("TRAPEZOIDAL", 20, 1, "HEUN"), ("SHOOTING", 4, 5, "RK4")])
def test_adjoint_identity_and_linearity(tr, N, cpi, method):
  """test_gpu_products.test_products_full_size_adjoint_identity_and_linearity's properties and bounds for the two forms that have none: <J v, lam> =
  <v, J^T lam>, J^T linear in lam, grad L = grad f + J^T lam with grad f from the eval kernel"""
  B = 65
  c = P.H.inputs("CARTPOLE", tr, N, cpi, method, B)
  eng = _engine(c)
  rng = np.random.default_rng(8)
  z, lam, v, p = c["z"], rng.standard_normal((B, eng.m)), c["v"], c["params"]
  lam2 = rng.standard_normal((B, eng.m))
  jv, jtl = eng.jvp(z, v, params=p), eng.vjp(z, lam, params=p)
  lhs, rhs = (jv * lam).sum(1), (v * jtl).sum(1)
  assert np.abs(lhs).max() > 0 and np.abs(lhs - rhs).max() <= 1e-10 * max(1.0, np.abs(lhs).max())
  comb = eng.vjp(z, 2.0 * lam - 0.5 * lam2, params=p)
  np.testing.assert_allclose(comb, 2.0 * jtl - 0.5 * eng.vjp(z, lam2, params=p), rtol=1e-11, atol=1e-11)
  g = eng.eval(z, params=p, want=("gradf",))["gradf"]
  gf = np.zeros((B, eng.n)); gf[:, eng.n - eng.ngrad:] = g
  assert np.abs(g).max() > 0
  np.testing.assert_allclose(eng.vjp(z, lam, params=p, add_gradf=True), gf + jtl, rtol=1e-12, atol=1e-12)
  eng.close()
