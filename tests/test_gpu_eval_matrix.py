"""myr_eval and myr_rollout on the device -- hs_eval_kernel (myriad_amd/csrc/hs_eval.h, both collocation schemes and the matrix-core pass of the
network system), shoot_eval_kernel without lamin (shoot_eval.h), rollout_kernel (rollout.h, myriad_hip.hip) -- against the oracle for every system,
and against themselves across workgroup forms, batch sizes, forms of the call and what ran before on the handle.  The cases and their references are
tests/eval_cases.py's; tests/test_eval_cases.py checks those references on themselves.  Everything goes through _lib.Engine.

Tolerances.  Bit equalities are exact.  A comparison with the oracle is held to
  bound(case, quantity) = min(CEIL, max(1e-13, 10 x response(case, quantity)))
of rel_error (the largest |d| / max|ref| of a row; eval_cases.py says what a row is): CEIL is 1e-12 for f and c, which the older eval tests already
hold them to, and 1e-11 for gradf, J, xs and cost (test_gpu_exgd_grad.ORACLE_TOL); `response` is the oracle's own answer to one ulp of its inputs,
10 x the project's margin for contracted multiply-adds and the device's libm; the floor is 30 x the worst figure the products matrix measured for
the sibling kernels on the same draws.  None of it comes from what these kernels return.  A reference row that is exactly zero (f and gradf of
TUMOUR under Hermite-Simpson, whose cost is terminal only; a state that never moves) is compared absolutely against 1e-13 max(1, max|input|).

MEASURED, on an MI355X with the cases as they stand: per quantity, the worst figure over every comparison with the oracle in this module (3 829 of
them; every comparison prints a `MEASURE quantity value case` line) and its case:
  f       1.96e-15   BACTERIA SHOOTING 3 x 2 Euler, row 0
  gradf   1.31e-14   VANDERPOL_ELASTIC SHOOTING 3 x 2 RK4, row 0
  c       1.83e-14   BEARPOPULATIONS SHOOTING 1 x 4 RK4, row 0
  J       8.91e-15   VANDERPOL_ELASTIC SHOOTING 3 x 2 RK4, row 2
  xs      2.56e-14   HIVTREATMENT Heun, S = 1 (one step of 10), row 1
  cost    1.12e-14   HARVEST midpoint, S = 1, row 0
The zero rows (TUMOUR Hermite-Simpson f and gradf) come back as exact zeros.  The one case listed as ill-conditioned, HIVTREATMENT midpoint S = 40
(eval_cases.ROLLOUT_ILL_CONDITIONED: the oracle answers one ulp with 2.5e-12), measures 2.1e-15 in xs and 1.5e-16 in cost.  No case is near its
bound, and no kernel changed.

Wall time, the whole module: 12 s on an MI355X machine (446 tests; the slowest, the first to load the library and build a case, 1.6 s; no other above
0.4 s).  tests/test_eval_cases.py: 32 s on a host without a device (476 tests).
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import eval_cases as EC
from myriad_amd import _lib
from myriad_amd.trajectory_optimizers import hs_dense_from_blocks, shoot_dense_from_blocks, trap_dense_from_blocks
from test_gpu_eval import _full_grad

pytestmark = pytest.mark.gpu

WANT = ("f", "gradf", "c", "jblk")
FORMS = tuple(itertools.product(("1", "4", "8"), ("0", "1")))      # (MYRIAD_EVAL_WPT, MYRIAD_EVAL_NT)
SAME_BLOCK = (("4", "1"), ("1", "0"), ("4", "0"), ("8", "0"))       # 256 threads: without NT the launcher always runs <4, false>


def _bits(*arrays):
  return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _engine(c, N=None):
  return _lib.Engine(c["name"], c["tr"], c["N"] if N is None else N, c["T"], controls_per_interval=c["cpi"], integration_method=c["method"])


def _eval(eng, c, want=WANT, params="case"):
  return eng.eval(c["z"], params=c["params"] if isinstance(params, str) else params, want=want)


def _all(out):
  return _bits(*[out[k] for k in WANT])


def _check(c, quantity, out, ref, top, what):
  """rows of `out` against rows of `ref` under bound(case, quantity); a zero reference row absolutely"""
  ref = np.atleast_2d(np.asarray(ref))
  out = np.asarray(out, dtype=np.float64).reshape(ref.shape)
  assert np.isfinite(out).all(), (quantity, what)
  den = np.abs(ref).max(axis=-1)
  zero = den == 0.0
  if zero.any():
    a = float(np.abs(out[zero]).max())
    print(f"MEASURE {quantity}_zero_row {a:.3e} {what}")
    assert a <= EC.ZERO_ROW * max(1.0, top), (quantity, what, a)
  if (~zero).any():
    e = EC.rel_error(out[~zero], ref[~zero])
    print(f"MEASURE {quantity} {e:.3e} {what}")
    assert e <= EC.bound(c, quantity), (quantity, what, e, EC.bound(c, quantity))


def _dense(c, jblk):
  N, ns, nu = c["N"], c["ns"], c["nu"]
  blk = np.asarray(jblk).reshape(N, -1)
  if c["tr"] == "HERMITE_SIMPSON":
    J = hs_dense_from_blocks(blk, N, ns, nu)
  elif c["tr"] == "TRAPEZOIDAL":
    J = trap_dense_from_blocks(blk, N, ns, nu)
  else:
    J = shoot_dense_from_blocks(blk, N, EC.mc(c) * c["cpi"], ns, nu)
  rows = EC.jrows(c)
  return (J if rows is None else J[rows]).reshape(-1)


def _against_oracle(c, eng, out, rows, what, skip=()):
  """instances `rows` of a call's outputs (its row b is instance b of the case) against the case's reference"""
  ref = EC.eval_reference(c)
  g = _full_grad(eng, out["gradf"]) if "gradf" in out else None
  for b in rows:
    i = EC.row_index(c, b)
    top = float(np.abs(c["z"][b]).max())
    w = f"{what} row {b}"
    if "f" in out and "f" not in skip:
      _check(c, "f", out["f"][b:b + 1], ref["f"][i], top, w)
    if g is not None:
      _check(c, "gradf", g[b], ref["gradf"][i], top, w)
    if "c" in out:
      _check(c, "c", out["c"][b], ref["c"][i], top, w)
    if "jblk" in out:
      _check(c, "J", _dense(c, out["jblk"][b]), ref["J"][i], top, w)


# ---- 1. parity, every system ------------------------------------------------------------------------------------------------------------------
PARITY = EC.parity_cases()


@pytest.mark.parametrize("thunk", [t for _, t in PARITY], ids=[i for i, _ in PARITY])
def test_eval_parity_with_the_oracle(thunk):
  c = thunk()
  B = c["z"].shape[0]
  kept = (c["z"].copy(), c["params"].copy())
  eng = _engine(c)
  assert (eng.n, eng.m, eng.ns, eng.nu) == (c["n"], c["m"], c["ns"], c["nu"])
  out = _eval(eng, c)
  _against_oracle(c, eng, out, range(B), EC.what(c))
  assert _bits(*kept) == _bits(c["z"], c["params"])
  if c["params"].ndim == 2:      # the shared-parameter form = the same row for every instance; and the rows of the case do differ
    shared = _eval(eng, c, params=c["params"][0].copy())
    assert _all(shared) == _all(_eval(eng, c, params=np.tile(c["params"][0], (B, 1))))
    assert _bits(shared["c"][0]) == _bits(out["c"][0]) and _bits(shared["c"][1:]) != _bits(out["c"][1:])
  eng.close()


# ---- 2. workgroup forms of hs_eval_kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tr,N", EC.FORM_CASES, ids=[f"{a}-{b}-{n}" for a, b, n in EC.FORM_CASES])
def test_workgroup_forms_of_hs_eval(name, tr, N, monkeypatch):
  """MYRIAD_EVAL_WPT x MYRIAD_EVAL_NT, read at myr_create: 64, 256 and 512 threads over K points and over the output elements, temporal and
  non-temporal stores.  c, jblk and gradf do not depend on the form; f is summed per wavefront and then across them, so its bits are those of
  every form with the same block size.  BEARPOPULATIONS (JPI = 75, odd) takes the scalar jblk store loop, and at B = 3 instance 1 starts at an odd
  offset; HIVTREATMENT (JPI = 90) is its even neighbour.  The network system deals 16-point tiles over the wavefronts."""
  c = EC.form_case(name, tr, N)
  outs = {}
  for wpt, nt in FORMS:
    monkeypatch.setenv("MYRIAD_EVAL_WPT", wpt)
    monkeypatch.setenv("MYRIAD_EVAL_NT", nt)
    eng = _engine(c)
    outs[wpt, nt] = _eval(eng, c)
    w = f"{EC.what(c)} WPT={wpt} NT={nt}"
    if (wpt, nt) == FORMS[0]:
      _against_oracle(c, eng, outs[wpt, nt], (0, EC.B - 1), w)
    else:      # (c, jblk and gradf have the bits of the first form, below)
      _against_oracle(c, eng, {"f": outs[wpt, nt]["f"]}, (0, EC.B - 1), w)
    eng.close()
  first = outs[FORMS[0]]
  for form, out in outs.items():
    assert _bits(out["c"], out["jblk"], out["gradf"]) == _bits(first["c"], first["jblk"], first["gradf"]), form
  for form in SAME_BLOCK:
    assert _bits(outs[form]["f"]) == _bits(outs[SAME_BLOCK[0]]["f"]), form


# ---- 3. batch shapes: a row's result does not depend on its batch -----------------------------------------------------------------------------
def _batch_shapes(c, batches):
  eng = _engine(c)
  top = max(batches)
  p0 = c["params"][0].copy()
  alone = [_eval(eng, EC.one(c, b)) for b in range(top)]
  alone_shared = [_eval(eng, EC.one(c, b), params=p0) for b in range(top)]
  assert _all(alone_shared[0]) == _all(alone[0]) and _all(alone_shared[1]) != _all(alone[1])
  for B in batches:
    h = EC.head(c, B)
    out = _eval(eng, h)
    _against_oracle(c, eng, out, sorted({0, B - 1}), f"{EC.what(c)} B={B}")
    shared = _eval(eng, h, params=p0)
    for k in WANT:
      assert out[k].shape[0] == B
      assert _bits(out[k]) == _bits(*[alone[b][k] for b in range(B)]), (B, k)
      assert _bits(shared[k]) == _bits(*[alone_shared[b][k] for b in range(B)]), (B, k, "shared")
  eng.close()


@pytest.mark.parametrize("name,I,cpi,method", EC.SHOOT_BATCH_CASES)
def test_batch_shapes_of_shoot_eval(name, I, cpi, method):
  """one trajectory per lane, 64 to a block, the states of the current interval in b (cpi + 1) NS doubles of the handle's scratch: B = 63, 65, 257
  are a ragged wavefront, one lane of a second, one lane of a fifth"""
  _batch_shapes(EC.shoot_batch_case(name, I, cpi, method), EC.SHOOT_BATCHES)


@pytest.mark.parametrize("tr", ["HERMITE_SIMPSON", "TRAPEZOIDAL"])
def test_batch_shapes_of_hs_eval(tr):
  _batch_shapes(EC.colloc_batch_case(tr), EC.COLLOC_BATCHES)


def test_a_grid_beyond_65535_workgroups():
  """CARTPOLE Hermite-Simpson N = 1 at B = 70 000: one workgroup per instance.  Three distinct rows tiled; every row has the bits of its source
  row in a B = 3 call."""
  c = EC.eval_case("closed", "CARTPOLE", "HERMITE_SIMPSON", 1)
  big_B = 70_000
  reps = -(-big_B // EC.B)
  z, p = np.tile(c["z"], (reps, 1))[:big_B], np.tile(c["params"], (reps, 1))[:big_B]
  eng = _engine(c)
  small = _eval(eng, c, want=("f", "c"))
  big = eng.eval(z, params=p, want=("f", "c"))
  eng.close()
  assert set(big) == {"f", "c"} and len({_bits(small["c"][b]) for b in range(EC.B)}) == EC.B
  for k in ("f", "c"):
    assert (big[k] == np.tile(small[k], (reps,) + (1,) * (small[k].ndim - 1))[:big_B]).all(), k


# ---- 4. forms of the call ----------------------------------------------------------------------------------------------------------------------
CALL_CASES = (("HERMITE_SIMPSON", EC.HS_N, 1, "HEUN"), ("TRAPEZOIDAL", EC.TRAP_N, 1, "HEUN"), ("SHOOTING", 3, 2, "RK4"))


@pytest.mark.parametrize("tr,N,cpi,method", CALL_CASES)
def test_each_output_alone_and_every_pair(tr, N, cpi, method):
  c = EC.eval_case("closed", "CARTPOLE", tr, N, cpi, method)
  kept = (c["z"].copy(), c["params"].copy())
  eng = _engine(c)
  full = _eval(eng, c)
  for want in [(k,) for k in WANT] + list(itertools.combinations(WANT, 2)):
    out = _eval(eng, c, want=want)
    assert set(out) == set(want)
    for k in want:
      assert _bits(out[k]) == _bits(full[k]), (want, k)
    assert _bits(*kept) == _bits(c["z"], c["params"])
  assert _eval(eng, c, want=()) == {}
  eng.close()


@pytest.mark.parametrize("tr,N,cpi,method", CALL_CASES)
def test_device_pointers_give_the_bits_of_the_host_path(tr, N, cpi, method):
  import torch
  c = EC.eval_case("closed", "CARTPOLE", tr, N, cpi, method)
  B = c["z"].shape[0]
  eng = _engine(c)
  host = _eval(eng, c)
  dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).cuda()      # (a copy: the arrays of a case are read-only)
  zt, pt = dev(c["z"]), dev(c["params"])
  mk = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
  f, g, cc, j = mk(B), mk(B, eng.ngrad), mk(B, eng.m), mk(B, eng.jblk)
  torch.cuda.synchronize()
  eng.eval_device(B, zt, params=pt, params_stride=eng.np, f=f, gradf=g, c=cc, jblk=j)
  torch.cuda.synchronize()
  for k, t in zip(WANT, (f, g, cc, j)):
    assert _bits(t.cpu().numpy()) == _bits(host[k]), k
  assert _bits(zt.cpu().numpy(), pt.cpu().numpy()) == _bits(c["z"], c["params"])
  eng.close()


def test_the_shooting_scratch_grows_and_the_result_stays():
  """on one handle B = 1, then B = 257 (ensure_buf grows the per-lane scratch), then B = 1 again"""
  c = EC.shoot_batch_case("CARTPOLE", 4, 3, "RK4")
  eng = _engine(c)
  first = _eval(eng, EC.head(c, 1))
  big = _eval(eng, c)
  assert _all(_eval(eng, EC.head(c, 1))) == _all(first)
  assert _bits(*[big[k][0] for k in WANT]) == _all(first)
  eng.close()


@pytest.mark.parametrize("tr,N,cpi,method", CALL_CASES)
def test_eval_after_a_solve_and_a_rollout_on_the_handle(tr, N, cpi, method):
  c = EC.eval_case("closed", "CARTPOLE", tr, N, cpi, method)
  fresh = _engine(c)
  want = _all(_eval(fresh, c))
  fresh.close()
  eng = _engine(c)
  opts = eng.default_opts()
  opts.max_iter = 3
  wide = np.where(np.arange(c["n"]) < c["ns"], 0.0, 50.0)
  res = eng.solve(c["z"], c["z"] - wide, c["z"] + wide, params=c["params"], opts=opts)
  assert res["z"].shape == c["z"].shape
  assert _all(_eval(eng, c)) == want
  r = EC.rollout_case("closed", "CARTPOLE", method, EC.ROWS_S)
  xs, cost = eng.rollout(r["x0"], r["us"], r["S"], params=r["params"])
  assert np.isfinite(xs).all() and np.isfinite(cost).all()
  assert _all(_eval(eng, c)) == want
  eng.close()


# ---- 5. capacity -------------------------------------------------------------------------------------------------------------------------------
CAPACITY_TEXT = "hs_eval: intervals too large for the 160 KiB LDS record"


def test_eval_at_the_capacity_edge(monkeypatch):
  """hs_eval_lds_bytes (test_eval_cases.py restates it): N = 347 needs 163 728 of the 163 840 bytes with eight wavefronts, N = 348 more with one"""
  c = EC.capacity_case()
  outs = {}
  for wpt in ("1", "8"):
    monkeypatch.setenv("MYRIAD_EVAL_WPT", wpt)
    eng = _engine(c)
    outs[wpt] = _eval(eng, c)
    if wpt == "1":
      _against_oracle(c, eng, outs[wpt], (1,), f"{EC.what(c)} WPT={wpt}")
    else:
      _against_oracle(c, eng, {"f": outs[wpt]["f"]}, (1,), f"{EC.what(c)} WPT={wpt}")
    eng.close()
  assert _bits(*[outs["8"][k] for k in ("gradf", "c", "jblk")]) == _bits(*[outs["1"][k] for k in ("gradf", "c", "jblk")])


@pytest.mark.parametrize("nt", ["0", "1"])
@pytest.mark.parametrize("wpt", ["1", "4", "8"])
def test_eval_beyond_the_capacity_edge_is_refused(wpt, nt, monkeypatch):
  """the launcher steps 8 -> 4 -> 1 wavefronts down and then refuses; nothing is written, and a handle created afterwards works"""
  monkeypatch.setenv("MYRIAD_EVAL_WPT", wpt)
  monkeypatch.setenv("MYRIAD_EVAL_NT", nt)
  c = EC.capacity_case()
  eng = _engine(c, EC.CAPACITY_N + 1)
  z = np.random.default_rng(348).standard_normal((2, eng.n))
  z_in = z.copy()
  f, g, cc, j = np.full(2, 7.0), np.full((2, eng.ngrad), 7.0), np.full((2, eng.m), 7.0), np.full((2, eng.jblk), 7.0)
  rc = eng.lib.myr_eval(eng._h, 2, z.ctypes.data, None, 0, f.ctypes.data, g.ctypes.data, cc.ctypes.data, j.ctypes.data, _lib.MEM_HOST)
  assert rc == -4                                                                               # MYR_E_CAPACITY
  assert eng.lib.myr_last_error().decode() == CAPACITY_TEXT
  assert _bits(z) == _bits(z_in) and all((a == 7.0).all() for a in (f, g, cc, j))
  eng.close()
  small = EC.eval_case("closed", "CARTPOLE", "HERMITE_SIMPSON", EC.HS_N)
  eng = _engine(small)
  _against_oracle(small, eng, _eval(eng, small), range(EC.B), f"{EC.what(small)} after the refusal WPT={wpt} NT={nt}")
  eng.close()


@pytest.mark.parametrize("name,N,lands", EC.STEP_DOWN)
def test_the_step_down_in_front_of_the_refusal(name, N, lands, monkeypatch):
  """horizons that fit the 160 KiB with 4 or 1 wavefronts and not with 8 (test_eval_cases.test_step_down_arithmetic): asked for 8, the launcher
  steps down and launches; the result has the bits of the form it lands on, and is the oracle's"""
  c = EC.form_case(name, "HERMITE_SIMPSON", N)
  monkeypatch.setenv("MYRIAD_EVAL_NT", "1")
  outs = {}
  for wpt in ("8", str(lands)):
    monkeypatch.setenv("MYRIAD_EVAL_WPT", wpt)
    eng = _engine(c)
    outs[wpt] = _eval(eng, c)
    eng.close()
  _against_oracle(c, eng, outs["8"], (0, EC.B - 1), f"{EC.what(c)} WPT=8 -> {lands}")
  assert _all(outs["8"]) == _all(outs[str(lands)])


# ---- 6. myr_rollout ----------------------------------------------------------------------------------------------------------------------------
def _rollout_engine(c):
  return _lib.Engine(c["name"], "SHOOTING", 1, c["T"], controls_per_interval=c["S"], integration_method=c["method"])


def _rollout(eng, c, want_xs=True, params="case"):
  return eng.rollout(c["x0"], c["us"], c["S"], params=c["params"] if isinstance(params, str) else params, want_xs=want_xs)


def _rollout_against_oracle(c, xs, cost, rows, what):
  ref = EC.rollout_reference(c)
  for b in rows:
    i = EC.row_index(c, b)
    top = max(float(np.abs(c["x0"][b]).max()), float(np.abs(c["us"][b]).max()))
    _check(c, "xs", EC._rows_of_xs(xs[b]), EC._rows_of_xs(ref["xs"][i]), top, f"{what} row {b}")
    _check(c, "cost", cost[b:b + 1], ref["cost"][i], top, f"{what} row {b}")


def _rollout_parity(c):
  B = c["x0"].shape[0]
  kept = (c["x0"].copy(), c["us"].copy(), c["params"].copy())
  eng = _rollout_engine(c)
  xs, cost = _rollout(eng, c)
  assert xs.shape == (B, c["S"] + 1, c["ns"]) and _bits(xs[:, 0]) == _bits(c["x0"])
  _rollout_against_oracle(c, xs, cost, range(B), EC.rollout_what(c))
  none, cost_only = _rollout(eng, c, want_xs=False)
  assert none is None and _bits(cost_only) == _bits(cost)
  assert _bits(*kept) == _bits(c["x0"], c["us"], c["params"])
  if c["params"].ndim == 2:
    shared = _rollout(eng, c, params=c["params"][0].copy())
    assert _bits(*shared) == _bits(*_rollout(eng, c, params=np.tile(c["params"][0], (B, 1))))
    assert _bits(shared[0][0]) == _bits(xs[0]) and _bits(shared[0][1:]) != _bits(xs[1:])
  eng.close()


ROLLOUT_PARITY = EC.rollout_parity_cases()


@pytest.mark.parametrize("thunk", [t for _, t in ROLLOUT_PARITY], ids=[i for i, _ in ROLLOUT_PARITY])
def test_rollout_parity_with_the_oracle(thunk):
  _rollout_parity(thunk())


ROWS = EC.rows_cases()


@pytest.mark.parametrize("thunk", [t for _, t in ROWS], ids=[i for i, _ in ROWS])
def test_rollout_control_rows(thunk):
  """u_rows exactly consumed, longer (the terminal cost takes the array's last row, as the oracle's us[-1] does), S (the last step clamps) and 1 (a
  constant control), on a plain system, one with a terminal cost and one with time in the cost"""
  _rollout_parity(thunk())


@pytest.mark.parametrize("name,method,S", [("CARTPOLE", "RK4", 7), ("HARVEST", "HEUN", 40)])
def test_batch_shapes_of_rollout(name, method, S):
  c = EC.rollout_batch_case(name, method, S)
  eng = _rollout_engine(c)
  top = max(EC.ROLLOUT_BATCHES)
  p0 = c["params"][0].copy()
  alone = [_rollout(eng, EC.one(c, b)) for b in range(top)]
  alone_shared = [_rollout(eng, EC.one(c, b), params=p0) for b in range(top)]
  assert _bits(*alone_shared[0]) == _bits(*alone[0]) and _bits(*alone_shared[1]) != _bits(*alone[1])
  for B in EC.ROLLOUT_BATCHES:
    h = EC.head(c, B)
    xs, cost = _rollout(eng, h)
    _rollout_against_oracle(c, xs, cost, sorted({0, B - 1}), f"{EC.rollout_what(c)} B={B}")
    assert _bits(xs) == _bits(*[a[0] for a in alone[:B]]) and _bits(cost) == _bits(*[a[1] for a in alone[:B]]), B
    xs, cost = _rollout(eng, h, params=p0)
    assert _bits(xs) == _bits(*[a[0] for a in alone_shared[:B]]) and _bits(cost) == _bits(*[a[1] for a in alone_shared[:B]]), (B, "shared")
  eng.close()


@pytest.mark.parametrize("method", EC.METHODS)
def test_rollout_device_pointers_give_the_bits_of_the_host_path(method):
  import torch
  c = EC.rollout_case("closed", "CARTPOLE", method, EC.ROWS_S)
  B, S = c["x0"].shape[0], c["S"]
  eng = _rollout_engine(c)
  xs, cost = _rollout(eng, c)
  dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).cuda()      # (a copy: the arrays of a case are read-only)
  x0t, ust, pt = dev(c["x0"]), dev(c["us"]), dev(c["params"])
  xst = torch.full((B, S + 1, c["ns"]), float("nan"), dtype=torch.float64, device="cuda")
  ct = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
  torch.cuda.synchronize()
  p = C.c_void_p
  rc = eng.lib.myr_rollout(eng._h, B, S, c["us"].shape[1], p(x0t.data_ptr()), p(ust.data_ptr()), p(pt.data_ptr()), eng.np, p(xst.data_ptr()),
                           p(ct.data_ptr()), _lib.MEM_DEVICE)
  assert rc == 0, eng.lib.myr_last_error().decode()
  torch.cuda.synchronize()
  assert _bits(xst.cpu().numpy(), ct.cpu().numpy()) == _bits(xs, cost)
  assert _bits(x0t.cpu().numpy(), ust.cpu().numpy(), pt.cpu().numpy()) == _bits(c["x0"], c["us"], c["params"])
  eng.close()


@pytest.mark.parametrize("method", EC.METHODS)
@pytest.mark.parametrize("name", EC.ROWS_SYSTEMS)
def test_single_shooting_is_the_rollout(name, method):
  """the device-side twin of test_eval_cases.test_single_shooting_is_the_rollout_on_the_oracle: shooting eval at I = 1, cpi = S (ShootCore::sval)
  against the rollout of the same (x0, us) (Rollout::run): f against cost, c + x1 against xs[S].  Both are held to the oracle's rollout, so the two
  paths agree within twice the bound."""
  r = EC.rollout_case("closed", name, method, EC.ROWS_S)
  ref = EC.rollout_reference(r)
  B, S = r["x0"].shape[0], r["S"]
  x1 = ref["xs"][:, S] + 0.25
  z = np.concatenate([r["x0"], x1, r["us"].reshape(B, -1)], axis=1)
  sh = _lib.Engine(name, "SHOOTING", 1, r["T"], controls_per_interval=S, integration_method=method)
  assert sh.n == z.shape[1]
  out = sh.eval(z, params=r["params"], want=("f", "c"))
  sh.close()
  top = float(np.abs(z).max())
  _check(r, "cost", out["f"][:, None], ref["cost"], top, f"{EC.rollout_what(r)} shooting f")
  _check(r, "xs", out["c"] + x1, ref["xs"][:, S], top, f"{EC.rollout_what(r)} shooting c + x1")
  eng = _rollout_engine(r)
  xs, cost = _rollout(eng, r)
  eng.close()
  _check(r, "cost", cost[:, None], ref["cost"], top, f"{EC.rollout_what(r)} rollout cost")
  _check(r, "xs", xs[:, S], ref["xs"][:, S], top, f"{EC.rollout_what(r)} rollout xs[S]")
