"""Inputs and oracle references shared by the tests of the two entry points everything else rests on -- myr_eval and myr_rollout
(test_eval_cases.py, test_gpu_eval_matrix.py).

Nothing is drawn where a draw exists:
  eval, closed-form systems   hvp_cases._draw (seed 0 = hvp_cases.inputs): z and a parameter row per instance; the reference through
                              hvp_cases._transcription at the instance's own row
  eval, elastic twins         the recipe of test_gpu_elastic.test_twin_callbacks_match_the_oracle: O.Elastic(base, rho = 37.5), the guess x (1 + 5 %)
                              + 0.3 N(0, 1), with a parameter row per instance (the defaults, rho among them, moved by up to 5 %); also under SHOOTING
  eval, NODE_CARTPOLE         node_hvp_cases.inputs / _transcription, the committed weights shared by the batch
  rollout                     fit_cases.inputs(per_instance=True): x0 = xs_obs[:, 0], us, params; T = fit_cases.horizon (steps of at most 0.05);
                              the reference is O.get_state_trajectory_and_cost on fit_cases.make_system at the instance's row with T set.  The twins
                              (controls and slacks from fit_cases._controls: a slack lies inside [-0.5, 0.5]) and the network system have no draw
                              anywhere and get one here.

The reference of an instance: f, gradf (the full n-vector), c and the dense J of O.Callbacks; for a rollout xs and cost.  Long horizons keep of J
only the rows of the first and the last interval (`jrows`).

Conditioning, recorded with every case (`response`, one figure per quantity): the oracle evaluates every reference row a second time from inputs
-- z or x0 and us, and the parameter row -- each entry moved by -1, 0 or +1 ulp (a fixed pattern); the figure is the largest rel_error between the two
runs.  It measures the reference alone.  An eval case above MAX_RESPONSE is redrawn from the seeds 0 .. 19; test_eval_cases.py asserts the figure.
The weights of the network system are not moved (4 804 entries shared by every case).

rel_error is exgd_grad_cases': the largest |d| / max|ref| of a row.  A row is an instance (J flattened), and for the states of a rollout one
state component of an instance over time, so that a component of order 0.01 is not measured against one of order 1 000 (HIVTREATMENT).

TIMBERHARVEST: its default r is 0, which makes the time argument of its cost invisible; `discounted=True` replaces that one parameter by 0.3, as
products_cases does.
"""
import functools

import numpy as np
import torch

import fit_cases as F
import hvp_cases as H
import node_hvp_cases as NH
from exgd_grad_cases import rel_error
from hvp_cases import O
from products_cases import DISCOUNT_R, MAX_RESPONSE, SHOOT_EXTRA_SHAPES, SHOOT_EXTRA_SYSTEMS, SHOOT_SHAPES  # noqa: F401

SYSTEMS = H.SYSTEMS
METHODS = F.METHODS
TWINS = ("PENDULUM", "ROCKETLANDING", "CARTPOLE", "VANDERPOL", "MOUNTAINCAR")
TWIN_RHO = 37.5
B = 3
HS_N, TRAP_N = 6, 7
TWIN_SHAPES = (("HERMITE_SIMPSON", 5, 1, "HEUN"), ("TRAPEZOIDAL", 9, 1, "HEUN"), ("SHOOTING", 3, 2, "HEUN"), ("SHOOTING", 3, 2, "RK4"))
NODE_SHAPES = (("HERMITE_SIMPSON", 6, 1, "HEUN"),) + tuple(("SHOOTING", 4, 3, m) for m in METHODS)
DENSE_N = 33              # up to this horizon a shape case holds the dense J, above it the rows of the first and the last interval
# section 2 of the GPU module: horizons at the lane-loop edges of hs_eval_kernel (K = 2 N + 1 or N + 1 on either side of 64, 256 and 512 threads)
FORM_CASES = ([("CARTPOLE", "HERMITE_SIMPSON", N) for N in (1, 31, 32, 127, 128, 255, 256)] +
              [("CARTPOLE", "TRAPEZOIDAL", N) for N in (63, 64, 255, 256, 511, 512)] +
              [("BEARPOPULATIONS", "HERMITE_SIMPSON", N) for N in (6, 7)] + [("HIVTREATMENT", "HERMITE_SIMPSON", N) for N in (6, 7)] +
              [("NODE_CARTPOLE", "HERMITE_SIMPSON", N) for N in (1, 7, 8, 24, 32)])
# section 3: one lane per instance (SHOOTING), one workgroup per instance (collocation)
SHOOT_BATCH_CASES = (("CARTPOLE", 4, 3, "RK4"), ("VANDERPOL", 1, 50, "HEUN"))
SHOOT_BATCHES = (1, 63, 65, 257)
COLLOC_BATCH_N = 13
COLLOC_BATCHES = (1, 37, 257)
CAPACITY_N = 347          # CARTPOLE Hermite-Simpson: the largest horizon whose records fit the 160 KiB of LDS (hs_eval_lds_bytes, test_eval_cases.py)
# (system, N, wavefronts it lands on): Hermite-Simpson horizons that do not fit with eight wavefronts' partial sums and do with fewer, so that the
# launcher's step-down 8 -> 4 -> 1 ends in a launch (CARTPOLE has no such horizon: a point more is 464 bytes, eight wavefronts are 56)
STEP_DOWN = (("VANDERPOL", 926, 4), ("CANCERTREATMENT", 2044, 1))
ROLLOUT_NODE_S = 5
ROLLOUT_TWIN_S = 7
ROWS_S = 7                # control-row cases: S steps; rows exactly consumed, 2 S + 5, S and 1
ROWS_SYSTEMS = ("CARTPOLE", "BACTERIA", "HARVEST")
ROLLOUT_BATCHES = (1, 63, 65, 257)
EVAL_QUANTITIES = ("f", "gradf", "c", "J")
ROLLOUT_QUANTITIES = ("xs", "cost")
# eval cases whose oracle answers one ulp with more than MAX_RESPONSE whatever the seed, by id, each with the reason (none: every case is
# well conditioned at seed 0)
ILL_CONDITIONED = {}
# ... and rollout cases (fit_cases.inputs has one draw per case: nothing to redraw from).  fit_cases.horizon keeps HIVTREATMENT at T = 10, steps of
# 0.25 against the decay rate m_3 = 4.4: h m_3 = 1.1, where the reference's "midpoint" (x + h f(x + h f(x))) multiplies that mode by
# 1 - 1.1 + 1.21 = 1.11 a step -- the virus count swings up to 330 from 1.5 (under the other three rules it decays) -- and the oracle answers one
# ulp with 2.5e-12 in the states (row 1: 1.4e-12 even of the largest state) and 2.3e-13 in the cost.  Its bound is then the ceiling, 1e-11.
ROLLOUT_ILL_CONDITIONED = {"HIVTREATMENT-MIDPOINT-S40": "h m_3 = 1.1 is outside the stable range of the reference's midpoint rule"}


def _freeze(obj):
  for a in (obj.values() if isinstance(obj, dict) else obj):
    if isinstance(a, np.ndarray):
      a.setflags(write=False)
  return obj


def _moved(a, rng):
  """every entry moved by -1, 0 or +1 ulp"""
  return a * (1.0 + 2.0 ** -52 * rng.integers(-1, 2, a.shape))


def _rows_of_xs(xs):
  """[.., S+1, ns] -> [.., ns, S+1]: one row per state component"""
  return np.swapaxes(xs, -1, -2)


# ---- eval ------------------------------------------------------------------------------------------------------------------------------------
def mc(c):
  return 2 if (c["tr"] == "SHOOTING" and c["method"] == "RK4") else 1


def transcription(c, b, prow=None):
  """the oracle's transcription of instance b at its own parameter row (or at `prow`)"""
  if c["kind"] == "node":
    import node_shoot_exgd_grad_cases as NSG
    return NH._transcription(c["tr"], c["N"], c["cpi"], c["method"], c["T"], NSG._leaves(False))
  prow = [float(v) for v in (c["params"][b] if prow is None else prow)]
  if c["kind"] == "twin":
    s = O.Elastic(F.make_system(c["base"], prow[:-1]), prow[-1])
    s.T = c["T"]
    with torch.no_grad():
      if c["tr"] == "SHOOTING":
        return O.make_transcription(s, "SHOOTING", c["N"], c["cpi"], integration_method=c["method"])
      return O.make_transcription(s, "COLLOCATION", c["N"], quadrature_rule=c["tr"])
  return H._transcription(c["name"], c["tr"], c["N"], c["cpi"], c["method"], c["T"], prow)[1]


def jrows(c):
  """the rows of J a case holds: None (all), or those of the first and the last interval"""
  if c["N"] <= DENSE_N or c["tr"] == "SHOOTING" or c["N"] == CAPACITY_N:      # (the capacity case is compared densely)
    return None
  ns, N = c["ns"], c["N"]
  one = np.r_[0:ns, (N - 1) * ns:N * ns]
  return one if c["tr"] == "TRAPEZOIDAL" else np.r_[one, N * ns + one]


def oracle_row(c, b, z=None, prow=None):
  """{f, gradf, c, J} of instance b from O.Callbacks"""
  tr = transcription(c, b, prow)
  cb = O.Callbacks(tr)
  z = c["z"][b] if z is None else z
  rows = jrows(c)
  if rows is None:
    J = cb.jac(z)
  else:
    idx = torch.as_tensor(rows)
    J = torch.func.jacrev(lambda x: tr.constraints(x)[idx])(O._t(z)).numpy()
  return dict(f=np.array([cb.fun(z)]), gradf=cb.grad(z), c=cb.cons(z), J=J.reshape(-1))


def _stack(rows):
  return _freeze({k: np.stack([r[k] for r in rows]) for k in rows[0]})


def _eval_reference(c, rows):
  """(reference of `rows`, response per quantity)"""
  with np.errstate(all="ignore"):
    ref = _stack([oracle_row(c, b) for b in rows])
    rng = np.random.default_rng(12345)
    resp = dict.fromkeys(EVAL_QUANTITIES, 0.0)
    for i, b in enumerate(rows):
      z = _moved(c["z"][b], rng)
      prow = None if c["kind"] == "node" else _moved(c["params"][b], rng)
      r = oracle_row(c, b, z, prow)
      for q in EVAL_QUANTITIES:
        e = rel_error(r[q][None], ref[q][i:i + 1])
        resp[q] = max(resp[q], e if np.isfinite(e) else np.inf)
  return ref, resp


def _well_conditioned(draw, rows_of, what):
  """(case, reference) of the first of the seeds 0 .. 19 whose reference is finite and answers one ulp within MAX_RESPONSE; failing that the
  seed-0 case with its figure, which test_eval_cases.py then wants listed in ILL_CONDITIONED"""
  first = None
  for seed in range(20):
    c = draw(seed)
    rows = tuple(rows_of(c))
    ref, resp = _eval_reference(c, rows)
    c.update(seed=seed, rows=rows, response=resp)
    if first is None:
      first = (c, ref)
    if all(np.isfinite(a).all() for a in ref.values()) and max(resp.values()) <= MAX_RESPONSE:
      return _freeze(c), ref
  assert all(np.isfinite(a).all() for a in first[1].values()), f"{what}: the oracle is not finite at any seed"
  return _freeze(first[0]), first[1]


def _closed_draw(name, tr, N, cpi, method, batch, discounted):
  def draw(seed):
    c = dict(H._draw(name, tr, N, cpi, method, batch, seed, False), kind="closed")
    if discounted:
      assert name == "TIMBERHARVEST"
      p = c["params"].copy()
      p[:, O.SYSTEMS[name].param_names.index("r")] = DISCOUNT_R
      c["params"] = p
    return c
  return draw


def _twin_draw(base, tr, N, cpi, method, batch):
  def draw(seed):
    s = O.Elastic(O.SYSTEMS[base](), TWIN_RHO)
    with torch.no_grad():
      t = (O.make_transcription(s, "SHOOTING", N, cpi, integration_method=method) if tr == "SHOOTING"
           else O.make_transcription(s, "COLLOCATION", N, quadrature_rule=tr))
    rng = np.random.default_rng(5 + 100000 * seed)
    n = t.guess.size
    z = t.guess[None] * (1.0 + 0.05 * rng.standard_normal((batch, n))) + 0.3 * rng.standard_normal((batch, n))
    p0 = s.params()
    params = p0 * (1.0 + 0.05 * (2.0 * rng.random((batch, p0.size)) - 1.0))
    return dict(kind="twin", name=base + "_ELASTIC", base=base, tr=tr, N=N, cpi=cpi, method=method, T=float(s.T), z=z, params=params, n=n,
                m=int(t.constraints(O._t(z[0])).numel()), ns=s.ns, nu=s.nu)
  return draw


def _node_draw(tr, N, cpi, method, batch):
  def draw(seed):
    c = NH._draw(tr, N, cpi, method, batch, seed)
    return dict(kind="node", name="NODE_CARTPOLE", tr=tr, N=N, cpi=cpi, method=method, T=c["T"], z=c["z"], params=c["params"], n=c["n"], m=c["m"],
                ns=NH.NS, nu=NH.NU)
  return draw


def edge_rows(batches):
  """rows 0 and B - 1 of every batch size"""
  return tuple(sorted({0} | {b - 1 for b in batches}))


@functools.lru_cache(maxsize=None)
def _eval_case(kind, name, tr, N, cpi, method, batch, discounted, rows):
  if kind == "closed":
    draw = _closed_draw(name, tr, N, cpi, method, batch, discounted)
  else:
    draw = _twin_draw(name, tr, N, cpi, method, batch) if kind == "twin" else _node_draw(tr, N, cpi, method, batch)
  return _well_conditioned(draw, (lambda c: range(batch)) if rows is None else (lambda c: rows), f"{name} {tr} {N}x{cpi} {method}")


def eval_case(kind, name, tr, N, cpi=1, method="HEUN", batch=B, discounted=False, rows=None):
  """a case of myr_eval; `rows`: the instances its reference holds (default: all)"""
  key = (kind, name, tr, N, cpi, method, batch, discounted, rows)
  c = _eval_case(*key)[0]
  c.setdefault("key", key)
  return c


def eval_reference(c):
  """{f [R][1], gradf [R][n], c [R][m], J [R][.]} of the case's `rows`, read-only"""
  return _eval_case(*c["key"])[1]


def row_index(c, b):
  return c["rows"].index(b)


def what(c):
  return "%s %s %dx%d %s" % (c["name"], c["tr"], c["N"], c["cpi"], c["method"]) + (" r=0.3" if c["key"][7] else "")


def parity_cases():
  """every case of section 1 of the GPU module, as (id, thunk)"""
  out = []
  P = functools.partial
  for name in SYSTEMS:
    out.append((f"{name}-HERMITE_SIMPSON", P(eval_case, "closed", name, "HERMITE_SIMPSON", HS_N)))
    out.append((f"{name}-TRAPEZOIDAL", P(eval_case, "closed", name, "TRAPEZOIDAL", TRAP_N)))
    for I, cpi, m in SHOOT_SHAPES:
      out.append((f"{name}-{I}x{cpi}-{m}", P(eval_case, "closed", name, "SHOOTING", I, cpi, m)))
  for name in SHOOT_EXTRA_SYSTEMS:
    for I, cpi, m in SHOOT_EXTRA_SHAPES:
      out.append((f"{name}-{I}x{cpi}-{m}", P(eval_case, "closed", name, "SHOOTING", I, cpi, m)))
  out.append(("TIMBERHARVEST-HERMITE_SIMPSON-r0.3", P(eval_case, "closed", "TIMBERHARVEST", "HERMITE_SIMPSON", HS_N, discounted=True)))
  out.append(("TIMBERHARVEST-TRAPEZOIDAL-r0.3", P(eval_case, "closed", "TIMBERHARVEST", "TRAPEZOIDAL", TRAP_N, discounted=True)))
  for I, cpi, m in SHOOT_SHAPES:
    out.append((f"TIMBERHARVEST-{I}x{cpi}-{m}-r0.3", P(eval_case, "closed", "TIMBERHARVEST", "SHOOTING", I, cpi, m, discounted=True)))
  for base in TWINS:
    for tr, N, cpi, m in TWIN_SHAPES:
      out.append((f"{base}_ELASTIC-{tr}-{N}x{cpi}-{m}", P(eval_case, "twin", base, tr, N, cpi, m)))
  for tr, N, cpi, m in NODE_SHAPES:
    out.append((f"NODE_CARTPOLE-{tr}-{N}x{cpi}-{m}", P(eval_case, "node", "NODE_CARTPOLE", tr, N, cpi, m)))
  return out


def form_case(name, tr, N):
  """section 2: B = 3, the oracle on rows 0 and B - 1"""
  return eval_case("node" if name == "NODE_CARTPOLE" else "closed", name, tr, N, rows=(0, B - 1))


def shoot_batch_case(name, I, cpi, method):
  return eval_case("closed", name, "SHOOTING", I, cpi, method, batch=max(SHOOT_BATCHES), rows=edge_rows(SHOOT_BATCHES))


def colloc_batch_case(tr):
  return eval_case("closed", "CARTPOLE", tr, COLLOC_BATCH_N, batch=max(COLLOC_BATCHES), rows=edge_rows(COLLOC_BATCHES))


def capacity_case():
  """B = 2, the oracle on the last instance (its dense J is 2 776 x 3 475)"""
  return eval_case("closed", "CARTPOLE", "HERMITE_SIMPSON", CAPACITY_N, batch=2, rows=(1,))


def head(c, batch):
  """the leading instances of a case (eval or rollout)"""
  out = dict(c)
  for k in ("z", "x0", "us"):
    if k in c:
      out[k] = c[k][:batch]
  if c["params"].ndim == 2:
    out["params"] = c["params"][:batch]
  return out


def one(c, b):
  """instance b alone"""
  out = dict(c)
  for k in ("z", "x0", "us"):
    if k in c:
      out[k] = c[k][b:b + 1]
  if c["params"].ndim == 2:
    out["params"] = c["params"][b:b + 1]
  return out


# ---- rollout ---------------------------------------------------------------------------------------------------------------------------------
def rollout_system(c, b, prow=None):
  """the oracle's system of instance b, with the case's horizon"""
  if c["kind"] == "node":
    import node_shoot_exgd_grad_cases as NSG
    s = O.NodeCartPole(NSG._leaves(False))
  else:
    prow = [float(v) for v in (c["params"][b] if prow is None else prow)]
    s = O.Elastic(F.make_system(c["base"], prow[:-1]), prow[-1]) if c["kind"] == "twin" else F.make_system(c["name"], prow)
  s.T = c["T"]
  return s


def oracle_rollout(c, b, x0=None, us=None, prow=None):
  with torch.no_grad():
    xs, cost = O.get_state_trajectory_and_cost(rollout_system(c, b, prow), c["S"], c["method"], c["x0"][b] if x0 is None else x0,
                                               c["us"][b] if us is None else us)
  return dict(xs=xs, cost=np.array([cost]))


def _rollout_reference(c, rows):
  with np.errstate(all="ignore"):
    ref = _stack([oracle_rollout(c, b) for b in rows])
    rng = np.random.default_rng(12345)
    resp = dict.fromkeys(ROLLOUT_QUANTITIES, 0.0)
    for i, b in enumerate(rows):
      prow = None if c["kind"] == "node" else _moved(c["params"][b], rng)
      r = oracle_rollout(c, b, _moved(c["x0"][b], rng), _moved(c["us"][b], rng), prow)
      e = (rel_error(_rows_of_xs(r["xs"][None]), _rows_of_xs(ref["xs"][i:i + 1])), rel_error(r["cost"][None], ref["cost"][i:i + 1]))
      for q, v in zip(ROLLOUT_QUANTITIES, e):
        resp[q] = max(resp[q], v if np.isfinite(v) else np.inf)
  c.update(rows=tuple(rows), response=resp)
  return _freeze(c), ref


def _closed_rollout(name, method, S, u_rows, batch, discounted):
  """fit_cases.inputs at S steps and the most control rows it draws for them, cut to u_rows; u_rows = 2 S + 5 takes the controls of the draw
  at S + 2 steps (2 (S + 2) + 1 rows)"""
  S_draw = S + 2 if u_rows > 2 * S + 1 else S
  xs_obs, us, params = F.inputs(name, method, True, batch, S_draw, True)
  assert us.shape[1] >= u_rows
  if discounted:
    params = params.copy()
    params[:, O.SYSTEMS[name].param_names.index("r")] = DISCOUNT_R
  s = O.SYSTEMS[name]()
  return dict(kind="closed", name=name, method=method, S=S, T=F.horizon(name, S), x0=xs_obs[:, 0].copy(), us=us[:, :u_rows].copy(), params=params,
              ns=s.ns, nu=s.nu)


def _twin_rollout(base, method, S, u_rows, batch):
  s = O.Elastic(O.SYSTEMS[base](), TWIN_RHO)
  rng = np.random.default_rng(77000 + 100 * TWINS.index(base) + 10 * METHODS.index(method) + S)
  us = F._controls(s, rng, batch, u_rows)
  x0 = np.tile(s.x_0, (batch, 1)).astype(np.float64)
  x0 = x0 + 0.05 * rng.standard_normal(x0.shape) * np.maximum(1.0, np.abs(x0))
  p0 = s.params()
  params = p0 * (1.0 + 0.05 * (2.0 * rng.random((batch, p0.size)) - 1.0))
  return dict(kind="twin", name=base + "_ELASTIC", base=base, method=method, S=S, T=min(float(s.T), 0.05 * S), x0=x0, us=us, params=params,
              ns=s.ns, nu=s.nu)


def _node_rollout(method, S, u_rows, batch):
  rng = np.random.default_rng(78000 + 10 * METHODS.index(method) + S)
  return dict(kind="node", name="NODE_CARTPOLE", method=method, S=S, T=0.05 * S, x0=0.5 * rng.standard_normal((batch, NH.NS)),
              us=rng.uniform(-5.0, 5.0, (batch, u_rows, NH.NU)), params=NH.weights()[1], ns=NH.NS, nu=NH.NU)


def consumed_rows(method, S):
  """the control rows S steps read: S + 1, RK4 2 S + 1"""
  return 2 * S + 1 if method == "RK4" else S + 1


@functools.lru_cache(maxsize=None)
def _rollout_case(kind, name, method, S, u_rows, batch, discounted, rows):
  if kind == "closed":
    c = _closed_rollout(name, method, S, u_rows, batch, discounted)
  elif kind == "twin":
    c = _twin_rollout(name, method, S, u_rows, batch)
  else:
    c = _node_rollout(method, S, u_rows, batch)
  return _rollout_reference(c, range(batch) if rows is None else rows)


def rollout_case(kind, name, method, S, u_rows=None, batch=B, discounted=False, rows=None):
  key = (kind, name, method, S, consumed_rows(method, S) if u_rows is None else u_rows, batch, discounted, rows)
  c = _rollout_case(*key)[0]
  c.setdefault("key", key)
  return c


def rollout_reference(c):
  """{xs [R][S+1][ns], cost [R][1]} of the case's `rows`, read-only"""
  return _rollout_case(*c["key"])[1]


def rollout_what(c):
  return "%s %s S=%d u_rows=%d" % (c["name"], c["method"], c["S"], c["us"].shape[1]) + (" r=0.3" if c["key"][6] else "")


def rollout_parity_cases():
  """section 6, parity: (id, thunk)"""
  out = []
  P = functools.partial
  for name in SYSTEMS:
    for m in METHODS:
      out.append((f"{name}-{m}-S{F.steps_for(name)}", P(rollout_case, "closed", name, m, F.steps_for(name))))
      out.append((f"{name}-{m}-S1", P(rollout_case, "closed", name, m, 1)))
  for m in METHODS:
    out.append((f"TIMBERHARVEST-{m}-S40-r0.3", P(rollout_case, "closed", "TIMBERHARVEST", m, 40, discounted=True)))
  for base in TWINS:
    for m in METHODS:
      out.append((f"{base}_ELASTIC-{m}-S{ROLLOUT_TWIN_S}", P(rollout_case, "twin", base, m, ROLLOUT_TWIN_S)))
  for m in METHODS:
    out.append((f"NODE_CARTPOLE-{m}-S{ROLLOUT_NODE_S}", P(rollout_case, "node", "NODE_CARTPOLE", m, ROLLOUT_NODE_S)))
  return out


def rows_variants(method, S=ROWS_S):
  """u_rows of the control-row cases: exactly consumed | longer | the last step clamps | a constant control"""
  return (consumed_rows(method, S), 2 * S + 5, S, 1)


def rows_cases():
  out = []
  for name in ROWS_SYSTEMS:
    for m in METHODS:
      for R in rows_variants(m):
        out.append((f"{name}-{m}-rows{R}", functools.partial(rollout_case, "closed", name, m, ROWS_S, R)))
  return out


def rollout_batch_case(name, method, S):
  return rollout_case("closed", name, method, S, batch=max(ROLLOUT_BATCHES), rows=edge_rows(ROLLOUT_BATCHES))


# ---- the bound a device result is held to -------------------------------------------------------------------------------------------------------
CEIL = {"f": 1e-12, "c": 1e-12, "gradf": 1e-11, "J": 1e-11, "xs": 1e-11, "cost": 1e-11}
FLOOR = 1e-13
ZERO_ROW = 1e-13          # a reference row that is exactly zero: |out| <= ZERO_ROW max(1, max|input|), absolutely


def bound(c, quantity):
  """min(CEIL, max(1e-13, 10 x response)): the ceiling the project already holds the quantity to, the floor 30 x the worst figure of the sibling
  kernels on the same draws, 10 x the reference's own answer to one ulp in between"""
  return min(CEIL[quantity], max(FLOOR, 10.0 * c["response"][quantity]))
