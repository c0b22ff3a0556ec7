"""CPU tests of the solver core (myriad_amd/csrc/hs_solver.h) through its TEST-ONLY host build (tests/hostsim):
one Newton/SQP step against a dense KKT solve built from the oracle, full solves against the golden trajectories.
The same templates are what the HIP kernel instantiates per lane; the GPU-side parity tests are in test_gpu_solve.py."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import myriad_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def sim():
  subprocess.run(["bash", os.path.join(HERE, "hostsim", "build.sh")], check=True)
  lib = C.CDLL(os.path.join(HERE, "hostsim", "libhostsim.so"))
  dp = C.c_void_p
  lib.hostsim_step.argtypes = [C.c_int, C.c_int, C.c_double] + [dp] * 6 + [C.c_double] + [dp] * 4
  lib.hostsim_solve.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, dp, dp, C.c_int, C.c_int, C.c_double,
                                C.c_double, C.c_double, C.c_double, dp, dp, dp, dp, dp]
  lib.hostsim_rollout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, dp, dp]
  lib.hostsim_rollout.restype = C.c_double
  return lib


A = lambda a: a.ctypes.data
SID = {"CARTPOLE": 0, "VANDERPOL": 1, "CANCERTREATMENT": 2, "SIMPLECASE": 3}


@pytest.mark.parametrize("name,N,seed", [("CARTPOLE", 6, 1), ("CARTPOLE", 12, 2), ("SIMPLECASE", 4, 5)])
def test_riccati_step_equals_dense_kkt_solve(sim, name, N, seed):
  """dz from the stage-wise recursion (terminal multipliers, mu-linear right-hand side, adjoint lambda) equals the
  solution of the full dense primal-dual KKT system assembled from the oracle's f, c, J and torch's exact Hessian."""
  s = O.SYSTEMS[name](); tr = O.hermite_simpson(s, N); cb = O.Callbacks(tr)
  rng = np.random.default_rng(seed)
  n, ns, K = tr.guess.size, s.ns, 2 * N + 1
  m = 2 * N * ns
  lb, ub = tr.bounds[:, 0].copy(), tr.bounds[:, 1].copy()
  free = lb < ub
  z = tr.guess + 0.05 * rng.standard_normal(n); z[~free] = lb[~free]
  hasL, hasU = free & np.isfinite(lb), free & np.isfinite(ub)
  zL = np.where(hasL, rng.uniform(0.5, 1.5, n), 0.0); zU = np.where(hasU, rng.uniform(0.5, 1.5, n), 0.0)
  nuT = 0.3 * rng.standard_normal(ns); mu = 0.1
  lam, dz, nu, info = np.zeros(m), np.zeros(n), np.zeros(ns), np.zeros(16)
  zz = z.copy()
  assert sim.hostsim_step(SID[name], N, s.T, A(zz), A(lb), A(ub), A(zL), A(zU), A(nuT), mu, A(lam), A(dz), A(nu), A(info)) == 0
  f, g, c, J = cb.fun(z), cb.grad(z), cb.cons(z), cb.jac(z)
  assert info[0] == pytest.approx(f, rel=1e-13, abs=1e-15) and info[1] == pytest.approx(np.abs(c).sum(), rel=1e-13)
  # adjoint multipliers: x-row stationarity holds by construction
  r = g - zL + zU + J.T @ lam
  tp = ~free[(K - 1) * ns:K * ns]
  r[(K - 1) * ns:K * ns] += np.where(tp, nuT, 0)
  assert np.abs(r[ns:K * ns]).max() < 1e-11
  assert info[3] == pytest.approx(np.abs(r[K * ns:]).max(), rel=1e-9)
  if info[8] != 0:
    pytest.skip("inertia correction active at this point")
  W = torch.func.hessian(lambda zt, lt: tr.objective(zt) + (lt * tr.constraints(zt)).sum())(torch.as_tensor(z), torch.as_tensor(lam)).numpy()
  sl, su = np.where(hasL, z - lb, 1.0), np.where(hasU, ub - z, 1.0)
  Sig = np.where(hasL, zL / sl, 0) + np.where(hasU, zU / su, 0)
  gb = g - np.where(hasL, mu / sl, 0) + np.where(hasU, mu / su, 0)
  fi = np.where(free)[0]
  H = W[np.ix_(fi, fi)] + np.diag(Sig[fi])
  KKT = np.block([[H, J[:, fi].T], [J[:, fi], np.zeros((m, m))]])
  sol = np.linalg.solve(KKT, -np.concatenate([gb[fi], c]))
  dzd = np.zeros(n); dzd[fi] = sol[:fi.size]
  assert np.abs(dz - dzd).max() <= 1e-8 * max(1.0, np.abs(dzd).max())
  assert info[7] == pytest.approx(gb @ dzd, rel=1e-7)


def _solve(sim, name, N, T, z0, lb, ub, max_iter=1000):
  B, n = z0.shape
  m = 2 * N * O.SYSTEMS[name]().ns
  z = z0.copy(); lam = np.zeros((B, m)); cost = np.zeros(B)
  st = np.zeros(B, np.int32); it = np.zeros(B, np.int32); kkt = np.zeros((B, 3))
  lb = np.ascontiguousarray(lb); ub = np.ascontiguousarray(ub)
  sim.hostsim_solve(SID[name], N, T, B, A(z), A(lb), A(ub), None, 0, max_iter, 1e-8, 1e-6, 1e-7, 0.1, A(lam), A(cost), A(st), A(it), A(kkt))
  return z, lam, cost, st, it, kkt


def test_solver_core_matches_golden_trajectories(sim, golden_dir):
  files = sorted(glob.glob(os.path.join(golden_dir, "solve_hs_cartpole_N*.npz")))
  assert files
  same_total = n_total = 0
  for path in files:
    d = np.load(path)
    N = int(d["N"])
    if N > 25:
      continue
    z, lam, cost, st, it, kkt = _solve(sim, "CARTPOLE", N, 2.0, d["z0"], d["lb"], d["ub"])
    assert (st == 0).all()
    same = np.isclose(cost, d["cost"], rtol=1e-9)
    assert (cost[~same] < d["cost"][~same]).all()           # other basin only if better (non-convex swing-up)
    assert np.abs(z[same] - d["z"][same]).max() < 1e-6
    same_total += int(same.sum()); n_total += same.size
  assert same_total >= n_total - 1


def test_solver_core_other_systems_converge_and_agree_with_slsqp(sim):
  """HS transcription of the other three hot-path systems (free terminal state / infinite bounds / log dynamics)."""
  for name, N in [("VANDERPOL", 20), ("CANCERTREATMENT", 20), ("SIMPLECASE", 10)]:
    s = O.SYSTEMS[name](); tr = O.hermite_simpson(s, N)
    z, lam, cost, st, it, kkt = _solve(sim, name, N, s.T, tr.guess[None], tr.bounds[None, :, 0], tr.bounds[None, :, 1])
    assert st[0] == 0, (name, st, kkt)
    cb = O.Callbacks(tr)
    assert np.abs(cb.cons(z[0])).max() <= 1e-8
    r = O.solve(tr, "SLSQP", extra_options={"ftol": 1e-13}, cb=cb)
    assert cost[0] <= r["cost"] + 1e-7 * max(1.0, abs(r["cost"])), (name, cost[0], r["cost"])
    assert cost[0] == pytest.approx(r["cost"], rel=1e-5)


@pytest.mark.parametrize("method,mid", [("EULER", 0), ("HEUN", 1), ("MIDPOINT", 2), ("RK4", 3)])
def test_rollout_core_matches_oracle(sim, method, mid):
  """csrc/rollout.h (what myr_rollout runs per lane) vs the oracle's get_state_trajectory_and_cost (utils.py:258-298)."""
  rng = np.random.default_rng(3)
  for name in ("CARTPOLE", "VANDERPOL", "CANCERTREATMENT", "SIMPLECASE"):
    s = O.SYSTEMS[name]()
    S = 17
    rows = (2 if method == "RK4" else 1) * S + 1
    us = 0.3 * rng.standard_normal((rows, 1))
    if name == "CANCERTREATMENT":
      us = np.abs(us)
    xs = np.zeros((S + 1, s.ns))
    c = sim.hostsim_rollout(SID[name], mid, S, s.T / S / 4, rows, A(np.ascontiguousarray(s.x_0)), A(us), None, A(xs))
    class Sh(type(s)):
      pass
    s2 = O.SYSTEMS[name](); s2.T = s.T / 4
    oxs, oc = O.get_state_trajectory_and_cost(s2, S, method, s.x_0, us)
    np.testing.assert_allclose(xs, oxs, rtol=1e-12, atol=1e-13)
    assert c == pytest.approx(oc, rel=1e-12, abs=1e-14)


def _os_lib(sim):
  dp = C.c_void_p
  sim.hostsim_solve_trap.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, dp, dp, C.c_int, C.c_int, dp, dp, dp, dp, dp]
  sim.hostsim_solve_shoot.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, dp, dp, C.c_int, C.c_int, dp, dp, dp, dp, dp]
  return sim


@pytest.mark.parametrize("name,N", [("CARTPOLE", 25), ("VANDERPOL", 30), ("CANCERTREATMENT", 30), ("SIMPLECASE", 20)])
def test_trapezoid_core_matches_oracle_slsqp(sim, name, N):
  """csrc/os_solver.h TrapCore (README.md:83's transcription) vs the oracle's SLSQP path."""
  sim = _os_lib(sim)
  s = O.SYSTEMS[name](); tr = O.trapezoidal(s, N); cb = O.Callbacks(tr)
  z = tr.guess[None].copy(); lb = np.ascontiguousarray(tr.bounds[None, :, 0]); ub = np.ascontiguousarray(tr.bounds[None, :, 1])
  lam = np.zeros((1, N * s.ns)); cost = np.zeros(1); st = np.zeros(1, np.int32); it = np.zeros(1, np.int32); kkt = np.zeros((1, 3))
  sim.hostsim_solve_trap(SID[name], N, s.T, 1, A(z), A(lb), A(ub), None, 0, 500, A(lam), A(cost), A(st), A(it), A(kkt))
  assert st[0] == 0
  assert np.abs(cb.cons(z[0])).max() <= 1e-8 and cb.fun(z[0]) == pytest.approx(cost[0], rel=1e-12)
  r = O.solve(tr, "SLSQP", extra_options={"ftol": 1e-13}, cb=cb)
  assert cost[0] == pytest.approx(r["cost"], rel=1e-7) and np.abs(z[0] - r["xs_and_us"]).max() < 1e-4
  rr = cb.grad(z[0]) + cb.jac(z[0]).T @ lam[0]
  inact = (lb[0] < ub[0]) & (z[0] - lb[0] > 1e-3) & (ub[0] - z[0] > 1e-3)
  assert np.abs(rr[inact]).max() < 1e-5


@pytest.mark.parametrize("name,I,cpi,method", [("SIMPLECASE", 10, 100, "HEUN"), ("VANDERPOL", 1, 50, "HEUN"),
                                               ("CANCERTREATMENT", 1, 100, "HEUN"), ("CARTPOLE", 10, 5, "HEUN"),
                                               ("SIMPLECASE", 4, 10, "EULER")])
def test_shooting_core_matches_oracle_slsqp(sim, name, I, cpi, method):
  """csrc/os_solver.h ShootCore (lifted step-level Riccati) on the BASELINE shooting shapes (configs 1, 3, 4) vs the
  oracle's SLSQP path; the survey's App. C costs are reproduced."""
  sim = _os_lib(sim)
  s = O.SYSTEMS[name](); tr = O.shooting(s, I, cpi, method); cb = O.Callbacks(tr)
  z = tr.guess[None].copy(); lb = np.ascontiguousarray(tr.bounds[None, :, 0]); ub = np.ascontiguousarray(tr.bounds[None, :, 1])
  lam = np.zeros((1, I * s.ns)); cost = np.zeros(1); st = np.zeros(1, np.int32); it = np.zeros(1, np.int32); kkt = np.zeros((1, 3))
  sim.hostsim_solve_shoot(SID[name], I, cpi, {"EULER": 0, "HEUN": 1}[method], s.T, 1, A(z), A(lb), A(ub), None, 0, 500,
                          A(lam), A(cost), A(st), A(it), A(kkt))
  assert st[0] == 0
  assert np.abs(cb.cons(z[0])).max() <= 1e-8 and cb.fun(z[0]) == pytest.approx(cost[0], rel=1e-11)
  r = O.solve(tr, "SLSQP", max_iter=500, extra_options={"ftol": 1e-13}, cb=cb)
  assert cost[0] == pytest.approx(r["cost"], rel=1e-6)
  survey = {("SIMPLECASE", 10): -1.3543305221, ("VANDERPOL", 1): 2.8731963348, ("CANCERTREATMENT", 1): 20.5735535185}
  if (name, I) in survey and method == "HEUN":
    assert cost[0] == pytest.approx(survey[(name, I)], rel=1e-4) and cost[0] <= survey[(name, I)] + 1e-9   # SLSQP at default ftol=1e-6 stops slightly short


# ---- the interior-point policy (myriad_amd/csrc/ip_policy.h): the rules the lane, wave and fused loops share, restated here ----
DELTA_WARM_DIV, PEN_RELAX, PEN_RELAX_MAX, PEN_RELAX_RATIO = 6.0, 5, 8, 10.0


def _ladder(sim, lm, delta_last, warm, warm_min=3e-3, rungs=8):
  sim.hostsim_policy_ladder.argtypes = [C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, C.c_void_p]
  out = np.zeros(rungs + 1)
  sim.hostsim_policy_ladder(lm, delta_last, warm, warm_min, rungs, A(out))
  return out[:rungs], out[rungs]


def _ladder_rule(lm, delta_last, warm, warm_min, rungs):
  d = lm
  if warm and delta_last > warm_min:
    d = max(d, delta_last / DELTA_WARM_DIV)
  seq = [d]
  for _ in range(rungs - 1):
    d = seq[-1]
    if d == 0.0:
      seq.append(max(1e-8, delta_last / 3.0) if delta_last > 0.0 else 1e-4)
    else:
      seq.append(d * (8.0 if delta_last > 0.0 else 100.0))
  return np.array(seq), (seq[-1] if seq[-1] > lm else 0.0)


def test_policy_ladder_from_a_cold_start(sim):
  """delta_last = 0: 0, 1e-4, then x 100 per rung (1e10 at rung 7 of this count); the closed ladder remembers its last rung"""
  seq, last = _ladder(sim, 0.0, 0.0, 1, rungs=9)
  want = np.array([0.0] + [1e-4 * 100.0 ** i for i in range(8)])
  np.testing.assert_allclose(seq, want, rtol=4e-16 * 8)      # (eight roundings at most)
  np.testing.assert_array_equal(seq[:4], [0.0, 1e-4, 1e-4 * 100.0, 1e-4 * 100.0 * 100.0])
  assert seq[8] > 1e8 and last == seq[8]
  np.testing.assert_array_equal(seq, _ladder_rule(0.0, 0.0, 1, 3e-3, 9)[0])
  # a ladder that ends at its first rung (delta = lm) leaves no memory
  assert _ladder(sim, 0.0, 0.0, 0, rungs=1)[1] == 0.0
  assert _ladder(sim, 3e-5, 0.0, 0, rungs=1) == (np.array([3e-5]), 0.0)


@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("lm", [0.0, 3e-5, 0.2])
def test_policy_ladder_after_a_correction(sim, warm, lm):
  """delta_last = 0.3: without delta_warm the first rung is the Levenberg-Marquardt floor and a zero rung is followed by
  delta_last / 3; with it the first rung is max(lm, delta_last / 6); every further rung x 8"""
  seq, last = _ladder(sim, lm, 0.3, warm, rungs=6)
  want, want_last = _ladder_rule(lm, 0.3, warm, 3e-3, 6)
  np.testing.assert_array_equal(seq, want)
  assert last == want_last
  assert seq[0] == (max(lm, 0.3 / 6.0) if warm else lm)
  assert seq[1] == (0.3 / 3.0 if seq[0] == 0.0 else seq[0] * 8.0)
  # below delta_warm_min the warm start does not apply
  assert _ladder(sim, lm, 1e-3, 1, rungs=1)[0][0] == lm


def _barrier(sim, mu, tol_stat=1e-6, tol_compl=1e-7, kmu=0.2, tmu=1.5, keps=10.0, sd=1.0, stat=0.0, cinf=0.0, cmin=1.0, cmax=0.0):
  sim.hostsim_policy_barrier.argtypes = [C.c_double] * 11 + [C.c_void_p]
  sim.hostsim_policy_barrier.restype = C.c_double
  mm = np.zeros(1)
  return sim.hostsim_policy_barrier(mu, tol_stat, tol_compl, kmu, tmu, keps, sd, stat, cinf, cmin, cmax, A(mm)), mm[0]


def _barrier_rule(mu, mu_min, kmu, tmu, keps, sd, stat, cinf, cmin, cmax):
  import math
  for _ in range(8):
    cerr = max(abs(cmax - mu), abs(cmin - mu)) if cmin <= cmax else 0.0
    emu = max(max(stat, cinf), cerr / sd)
    if emu <= keps * mu and mu > mu_min:
      mu = max(mu_min, min(kmu * mu, math.pow(mu, tmu)))
    else:
      break
  return mu


def test_policy_barrier_update(sim):
  """the chain of reductions mu <- max(mu_min, min(kappa_mu mu, mu^theta_mu)) while the barrier problem's error is within
  kappa_eps mu: down to mu_min = min(tol_compl, tol_stat) / 10, at most 8 per update"""
  tol = 2e-15      # pow() and a handful of roundings
  # no error at all (no bounded variable: compl_min > compl_max): the chain from 0.1 reaches the floor in 6 reductions
  mu, mu_min = _barrier(sim, 0.1)
  assert mu_min == min(1e-7, 1e-6) * 0.1 and mu == mu_min
  assert _barrier_rule(0.1, mu_min, 0.2, 1.5, 10.0, 1.0, 0.0, 0.0, 1.0, 0.0) == mu_min
  # the guard: kappa_mu = 0.9, theta_mu = 1 -> every reduction is x 0.9, and there are exactly 8 of them
  mu, mu_min = _barrier(sim, 0.1, kmu=0.9, tmu=1.0)
  np.testing.assert_allclose(mu, 0.1 * 0.9 ** 8, rtol=tol)
  np.testing.assert_allclose(mu, _barrier_rule(0.1, mu_min, 0.9, 1.0, 10.0, 1.0, 0.0, 0.0, 1.0, 0.0), rtol=tol)
  # the chain stops where the error exceeds kappa_eps mu: stationarity 3e-3 allows 0.1 -> 0.02 -> 0.0028.. -> 1.5e-4 and no further
  for kw in (dict(stat=3e-3), dict(cinf=3e-3), dict(stat=1e-9, cmin=0.0995, cmax=0.1008, sd=2.0), dict(stat=20.0)):
    mu, mu_min = _barrier(sim, 0.1, **kw)
    a = dict(sd=1.0, stat=0.0, cinf=0.0, cmin=1.0, cmax=0.0); a.update(kw)
    np.testing.assert_allclose(mu, _barrier_rule(0.1, mu_min, 0.2, 1.5, 10.0, a["sd"], a["stat"], a["cinf"], a["cmin"], a["cmax"]), rtol=tol)
  np.testing.assert_allclose(_barrier(sim, 0.1, stat=3e-3)[0], ((0.1 * 0.2) ** 1.5) ** 1.5, rtol=tol)
  assert _barrier(sim, 0.1, stat=20.0)[0] == 0.1
  # at the floor nothing moves
  assert _barrier(sim, 1e-8)[0] == 1e-8


def _penalty(sim, gphi, c1, floor_=None):
  sim.hostsim_policy_penalty.argtypes = [C.c_int] + [C.c_void_p] * 5
  n = len(gphi)
  g = np.asarray(gphi, float); c = np.asarray(c1, float); out = np.zeros(3 * n); slope = np.zeros(n)
  fl = None if floor_ is None else np.asarray(floor_, float)
  sim.hostsim_policy_penalty(n, A(g), A(c), None if fl is None else A(fl), A(out), A(slope))
  return out.reshape(n, 3), slope


def _penalty_rule(gphi, c1, floor_=None):
  pen, over, cuts, rows, slope = 1.0, 0, 0, [], []
  for i in range(len(gphi)):
    if c1[i] > 0.0:
      need = gphi[i] / (0.9 * c1[i])
      if pen < need:
        pen = need + 1.0
      want = max(2.0 * max(need, 0.0) + 1.0, 0.0 if floor_ is None else floor_[i])
      over = over + 1 if pen > PEN_RELAX_RATIO * want else 0
      if over >= PEN_RELAX and cuts < PEN_RELAX_MAX:
        pen, over, cuts = want, 0, cuts + 1
    rows.append((pen, over, cuts)); slope.append(gphi[i] - pen * c1[i])
  return np.array(rows), np.array(slope)


@pytest.mark.parametrize("floor_", [None, 0.0, 7.0, 400.0])
def test_policy_penalty_rule(sim, floor_):
  """the l1 penalty rises to need + 1, is reset to max(2 max(need, 0) + 1, floor) after PEN_RELAX consecutive iterations above
  PEN_RELAX_RATIO times that, at most PEN_RELAX_MAX times per solve; c1 = 0 leaves everything alone"""
  n = 80
  # need = 0.5 everywhere but for a spike every 6 iterations up to iteration 54 (need = 1000, 2000, ...); iteration 5 has c1 = 0
  gphi = np.full(n, 0.9 * 0.5); c1 = np.ones(n)
  gphi[0:60:6] = 0.9 * 1000.0 * (1.0 + np.arange(10))
  c1[5] = 0.0
  fl = None if floor_ is None else np.full(n, floor_)
  got, gslope = _penalty(sim, gphi, c1, fl)
  want, wslope = _penalty_rule(gphi, c1, fl)
  np.testing.assert_array_equal(got, want)
  np.testing.assert_array_equal(gslope, wslope)
  cut = np.flatnonzero(np.diff(got[:, 2]) > 0) + 1
  assert got[0, 0] == 1001.0 and got[6, 0] == 2001.0
  assert tuple(got[5]) == tuple(got[4])             # c1 = 0: penalty and counters untouched
  if floor_ == 400.0:
    # 10 x 400 is first exceeded by the spike of iteration 18 (penalty 4001): cuts at 23, 29, ..., 59, to the floor
    assert got[:19, 1].max() == 0
    np.testing.assert_array_equal(cut, np.arange(23, 60, 6))
    np.testing.assert_array_equal(got[cut, 0], 400.0)
  else:
    # iterations 1-4 count to 4, iteration 5 does not count, the spike of iteration 6 resets: no cut yet.  From then on five
    # iterations over -> a cut at 11, 17, ..., 53: eight of them, and no ninth after the spike of iteration 54
    assert tuple(got[4]) == (1001.0, 4, 0)
    np.testing.assert_array_equal(cut, np.arange(11, 54, 6))
    assert len(cut) == PEN_RELAX_MAX
    np.testing.assert_array_equal(got[cut, 0], max(2.0 * 0.5 + 1.0, floor_ or 0.0))
    assert tuple(got[-1]) == (10001.0, 25, PEN_RELAX_MAX)


def test_policy_park_record_round_trip(sim):
  """save / load of the state, its history and the pending step: every field comes back, at the documented offsets
  (0-11 mu, pen, pen_over, pen_cuts, stall, small_steps, delta_last, lm, nhist, hpos, hist_mu, hist_pen; 12-16 the step:
  on, ap, ad, mu, ksig; 17 nuT[NS]; 17 + NS hist[8]; NS = 4 here)"""
  sim.hostsim_policy_record.argtypes = [C.c_void_p] * 3
  NS = 4
  fields = np.array([3.25e-3, 41.5, 3, 2, 4, 1, 0.375, 1.2e-4, 3, 7, 3.25e-3, 41.5,       # the twelve scalars
                     1.0, 0.625, 0.5, 6.5e-3, 1e10,                                       # the pending step
                     -1.5, 2.5, 0.0, 1e-300,                                              # nuT
                     10.0, -11.0, 12.5, 0.0, 1e300, -0.0, 17.0, 18.0])                    # hist
  assert len(np.unique(fields[[0, 1, 6, 7, 13, 14, 15, 16]])) == 8
  sv = np.full(48, np.nan); back = np.full(fields.size, np.nan)
  n = sim.hostsim_policy_record(A(fields), A(sv), A(back))
  assert n == 17 + NS + 8 == fields.size
  np.testing.assert_array_equal(sv[:n], fields)
  assert np.isnan(sv[n:]).all()                     # nothing written behind the record
  np.testing.assert_array_equal(back, fields)
  # a step that is off
  fields[12] = 0.0
  sim.hostsim_policy_record(A(fields), A(sv), A(back))
  assert sv[12] == 0.0 and back[12] == 0.0
