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


# ---- the bound rules (myriad_amd/csrc/bound_rules.h): the treatment of one bounded variable that every solver form shares, restated here in
# the same operation order on IEEE doubles (numpy scalars: a division by zero gives inf as in C).  The twin is built without -march, so
# nothing is contracted into an fma, and on the host rcp_(x) is 1.0 / x: the exact rules must agree bit for bit (NaN where the twin has NaN).
F = np.float64
INF, NAN = F(np.inf), F(np.nan)
dmax = lambda a, b: a if a > b else b
dmin = lambda a, b: a if a < b else b


def _kind(l, u):
  fr = bool(l < u)
  return fr, fr and bool(l > -INF), fr and bool(u < INF)


def _bound_cases():
  """(l, u, zv) of every bound class -- pinned, lower only, upper only, two-sided, free, a NaN bound -- with slacks from 1e-300 to 1e300"""
  rng = np.random.default_rng(14)
  slacks = [1e-300, 1e-200, 3e-17, 1e-8, 0.25, 1.0, 7.0, 1e8, 1e150, 1e300]
  c = [(1.5, 1.5, 1.5), (0.0, 0.0, 0.3), (2.0, 1.0, 1.5), (-INF, INF, 0.7), (-INF, INF, -1e300), (-INF, -INF, 0.0), (INF, INF, 0.0),
       (NAN, 1.0, 0.5), (0.0, NAN, 0.5), (NAN, NAN, 0.5)]
  for s in slacks:
    c += [(0.0, INF, s), (-INF, 0.0, -s), (0.0, 1e300, s), (-1e300, 0.0, -s), (0.0, 2.0 * s, s)]
    c += [(1.0, INF, 1.0 + s), (-INF, -1.0, -1.0 - s)]      # (the slack is rounded at the small sizes: still the twin's operands)
  c += [(0.0, INF, -1e-3), (-INF, 0.0, 1e-3), (0.0, 1.0, 1.0), (0.0, 1.0, 0.0), (0.0, 1.0, 2.0)]      # on and beyond a bound
  for _ in range(60):
    l, w = rng.normal() * 10.0 ** rng.integers(-3, 4), 10.0 ** rng.uniform(-6, 3)
    t = rng.uniform(0.0, 1.0)
    kind = rng.integers(0, 4)
    c.append((l if kind & 1 else -INF, l + w if kind & 2 else INF, l + t * w))
  return [tuple(F(x) for x in t) for t in c]


BOUND_CASES = _bound_cases()


def _cols(rows):
  return [np.ascontiguousarray(np.array(r, dtype=np.float64)) for r in zip(*rows)]


def _start_rule(v0, l, u):
  k1 = k2 = F(1e-2)
  fr, hl, hu = _kind(l, u)
  width = (u - l) if (hl and hu) else INF
  pl = dmin(k1 * dmax(F(1.0), abs(l)), k2 * width)
  pu = dmin(k1 * dmax(F(1.0), abs(u)), k2 * width)
  v = v0
  v = dmax(v, l + pl) if hl else v
  v = dmin(v, u - pu) if hu else v
  v = v if fr else l
  return v, F(1.0 if hl else 0.0), F(1.0 if hu else 0.0)


def test_bound_start_rule(sim):
  """every bound class, the caller's value inside, on and outside the bounds: z, zL, zU bit for bit"""
  rows = [(v0, l, u) for (l, u, zv) in BOUND_CASES for v0 in (zv, l, u, F(-3.0), F(1e5), zv + F(1e-3))]
  v0, l, u = _cols(rows)
  out = np.zeros(3 * len(rows))
  sim.hostsim_bound_start.argtypes = [C.c_int] + [C.c_void_p] * 4
  sim.hostsim_bound_start(len(rows), A(v0), A(l), A(u), A(out))
  with np.errstate(all="ignore"):
    want = np.array([_start_rule(*r) for r in rows]).ravel()
  np.testing.assert_array_equal(out, want)
  assert {_kind(l, u) for (_, l, u) in rows} == {(False, False, False), (True, True, False), (True, False, True), (True, True, True), (True, False, False)}
  assert np.isnan(out).any()      # (a NaN bound pins the variable on it)


def _accept_rule(rcp, l, u, zv, d, zl, zu, ap, ad, mu, ksig):
  div = (lambda x, s: x * (F(1.0) / s)) if rcp else (lambda x, s: x / s)
  iks = F(1.0) / ksig
  fr, hl, hu = _kind(l, u)
  zn = zv + ap * d if fr else zv
  sl, su = (zv - l if hl else F(1.0)), (u - zv if hu else F(1.0))
  snl, snu = (zn - l if hl else F(1.0)), (u - zn if hu else F(1.0))
  vl = zl + ad * (-zl + div(mu - zl * d, sl))
  vu = zu + ad * (-zu + div(mu + zu * d, su))
  ml, mu_ = div(mu, snl), div(mu, snu)
  vl = dmax(dmin(vl, ksig * ml), ml * iks)
  vu = dmax(dmin(vu, ksig * mu_), mu_ * iks)
  return zn, (vl if hl else F(0.0)), (vu if hu else F(0.0))


def _step_rows():
  """the bound cases x steps towards and away from each bound x ad in {0, 1} x ksig = 1e10 and 1 (both ends of the band bind) x two mu"""
  rng = np.random.default_rng(15)
  rows = []
  for (l, u, zv) in BOUND_CASES:
    for d in (F(-0.5), F(0.5), F(0.0), F(-1e-3) * abs(zv), F(2.0) * abs(zv)):
      for ad in (F(0.0), F(1.0)):
        for ksig in (F(1e10), F(1.0)):
          rows.append((l, u, zv, d, F(rng.uniform(0.1, 3.0)), F(10.0 ** rng.uniform(-9, 2)), F(rng.uniform(0.0, 1.0)), ad, F(10.0 ** rng.integers(-9, 0)), ksig))
  for (l, u, zv) in BOUND_CASES[-60:]:
    rows.append((l, u, zv, F(rng.normal()), F(10.0 ** rng.uniform(-6, 2)), F(10.0 ** rng.uniform(-6, 2)), F(rng.uniform(0.0, 1.0)), F(rng.uniform(0.0, 1.0)),
                 F(10.0 ** rng.uniform(-9, 0)), F(10.0 ** rng.uniform(0.0, 10.0))))
  return rows


STEP_ROWS = _step_rows()      # (l, u, zv, d, zl, zu, ap, ad, mu, ksig)


@pytest.fixture(scope="module")
def accepted(sim):
  cols = _cols(STEP_ROWS)
  sim.hostsim_bound_accept.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 11
  got = {}
  for rcp in (0, 1):
    out = np.zeros(3 * len(STEP_ROWS))
    sim.hostsim_bound_accept(len(STEP_ROWS), rcp, *[A(c) for c in cols], A(out))
    got[rcp] = out
  return got


@pytest.mark.parametrize("rcp", [0, 1])
def test_bound_accept_rule(accepted, rcp):
  """new multipliers and their kappa_sigma band, dividing (rcp = 0) and multiplying by the reciprocal (rcp = 1): bit for bit"""
  with np.errstate(all="ignore"):
    want = np.array([_accept_rule(rcp, *r) for r in STEP_ROWS]).ravel()
  np.testing.assert_array_equal(accepted[rcp], want)
  # the flag is wired: some case has other bits with the reciprocal; and the band binds at both ends where ksig = 1
  assert (accepted[0].view(np.int64) != accepted[1].view(np.int64)).sum() > 0      # (bit patterns: a NaN does not count as a difference)
  one = np.array([r[9] == 1.0 and _kind(r[0], r[1])[1] and r[7] == 1.0 for r in STEP_ROWS])
  zl = accepted[rcp].reshape(-1, 3)[:, 1]
  with np.errstate(all="ignore"):
    m = np.array([(r[8] * (F(1.0) / (r[2] + r[6] * r[3] - r[0])) if rcp else r[8] / (r[2] + r[6] * r[3] - r[0])) for r in STEP_ROWS])
  assert one.sum() > 50 and (zl[one] == m[one]).all()


def _terms_rule(zv, l, u, zl, zu, cmax, cmin):
  fr, hl, hu = _kind(l, u)
  sl, su = (zv - l if hl else F(1.0)), (u - zv if hu else F(1.0))
  zlv, zuv = (zl if hl else F(0.0)), (zu if hu else F(0.0))
  il, iu = (F(1.0) / sl if hl else F(0.0)), (F(1.0) / su if hu else F(0.0))
  cl, cu = sl * zlv, su * zuv
  cmax = dmax(cmax, dmax(cl if hl else cmax, cu if hu else cmax))
  cmin = dmin(cmin, dmin(cl if hl else cmin, cu if hu else cmin))
  return zlv * il + zuv * iu, iu - il, zuv - zlv, F(0.0 if fr else 1.0), cmax, cmin


def test_bound_terms_rule(sim):
  """barrier Hessian, mu-coefficient, multiplier difference, pinned flag and the complementarity extremes: bit for bit"""
  rows = [(r[2], r[0], r[1], r[4], r[5], cx, cn) for r in STEP_ROWS[::3] for (cx, cn) in ((F(0.0), INF), (F(0.5), F(1e-4)))]
  cols = _cols(rows)
  out = np.zeros(6 * len(rows))
  sim.hostsim_bound_terms.argtypes = [C.c_int] + [C.c_void_p] * 8
  sim.hostsim_bound_terms(len(rows), *[A(c) for c in cols], A(out))
  with np.errstate(all="ignore"):
    want = np.array([_terms_rule(*r) for r in rows]).ravel()
  np.testing.assert_array_equal(out, want)


def _limits_rule(zv, l, u, zl, zu, d, mu, wg, tau):
  rcp = lambda x: F(1.0) / x
  fr, hl, hu = _kind(l, u)
  sl, su = (zv - l if hl else F(1.0)), (u - zv if hu else F(1.0))
  zlv, zuv = (zl if hl else F(1.0)), (zu if hu else F(1.0))
  rsl, rsu = rcp(sl), rcp(su)
  gb = wg
  gb = gb - (mu * rsl if hl else F(0.0))
  gb = gb + (mu * rsu if hu else F(0.0))
  dzl = -zlv + (mu - zlv * d) * rsl
  dzu = -zuv + (mu + zuv * d) * rsu
  tol_, tou_ = hl and bool(d < 0.0), hu and bool(d > 0.0)
  ap_ = tau * (sl if tol_ else su) * rcp(abs(d)) if (tol_ or tou_) else F(1.0)
  ad_l = -tau * zlv * rcp(dzl) if (hl and dzl < 0.0) else F(1.0)
  ad_u = -tau * zuv * rcp(dzu) if (hu and dzu < 0.0) else F(1.0)
  return dmin(F(1.0), ap_), dmin(F(1.0), dmin(ad_l, ad_u)), F(0.0) + (gb * d if fr else F(0.0))


def test_step_limits_rule(sim):
  """fraction-to-the-boundary limits of the point and of both multipliers, and the merit slope's term: bit for bit"""
  rows = [(r[2], r[0], r[1], r[4], r[5], r[3], r[8], F(0.37) * r[6], dmax(F(0.99), F(1.0) - r[8])) for r in STEP_ROWS[::2]]
  cols = _cols(rows)
  out = np.zeros(3 * len(rows))
  sim.hostsim_step_limits.argtypes = [C.c_int] + [C.c_void_p] * 10
  sim.hostsim_step_limits(len(rows), *[A(c) for c in cols], A(out))
  with np.errstate(all="ignore"):
    want = np.array([_limits_rule(*r) for r in rows]).ravel()
  np.testing.assert_array_equal(out, want)
  assert (out.reshape(-1, 3)[:, 0] < 1.0).sum() > 20 and (out.reshape(-1, 3)[:, 1] < 1.0).sum() > 20


@pytest.mark.parametrize("k", [2, 10, 28])
def test_slack_log_value(sim, k):
  """SlackLog::value() of points of k variables against R = fsum(log s_i) over the same clamped slacks, within
  2^-52 (k + |log slk| + 2 |sexp| ln 2 + |R| + sum |log s_i|): k roundings of the mantissa product (and of the pairs), one of the log, the
  product with the rounded ln 2, the final sum, the reference's own logs.  slack_pair and the violation count are exact."""
  import math
  rng = np.random.default_rng(16 + k)
  one_sided = [c for c in BOUND_CASES if _kind(c[0], c[1]) in ((True, True, False), (True, False, True), (True, False, False))]
  # (the product of a two-sided pair must be a normal double: 1e-200 on both sides or 1e150 x 1e300 are left to the one-sided cases)
  with np.errstate(all="ignore"):
    two_sided = [c for c in BOUND_CASES if _kind(c[0], c[1]) == (True, True, True) and (c[2] - c[0] <= 0.0 or c[1] - c[2] <= 0.0 or 1e-290 < (c[2] - c[0]) * (c[1] - c[2]) < 1e290)]
  other = [c for c in BOUND_CASES if not _kind(c[0], c[1])[0]]
  pool = one_sided + two_sided + other
  points = [[pool[i] for i in rng.integers(0, len(pool), k)] for _ in range(40)]
  points.append([c for c in one_sided if c[2] in (1e300, -1e300)][:k] * k)      # all large, all small: the exponents add up, nothing overflows
  points.append([c for c in one_sided if c[2] in (1e-300, -1e-300)][:k] * k)
  points = [p[:k] for p in points]
  flat = [c for p in points for c in p]
  l, u, v = _cols(flat)
  out, pairs = np.zeros(4 * len(points)), np.zeros(len(flat))
  sim.hostsim_slack_log.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5
  sim.hostsim_slack_log(len(points), k, A(v), A(l), A(u), A(out), A(pairs))
  worst = 0.0
  for p, pt in enumerate(points):
    s, bad = [], 0
    for i, (lo, up, x) in enumerate(pt):
      fr, hl, hu = _kind(lo, up)
      sl, su = (x - lo if hl else F(1.0)), (up - x if hu else F(1.0))
      bad += (0 if sl > 0.0 else 1) + (0 if su > 0.0 else 1)
      sl, su = (sl if sl > 0.0 else F(1.0)), (su if su > 0.0 else F(1.0))
      assert pairs[p * k + i] == sl * su
      s += [float(sl), float(su)]
    got, slk, sexp, nbad = out[4 * p:4 * p + 4]
    assert nbad == bad
    R = math.fsum(math.log(x) for x in s)
    bound = 2.0 ** -52 * (k + abs(math.log(slk)) + 2.0 * abs(sexp) * math.log(2.0) + abs(R) + sum(abs(math.log(x)) for x in s))
    assert np.isfinite(got) and np.isfinite(bound) and abs(got - R) <= bound, (p, got, R, bound)
    worst = max(worst, abs(got - R) / bound if bound > 0.0 else 0.0)
  print(f"k = {k}: largest |value - R| / bound = {worst:.3f}")
  assert sum(out[3::4] > 0) > 3      # (some points hold a violated bound)
