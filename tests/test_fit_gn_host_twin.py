"""Gauss-Newton fit (myriad_amd/csrc/fit_gn.h: FitGnLane<Sys>; experiments/mle_sysid.py: the Levenberg-Marquardt drivers) on the host.

The twin (tests/hostsim/fit_gn_twin.cpp) is the device code's own FitGnLane<Sys> compiled with g++ and looped over a batch.

Twin against the oracle.  The reference is J = d xh / d p of the oracle's rollout (forward-mode autograd, one pass per parameter; central
differences for HIVTREATMENT), grad and gn formed from it in numpy (tests/fit_gn_cases.py).  Matrix: CARTPOLE, VANDERPOL, CANCERTREATMENT,
PENDULUM, HIVTREATMENT, ROCKETLANDING, HARVEST x 4 integrators, unweighted and weighted, RK4 also with u_rows = 2S+1; B = 3.
Measured over the six autograd systems (both sides fp64, they differ in the order of their sums):
  largest |dgn| / max|gn|         1.1e-15   -> asserted 1.1e-14
  largest |dgrad| / max|grad|     1.2e-13   -> asserted 1.2e-12
HIVTREATMENT (central differences): to the relative tolerance 1e-6 the differences resolve (measured 2.5e-08 at worst, grad and gn).

Forward against reverse.  The twin's grad (forward sensitivities) against fit_twin's (reverse sweep) on the same inputs, all 20 systems, HEUN and
RK4: largest |dgrad| / max|grad| 3.6e-15 -> asserted 3.6e-14; the losses are equal to the bit.

Levenberg-Marquardt on the twin.  Noise-free data (the twin's rollout at the default parameters), start = the defaults moved by up to 5 %, HEUN,
B = 8, S = steps_for(name), all np parameters free.  Conditions: at most 30 iterations and final loss <= 1e-12 x initial loss.  All six candidate
systems meet both and are kept (iterations; final / initial loss; largest relative parameter error where gn has full rank):
  CARTPOLE         5    1.5e-28   2.2e-16
  VANDERPOL        4    1.6e-25   1.8e-15
  PENDULUM         4    1.4e-26   (rank 1 of 3)
  MOUNTAINCAR     13    5.7e-25   5.6e-14
  CANCERTREATMENT  5    4.9e-27   (rank 2 of 3)
  GLUCOSE          5    1.9e-27   (rank 3 of 5)
PENDULUM's dynamics hold g / length only and m not at all -- gn has rank 1, the loss is driven to rounding level along the one direction the data
see --, and the cost-only parameters of CANCERTREATMENT (a) and GLUCOSE (A, l) have rows and columns of 0: no parameter error is asserted for them.
"""
import numpy as np
import pytest

import fit_cases as F
import fit_gn_cases as G
from myriad_amd import _lib

GN_TOL = 1.1e-14       # 10 x measured
GRAD_TOL = 1.2e-12     # 10 x measured
FR_TOL = 3.6e-14       # 10 x measured
FULL_RANK = {"CARTPOLE": 2.2e-15, "VANDERPOL": 1.8e-14, "MOUNTAINCAR": 5.6e-13}      # relative parameter error asserted: 10 x measured


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
  return G.build_twin(tmp_path_factory.mktemp("fit_gn_twin"))


@pytest.fixture(scope="module")
def fit_twin(tmp_path_factory):
  return F.build_twin(tmp_path_factory.mktemp("fit_twin"))


# ---- twin against the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.GN_SYSTEMS)
def test_twin_matches_oracle(twin, name):
  for (_, method, long_u, weighted) in F.matrix((name,)):
    xs_obs, us, params = F.inputs(name, method, long_u)
    S = xs_obs.shape[1] - 1
    ref_loss, ref_grad, ref_gn = G.reference(name, method, long_u, weighted)
    wt = F.decaying_wt(S) if weighted else None
    loss, grad, gn = G.twin_fit_gn(twin, name, method, F.horizon(name), xs_obs, us, params, wt)
    eg, en = G.rel_errors(grad, gn, ref_grad, ref_gn)
    el = float((np.abs(loss - ref_loss) / ref_loss).max())
    print(f"{name} {method} u_rows={us.shape[1]} wt={'decaying' if weighted else 'none'}: dloss {el:.2e} dgrad {eg:.2e} dgn {en:.2e}")
    assert (ref_loss > 0).all() and np.abs(ref_grad).max() > 0 and np.abs(ref_gn).max() > 0
    assert el <= 2.7e-12, (method, long_u, weighted, el)                   # test_fit_host_twin.py's bound: the loss is FitLane's
    fd = name in F.FD_SYSTEMS
    assert eg <= (F.FD_RTOL if fd else GRAD_TOL), (method, long_u, weighted, eg)
    assert en <= (F.FD_RTOL if fd else GN_TOL), (method, long_u, weighted, en)


# ---- forward against reverse ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.SYSTEMS)
def test_forward_gradient_equals_reverse_gradient(twin, fit_twin, name):
  for method in ("HEUN", "RK4"):
    xs_obs, us, params = F.inputs(name, method)
    wt = F.decaying_wt(xs_obs.shape[1] - 1)
    loss, grad, _ = G.twin_fit_gn(twin, name, method, F.horizon(name), xs_obs, us, params, wt)
    rloss, rgrad = F.twin_loss_grad(fit_twin, name, method, F.horizon(name), xs_obs, us, params, wt)
    e = float((np.abs(grad - rgrad).max(axis=-1) / np.abs(rgrad).max(axis=-1)).max())
    print(f"{name} {method}: forward against reverse dgrad {e:.2e}")
    assert loss.tobytes() == rloss.tobytes()
    assert e <= FR_TOL, (method, e)


# ---- structure -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.SYSTEMS)
def test_gn_is_symmetric_and_positive_semidefinite(twin, name):
  for method, weighted in (("RK4", False), ("HEUN", True)):
    xs_obs, us, params = F.inputs(name, method)
    wt = F.decaying_wt(xs_obs.shape[1] - 1) if weighted else None
    _, _, gn = G.twin_fit_gn(twin, name, method, F.horizon(name), xs_obs, us, params, wt)
    assert gn.tobytes() == np.ascontiguousarray(gn.transpose(0, 2, 1)).tobytes()
    for b in range(gn.shape[0]):
      assert np.linalg.eigvalsh(gn[b]).min() >= -1e-12 * np.trace(gn[b]), (method, b)
    # gn without grad and loss: the same bits
    _, none, only = G.twin_fit_gn(twin, name, method, F.horizon(name), xs_obs, us, params, wt, want_grad=False)
    assert none is None and only.tobytes() == gn.tobytes()


@pytest.mark.parametrize("name", sorted(F.COST_ONLY))
def test_cost_only_parameters_get_exact_zeros(twin, name):
  xs_obs, us, params = F.inputs(name, "RK4")
  _, grad, gn = G.twin_fit_gn(twin, name, "RK4", F.horizon(name), xs_obs, us, params)
  names = F.O.SYSTEMS[name].param_names
  for k in F.COST_ONLY[name]:
    i = names.index(k)
    for a in (grad[:, i], gn[:, i, :], gn[:, :, i]):
      assert (a == 0.0).all() and not np.signbit(a).any(), (k, a)
  others = [i for i, k in enumerate(names) if k not in F.COST_ONLY[name]]
  assert (gn[:, others, others] > 0.0).all()


def test_per_instance_parameters_and_defaults(twin):
  """a parameter row per trajectory gives the rows of single calls, bitwise; params = None runs the defaults"""
  xs_obs, us, params = F.inputs("CARTPOLE", "HEUN", per_instance=True)
  T = F.horizon("CARTPOLE")
  loss, grad, gn = G.twin_fit_gn(twin, "CARTPOLE", "HEUN", T, xs_obs, us, params)
  for b in range(F.B):
    l1, g1, n1 = G.twin_fit_gn(twin, "CARTPOLE", "HEUN", T, xs_obs[b:b + 1], us[b:b + 1], params[b])
    assert l1.tobytes() == loss[b:b + 1].tobytes() and g1.tobytes() == grad[b:b + 1].tobytes() and n1.tobytes() == gn[b:b + 1].tobytes()
  ref = G.reference("CARTPOLE", "HEUN", per_instance=True)
  eg, en = G.rel_errors(grad, gn, ref[1], ref[2])
  assert eg <= GRAD_TOL and en <= GN_TOL
  dflt = G.twin_fit_gn(twin, "CARTPOLE", "HEUN", T, xs_obs, us, None)
  same = G.twin_fit_gn(twin, "CARTPOLE", "HEUN", T, xs_obs, us, F.O.CartPole().params())
  assert all(a.tobytes() == b.tobytes() for a, b in zip(dflt, same))


def test_second_order_model(twin):
  """loss(p + d) = loss + grad . d + d . gn d / 2 up to the residual-curvature term the Gauss-Newton matrix leaves out and O(|d|^3): on
  noise-free data at the parameters that made them (r = 0) the term vanishes, loss and grad are 0 and d . gn d / 2 is the loss at p + d to O(|d|^3)"""
  name = "CARTPOLE"
  x0, us, _ = G.lm_inputs(name)
  data, T = G.lm_data(twin, name), F.horizon(name)
  p = F.O.CartPole().params()
  loss, grad, gn = G.twin_fit_gn(twin, name, "HEUN", T, data, us, p)
  assert (loss == 0.0).all() and (grad == 0.0).all()
  d = 1e-4 * p * np.array([1.0, -0.5, 0.7, -1.0])
  moved = G.twin_fit_gn(twin, name, "HEUN", T, data, us, p + d)[0].sum()
  model = 0.5 * d @ gn.sum(0) @ d
  assert abs(moved - model) <= 1e-3 * model, (moved, model)      # |d| / |p| = 1e-4: the cubic term is of that relative size


# ---- Levenberg-Marquardt on the twin ---------------------------------------------------------------------------------------------------------
def _lm(twin, name, max_iter=G.LM_MAX_ITER):
  x0, us, start = G.lm_inputs(name)
  data, T = G.lm_data(twin, name), F.horizon(name)

  def fit_gn(p):
    loss, grad, gn = G.twin_fit_gn(twin, name, "HEUN", T, data, us, p)
    return loss.sum(), grad.sum(0), gn.sum(0)
  return G.lm_run(fit_gn, start, max_iter)


@pytest.mark.parametrize("name", G.LM_SYSTEMS)
def test_levenberg_marquardt_reaches_rounding_level(twin, name):
  lm = _lm(twin, name, max_iter=50)
  p0 = F.O.SYSTEMS[name]().params()
  err = float((np.abs(lm.vector - p0) / np.abs(p0)).max())
  print(f"{name}: {lm.iterations} iterations, loss {lm.loss0:.3e} -> {lm.loss:.3e} (ratio {lm.loss / lm.loss0:.1e}), parameter error {err:.1e}")
  assert lm.iterations <= G.LM_MAX_ITER
  assert lm.loss <= G.LM_RATIO * lm.loss0
  if name in FULL_RANK:
    assert np.linalg.matrix_rank(lm.gn, hermitian=True) == p0.size
    assert err <= FULL_RANK[name], err


def test_thirty_gradient_steps_do_not_reach_it(twin, fit_twin):
  """the ratio is out of a first-order method's reach in 30 calls: Adam(1e-3), the recipe of run_mle_sysid, on CARTPOLE's problem"""
  from myriad_amd.experiments.mle_sysid import Adam
  name = "CARTPOLE"
  x0, us, start = G.lm_inputs(name)
  data, T = G.lm_data(twin, name), F.horizon(name)
  p, opt, losses = {"p": start.copy()}, Adam(1e-3), []
  for _ in range(G.LM_MAX_ITER + 1):
    loss, grad = F.twin_loss_grad(fit_twin, name, "HEUN", T, data, us, p["p"])
    losses.append(loss.sum())
    p = opt.update(p, {"p": grad.sum(0)})
  assert min(losses) > 1e-3 * losses[0]


# ---- the drivers -------------------------------------------------------------------------------------------------------------------------------
def test_lockstep_equals_separate_runs(twin):
  from myriad_amd.defaults import param_guesses
  from myriad_amd.experiments.mle_sysid import run_mle_sysid_gn, run_mle_sysid_gn_sets
  hp, cfg, datasets, truth, make_fit = G.driver_problem(twin, "VANDERPOL", 3)
  E = datasets.shape[0]
  # set 1 starts at its own truth: its first trial point cannot lower a loss of 0, it stops at once and leaves the later calls
  guesses = [dict(param_guesses[hp.system]) for _ in range(E)]
  guesses[1] = {"a": float(truth[1, 0])}
  fit = make_fit()
  runs = run_mle_sysid_gn_sets(hp, cfg, datasets, guesses=guesses, fit=fit)
  assert len(runs) == E
  for e in range(E):
    single = run_mle_sysid_gn(hp, cfg, datasets[e], fit=make_fit(), guess=guesses[e])
    assert set(single) == {"params", "last_params", "epochs", "train_losses", "val_losses", "iterations", "gn", "covariance"}
    for k in ("params", "last_params", "epochs", "train_losses", "val_losses", "iterations"):
      assert runs[e][k] == single[k], (e, k)                        # equal floats, not close ones
    assert runs[e]["gn"].tobytes() == single["gn"].tobytes() and runs[e]["covariance"].tobytes() == single["covariance"].tobytes()
  assert runs[1]["iterations"] == 0 and runs[0]["iterations"] > 1 and runs[2]["iterations"] > 1
  sets_calls = [n for kind, n in fit.engine.calls if kind == "fit_gn_sets"]
  assert sets_calls[0] == 3 and sets_calls[1] == 2 and len(sets_calls) == 1 + max(r["iterations"] for r in runs)
  for e in (0, 2):
    assert runs[e]["train_losses"][-1] <= 1e-12 * runs[e]["train_losses"][0]
    assert abs(runs[e]["last_params"]["a"] - truth[e, 0]) <= 1e-9 * truth[e, 0]


def test_sign_rule_and_fitted_keys(twin):
  """CARTPOLE's dynamics take |p|: a negative key gets the sign on grad and sign_i sign_j on gn; keys that are not fitted drop out"""
  from myriad_amd.experiments.mle_sysid import loss_weights
  hp, cfg, datasets, truth, make_fit = G.driver_problem(twin, "CARTPOLE", 1)
  fit = make_fit()
  pos = {"g": 10.0, "m2": 0.2, "length": 0.6}
  neg = {"g": 10.0, "m2": -0.2, "length": 0.6}
  v, g, G_ = fit.value_grad_gn(pos, datasets[0, :5])
  vn, gn_, Gn = fit.value_grad_gn(neg, datasets[0, :5])
  assert v == vn and G_.shape == (3, 3) and list(g) == ["g", "m2", "length"]
  s = np.array([1.0, -1.0, 1.0])
  assert np.array_equal(np.array(list(gn_.values())), np.array(list(g.values())) * s) and np.array_equal(Gn, G_ * np.outer(s, s))
  full = fit.engine.fit_gn(datasets[0, :5, :, :4], datasets[0, :5, :, 4:], params=np.array([10.0, 1.0, 0.2, 0.6]),
                           wt=loss_weights(hp, 5, 0), reduce=True)
  assert np.array_equal(G_, full["gn"][np.ix_([0, 2, 3], [0, 2, 3])])
  vs, gs, Gs = fit.values_grads_gns([pos, neg], datasets[0, :5])
  assert vs == [v, vn] and gs == [g, gn_] and np.array_equal(Gs[0], G_) and np.array_equal(Gs[1], Gn)


def test_parameter_covariance():
  from myriad_amd.experiments.mle_sysid import parameter_covariance
  rng = np.random.default_rng(5)
  J = rng.standard_normal((40, 3))
  J[:, 1] = 0.0                                                   # a parameter the data do not see
  r = 0.1 * rng.standard_normal(40)
  cov = parameter_covariance(2.0 * J.T @ J, r @ r, 40)
  on = [0, 2]
  ref = (r @ r) / (40 - 2) * np.linalg.inv(J[:, on].T @ J[:, on])
  assert np.allclose(cov[np.ix_(on, on)], ref, rtol=1e-12, atol=0.0) and (cov[1] == 0.0).all() and (cov[:, 1] == 0.0).all()


# ---- the library without a device ----------------------------------------------------------------------------------------------------------------
def test_null_handle_is_an_argument_error():
  lib = _lib.load()
  assert "myr_fit_gn" in _lib.EXPORTS and "myr_fit_gn_sets" in _lib.EXPORTS
  a = np.zeros(8)
  p = a.ctypes.data
  assert lib.myr_fit_gn(None, 1, 1, 1, p, p, None, p, 0, p, p, p, 0, _lib.MEM_HOST) == -1
  assert b"myr_fit_gn:" in lib.myr_last_error()
  assert lib.myr_fit_gn_sets(None, 1, 1, 1, 1, p, p, 0, None, p, p, p, p, 0, _lib.MEM_HOST) == -1
  assert b"myr_fit_gn_sets:" in lib.myr_last_error()
  assert lib.myr_version().decode() == "myriad_hip 0.10 (gfx950)"
