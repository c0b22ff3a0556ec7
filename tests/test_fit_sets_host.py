"""The host side of the ensemble fit (myr_fit_grad_sets, neural_ode/node_training.train_ensemble) that needs no device: the export and its
null-handle refusal, and train_ensemble = E separate `train` runs on a stub loss -- records, best parameters and last epochs, to the bit."""
import numpy as np

from myriad_amd import _lib
from myriad_amd.config import HParams, OptimizerType
from myriad_amd.neural_ode import node_training
from myriad_amd.systems import SystemType
from myriad_amd.systems.neural_ode import flat_from_mapping, mapping_from_flat


def test_null_handle_is_an_argument_error():
  lib = _lib.load()
  assert "myr_fit_grad_sets" in _lib.EXPORTS
  a = np.zeros(8)
  rc = lib.myr_fit_grad_sets(None, 1, 1, 1, 1, a.ctypes.data, a.ctypes.data, 0, None, a.ctypes.data, a.ctypes.data, a.ctypes.data, 0, _lib.MEM_HOST)
  assert rc == -1 and b"myr_fit_grad_sets" in lib.myr_last_error()
  assert lib.myr_version().decode().startswith("myriad_hip 0.10")


class QuadraticFit:
  """A loss with the interfaces of NodeFitLoss and no device: loss(p, data) = sum_k (p[k] - c_k(data))^2 over the first four weights, c(data) the
  mean of the data's state columns -- every set is pulled towards the centre of its own minibatch."""

  def __init__(self):
    self.calls = []                                               # (kind, number of sets) of every ensemble call

  @staticmethod
  def _one(flat, data):
    c = np.asarray(data, dtype=np.float64)[:, :, :4].mean(axis=(0, 1))
    d = flat[:4] - c
    g = np.zeros_like(flat)
    g[:4] = 2.0 * d
    return float((d * d).sum()), g

  def value_and_grad(self, params, minibatch):
    v, g = self._one(flat_from_mapping(params), minibatch)
    return v, mapping_from_flat(g)

  def __call__(self, params, minibatch):
    return self.value_and_grad(params, minibatch)[0]

  def values_and_grads(self, params_sets, minibatches, want_grad=True):
    mb = np.asarray(minibatches)
    out = [self._one(p, mb if mb.ndim == 3 else mb[e]) for e, p in enumerate(params_sets)]
    self.calls.append(("grad" if want_grad else "loss", len(out)))
    return [v for v, _ in out], (np.stack([g for _, g in out]) if want_grad else None)

  def values(self, params_sets, minibatches):
    return self.values_and_grads(params_sets, minibatches, want_grad=False)[0]


def _setup():
  hp = HParams(system=SystemType.CARTPOLE, optimizer=OptimizerType.SHOOTING, intervals=1, controls_per_interval=3, train_size=5, val_size=2,
               test_size=2, minibatch_size=2, num_epochs=9, loss_recording_frequency=3, early_stop_check_frequency=2, early_stop_threshold=2,
               learning_rate=1e-2, seed=7)
  rng = np.random.default_rng(0)
  E = 3
  params = rng.standard_normal((E, 4804))
  train_data = rng.standard_normal((E, 6, 4, 5))                  # (one row more than train_size: the permutation draws from all of them)
  val_data = train_data[:, :2] + 0.01 * rng.standard_normal((E, 2, 4, 5))
  # set 1: the validation centre lies away from the training centre, on the far side of the start -- training makes its validation loss worse
  val_data[1, :, :, :4] = (2.0 * params[1, :4] - train_data[1, :, :, :4].mean(axis=(0, 1)))[None, None, :]
  return hp, E, params, train_data, val_data


def test_lockstep_equals_separate_runs():
  hp, E, params, train_data, val_data = _setup()
  singles = [node_training.train(hp, 1.0, mapping_from_flat(params[e]), train_data[e], val_data[e], rng=np.random.default_rng(hp.seed + e),
                                 fit=QuadraticFit()) for e in range(E)]
  fit = QuadraticFit()
  runs = node_training.train_ensemble(hp, 1.0, params.copy(), train_data, val_data, fit=fit)
  assert len(runs) == E
  for e, ((best, epoch, record), (sbest, sepoch, srecord)) in enumerate(zip(runs, singles)):
    assert epoch == sepoch, e
    assert record == srecord, e                                   # equal floats, not close ones
    assert flat_from_mapping(best).tobytes() == flat_from_mapping(sbest).tobytes(), e
  # set 1 stopped early, the others ran to the end; once it had stopped the calls carried two sets
  assert [ep for _, ep, _ in runs] == [8, 4, 8]
  assert fit.calls[0] == ("loss", 3) and fit.calls[-1] == ("grad", 2) and ("grad", 3) in fit.calls
  # mappings as input, explicit generators, shared data: the same entry points
  again = node_training.train_ensemble(hp, 1.0, [mapping_from_flat(p) for p in params], train_data, val_data,
                                       rngs=[np.random.default_rng(hp.seed + e) for e in range(E)], fit=QuadraticFit())
  assert [r[2] for r in again] == [r[2] for r in runs]
  shared = node_training.train_ensemble(hp, 1.0, params[:2].copy(), train_data[0], val_data[0], fit=QuadraticFit())
  one = node_training.train(hp, 1.0, mapping_from_flat(params[1]), train_data[0], val_data[0], rng=np.random.default_rng(hp.seed + 1), fit=QuadraticFit())
  assert shared[1][2] == one[2] and shared[1][1] == one[1] and flat_from_mapping(shared[1][0]).tobytes() == flat_from_mapping(one[0]).tobytes()


def test_adam_sets_rows_are_optimisers_of_their_own():
  """rows that sit out steps keep their moments and their own step count: every row follows an mle_sysid.Adam of its own, to the bit"""
  from myriad_amd.experiments.mle_sysid import Adam
  rng = np.random.default_rng(3)
  P = rng.standard_normal((3, 7))
  opt, singles, ref = node_training.AdamSets(P.shape, 3e-3), [Adam(3e-3) for _ in range(3)], P.copy()
  for rows in ([0, 1, 2], [0, 2], [2], [1, 2], [0, 1, 2]):
    g = rng.standard_normal((len(rows), 7)) * 10.0 ** rng.integers(-3, 2, (len(rows), 7))
    P[rows] = opt.update(rows, P[rows], g)
    for i, r in enumerate(rows):
      ref[r] = singles[r].update({"p": ref[r]}, {"p": g[i]})["p"]
  assert opt.t == [3, 3, 5] and P.tobytes() == ref.tobytes()
