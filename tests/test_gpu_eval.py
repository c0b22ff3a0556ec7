"""GPU parity tests of the hs_eval kernel (through the C-ABI) against the oracle and the golden vectors."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _engine(name, N, T, **kw):
  from myriad_amd import _lib
  return _lib.Engine(name, "HERMITE_SIMPSON", N, T, **kw)


def _full_grad(eng, g):
  """Expand the kernel's gradient output to the full z layout."""
  if eng.ngrad == eng.n:
    return g
  out = np.zeros((g.shape[0], eng.n))
  out[:, eng.x_rows * eng.ns:] = g
  return out


def test_eval_matches_golden_vectors(golden_dir):
  files = sorted(glob.glob(os.path.join(golden_dir, "eval_hs_*.npz")))
  assert len(files) >= 5
  for path in files:
    name = os.path.basename(path).split("_")[2].upper()
    d = np.load(path)
    eng = _engine(name, int(d["N"]), float(d["T"]))
    out = eng.eval(d["z"], params=d["params"])
    np.testing.assert_allclose(out["f"], d["f"], rtol=1e-12, err_msg=path)
    np.testing.assert_allclose(out["c"], d["c"], rtol=1e-12, atol=1e-12, err_msg=path)
    np.testing.assert_allclose(out["jblk"].reshape(d["jblk"].shape), d["jblk"], rtol=1e-12, atol=1e-12, err_msg=path)
    np.testing.assert_allclose(_full_grad(eng, out["gradf"]), d["gradf"], rtol=1e-12, atol=1e-13, err_msg=path)
    eng.close()


@pytest.mark.parametrize("wpt", ["1", "4", "8"])
def test_eval_matches_oracle_random_batch(wpt, monkeypatch):
  """Seeded random batch, ragged batch size, per-instance parameters, every workgroup shape."""
  from oracle import myriad_oracle as O
  monkeypatch.setenv("MYRIAD_EVAL_WPT", wpt)
  N, B = 13, 37
  rng = np.random.default_rng(7)
  params = np.array([9.81, 1.0, 0.3, 0.5]) * (1 + 0.2 * rng.uniform(-1, 1, (B, 4)))
  eng = _engine("CARTPOLE", N, 2.0)
  tr0 = O.hermite_simpson(O.CartPole(), N)
  z = tr0.guess[None] + 0.5 * rng.standard_normal((B, tr0.guess.size))
  out = eng.eval(z, params=params)
  for b in range(0, B, 6):
    s = O.CartPole(*params[b])
    cb = O.Callbacks(O.hermite_simpson(s, N))
    np.testing.assert_allclose(out["c"][b], cb.cons(z[b]), rtol=1e-12, atol=1e-12)
    J = O.hs_dense_from_blocks(out["jblk"][b].reshape(N, -1), N, 4, 1)
    np.testing.assert_allclose(J, cb.jac(z[b]), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(out["f"][b], cb.fun(z[b]), rtol=1e-12)
    np.testing.assert_allclose(_full_grad(eng, out["gradf"])[b], cb.grad(z[b]), rtol=1e-12, atol=1e-13)


def test_eval_edge_cases():
  from myriad_amd import _lib
  eng = _engine("CARTPOLE", 1, 2.0)            # smallest transcription: one interval
  z = np.zeros((1, eng.n)); z[0, -3:] = [1., 2., 3.]
  out = eng.eval(z)
  assert out["f"][0] == pytest.approx((2.0 / 6) * (1 + 4 * 4 + 9))
  assert eng.eval(np.zeros((0, eng.n)))["c"].shape == (0, eng.m)      # empty batch
  out = eng.eval(z, want=("c",))                                        # NULL outputs are skipped
  assert set(out) == {"c"}
  with pytest.raises(ValueError):
    eng.eval(np.zeros((2, eng.n + 1)))
  trap = _lib.Engine("CARTPOLE", "TRAPEZOIDAL", 4, 2.0)
  assert (trap.n, trap.m, trap.jblk) == (25, 16, 4 * (2 * 16 + 2 * 4))
  rk = _lib.Engine("CARTPOLE", "SHOOTING", 2, 2.0, controls_per_interval=3, integration_method="RK4")
  assert (rk.n, rk.m, rk.jblk) == (3 * 4 + (2 * 6 + 1) * 1, 2 * 4, 2 * (16 + 4 * (2 * 3 + 1)))      # RK4: 2 control rows per step
  assert rk.eval(np.zeros((1, rk.n)))["c"].shape == (1, 8)


def test_eval_full_size_properties():
  """BASELINE config 2 size (N=100, B=4096): size-independent properties -- a feasible trajectory built by
  construction has zero interpolation residual; J blocks are linear in h-scaled A/B; device == host path."""
  import torch
  torch.cuda.init()                      # make torch own a context before the library allocates
  from myriad_amd import _lib
  from oracle import myriad_oracle as O
  N, B = 100, 4096
  eng = _engine("CARTPOLE", N, 2.0, max_batch=B)
  s = O.CartPole()
  x0 = O.random_x0(s, B)
  K = 2 * N + 1
  lin = np.linspace(0., 1., K)[None, :, None]
  xs = x0[:, None, :] * (1 - lin) + s.x_T[None, None, :] * lin
  z = np.concatenate([xs.reshape(B, -1), np.zeros((B, K))], axis=1)
  host = eng.eval(z)
  # device-pointer path must give bitwise the same result as the host-staged path
  zt = torch.from_numpy(z).cuda()
  f = torch.empty(B, dtype=torch.float64, device="cuda"); g = torch.empty(B, eng.ngrad, dtype=torch.float64, device="cuda")
  c = torch.empty(B, eng.m, dtype=torch.float64, device="cuda"); j = torch.empty(B, eng.jblk, dtype=torch.float64, device="cuda")
  torch.cuda.synchronize()
  eng.eval_device(B, zt, f=f, gradf=g, c=c, jblk=j)
  assert np.array_equal(c.cpu().numpy(), host["c"]) and np.array_equal(j.cpu().numpy(), host["jblk"])
  assert np.array_equal(f.cpu().numpy(), host["f"]) and g.cpu().numpy().tobytes() == host["gradf"].tobytes()
  # u = 0 -> objective and its gradient vanish (g = u^2)
  assert np.all(host["f"] == 0) and np.all(host["gradf"] == 0)
  # spot-check 3 instances against the oracle at full size
  cb_cache = {}
  for b in (0, 1777, 4095):
    sb = O.CartPole(); sb.x_0 = x0[b]
    cb = O.Callbacks(O.hermite_simpson(sb, N))
    np.testing.assert_allclose(host["c"][b], cb.cons(z[b]), rtol=1e-12, atol=1e-12)
