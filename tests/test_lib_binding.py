"""The derivative and fit methods of myriad_amd._lib.Engine (exgd_grad*, hvp*, fit_grad*, fit_gn* and their _device / _probe forms) against a recording fake of the library: which
C function each calls, every scalar, which pointers are null, the shape of every array handed over, and the dict that comes back.  No library is
loaded and no GPU is needed: the Engine is made without a handle, and _addr hands the arrays through instead of their addresses."""
import re
import types

import numpy as np
import pytest

from myriad_amd import _lib

N, M, NS, NU = 35, 24, 4, 1      # CARTPOLE, Hermite-Simpson, 3 intervals
B, E, R = 3, 2, 2
HOST, DEVICE = _lib.MEM_HOST, _lib.MEM_DEVICE

_GRAD_TAIL = ("eta_x", "eta_v", "nsteps", "seed_z", "seed_lam", "grad", "grad_stride", "dz0", "dlam0", "mem")
_HVP_TAIL = ("with_cost", "out_z", "out_p", "p_stride", "mem")
ORDER = {
  "myr_exgd_grad": ("B", "z", "lam", "lb", "ub", "params", "stride") + _GRAD_TAIL,
  "myr_exgd_grad_shoot": ("B", "z", "lam", "lb", "ub", "params", "stride") + _GRAD_TAIL,
  "myr_exgd_grad_node": ("B", "z", "lam", "lb", "ub", "params") + _GRAD_TAIL,
  "myr_exgd_grad_node_shoot": ("B", "z", "lam", "lb", "ub", "params") + _GRAD_TAIL,
  "myr_exgd_grad_node_sets": ("E", "R", "z", "lam", "lb", "ub", "params") + _GRAD_TAIL,
  "myr_hvp": ("B", "z", "lam", "v", "params", "stride") + _HVP_TAIL,
  "myr_hvp_node": ("B", "z", "lam", "v", "params") + _HVP_TAIL,
  "myr_hvp_node_sets": ("E", "R", "z", "lam", "v", "params") + _HVP_TAIL,
}
_FIT_SINGLE = ("B", "num_steps", "u_rows", "xs_obs", "us", "wt", "params", "stride", "loss", "grad")
_FIT_SETS = ("E", "R", "num_steps", "u_rows", "xs_obs", "us", "data_shared", "wt", "params", "loss", "grad")
ORDER.update({
  "myr_fit_grad": _FIT_SINGLE + ("grad_stride", "mem"), "myr_fit_gn": _FIT_SINGLE + ("gn", "out_stride", "mem"),
  "myr_fit_grad_sets": _FIT_SETS + ("grad_stride", "mem"), "myr_fit_gn_sets": _FIT_SETS + ("gn", "out_stride", "mem"),
})
# method -> (C function, parameter sets?, Gauss-Newton matrix?)
FITS = {"fit_grad": ("myr_fit_grad", False, False), "fit_gn": ("myr_fit_gn", False, True),
        "fit_grad_sets": ("myr_fit_grad_sets", True, False), "fit_gn_sets": ("myr_fit_gn_sets", True, True)}
S, U, NP = 4, 6, 4      # steps, control rows and parameters of the fit calls
# method -> (C function, network system?, weight sets?)
GRADS = {"exgd_grad": ("myr_exgd_grad", False, False), "exgd_grad_shoot": ("myr_exgd_grad_shoot", False, False),
         "exgd_grad_node": ("myr_exgd_grad_node", True, False), "exgd_grad_node_shoot": ("myr_exgd_grad_node_shoot", True, False),
         "exgd_grad_node_sets": ("myr_exgd_grad_node_sets", True, True)}
HVPS = {"hvp": ("myr_hvp", False, False), "hvp_node": ("myr_hvp_node", True, False), "hvp_node_sets": ("myr_hvp_node_sets", True, True)}


class FakeLib:
  """every attribute is a C function that records its call and returns MYR_OK"""
  def __init__(self):
    self.calls = []

  def __getattr__(self, name):
    def fn(*args):
      self.calls.append((name, args))
      return 0
    return fn


@pytest.fixture
def engine(monkeypatch):
  monkeypatch.setattr(_lib, "_addr", lambda a: a)      # the arrays themselves reach the fake
  def make(npar):
    eng = object.__new__(_lib.Engine)
    eng.lib, eng._h = FakeLib(), types.SimpleNamespace(value=0)
    eng.n, eng.m, eng.ns, eng.nu, eng.np = N, M, NS, NU, npar
    return eng
  return make


def _last(eng, fn):
  """the one call the method made, as {argument name: value}"""
  assert len(eng.lib.calls) == 1, eng.lib.calls
  name, args = eng.lib.calls.pop()
  assert name == fn and args[0] is eng._h and len(args) == 1 + len(ORDER[fn])
  return dict(zip(ORDER[fn], args[1:]))


def _shape(a):
  return None if a is None else a.shape


def _inputs(sets, rng):
  lead = (E, R) if sets else (B,)
  return lead, rng.standard_normal(lead + (N,)), rng.standard_normal(lead + (M,))


@pytest.mark.parametrize("method", list(GRADS))
def test_exgd_grad_host_forms(engine, method):
  fn, node, sets = GRADS[method]
  eng = engine(4804 if node else 4)
  rng = np.random.default_rng(0)
  lead, z, lam = _inputs(sets, rng)
  sizes = dict(E=E, R=R) if sets else dict(B=B)
  if sets:
    forms = [(rng.standard_normal((E, eng.np)), (E, eng.np), None)]
  elif node:
    forms = [(rng.standard_normal(eng.np), (eng.np,), None)]
  else:
    forms = [(None, None, 0), (np.ones(eng.np), (eng.np,), 0), (np.ones((B, eng.np)), (B, eng.np), eng.np)]
  for p, pshape, ps in forms:
    for reduce in (False, True):
      for want_start in (True, False):
        for seed_lam in (None, np.ones(M)):      # lb, ub and the seeds broadcast to the batch
          kw = dict(seed_lam=seed_lam, reduce=reduce, want_start=want_start)
          if node:
            out = getattr(eng, method)(z, lam, -np.ones(N), 2.0, 0.25, 0.5, 7, np.ones(N), p, **kw)
          else:
            out = getattr(eng, method)(z, lam, -np.ones(N), 2.0, 0.25, 0.5, 7, np.ones(N), params=p, **kw)
          a = _last(eng, fn)
          assert {k: a[k] for k in sizes} == sizes
          assert (a["eta_x"], a["eta_v"], a["nsteps"], a["grad_stride"], a["mem"]) == (0.25, 0.5, 7, 0 if reduce else eng.np, HOST)
          assert isinstance(a["eta_x"], float) and isinstance(a["nsteps"], int)
          if not node:
            assert a["stride"] == ps
          assert _shape(a["params"]) == pshape
          for k, w in (("z", N), ("lam", M), ("lb", N), ("ub", N), ("seed_z", N)):
            assert a[k].shape == lead + (w,) and a[k].flags.c_contiguous and a[k].dtype == np.float64, k
          assert (a["lb"] == -1.0).all() and (a["ub"] == 2.0).all()
          assert _shape(a["seed_lam"]) == (None if seed_lam is None else lead + (M,))
          gshape = (lead[:-1] if reduce else lead) + (eng.np,)
          assert a["grad"].shape == gshape
          assert _shape(a["dz0"]) == (lead + (N,) if want_start else None) and _shape(a["dlam0"]) == (lead + (M,) if want_start else None)
          assert set(out) == ({"grad", "dz0", "dlam0"} if want_start else {"grad"})
          assert out["grad"] is a["grad"]
          if want_start:
            assert out["dz0"] is a["dz0"] and out["dlam0"] is a["dlam0"]


@pytest.mark.parametrize("method", list(HVPS))
def test_hvp_host_forms(engine, method):
  fn, node, sets = HVPS[method]
  eng = engine(4804 if node else 4)
  rng = np.random.default_rng(1)
  lead, z, lam = _inputs(sets, rng)
  v = rng.standard_normal(z.shape)
  sizes = dict(E=E, R=R) if sets else dict(B=B)
  if sets:
    forms = [(rng.standard_normal((E, eng.np)), (E, eng.np), None)]
  elif node:
    forms = [(rng.standard_normal(eng.np), (eng.np,), None)]
  else:
    forms = [(None, None, 0), (np.ones(eng.np), (eng.np,), 0), (np.ones((B, eng.np)), (B, eng.np), eng.np)]
  for p, pshape, ps in forms:
    for lam_ in (lam, None):
      for with_cost in (True, False):
        for want_z in (True, False):
          for want_p in (True, False):
            for reduce in (False, True):
              out = getattr(eng, method)(z, lam_, v, p, with_cost=with_cost, want_z=want_z, want_p=want_p, reduce=reduce)
              a = _last(eng, fn)
              assert {k: a[k] for k in sizes} == sizes
              assert (a["with_cost"], a["p_stride"], a["mem"]) == (int(with_cost), 0 if reduce else eng.np, HOST)
              if not node:
                assert a["stride"] == ps
              assert _shape(a["params"]) == pshape
              assert a["z"].shape == lead + (N,) and a["v"].shape == lead + (N,) and _shape(a["lam"]) == (None if lam_ is None else lead + (M,))
              assert _shape(a["out_z"]) == (lead + (N,) if want_z else None)
              assert _shape(a["out_p"]) == (((lead[:-1] if reduce else lead) + (eng.np,)) if want_p else None)
              assert set(out) == ({"hz"} if want_z else set()) | ({"hp"} if want_p else set())
              assert out.get("hz") is a["out_z"] and out.get("hp") is a["out_p"]


def test_a_single_instance_is_a_batch_of_one(engine):
  eng = engine(4)
  out = eng.exgd_grad(np.zeros(N), np.zeros(M), -1.0, 1.0, 0.1, 0.1, 1, np.ones(N))
  a = _last(eng, "myr_exgd_grad")
  assert a["B"] == 1 and a["z"].shape == (1, N) and a["lb"].shape == (1, N) and out["grad"].shape == (1, 4)
  out = eng.hvp(np.zeros(N), np.zeros(M), np.ones(N), want_p=True, reduce=True)
  a = _last(eng, "myr_hvp")
  assert a["B"] == 1 and a["lam"].shape == (1, M) and out["hp"].shape == (4,)


def test_value_errors(engine):
  cf, net = engine(4), engine(4804)
  z, lam, v = np.zeros((B, N)), np.zeros((B, M)), np.zeros((B, N))
  z3, lam3, w = np.zeros((E, R, N)), np.zeros((E, R, M)), np.zeros((E, 4804))
  g = (-1.0, 1.0, 0.1, 0.1, 1, np.ones(N))      # lb, ub, eta_x, eta_v, nsteps, seed_z
  for method in ("exgd_grad", "exgd_grad_shoot"):
    f = getattr(cf, method)
    with pytest.raises(ValueError, match="params must have np entries"):
      f(z, lam, *g, params=np.ones(5))
    with pytest.raises(ValueError, match=r"params must be \[B,4\]"):
      f(z, lam, *g, params=np.ones((2, 4)))
    with pytest.raises(ValueError, match="z and lam must have the same batch size"):
      f(z, lam[:2], *g)
    with pytest.raises(ValueError, match=r"z must be \[B,35\]"):
      f(z[:, :30], lam, *g)
    with pytest.raises(ValueError, match=r"lam must be \[B,24\]"):
      f(z, lam[:, :20], *g)
  for method in ("exgd_grad_node", "exgd_grad_node_shoot"):
    f = getattr(net, method)
    with pytest.raises(ValueError, match="params must be the 4804 shared weights"):
      f(z, lam, *g, np.ones(7))
    with pytest.raises(ValueError, match="params must be the 4804 shared weights"):
      f(z, lam, *g, np.ones((B, 4804)))
    with pytest.raises(ValueError, match="z and lam must have the same batch size"):
      f(z, lam[:2], *g, np.ones(4804))
  with pytest.raises(ValueError, match=r"params must be \[E,4804\]: a weight set per row"):
    net.exgd_grad_node_sets(z3, lam3, *g, np.ones(4804))
  with pytest.raises(ValueError, match=r"z must be \[E = 2, R, 35\] with R >= 1"):
    net.exgd_grad_node_sets(np.zeros((3, R, N)), lam3, *g, w)
  with pytest.raises(ValueError, match=r"lam must be \[E = 2, R = 2, 24\]"):
    net.exgd_grad_node_sets(z3, np.zeros((E, 3, M)), *g, w)
  with pytest.raises(ValueError, match="params must have np entries"):
    cf.hvp(z, lam, v, params=np.ones(5))
  with pytest.raises(ValueError, match=r"params must be \[B,4\]"):
    cf.hvp(z, lam, v, params=np.ones((2, 4)))
  with pytest.raises(ValueError, match="params must be the 4804 shared weights"):
    net.hvp_node(z, lam, v, np.ones(7))
  for f, p in ((cf.hvp, None), (net.hvp_node, np.ones(4804))):
    with pytest.raises(ValueError, match="z, lam and v must have the same batch size"):
      f(z, lam, v[:2], p)
    with pytest.raises(ValueError, match="z, lam and v must have the same batch size"):
      f(z, lam[:2], v, p)
  with pytest.raises(ValueError, match=r"params must be \[E,4804\]: a weight set per row"):
    net.hvp_node_sets(z3, lam3, z3, np.ones(4804))
  with pytest.raises(ValueError, match=r"z must be \[E = 2, R, 35\] with R >= 1"):
    net.hvp_node_sets(np.zeros((E, 0, N)), lam3, z3, w)
  with pytest.raises(ValueError, match=r"v must be \[E = 2, R = 2, 35\]"):
    net.hvp_node_sets(z3, lam3, np.zeros((E, 3, N)), w)
  with pytest.raises(ValueError, match=r"lam must be \[E = 2, R = 2, 24\]"):
    net.hvp_node_sets(z3, np.zeros((E, R, 20)), z3, w)
  assert not cf.lib.calls and not net.lib.calls      # nothing reached the library


def test_device_forms_hand_their_arguments_through(engine):
  """every array is whatever the caller gave (a device tensor), every size an int, MYR_MEM_DEVICE last"""
  eng = engine(4804)
  t = {k: object() for k in ("z", "lam", "lb", "ub", "v", "seed_z", "seed_lam", "grad", "dz0", "dlam0", "params", "out_z", "out_p")}
  for method, fn, lead in (("exgd_grad_device", "myr_exgd_grad", (5,)), ("exgd_grad_shoot_device", "myr_exgd_grad_shoot", (5,)),
                           ("exgd_grad_node_device", "myr_exgd_grad_node", (5,)), ("exgd_grad_node_shoot_device", "myr_exgd_grad_node_shoot", (5,)),
                           ("exgd_grad_node_sets_device", "myr_exgd_grad_node_sets", (E, R))):
    head = lead + (t["z"], t["lam"], t["lb"], t["ub"], 0.25, 0.5, np.int64(7), t["seed_z"], t["grad"], np.int64(4804))
    closed = "node" not in method
    # the optional arrays: absent, then present (closed form: params and its stride by keyword; the network: params positional)
    if closed:
      getattr(eng, method)(*head)
      a = _last(eng, fn)
      assert a["params"] is None and a["stride"] == 0
      getattr(eng, method)(*head, seed_lam=t["seed_lam"], params=t["params"], params_stride=4804, dz0=t["dz0"], dlam0=t["dlam0"])
      full = _last(eng, fn)
      assert full["stride"] == 4804
    else:
      getattr(eng, method)(*head, t["params"])
      a = _last(eng, fn)
      getattr(eng, method)(*head, t["params"], seed_lam=t["seed_lam"], dz0=t["dz0"], dlam0=t["dlam0"])
      full = _last(eng, fn)
      assert a["params"] is t["params"]
    assert full["params"] is t["params"]
    for c, present in ((a, False), (full, True)):
      assert tuple(c[k] for k in (("E", "R") if len(lead) == 2 else ("B",))) == lead
      assert all(c[k] is t[k] for k in ("z", "lam", "lb", "ub", "seed_z", "grad"))
      assert (c["eta_x"], c["eta_v"], c["nsteps"], c["grad_stride"], c["mem"]) == (0.25, 0.5, 7, 4804, DEVICE)
      assert type(c["nsteps"]) is int and type(c["grad_stride"]) is int
      for k in ("seed_lam", "dz0", "dlam0"):
        assert c[k] is (t[k] if present else None)
  for method, fn, lead in (("hvp_device", "myr_hvp", (5,)), ("hvp_node_device", "myr_hvp_node", (5,)), ("hvp_node_sets_device", "myr_hvp_node_sets", (E, R))):
    head = lead + (t["z"], t["lam"], t["v"])
    if method == "hvp_device":
      eng.hvp_device(*head)
      a = _last(eng, fn)
      assert a["params"] is None and a["stride"] == 0
      eng.hvp_device(*head, out_z=t["out_z"], out_p=t["out_p"], p_stride=np.int64(4804), params=t["params"], params_stride=4804, with_cost=False)
      full = _last(eng, fn)
      assert full["stride"] == 4804
    else:
      getattr(eng, method)(*head, t["params"])
      a = _last(eng, fn)
      getattr(eng, method)(*head, t["params"], out_z=t["out_z"], out_p=t["out_p"], p_stride=np.int64(4804), with_cost=False)
      full = _last(eng, fn)
      assert a["params"] is t["params"]
    assert full["params"] is t["params"]
    for c, present in ((a, False), (full, True)):
      assert tuple(c[k] for k in (("E", "R") if len(lead) == 2 else ("B",))) == lead
      assert c["z"] is t["z"] and c["lam"] is t["lam"] and c["v"] is t["v"]
      assert (c["with_cost"], c["p_stride"], c["mem"]) == ((0, 4804, DEVICE) if present else (1, 0, DEVICE))
      assert type(c["p_stride"]) is int
      assert c["out_z"] is (t["out_z"] if present else None) and c["out_p"] is (t["out_p"] if present else None)


def _fit_checks(a, out, gn, stride_key, reduce, lead, want_grad=True):
  """what the four host forms share: scalar types, the arrays made for the results and the dict that comes back"""
  assert (a["num_steps"], a["u_rows"], a[stride_key], a["mem"]) == (S, U, 0 if reduce else NP, HOST)
  assert all(type(a[k]) is int for k in ("num_steps", "u_rows", stride_key))
  for k in ("xs_obs", "us"):
    assert a[k].flags.c_contiguous and a[k].dtype == np.float64, k
  rows = lead[:-1] if reduce else lead
  assert a["loss"].shape == lead and _shape(a["grad"]) == (rows + (NP,) if want_grad else None)
  assert set(out) == {"loss"} | ({"grad"} if want_grad else set()) | ({"gn"} if gn else set())
  assert out["loss"] is a["loss"] and out.get("grad") is a["grad"]
  if gn:
    assert a["gn"].shape == rows + (NP, NP) and out["gn"] is a["gn"]


@pytest.mark.parametrize("method", ["fit_grad", "fit_gn"])
def test_fit_single_set_host_forms(engine, method):
  fn, _, gn = FITS[method]
  eng = engine(NP)
  rng = np.random.default_rng(2)
  stride_key = "out_stride" if gn else "grad_stride"
  xs_obs, us = rng.standard_normal((B, S + 1, NS)), rng.standard_normal((B, U, NU))
  for p, pshape, ps in ((None, None, 0), (np.ones(NP), (NP,), 0), (np.ones((B, NP)), (B, NP), NP)):
    for wt in (None, np.linspace(0.5, 1.5, S + 1)):
      for reduce in (False, True):
        out = getattr(eng, method)(xs_obs, us, p, wt=wt, reduce=reduce)
        a = _last(eng, fn)
        assert a["B"] == B and a["stride"] == ps and _shape(a["params"]) == pshape and _shape(a["wt"]) == (None if wt is None else (S + 1,))
        assert a["xs_obs"].shape == (B, S + 1, NS) and a["us"].shape == (B, U, NU)
        assert np.array_equal(a["xs_obs"], xs_obs) and np.array_equal(a["us"], us)
        _fit_checks(a, out, gn, stride_key, reduce, (B,))
  # one trajectory [S+1,ns], [u_rows,nu] is a batch of one; either array may come alone in that form; anything array-like is taken as float64
  for x, u in ((xs_obs[0], us[0]), (xs_obs[:1], us[0]), (xs_obs[0].astype(np.float32), us[0].tolist())):
    for reduce in (False, True):
      out = getattr(eng, method)(x, u, reduce=reduce)
      a = _last(eng, fn)
      assert a["B"] == 1 and a["xs_obs"].shape == (1, S + 1, NS) and a["us"].shape == (1, U, NU) and a["params"] is None and a["stride"] == 0
      _fit_checks(a, out, gn, stride_key, reduce, (1,))


@pytest.mark.parametrize("method", ["fit_grad_sets", "fit_gn_sets"])
def test_fit_sets_host_forms(engine, method):
  fn, _, gn = FITS[method]
  eng = engine(NP)
  rng = np.random.default_rng(3)
  stride_key = "out_stride" if gn else "grad_stride"
  params = rng.standard_normal((E, NP))
  for shared in (False, True):
    dlead = (R,) if shared else (E, R)
    xs_obs, us = rng.standard_normal(dlead + (S + 1, NS)), rng.standard_normal(dlead + (U, NU))
    for wt in (None, np.linspace(0.5, 1.5, S + 1)):
      for reduce in (False, True):
        for want_grad in ((True,) if gn else (True, False)):      # (fit_gn_sets always forms the gradient)
          kw = {} if gn else dict(want_grad=want_grad)
          out = getattr(eng, method)(xs_obs, us, params, wt=wt, reduce=reduce, **kw)
          a = _last(eng, fn)
          assert (a["E"], a["R"], a["data_shared"]) == (E, R, int(shared)) and type(a["data_shared"]) is int
          assert a["params"].shape == (E, NP) and _shape(a["wt"]) == (None if wt is None else (S + 1,))
          assert a["xs_obs"].shape == dlead + (S + 1, NS) and a["us"].shape == dlead + (U, NU)
          _fit_checks(a, out, gn, stride_key, reduce, (E, R), want_grad)


def test_fit_value_errors(engine):
  eng = engine(NP)
  m = lambda text: re.escape(text)
  xs_obs, us = np.zeros((B, S + 1, NS)), np.zeros((B, U, NU))
  for f in (eng.fit_grad, eng.fit_gn):
    for bad in (np.zeros((B, S + 1, NS + 1)), np.zeros((B, 1, NS)), np.zeros((1, B, S + 1, NS))):
      with pytest.raises(ValueError, match=m("xs_obs must be [B,S+1,4] with S >= 1")):
        f(bad, us)
    for bad in (np.zeros((B - 1, U, NU)), np.zeros((B, U, NU + 1)), np.zeros((1, B, U, NU))):
      with pytest.raises(ValueError, match=m("us must be [B,u_rows,1]")):
        f(xs_obs, bad)
    with pytest.raises(ValueError, match="params must have np entries"):
      f(xs_obs, us, np.ones(NP + 1))
    with pytest.raises(ValueError, match=m("params must be [B,4]")):
      f(xs_obs, us, np.ones((B - 1, NP)))
    with pytest.raises(ValueError, match=m("expected shape (5,), got (4,)")):
      f(xs_obs, us, wt=np.ones(S))
  p = np.ones((E, NP))
  xs4, us4, xs3, us3 = np.zeros((E, R, S + 1, NS)), np.zeros((E, R, U, NU)), np.zeros((R, S + 1, NS)), np.zeros((R, U, NU))
  both = "xs_obs and us must both be [E,R,...] (data per set) or both [R,...] (data shared by the sets)"
  for f in (eng.fit_grad_sets, eng.fit_gn_sets):
    for bad in (np.ones(NP), np.ones((E, NP + 1)), np.ones((1, E, NP))):
      with pytest.raises(ValueError, match=m("params must be [E,4]")):
        f(xs4, us4, bad)
    for x, u in ((xs4, us3), (xs3, us4), (xs3[0], us3[0]), (xs4[None], us4[None])):
      with pytest.raises(ValueError, match=m(both)):
        f(x, u, p)
    for bad in (np.zeros((E + 1, R, S + 1, NS)), np.zeros((E, R, S + 1, NS + 1)), np.zeros((E, R, 1, NS)), np.zeros((E, 0, S + 1, NS))):
      with pytest.raises(ValueError, match=m("xs_obs must be [E,R,S+1,4] with R >= 1, S >= 1 and E = 2 as in params")):
        f(bad, us4, p)
    for bad in (np.zeros((R, S + 1, NS + 1)), np.zeros((R, 1, NS)), np.zeros((0, S + 1, NS))):
      with pytest.raises(ValueError, match=m("xs_obs must be [R,S+1,4] with R >= 1, S >= 1 and E = 2 as in params")):
        f(bad, us3, p)
    for bad in (np.zeros((E, R + 1, U, NU)), np.zeros((E + 1, R, U, NU)), np.zeros((E, R, U, NU + 1)), np.zeros((E, R, 0, NU))):
      with pytest.raises(ValueError, match=m("us must be [E,R,u_rows,1]")):
        f(xs4, bad, p)
    for bad in (np.zeros((R + 1, U, NU)), np.zeros((R, U, NU + 1)), np.zeros((R, 0, NU))):
      with pytest.raises(ValueError, match=m("us must be [R,u_rows,1]")):
        f(xs3, bad, p)
    with pytest.raises(ValueError, match=m("expected shape (5,), got (6,)")):
      f(xs4, us4, p, wt=np.ones(S + 2))
  assert not eng.lib.calls      # nothing reached the library


def test_fit_device_forms_hand_their_arguments_through(engine):
  """every array is whatever the caller gave (a device tensor), every size an int, MYR_MEM_DEVICE last; the optional arrays absent, then present"""
  eng = engine(NP)
  t = {k: object() for k in ("xs_obs", "us", "wt", "params", "loss", "grad", "gn")}
  i = np.int64
  for method, (fn, sets, gn) in FITS.items():
    lead = (i(E), i(R)) if sets else (i(5),)
    head = lead + (i(S), i(U), t["xs_obs"], t["us"])
    stride_key = "out_stride" if gn else "grad_stride"
    f = getattr(eng, method + "_device")
    if not sets:
      f(*head, t["gn"] if gn else t["grad"], i(NP))
      a = _last(eng, fn)
      f(*head, t["gn"] if gn else t["grad"], i(0), params=t["params"], params_stride=i(NP), wt=t["wt"], loss=t["loss"], **(dict(grad=t["grad"]) if gn else {}))
      full = _last(eng, fn)
      assert (a["stride"], full["stride"]) == (0, NP) and type(full["stride"]) is int
      assert (a[stride_key], full[stride_key]) == (NP, 0)
      absent = ("wt", "params", "loss") + (("grad",) if gn else ())
    else:
      f(*head, t["params"], *((t["gn"],) if gn else ()))
      a = _last(eng, fn)
      if gn:
        f(*head, t["params"], t["gn"], out_stride=i(NP), data_shared=True, wt=t["wt"], loss=t["loss"], grad=t["grad"])
      else:
        f(*head, t["params"], grad=t["grad"], grad_stride=i(NP), data_shared=True, wt=t["wt"], loss=t["loss"])
      full = _last(eng, fn)
      assert (a["data_shared"], full["data_shared"]) == (0, 1) and type(full["data_shared"]) is int
      assert (a[stride_key], full[stride_key]) == (0, NP)
      absent = ("wt", "loss", "grad")
    for c, present in ((a, False), (full, True)):
      assert tuple(c[k] for k in (("E", "R") if sets else ("B",))) == tuple(int(v) for v in lead)
      assert (c["num_steps"], c["u_rows"], c["mem"]) == (S, U, DEVICE)
      assert all(type(c[k]) is int for k in (("E", "R") if sets else ("B",)) + ("num_steps", "u_rows", stride_key))
      assert c["xs_obs"] is t["xs_obs"] and c["us"] is t["us"]
      for k in t:
        if k in c and k not in ("xs_obs", "us"):
          assert c[k] is (None if k in absent and not present else t[k]), (method, k)


def test_probes_make_the_empty_call(engine):
  """no instances, the required arrays present, the optional ones null, host memory: the library's checks run and nothing else"""
  eng = engine(4804)
  for method, fn in (("exgd_grad_probe", "myr_exgd_grad"), ("exgd_grad_shoot_probe", "myr_exgd_grad_shoot"), ("exgd_grad_node_probe", "myr_exgd_grad_node"),
                     ("exgd_grad_node_shoot_probe", "myr_exgd_grad_node_shoot"), ("exgd_grad_node_sets_probe", "myr_exgd_grad_node_sets")):
    getattr(eng, method)()
    a = _last(eng, fn)
    assert (a["E"], a["R"]) == (0, 1) if "sets" in fn else a["B"] == 0
    assert all(isinstance(a[k], np.ndarray) for k in ("z", "lam", "lb", "ub", "seed_z", "grad"))
    assert all(a[k] is None for k in ("seed_lam", "dz0", "dlam0"))
    assert (a["eta_x"], a["eta_v"], a["nsteps"], a["grad_stride"], a["mem"]) == (0.0, 0.0, 0, 0, HOST)
    if "node" in fn:
      assert isinstance(a["params"], np.ndarray)      # the network calls refuse null weights
    else:
      assert a["params"] is None and a["stride"] == 0
  for method, fn in (("hvp_node_probe", "myr_hvp_node"), ("hvp_node_sets_probe", "myr_hvp_node_sets")):
    getattr(eng, method)()
    a = _last(eng, fn)
    assert (a["E"], a["R"]) == (0, 1) if "sets" in fn else a["B"] == 0
    assert all(isinstance(a[k], np.ndarray) for k in ("z", "v", "params", "out_z"))
    assert a["lam"] is None and a["out_p"] is None
    assert (a["with_cost"], a["p_stride"], a["mem"]) == (1, 0, HOST)


def test_the_signature_table_covers_the_exports():
  """every exported function has its signature declared from the table load() reads"""
  table = _lib._SIGNATURES
  assert set(table) == set(_lib.EXPORTS) and list(table) == _lib.EXPORTS
  for fn, names in ORDER.items():
    assert len(table[fn][0]) == 1 + len(names), fn
