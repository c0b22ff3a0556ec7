"""The references of test_gpu_products_matrix.py checked on themselves, without a device (tests/products_cases.py): every case of the matrix
exists, is finite, clips enough and answers one bit of its input with less than a tenth of the ceiling; the autograd of the Lagrangian agrees with the oracle's dense Jacobian; neither term of grad L drowns the
other; and the TIMBERHARVEST case with r = 0.3 really discounts."""
import numpy as np
import pytest

import products_cases as P

DENSE_TOL = 1e-12        # J^T lam and J v from the dense Jacobian against the autograd of the Lagrangian, of the row's largest entry
VISIBLE = 1e-3           # max|jt| and max|grad f| against max|gl|
# Cases in which one term of grad L is below VISIBLE of the other, by construction of the system and not of the draw, each with its reason.  The
# comparison of gl still sees the smaller term -- 1e-5 of max|gl| stands eight digits above the 1e-11 it is held to --, and jt and jv are compared
# on their own.
#   TUMOUR under Hermite-Simpson   grad f = 0: the running cost is zero (tumour.py:100-101), the cost is terminal, and the Hermite-Simpson objective
#                                  takes no terminal cost (hermite_simpson.py:243-257; the trapezoidal and the shooting objectives do)
#   GLUCOSE                        the cost carries a factor of 100 000 (glucose.py:103-104): max|jt| = 1.5e-5 ... 3.2e-5 of max|gl| at lam = 0.1 N(0, 1)
#   BEARPOPULATIONS                c_p = 10 000 weighs the park population (bear_populations.py:109-110): max|jt| = 5e-4 ... 1.7e-3 of max|gl|
NO_COST_GRADIENT = {("TUMOUR", "HERMITE_SIMPSON")}
COST_SCALED_ABOVE_THE_CONSTRAINTS = {"GLUCOSE": 1e-5, "BEARPOPULATIONS": 4e-4}      # name -> what max|jt| / max|gl| must still reach
EPS = 2.0 ** -52

PARITY = P.parity_cases()


@pytest.mark.parametrize("thunk", [t for _, t in PARITY], ids=[i for i, _ in PARITY])
def test_parity_case(thunk):
  c = thunk()
  ref = P.forward_reference(c)
  B = c["z"].shape[0]
  assert ref["gl"].shape == (B, c["n"]) and ref["jv"].shape == (B, c["m"]) and ref["z_n"].shape == (B, c["n"]) and ref["lam_n"].shape == (B, c["m"])
  for k, a in ref.items():
    assert np.isfinite(a).all(), k
    assert not a.flags.writeable
  assert c["clipped"] >= P.MIN_CLIPPED, c["clipped"]
  assert c["response"] <= P.MAX_RESPONSE, c["response"]
  assert c["params"].shape[0] == B and (c["params"][0] != c["params"][1]).any()      # a parameter row per instance
  for b in range(B):
    jt, jv = P.dense_products(c, b)
    assert np.abs(jt - ref["jt"][b]).max() <= DENSE_TOL * np.abs(ref["jt"][b]).max(), b
    assert np.abs(jv - ref["jv"][b]).max() <= DENSE_TOL * np.abs(ref["jv"][b]).max(), b
    top = np.abs(ref["gl"][b]).max()
    # jt is gl - gf: the two autograd forms differ by the rounding of the subtraction
    assert np.abs(ref["gl"][b] - ref["gf"][b] - ref["jt"][b]).max() <= 8.0 * EPS * top, b
    assert np.abs(ref["jt"][b]).max() >= COST_SCALED_ABOVE_THE_CONSTRAINTS.get(c["name"], VISIBLE) * top, b
    if (c["name"], c["tr"]) in NO_COST_GRADIENT:
      assert (ref["gf"][b] == 0.0).all()
    else:
      assert np.abs(ref["gf"][b]).max() >= VISIBLE * top, b
  # the steps moved both iterates
  assert np.abs(ref["z_n"] - c["z"]).max() > 0 and np.abs(ref["lam_n"] - c["lam"]).max() > 0


def test_the_matrix_is_the_one_the_issue_names():
  import test_gpu_hvp
  assert P.SHOOT_EXTRA_SYSTEMS == test_gpu_hvp.PARITY
  assert len(P.SYSTEMS) == 20
  ids = [i for i, _ in PARITY]
  assert len(ids) == len(set(ids)) == 20 * 2 + 2 + 20 * 3 + 8 * 2 + 1


@pytest.mark.parametrize("which", ["HERMITE_SIMPSON", "TRAPEZOIDAL", "SHOOTING"])
def test_timberharvest_case_discounts(which):
  if which == "SHOOTING":
    plain, disc = P.shoot_case("TIMBERHARVEST", *P.DISCOUNT_SHOOT), P.shoot_case("TIMBERHARVEST", *P.DISCOUNT_SHOOT, discounted=True)
  else:
    plain, disc = P.colloc_case("TIMBERHARVEST", which), P.colloc_case("TIMBERHARVEST", which, discounted=True)
  r = P.O.SYSTEMS["TIMBERHARVEST"].param_names.index("r")
  assert (disc["params"][:, r] == P.DISCOUNT_R).all() and (np.abs(plain["params"][:, r]) == 0.0).all()
  keep = [k for k in range(plain["params"].shape[1]) if k != r]
  assert (disc["params"][:, keep] == plain["params"][:, keep]).all()
  for k in ("z", "lam", "v", "lb", "ub"):
    assert (disc[k] == plain[k]).all()
  a, b = P.forward_reference(plain)["gl"], P.forward_reference(disc)["gl"]
  assert (np.abs(a - b).max(axis=1) > 1e-3 * np.abs(a).max(axis=1)).all()
  assert disc["clipped"] >= P.MIN_CLIPPED


def test_node_case():
  c = P.node_case()
  ref = P.forward_reference(c)
  assert c["clipped"] >= P.MIN_CLIPPED and c["response"] <= P.MAX_RESPONSE and all(np.isfinite(a).all() for a in ref.values())
  for b in range(c["z"].shape[0]):
    jt, jv = P.dense_products(c, b)
    assert np.abs(jt - ref["jt"][b]).max() <= DENSE_TOL * np.abs(ref["jt"][b]).max()
    assert np.abs(jv - ref["jv"][b]).max() <= DENSE_TOL * np.abs(ref["jv"][b]).max()
    assert min(np.abs(ref["jt"][b]).max(), np.abs(ref["gf"][b]).max()) >= VISIBLE * np.abs(ref["gl"][b]).max()


def _check_rows(c, ref, dense=True):
  for k, a in ref.items():
    assert np.isfinite(a).all(), k
  if dense:
    for i, b in enumerate(c["rows"]):
      jt, jv = P.dense_products(c, b)
      assert np.abs(jt - ref["jt"][i]).max() <= DENSE_TOL * np.abs(ref["jt"][i]).max(), b
      assert np.abs(jv - ref["jv"][i]).max() <= DENSE_TOL * np.abs(ref["jv"][i]).max(), b


@pytest.mark.parametrize("N", P.PRODUCT_SHAPE_N)
@pytest.mark.parametrize("scheme", P.SCHEMES)
def test_product_shape_case(scheme, N):
  c, ref = P.product_shape(scheme, N)
  assert c["z"].shape[0] == max(P.PRODUCT_SHAPE_B) and c["rows"] == (0, 62, 64, 256)
  _check_rows(c, ref)


@pytest.mark.parametrize("scheme,N", P.EXGD_SHAPES)
def test_exgd_shape_case(scheme, N):
  c, refs = P.exgd_shape("CARTPOLE", scheme, N, max(P.EXGD_SHAPE_B), P.EXGD_SHAPE_STEPS)
  assert c["rows"] == (0, 129) and c["clipped"] >= P.MIN_CLIPPED and c["response"] <= P.MAX_RESPONSE and set(refs) == set(P.EXGD_SHAPE_STEPS)
  for ref in refs.values():
    _check_rows(c, ref, dense=False)
  assert np.abs(refs[10]["z_n"] - refs[1]["z_n"]).max() > 0


@pytest.mark.parametrize("name,scheme,N,B", P.EXGD_WIDE)
def test_exgd_wide_case(name, scheme, N, B):
  c, refs = P.exgd_shape(name, scheme, N, B, P.EXGD_SHAPE_STEPS)
  assert c["rows"] == (0, B - 1) and c["clipped"] >= P.MIN_CLIPPED
  if (name, scheme, N, B) != P.ILL_CONDITIONED:      # (products_cases.py: no draw of that case is well conditioned over ten steps; after one step it is)
    assert c["response"] <= P.MAX_RESPONSE
  assert P.response(c, refs[1], list(c["rows"]), 1) <= P.MAX_RESPONSE
  for ref in refs.values():
    _check_rows(c, ref, dense=False)


def test_capacity_case():
  c, refs = P.exgd_shape("CARTPOLE", "HERMITE_SIMPSON", P.CAPACITY_N, 2, (2,))
  assert c["clipped"] >= P.MIN_CLIPPED and c["response"] <= P.MAX_RESPONSE and np.isfinite(refs[2]["z_n"]).all() and np.isfinite(refs[2]["lam_n"]).all()
  # 2 n + m + K NS doubles + 16 bytes (colloc_exgd_lds_bytes): 288 N + 128 for CARTPOLE Hermite-Simpson
  def lds(N):
    K, n, m = P.E.dims("CARTPOLE", "HERMITE_SIMPSON", N)
    return (2 * n + m + K * c["ns"]) * 8 + 16
  assert lds(P.CAPACITY_N) == 288 * P.CAPACITY_N + 128 == 163712 <= 160 * 1024 < lds(P.CAPACITY_N + 1)


@pytest.mark.parametrize("name,I,cpi,method", P.SHOOT_SHAPE_CASES)
def test_shoot_shape_case(name, I, cpi, method):
  c, ref, refs = P.shoot_shape(name, I, cpi, method)
  assert c["rows"] == (0, 62, 64, 129) and c["clipped"] >= P.MIN_CLIPPED and c["response"] <= P.MAX_RESPONSE and set(refs) == set(P.SHOOT_SHAPE_STEPS)
  _check_rows(c, ref)
  for r in refs.values():
    _check_rows(c, r, dense=False)
