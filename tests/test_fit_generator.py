"""The generated parameter derivatives (myriad_amd/csrc/systems_dp_gen.h) are what tools/gen_systems.py --dp writes today, and the
header every solver kernel includes (systems_gen.h) is the one from before that generator option existed, byte for byte.  The generator needs
sympy, as tools/gen_systems.py always has: without it these tests fail, they do not skip."""
import hashlib
import importlib.util
import os


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "myriad_amd", "csrc")


def _generator():
  spec = importlib.util.spec_from_file_location("gen_systems", os.path.join(ROOT, "tools", "gen_systems.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_dp_header_is_reproduced_byte_for_byte(tmp_path):
  gen = _generator()
  gen.OUT_DP = str(tmp_path / "systems_dp_gen.h")
  gen.OUT = str(tmp_path / "systems_gen.h")          # (never written by --dp; kept away from the tree all the same)
  gen.main_dp()
  assert not os.path.exists(gen.OUT)
  with open(gen.OUT_DP, "rb") as a, open(os.path.join(CSRC, "systems_dp_gen.h"), "rb") as b:
    assert a.read() == b.read()


def test_dp_header_covers_the_twenty_systems_and_no_twin():
  txt = open(os.path.join(CSRC, "systems_dp_gen.h")).read()
  gen = _generator()
  names = [S["name"] for S in gen.systems()]
  for n in names:
    assert (f"struct SysDp<Sys{n}>" in txt) == (not n.endswith("_ELASTIC")), n
  assert sum(not n.endswith("_ELASTIC") for n in names) == 20
  assert "INVASIVEPLANT" not in txt


# sha256 of myriad_amd/csrc/systems_gen.h as committed in front of the change that added systems_dp_gen.h (`git show <parent>:myriad_amd/csrc/systems_gen.h`)
SYSTEMS_GEN_SHA256 = "a8f23274acd01a9e2fdadb6c5a20996e32eeb483aca4b1f7c78caa860c3ccfe8"


def test_systems_gen_h_did_not_move():
  """Every solver kernel includes systems_gen.h, and re-running sympy's CSE may reorder its code and with it the solvers' bits: adding the parameter
  derivatives left the file as it was.  The hash is pinned here, so the check needs no git history and never skips; a change that regenerates
  systems_gen.h on purpose (a new system) updates the constant in the same commit, where a reviewer sees it."""
  with open(os.path.join(CSRC, "systems_gen.h"), "rb") as f:
    assert hashlib.sha256(f.read()).hexdigest() == SYSTEMS_GEN_SHA256
