"""Stage (myriad_amd/csrc/host_stage.h: the staging of a C-ABI call's arrays in one growing device buffer) under AddressSanitizer +
UndefinedBehaviorSanitizer, as a program of its own on a malloc / memcpy backend (tests/hostsim/stage_check.cpp): the registration lists of
myr_eval, myr_solve, myr_solve_x0 and of the restoration working set at odd sizes -- alignment, disjoint carves inside the buffer, the size
bound, uploads and downloads of exactly the registered counts in registration order, what a device caller gets, null / empty arrays, and one
growth per larger call."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_stage_layout_and_copies_are_clean_under_asan_ubsan(tmp_path):
  exe = str(tmp_path / "stage_check")
  # (the sanitizer runtimes are linked statically: the program then runs whatever else the environment loads into a process)
  subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                  "-static-libasan", "-static-libubsan", os.path.join(HERE, "hostsim", "stage_check.cpp"), "-o", exe], check=True)
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
  r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
  assert "stage_check: ok" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
