"""The splat frame calls' host-only policy (csrc/splat_run.h), checked without a GPU: what an overlapped call's
front end waits for, the ring depth from PTGS_GS_OV_DEPTH, and which report of earlier frames a call returns.
tests/native/splat_run_check.cpp is a stand-alone program (its own main, ASan + UBSan linked in) that
enumerates every sequence of 9 calls over 5 kinds of call at each ring depth against a reference model with
an unbounded history, the 32 cases of the report latch against ptgs.h's table, and 9 depth strings.
With the sanitizers the whole enumeration runs in about 0.6 s, so nothing is shortened."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}

# 3 ring depths x (5 + 5^2 + .. + 5^9) steps of the depth-first walk, 32 latch cases, 9 depth strings
CASES = 3 * sum(5 ** i for i in range(1, 10)) + 32 + 9


@pytest.fixture(scope="module")
def run_check_bin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("splat_run_check") / "splat_run_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(NATIVE, "splat_run_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_header_has_no_hip_include():
    src = open(os.path.join(CSRC, "splat_run.h")).read()
    assert "#include <hip" not in src and "hip_runtime" not in src
    assert "__device__" not in src and "__global__" not in src


def test_wait_rule_report_latch_and_ring_depth(run_check_bin):
    r = subprocess.run([run_check_bin], capture_output=True, text=True, env={**os.environ, **SAN_ENV})
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    w = r.stdout.split()
    assert w[0] == "splat_run_check" and w[1] == "cases" and w[3:] == ["violations", "0"], r.stdout
    assert int(w[2]) == CASES == 7_324_256, (w[2], CASES)
