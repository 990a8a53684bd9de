"""The 3DGS forward pass's host planning (csrc/splat_plan.h), checked without a GPU: the header builds with a
host compiler alone, and tests/native/splat_plan_check.cpp (stand-alone, ASan + UBSan linked in) passes its pinned
plans of the benchmark's frames, the edges of the kernels' static limits and the invariants over a seeded sweep."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc")


@pytest.fixture(scope="module")
def plan_check_bin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "splat_plan_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "native", "splat_plan_check.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_plan_header_has_no_hip_include():
    src = open(os.path.join(CSRC, "splat_plan.h")).read()
    assert "#include <hip" not in src and "__device__" not in src and "__global__" not in src


def test_pinned_plans_edges_and_invariants(plan_check_bin):
    r = subprocess.run([plan_check_bin], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.startswith("ok: 200000 sweep rounds"), r.stdout[-2000:]
