"""The scene upload's host-only parts, checked without a GPU: the BVH try policy (csrc/bvh_tries.h) and the
argument checks and triangle flattening (csrc/scene_flatten.h). Both headers build with a host compiler
alone; tests/native/bvh_tries_check.cpp and tests/native/scene_flatten_check.cpp are stand-alone programs
(their own main, ASan + UBSan linked in).

bvh_tries_check pins the parsing of PTGS_BVH_TRIES / PTGS_BVH_NODE_LIMIT, runs the policy over a stub builder
that counts acquisitions and releases (an error on the n-th build, not supported on the first, an error in a
collapse, the LBVH's list with a need that never fits, hand-over), and over the host builder on soup(2500)
and the planar grid against trees built directly. The stack needs of the default list's four tries
(3:4:38, 4:4:38, 3:3:38, 3:2:38) are 18, 16, 18, 12 on soup(2500) and 17, 16, 19, 12 on the grid (BVH2 depth
12 on both), so a stack of the smallest need + 1 is first met by try 3, after three builds and four collapses,
and a stack of 17 by try 1. The GPU builders' later tries and their fallback to the host cannot be reached
on a GPU (the stack capacity is a compile-time constant no small scene exceeds): this is their coverage."""
import os
import subprocess

import numpy as np
import pytest

import bvh_soups as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


def _build(tmp_path_factory, name, extra_srcs=()):
    exe = str(tmp_path_factory.mktemp(name) / name)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, *extra_srcs,
           os.path.join(NATIVE, name + ".cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def tries_check_bin(tmp_path_factory):
    return _build(tmp_path_factory, "bvh_tries_check", [os.path.join(CSRC, "bvh.cpp")])


@pytest.fixture(scope="module")
def flatten_check_bin(tmp_path_factory):
    return _build(tmp_path_factory, "scene_flatten_check")


@pytest.mark.parametrize("header", ["bvh_tries.h", "scene_flatten.h"])
def test_headers_have_no_hip_include(header):
    src = open(os.path.join(CSRC, header)).read()
    assert "#include <hip" not in src and "__device__" not in src and "__global__" not in src


def test_parsing_and_stub_builder(tries_check_bin):
    r = subprocess.run([tries_check_bin], capture_output=True, text=True, env={**os.environ, **SAN_ENV})
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.strip() == "bvh_tries_check violations 0"


@pytest.mark.parametrize("name,needs", [("soup2500", [18, 16, 18, 12]), ("grid", [17, 16, 19, 12])])
def test_policy_with_the_host_builder(tries_check_bin, tmp_path, name, needs):
    path = os.path.join(str(tmp_path), "tris.bin")
    np.ascontiguousarray(B.get(name), np.float32).tofile(path)
    r = subprocess.run([tries_check_bin, path], capture_output=True, text=True, env={**os.environ, **SAN_ENV})
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "bvh_tries_check violations 0" and len(lines) == 2
    w = lines[0].split()
    assert w[0] == "policy" and w[2] == "depth2" and w[4] == "needs" and w[9] == "stop"
    got = [int(x) for x in w[5:9]]
    assert got == needs  # (the docstring's figures: the host build is deterministic)
    stop = int(w[10])
    assert stop == got.index(min(got)) and stop >= 1  # the smallest need + 1 is first met by a later try


def test_scene_validation_and_flattening(flatten_check_bin):
    r = subprocess.run([flatten_check_bin], capture_output=True, text=True, env={**os.environ, **SAN_ENV})
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    w = r.stdout.split()
    assert w[0] == "scene_flatten_check" and int(w[2]) >= 30 and w[3:] == ["violations", "0"]
