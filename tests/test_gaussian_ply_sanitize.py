"""The checkpoint loader under AddressSanitizer + UndefinedBehaviorSanitizer.

tests/native/gsply_fuzz.cpp is a stand-alone driver (its own main, no device code): built here with
g++ -fsanitize=address,undefined -fno-sanitize-recover=all from ply.cpp and image_decode.cpp (ply.cpp's
file reader) into an executable with the sanitizer runtimes linked in, under tests/native/_build/
(git-ignored), as tests/native/Makefile does for the other host parsers. The driver writes valid
checkpoints of every degree and format, loads them, then loads deterministic mutations (header numbers
replaced, properties deleted / duplicated, truncation, byte flips). A mutated file may be accepted or
rejected; a sanitizer report or an abort fails the test. Nothing here runs through python with a
preloaded runtime, and nothing runs on a GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc")
NATIVE = os.path.join(HERE, "native")


@pytest.fixture(scope="module")
def fuzz_bin():
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out_dir = os.path.join(NATIVE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "gsply_fuzz")
    srcs = [os.path.join(CSRC, "ply.cpp"), os.path.join(CSRC, "image_decode.cpp"), os.path.join(NATIVE, "gsply_fuzz.cpp")]
    deps = srcs + [os.path.join(CSRC, "image_decode.h"), os.path.join(ROOT, "include", "ptgs", "ptgs.h"),
                   os.path.join(ROOT, "include", "ptgs", "ptgs_host.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
               "-I", CSRC] + srcs + ["-o", out, "-lz", "-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return out


@pytest.mark.parametrize("seed", [0, 1])
def test_checkpoint_loader_under_asan_ubsan(fuzz_bin, tmp_path, seed):
    r = subprocess.run([fuzz_bin, str(tmp_path), "250", str(seed)], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
                            "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "no sanitizer report" in r.stdout
    print(r.stdout.strip())
