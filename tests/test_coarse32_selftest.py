"""CPU self-test of pass A's coarse walk on scaled 32-bit state (no GPU):
tools/coarse32_selftest.cpp steps dmf_brick.hpp's coarse_next32 / coarse_walk32 beside the
64-bit coarse_next over whole rays -- every step's axis, the stepped brick index, the two-word
path and the stated bound on |gamma| -- on random rays, brick-corner ties, axis-aligned and
planar rays, the largest |dq| of a 1024-cell axis, every sign octant, starts on a brick face and
rays of more than 32 boundaries.  Run plain and as an ASan + UBSan build, as test_selftests.py
runs the other self-tests."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "coarse32_selftest.cpp")
INC = ["-I", os.path.join(ROOT, "depth-map-fusion-utils_amd", "csrc")]
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build_and_run(out, args, opt):
    exe = os.path.join(out, "coarse32_selftest")
    subprocess.run(["g++", *opt, "-std=c++17", "-ffp-contract=off", *INC, SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)


@pytest.mark.timeout(300)
def test_coarse32_selftest(tmp_path):
    r = _build_and_run(str(tmp_path), ["3000000", "1"], ["-O2"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout.splitlines()[-1], r.stdout


@pytest.mark.timeout(300)
def test_coarse32_selftest_under_sanitizers(tmp_path):
    r = _build_and_run(str(tmp_path), ["200000", "5"], SAN)
    assert r.returncode == 0 and " 0 failures" in r.stdout.splitlines()[-1], r.stdout + r.stderr
