"""The paired Poly1305 reduction and poly_tag's pair loop without a GPU.

tests/csrc/test_poly_pair.cpp includes milli_quic_amd/csrc/mq_poly26.h and mq_poly_sched.h (the
arithmetic and the schedule the kernel itself calls). It checks p26_mul2 against plain arithmetic mod
2^130 - 5 on random operands and on the corner operands of its documented bound (every column sum
below 2^58, the result congruent and inside p26_mul's output bounds), and replays poly_tag's whole
step loop with the pair loop on real bytes for lane groups of 4 and 8, with and without the edge
steps, over waves of packets of different geometry with some inactive: every tag equals a serial
Poly1305 of the RFC 8439 MAC input, the addresses loaded are those of the loop without pairs, and lean
stretches of 0, 1, 2, 3, 4, 5, 16 and 17 steps all occur. Built as a plain host binary with
AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_poly_pair_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "test_poly_pair"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "milli_quic_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "test_poly_pair.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "poly pair ok" in r.stdout
