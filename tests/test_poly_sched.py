"""The interleaved Poly1305's per-lane schedule without a GPU.

tests/csrc/test_poly_sched.cpp replays the step loop of mq_chacha.hip's poly_tag on the host over
milli_quic_amd/csrc/mq_poly_sched.h (the arithmetic the kernel itself calls): lane groups of 1, 2, 4
and 8, AAD of 1..48 B, ciphertext of 0..640 B, and waves of 2-8 packets of different geometry with
some inactive. It asserts that every MAC block is absorbed exactly once on the right lane and step,
that the lean stretch holds only whole ciphertext blocks and that no load passes the tag by more
than 19 bytes. Built as a plain host binary with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_poly_schedule_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "test_poly_sched"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "csrc", "test_poly_sched.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "poly sched ok" in r.stdout
