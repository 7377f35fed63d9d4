"""The workspace carving without a GPU and without the library: tests/csrc/test_workspace.cpp includes only
milli_quic_amd/csrc/mq_workspace.h and is built with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer, then run as a child process (as tests/test_opts.py runs its program). It checks
key_bits at the edges of the key ranges the sorts see (never above 32 bits), and the carve type: pieces
256-aligned relative to the base, disjoint and in order, the null-base pass giving the same total as the real
one, take<T>(0) taking nothing, and a count near 2^32 of 8-byte items not wrapping."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_stand_alone(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "test_workspace"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "milli_quic_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "test_workspace.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok workspace", r.stdout
