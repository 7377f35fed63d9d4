"""The diagnostic switch table without a GPU and without the library: tests/csrc/test_opts.cpp includes
only milli_quic_amd/csrc/mq_opts.h and is built with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer, then run as a child process (as tests/test_poly_states.py runs its
replay). It checks the name table against the enum, the environment parsing rules (unset, empty,
non-numeric and negative values are unset), that values set at run time read back, that the
environment is read once only, and that a Switches snapshot keeps the values it was taken under."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_switch_table_stand_alone(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "test_opts"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "milli_quic_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "test_opts.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok 13 switches", r.stdout
