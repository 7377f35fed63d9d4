"""The two-lane ChaCha20 block of seal's header-protection pool entries without a GPU.

tests/csrc/test_chacha_pair.cpp includes milli_quic_amd/csrc/mq_chacha_pair.h (the block function the
kernel itself calls, mq_chacha.hip cc_pool_seal) with a host word type that holds both lanes and a
swap for the exchange, and compares keystream words 0 and 1 (and the other half's 2 and 3) with a
plain RFC 8439 block function: on the RFC 8439 §2.3.2 vector, on the ChaCha20 header-protection
vectors of tests/golden/hp_vectors.json (counters 0 and 0xffffffff included; the mask itself is
checked too) and on 4096 random key, counter and nonce sets. Built as a plain host binary with
AddressSanitizer and UndefinedBehaviorSanitizer."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHACHA = 2  # MQ_SUITE_CHACHA20


def test_chacha_pair_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    with open(os.path.join(ROOT, "tests", "golden", "hp_vectors.json")) as fh:
        cases = [c for c in json.load(fh)["cases"] if c["suite"] == CHACHA]
    assert len(cases) >= 8 and any(c["sample"].startswith("ffffffff") for c in cases)
    vec = tmp_path / "hp_vectors.txt"
    vec.write_text("".join(f"{c['hp']} {c['sample']} {c['mask']}\n" for c in cases))
    exe = tmp_path / "test_chacha_pair"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "milli_quic_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "test_chacha_pair.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    assert f"{len(cases)} hp vectors" in r.stdout and "chacha pair ok" in r.stdout
