"""Poly1305 value boundaries without a GPU: crafted packets (tests/poly_states.py) whose accumulator
ends on 0, 1, 4, 5, 6, p-1, p-5, p-6, 2^128-1, 2^128, 2^129 or gives a tag of sixteen 0x00 / 0xFF bytes,
for ciphertext of 16, 17, 33, 1171 and 16384 B, AAD of 0, 13 and 29 B, the other blocks random, 0x00
or 0xFF.

1. The oracle against the big-integer reference: aead_seal gives exactly the crafted ciphertext and
   the big-integer tag, aead_open accepts it and refuses the tag shifted by +-5 (p = -5 mod 2^128:
   what a missing or a spurious final subtraction yields). This pins the checker of the GPU tests.
2. tests/csrc/test_poly_states.cpp (g++, AddressSanitizer and UndefinedBehaviorSanitizer, run as a
   child process) replays every vector through mq_poly26.h as the kernels schedule it: serial Horner,
   poly_tag's step loop for lane groups of 4 and 8 with and without the pair loop, the resident
   server's 64-way Horner with its 64-bit limb sums. Every tag matches; in the serial replay every
   vector with a target in 0 .. 4 enters p26_finish at or above p; in each interleaved schedule some
   vector of every ciphertext length does; in every schedule but the resident one (whose limb sums
   arrive normalised) some vector enters with a limb >= 2^26."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import poly_states as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHACHA = 2  # MQ_SUITE_CHACHA20
CT_LENS = (16, 17, 33, 1171, 16384)
AAD_LENS = (0, 13, 29)
WHERES = ("first", "last", "lean")
SCHEDULES = ("serial", "g4", "g4p", "g8", "g8p", "resident")
# the failing vectors of p26_finish's second carry pass (see test_second_fold_carry_reaches_limb_four)
NAMED = (("2^128", 1171, 13, "random"), ("2^128", 16, 13, "ones"), ("2^129", 16384, 0, "ones"))


@functools.lru_cache(maxsize=None)
def vectors():
    """(target, fill, ct_len, aad_len) -> (key, nonce, aad, ct, tag, otk), from fixed seeds. A packet
    of one ciphertext block redraws its AAD bytes, and without AAD its nonce."""
    out = {}
    for ti, target in enumerate(ps.TARGETS):
        for fi, fill in enumerate(ps.FILLS):
            for ci, ct_len in enumerate(CT_LENS):
                for ai, aad_len in enumerate(AAD_LENS):
                    rng = np.random.default_rng([ti, fi, ci, ai])
                    key = rng.bytes(32)
                    where = WHERES[(ti + fi + ci + ai) % 3]
                    nonce, aad, ct, tag = ps.craft_any_nonce(key, aad_len, ct_len, target, where, fill, rng)
                    out[target, fill, ct_len, aad_len] = (key, nonce, aad, ct, tag, ps.one_time_key(key, nonce)[2])
    return out


def test_reference_against_rfc8439():
    # RFC 8439 §2.8.2: the reference of this module is the RFC's
    key = bytes(range(0x80, 0xA0))
    nonce = bytes.fromhex("070000004041424344454647")
    aad = bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
    pt = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
          b"sunscreen would be it.")
    out = ps.aead_seal(key, nonce, aad, pt)
    assert out[:16].hex() == "d31a8d34648e60db7b86afbc53ef7ec2"
    assert out[-16:].hex() == "1ae10b594f09e26a7e902ecbd0600691"
    assert ps.plaintext_for(out[:-16], ps.keystream(key, nonce, len(pt))) == pt


def test_targets_are_reached():
    for (target, fill, ct_len, aad_len), (key, nonce, aad, ct, tag, _) in vectors().items():
        r, s, _ = ps.one_time_key(key, nonce)
        h = ps.accumulator(r, ps.poly_blocks(ps.mac_input(aad, ct)))
        assert h == ps.target_value(target, s) and len(ct) == ct_len and len(aad) == aad_len
        if target == ps.TAG_ZERO:
            assert tag == bytes(16)
        if target == ps.TAG_ONES:
            assert tag == b"\xff" * 16
    assert len(vectors()) == len(ps.TARGETS) * 3 * len(CT_LENS) * len(AAD_LENS)


@pytest.mark.parametrize("ct_len", CT_LENS)
def test_oracle_against_big_integers(orc, ct_len):
    for (target, fill, n, aad_len), (key, nonce, aad, ct, tag, _) in vectors().items():
        if n != ct_len:
            continue
        what = (target, fill, ct_len, aad_len)
        pt = ps.plaintext_for(ct, ps.keystream(key, nonce, ct_len))
        rc, sealed, _ = orc.aead_seal(CHACHA, key, nonce, aad, pt)
        assert rc == 0 and sealed[:-16] == ct, what
        assert sealed[-16:] == tag, what
        rc, back = orc.aead_open(CHACHA, key, nonce, aad, ct + tag)
        assert rc == 0 and back == pt, what
        for d in (-5, 5):
            rc, back = orc.aead_open(CHACHA, key, nonce, aad, ct + ps.shifted_tag(tag, d))
            assert rc != 0 and back == ct + ps.shifted_tag(tag, d), (what, d)


def build_replay(tmp_path, include=None):
    """The host program, built as tests/test_poly_pair.py builds its own; include: a directory whose
    mq_poly26.h stands in for the library's (the mutation checks of the arithmetic)."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "test_poly_states"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror"] + (["-I", str(include)] if include else []) +
                   ["-I", os.path.join(ROOT, "milli_quic_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "test_poly_states.cpp"), "-o", str(exe)], check=True)
    return exe


def run_replay(exe, tmp_path, vecs):
    path = tmp_path / "vectors.txt"
    with open(path, "w") as f:
        for (target, fill, ct_len, aad_len), (key, nonce, aad, ct, tag, otk) in vecs.items():
            small = int(isinstance(ps.TARGETS[target], int) and ps.TARGETS[target] < 5)
            f.write(f"{target}/{fill}/{aad_len} {small} {otk.hex()} {aad_len} {ct_len} {ps.mac_input(aad, ct).hex()} {tag.hex()}\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, env=env, timeout=600)
    rows = []
    for line in r.stdout.splitlines():
        t = line.split()
        if t and t[0] == "vec":
            rows.append(dict(name=t[1], ct_len=int(t[2]), small=t[3] == "1", schedule=t[4],
                             **{k: v == "1" for k, v in (x.split("=") for x in t[5:])}))
    return r, rows


def test_host_replay_asan_ubsan(tmp_path):
    r, rows = run_replay(build_replay(tmp_path), tmp_path, vectors())
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("schedule")))
    assert r.returncode in (0, 1), r.stderr
    assert len(rows) == len(vectors()) * len(SCHEDULES)
    wrong = [(x["name"], x["ct_len"], x["schedule"]) for x in rows if not x["match"]]
    assert not wrong, (len(wrong), wrong[:12])
    assert r.returncode == 0 and "poly states ok" in r.stdout
    serial_small = [x for x in rows if x["schedule"] == "serial" and x["small"]]
    assert len(serial_small) == 3 * 3 * len(CT_LENS) * len(AAD_LENS) and all(x["ge_p"] for x in serial_small)
    for s in SCHEDULES:
        mine = [x for x in rows if x["schedule"] == s]
        if s != "serial":
            assert {x["ct_len"] for x in mine if x["ge_p"]} == set(CT_LENS), s
        # p26_from_sums hands p26_finish normalised limbs: its second pass folds a carry of at most one
        # into a limb 0 of a few units (the value was 2^130 + e, e < 5 * 64), so no limb can reach 2^26
        # there; every other schedule must have sent one in
        assert any(x["limb26"] for x in mine) == (s != "resident"), s


def test_second_fold_carry_reaches_limb_four(tmp_path):
    # The vectors that failed before p26_finish carried its second pass through limb 4: a lane sum
    # c 2^130 + L with L = 2^128 - 5 c (or 2^129 - 5 c) has limbs 1 .. 3 all ones, the fold's + 5 c
    # ripples a carry up to limb 3 or 4, and the pass stopped at limb 2, which the word packing then
    # read as 2^26. Wrong in every lane schedule (c >= 1), right in the serial one (c = 0).
    vecs = {(t, fill, n, a): vectors()[t, fill, n, a] for t, n, a, fill in NAMED}
    r, rows = run_replay(build_replay(tmp_path), tmp_path, vecs)
    assert r.returncode == 0, (r.stderr, [x for x in rows if not x["match"]])
    assert len(rows) == len(NAMED) * len(SCHEDULES) and all(x["match"] for x in rows)
    lanes = [x for x in rows if x["schedule"] in ("g4", "g4p", "g8", "g8p")]
    assert len(lanes) == 4 * len(NAMED) and all(x["ge_p"] for x in lanes)  # group sums above 2^130: the fold ran
