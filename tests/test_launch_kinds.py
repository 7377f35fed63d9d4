"""Which kernel family a batch runs, pinned without a GPU: mq_debug_chacha_flat_kind,
mq_debug_aes_flat_kind and mq_debug_aes_list_kind over a ladder of batch sizes, key-table sizes and
bytes per packet on both sides of every threshold, with and without MQ_BATCH_LEN_HINT, under each
value of the switches that steer the choice. The expected values (tests/golden/launch_kinds.json)
were recorded from the library as it stood before the launchers took argument structs and one
switch snapshot per call: the decisions must not move.

    MQ_LIB=<a build of libmq_aead.so> python tests/test_launch_kinds.py --record

rewrites the table from that build."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from milli_quic_amd import _lib  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "launch_kinds.json")
NS = (1, 7, 8, 9, 511, 512, 513, 4096, 1 << 20, 1 << 30, (1 << 30) + 1)
ROWS = (1, 2, 3, 2048)
BPPS = (400, 401, 640, 641, 1216, 1217, 1536, 1537, 1584, 1585)
# unset, then every documented value of each switch (mq_opts.h)
SETTINGS = ((None, None), ("MQ_AES_NARROW", 0), ("MQ_AES_NARROW", 1), ("MQ_AES_NARROW", 2), ("MQ_AES_SEG", 0),
            ("MQ_AES_SEG", 1), ("MQ_CC_NARROW", 0), ("MQ_CC_NARROW", 1))
SWITCHES = sorted({name for name, _ in SETTINGS if name})


def setting_name(name, value):
    return "unset" if name is None else f"{name}={value}"


def flat_kinds(fn, suite):
    """fn over n x bytes per packet x (arena-derived, hinted): the hinted call's arena says 2^40 B."""
    out = []
    for n in NS:
        for bpp in BPPS:
            out.append(fn(bpp * n, n, suite))
            out.append(fn(1 << 40, n, suite | _lib.MQ_BATCH_LEN_HINT(bpp)))
    return out


def walk(lib):
    """{setting: {function: [values in ladder order]}}; every switch is back as it was afterwards."""
    before = {s: lib.mq_debug_option_get(s.encode()) for s in SWITCHES}
    table = {}
    try:
        for name, value in SETTINGS:
            for s in SWITCHES:
                assert lib.mq_debug_option(s.encode(), value if s == name else -1) == _lib.MQ_OK
            table[setting_name(name, value)] = {
                "chacha_flat": flat_kinds(lib.mq_debug_chacha_flat_kind, _lib.MQ_SUITE_CHACHA20),
                "aes_flat": flat_kinds(lib.mq_debug_aes_flat_kind, _lib.MQ_SUITE_AES128GCM),
                "aes_list": [lib.mq_debug_aes_list_kind(n, rows) for n in NS for rows in ROWS],
            }
    finally:
        for s, v in before.items():
            lib.mq_debug_option(s.encode(), v)
    assert {s: lib.mq_debug_option_get(s.encode()) for s in SWITCHES} == before
    return table


def test_ladder_matches_recorded_table(mqlib):
    with open(TABLE) as f:
        want = json.load(f)
    assert want["n"] == list(NS) and want["n_rows"] == list(ROWS) and want["bpp"] == list(BPPS)
    got = walk(mqlib)
    assert sorted(got) == sorted(want["kinds"]) and len(got) == len(SETTINGS)
    for setting, fns in want["kinds"].items():
        for fn, values in fns.items():
            assert len(values) == (len(NS) * len(ROWS) if fn == "aes_list" else len(NS) * len(BPPS) * 2)
            assert got[setting][fn] == values, (setting, fn)


def test_table_covers_every_family():
    # the ladder reaches each value the reporters can give, so a table of one constant cannot pass
    with open(TABLE) as f:
        kinds = json.load(f)["kinds"]
    seen = {fn: set() for fn in ("chacha_flat", "aes_flat", "aes_list")}
    for fns in kinds.values():
        for fn, values in fns.items():
            seen[fn].update(values)
    assert seen["chacha_flat"] == {0, 1, 2, 3} and seen["aes_flat"] == {2, 4, 8}
    assert {v & 0xFF for v in seen["aes_list"]} == {0, 1, 2, 3}
    assert {v >> 8 for v in seen["aes_list"]} == {0, 2, 4, 8}


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(TABLE, "w") as f:
        json.dump({"n": NS, "n_rows": ROWS, "bpp": BPPS, "kinds": walk(_lib.load())}, f, separators=(",", ":"))
        f.write("\n")
