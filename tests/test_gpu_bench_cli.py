"""bench.py as the command it is run as, on a small batch: a plain run prints the result line
without the oracle parity or the CPU baselines, --full brings them back, --steps sets the number of
timed steps, and --dump-outputs writes what the last step left — checked against the oracle's
seal + open of the same batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytest.importorskip("torch")

import bench  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 3000  # not a multiple of the tile; below bench.DUMP_SAMPLE, so every packet's bytes are written


def run_bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--packets", str(N),
                        "--warmup-seconds", "0", *argv], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["b", "e"])
def test_plain_run_and_dump_vs_oracle(tmp_path, orc, cfg):
    d = run_bench("--steps", "3", "--warmup", "1", "--config", cfg, "--dump-outputs", str(tmp_path))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["warmup_extra"]["steps"] == 0
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert len(d["roofline"]["per_step_ms"]["seal"]["first5"]) == 3  # --steps timed steps, no more
    # value = wire bytes x 2 / the time of one step (ms_per_step is rounded to 1e-4 ms, a step of this
    # batch takes some 0.05 ms: 1 % covers the rounding of both)
    assert d["value"] == pytest.approx(d["config"]["wire_bytes_per_gpu"] * 2 / (d["ms_per_step"] * 1e-3) / 2 ** 30,
                                       rel=1e-2)
    assert d["cpu_baseline"] is None and "cpu_openssl" not in d
    assert d["parity"]["match"] and "oracle_sample_tag_checksum" not in d["parity"]
    # the dump: the arena after seal + open, the statuses and the packet numbers, as the oracle has them
    w, _ = bench.build_shard(cfg, N, 0, 1, bench.rank_keys(cfg, 1, None, "cpu"))
    ref = w.arena.copy()
    assert (orc.batch_seal(w.keys, ref, w.seal_desc, w.suite_hint) == 0).all()
    st, _ = orc.batch_open(w.keys, ref, w.open_desc, w.suite_hint)
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["pn", "sample_bytes", "sample_index", "status"]
    assert got["status"].dtype == np.float32 and (got["status"] == st).all() and (st == 0).all()
    assert got["pn"].dtype == np.float64 and (got["pn"] == w.pns.astype(np.float64)).all()
    assert (got["sample_index"] == np.arange(N)).all()
    want = np.concatenate([ref[int(o):int(o) + int(ln)] for o, ln in zip(w.seal_desc["offset"], w.seal_desc["len"])])
    assert got["sample_bytes"].dtype == np.float32 and got["sample_bytes"].shape == want.shape
    assert (got["sample_bytes"] == want).all()


@pytest.mark.gpu
def test_full_run_brings_the_oracle_parity():
    # the CPU baselines of --full time seconds of CPU work each: left out here (--no-cpu-baseline)
    d = run_bench("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    p = d["parity"]
    assert p["match"] and p["sample_packets"] == N and p["sample_tag_checksum"] == p["oracle_sample_tag_checksum"]
    assert p["failures"] == 0 and d["cpu_baseline"] is None
    assert d["steps"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
