"""A/B of library builds on bench.py itself: alternates one bench.py child process per library,
`rounds` times, and compares every library's median ms_per_step with the first one's, against the
first one's own spread (max - min over its runs): a difference inside that spread is no difference.
A library is a path (e.g. a copy of tools/build_rev.sh's output) or `product` (the tree's build).
Usage: python tools/ab_bench.py ROUNDS LIB_A LIB_B [LIB_C ...] [-- bench.py arguments...]"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    rounds, rest = int(sys.argv[1]), sys.argv[2:]
    cut = rest.index("--") if "--" in rest else len(rest)
    libs, extra = rest[:cut], rest[cut + 1:]
    res = {lib: [] for lib in libs}
    print(f"# bench.py --gpus 1 {' '.join(extra)}: {rounds} alternations, one child process per run", flush=True)
    for _ in range(rounds):
        for lib in libs:
            env = dict(os.environ)
            env.pop("MQ_LIB", None)
            if lib != "product":
                env["MQ_LIB"] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra,
                               capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
            js = [x for x in p.stdout.splitlines() if x.startswith("{")]
            if p.returncode != 0 or not js:
                print(lib, "FAILED rc", p.returncode, p.stderr[-800:], flush=True)
                sys.exit(1)
            j = json.loads(js[-1])
            rf = j["roofline"]
            res[lib].append((j["ms_per_step"], j["value"], rf["seal_ms"], rf["open_ms"]))
            print(f"  {lib} ms_per_step {j['ms_per_step']:.4f}  {j['value']:.1f} GiB/s  seal {rf['seal_ms']:.4f} "
                  f"open {rf['open_ms']:.4f}", flush=True)
    for lib in libs:
        a = np.array(res[lib])
        ms = a[:, 0]
        print(f"{lib} median ms_per_step {np.median(ms):.4f} (min {ms.min():.4f} max {ms.max():.4f}, spread "
              f"{ms.max() - ms.min():.4f})  median {np.median(a[:, 1]):.1f} GiB/s  seal {np.median(a[:, 2]):.4f} "
              f"open {np.median(a[:, 3]):.4f}", flush=True)
    a = np.array(res[libs[0]])[:, 0]
    for lib in libs[1:]:
        b = np.array(res[lib])[:, 0]
        print(f"gain of {lib} {np.median(a) - np.median(b):.4f} ms ({(np.median(a) / np.median(b) - 1) * 100:.2f} %) "
              f"vs {libs[0]}'s spread {a.max() - a.min():.4f} ms", flush=True)


if __name__ == "__main__":
    main()
