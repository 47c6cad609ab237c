#!/usr/bin/env python3
"""A block template's two merkle trees, measured (docs/POOL.md "Real templates and the template tree"): where the GPU
starts to win.

For n in 8, 64, 512, 4096, 16384 and 65536 leaves per tree (the coinbase slot and n - 1 transactions), the txid tree
and the wtxid tree together, as the pool asks for them:
  gpu     the wall-clock round trip of pool.batch.template_tree(device="cuda:0") (p50 and p99 over --reps calls after
          two warm-ups): leaves packed, one pinned buffer in, otd_merkle_tree (one launch up to 512 leaves, two above),
          one pinned buffer out, one synchronise, rows unpacked
  cpu     template_tree(device="cpu"), the native merkle_tree_cpu, on the same host
  python  template_tree(device=None): merkle_branches and merkle_root_full, what the pool did before

Every CPU time is the median of five runs after two warm-ups, with min and max. This process is the only one with
the GPU open. The three paths must agree, or the tool fails. ``template_min_gpu`` is the rule of
tools/bench_job_roots.py against the native CPU time. Output: one JSON document (--out FILE writes it there too).
"""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_job_roots import cpu_ms, min_gpu_default  # noqa: E402
from bench_verify_live import RUNS, WARMUPS  # noqa: E402

SIZES = (8, 64, 512, 4096, 16384, 65536)


def measure(device: str, reps: int) -> list:
    from otedama_amd.pool.batch import template_tree

    rows = []
    for n in SIZES:
        txids = [hashlib.sha256(b"bench-template-tree/t/%d" % i).digest() for i in range(n - 1)]
        wtxids = [hashlib.sha256(b"bench-template-tree/w/%d" % i).digest() for i in range(n - 1)]
        lat = []
        for r in range(WARMUPS + reps):
            t0 = time.perf_counter()
            got = template_tree(txids, wtxids, device)
            if r >= WARMUPS:
                lat.append((time.perf_counter() - t0) * 1e3)
        lat.sort()
        # nearest rank: with the default 1000 calls p99 is the 990th smallest, ten samples below the maximum
        row = {"n": n, "gpu_ms": {"p50": lat[(len(lat) - 1) // 2], "p99": lat[max(0, -(-99 * len(lat) // 100) - 1)],
                                  "min": lat[0], "max": lat[-1], "calls": len(lat)},
               "cpu_ms": cpu_ms(lambda: template_tree(txids, wtxids, "cpu")),
               "python_ms": cpu_ms(lambda: template_tree(txids, wtxids))}
        row["equal"] = got == template_tree(txids, wtxids, "cpu") == template_tree(txids, wtxids)
        assert row["equal"], f"the three paths disagree at n = {n}"
        rows.append(row)
    return rows


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--reps", type=int, default=1000, help="timed template_tree calls on the device per size")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = measure(args.device, args.reps)
    doc = {"tool": "tools/bench_template_tree.py", "device": args.device, "warmups": WARMUPS, "runs": RUNS,
           "reps": args.reps, "rows": rows, "template_min_gpu": min_gpu_default(rows)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
