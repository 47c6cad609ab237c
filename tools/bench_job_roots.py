#!/usr/bin/env python3
"""A job's fan-out to n standard channels, measured (docs/POOL.md "Job fan-out"): where the GPU starts to win.

For n in 1, 8, 64, 512, 4096, 32768 and 65536 prefixes of the pool's own coinbase with 12 merkle branches:
  gpu     the wall-clock round trip of ChannelRoots.roots (p50 and p99 over --reps calls after two warm-ups): prefix
          rows packed, one pinned buffer in, otd_channel_roots, one pinned buffer out, one synchronise, roots unpacked
  cpu     pool.batch.channel_roots(device="cpu"), the native share_roots_cpu, on the same host
  python  pool.batch.channel_roots(device=None), what PoolServer.merkle_root_for does per channel

Every CPU time is the median of five runs after two warm-ups, with min and max. This process is the only one with
the GPU open. ``job_min_gpu`` is the rule of tools/bench_verify_live.py against the native CPU time. Output: one JSON
document (--out FILE writes it there too).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_verify_live import RUNS, WARMUPS, pool_share_job, spread  # noqa: E402

SIZES = (1, 8, 64, 512, 4096, 32768, 65536)


def cpu_ms(fn) -> dict:
    times = []
    for r in range(WARMUPS + RUNS):
        t0 = time.perf_counter()
        fn()
        if r >= WARMUPS:
            times.append((time.perf_counter() - t0) * 1e3)
    return spread(times)


def measure(device: str, reps: int) -> list:
    from otedama_amd.ops.roots import ChannelRoots
    from otedama_amd.pool.batch import channel_roots

    job = pool_share_job(4095)
    op = ChannelRoots(device)
    prep = op.prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, job.branches)
    rows = []
    for n in SIZES:
        prefixes = [(0x01020000 + i).to_bytes(job.en_size, "big") for i in range(n)]
        lat = []
        for r in range(WARMUPS + reps):
            t0 = time.perf_counter()
            got = op.roots(prep, prefixes)
            if r >= WARMUPS:
                lat.append((time.perf_counter() - t0) * 1e3)
        lat.sort()
        # nearest rank: with the default 1000 calls p99 is the 990th smallest, ten samples below the maximum
        row = {"n": n, "gpu_ms": {"p50": lat[(len(lat) - 1) // 2], "p99": lat[max(0, -(-99 * len(lat) // 100) - 1)],
                                  "min": lat[0], "max": lat[-1], "calls": len(lat)},
               "cpu_ms": cpu_ms(lambda: channel_roots(job, prefixes, "cpu")),
               "python_ms": cpu_ms(lambda: channel_roots(job, prefixes))}
        row["equal"] = got == channel_roots(job, prefixes, "cpu") == channel_roots(job, prefixes)
        rows.append(row)
    return rows


def min_gpu_default(rows: list):
    """The smallest measured n whose GPU p50 is at or below the native CPU time, rounded up to a power of two; None =
    the GPU never won."""
    for row in rows:
        if row["gpu_ms"]["p50"] <= row["cpu_ms"]["median"]:
            return 1 << (row["n"] - 1).bit_length()
    return None


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--reps", type=int, default=1000, help="timed ChannelRoots.roots calls per size")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = measure(args.device, args.reps)
    doc = {"tool": "tools/bench_job_roots.py", "device": args.device, "warmups": WARMUPS, "runs": RUNS,
           "reps": args.reps, "rows": rows, "job_min_gpu": min_gpu_default(rows)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
