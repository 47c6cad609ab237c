#!/usr/bin/env python3
"""A job's Noise frames sealed in one batch, measured (docs/POOL.md "Frame sealing"): where the GPU starts to win.

For n in 64, 512, 4096, 16384 and 65536 frames of 55 bytes (an encoded NewMiningJob), and again for the same n with
every second frame 653 bytes (a NewExtendedMiningJob at 12 branches with a 240-byte coinbase):
  kernel  otd_aead_seal alone, device events around FrameSeal.launch on buffers already on the device (median of 50)
  gpu     the wall-clock round trip of pool.batch.seal_frames(device="cuda:N") (p50 and p99 over --reps calls after two
          warm-ups): frames packed, one pinned buffer in, the kernel, one pinned buffer out, one synchronise, keys
          wiped, frames unpacked. A cell stops early once it has run --cell-seconds; "calls" says how many it made.
  cpu     seal_frames(device="cpu"), the native aead_seal_many_cpu, on the same host
  python  seal_frames(device=None), one utils.aead.seal a frame, what CipherState.encrypt does per message

Every CPU time is the median of five runs after two warm-ups, with min and max. This process is the only one with
the GPU open. ``seal_min_gpu`` is the rule of tools/bench_job_roots.py against the native CPU time, on the 55-byte
column; None means the GPU won at no measured size.

--end-to-end: one pool in this process with 2048 and with 10000 Noise connections over transports that only count
bytes (no sockets), one standard channel each, and the wall time of new_block() with seal_device off, cpu and the
device (seal_min_gpu=1, so the device is used). --job-device (default cpu) is the same in all three settings.

Output: one JSON document (--out FILE writes it there too).
"""
import argparse
import asyncio
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_job_roots import cpu_ms  # noqa: E402
from bench_verify_live import ADDR, RUNS, WARMUPS, spread  # noqa: E402

SIZES = (64, 512, 4096, 16384, 65536)
SMALL, LARGE = 55, 653
CROWDS = (2048, 10000)


def make_frames(n: int, mixed: bool) -> list:
    r = random.Random(f"bench-seal.{n}.{mixed}")
    return [(r.randbytes(32), 2 + i % 5, r.randbytes(LARGE if mixed and i % 2 else SMALL)) for i in range(n)]


def kernel_ms(op, frames) -> dict:
    import torch

    from otedama_amd.ops.seal_rows import pack_frames

    packed, out_bytes = pack_frames(frames)
    src = torch.frombuffer(packed, dtype=torch.uint8).to(op.device)
    out = torch.empty(out_bytes, dtype=torch.uint8, device=op.device)
    times = []
    for r in range(WARMUPS + 50):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        op.launch(src, len(frames), out)
        b.record()
        b.synchronize()
        if r >= WARMUPS:
            times.append(a.elapsed_time(b))
    return spread(times)


def measure(device: str, reps: int, cell_seconds: float) -> list:
    from otedama_amd.ops.seal import FrameSeal
    from otedama_amd.pool.batch import seal_frames

    op = FrameSeal(device)
    rows = []
    for mixed in (False, True):
        for n in SIZES:
            frames = make_frames(n, mixed)
            lat, t_cell = [], time.perf_counter()
            for r in range(WARMUPS + reps):
                t0 = time.perf_counter()
                got = seal_frames(frames, device)
                if r >= WARMUPS:
                    lat.append((time.perf_counter() - t0) * 1e3)
                    if time.perf_counter() - t_cell > cell_seconds:
                        break
            lat.sort()
            row = {"n": n, "mixed": mixed, "plain_bytes": sum(len(f[2]) for f in frames),
                   "kernel_ms": kernel_ms(op, frames),
                   "gpu_ms": {"p50": lat[(len(lat) - 1) // 2], "p99": lat[max(0, -(-99 * len(lat) // 100) - 1)],
                              "min": lat[0], "max": lat[-1], "calls": len(lat)},
                   "cpu_ms": cpu_ms(lambda: seal_frames(frames, "cpu")),
                   "python_ms": cpu_ms(lambda: seal_frames(frames))}
            row["equal"] = got == seal_frames(frames, "cpu") == seal_frames(frames)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def min_gpu_default(rows: list):
    """The smallest measured n of the 55-byte column whose GPU p50 is at or below the native CPU time, rounded up to
    a power of two; None = the GPU never won."""
    for row in rows:
        if not row["mixed"] and row["gpu_ms"]["p50"] <= row["cpu_ms"]["median"]:
            return 1 << (row["n"] - 1).bit_length()
    return None


class CountingTransport:
    """What a Noise writer writes to: counts, keeps nothing."""

    def __init__(self):
        self.bytes = self.writes = 0

    def write(self, b):
        self.bytes += len(b)
        self.writes += 1

    def close(self):
        pass


async def crowd_pool(n: int, seal_device: str, job_device: str):
    """A pool that never listens, with n Noise connections set up and one standard channel open on each."""
    from otedama_amd.pool.server import PoolOptions, PoolServer, _V2Conn
    from otedama_amd.stratum import messages as M
    from otedama_amd.stratum import noise

    pool = PoolServer(PoolOptions(payout_address=ADDR, job_interval=3600, block_interval=3600, noise=True, n_txs=4095,
                                  initial_difficulty=1.0, fixed_difficulty=True, seal_device=seal_device,
                                  seal_min_gpu=1, job_device=job_device))
    pool.log = lambda level, msg: None
    pool.new_block()
    r = random.Random(f"bench-seal-crowd.{n}")
    sinks = []
    for i in range(n):
        sink = CountingTransport()
        c = _V2Conn(pool, None, noise.EncryptedWriter(sink, noise.CipherState(r.randbytes(32))))
        await c._handle(M.SetupConnection(flags=M.FLAG_REQUIRES_VERSION_ROLLING, vendor="bench"))
        await c._handle(M.OpenMiningChannel(req_id=i, user=f"{ADDR}.w{i}", nominal_hashrate=0.0))
        assert len(c.channels) == 1
        pool._v2.add(c)
        sinks.append(sink)
    return pool, sinks


def end_to_end(device: str, job_device: str) -> list:
    async def one(n: int, seal_device: str) -> dict:
        pool, sinks = await crowd_pool(n, seal_device, job_device)
        try:
            times = []
            for r in range(WARMUPS + RUNS):
                before = sum(s.bytes for s in sinks)
                t0 = time.perf_counter()
                pool.new_block()
                if r >= WARMUPS:
                    times.append((time.perf_counter() - t0) * 1e3)
                sent = sum(s.bytes for s in sinks) - before
            return {"connections": n, "seal_device": seal_device, "new_block_ms": spread(times), "bytes_a_block": sent,
                    "seal": pool.seal_stats(), "jobs": pool.jobs_stats()}
        finally:
            await pool.stop()

    rows = []
    for n in CROWDS:
        for seal_device in ("", "cpu", device):
            row = asyncio.run(one(n, seal_device))
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--reps", type=int, default=1000, help="timed seal_frames calls per size on the device")
    ap.add_argument("--cell-seconds", type=float, default=45.0, help="a size's device calls stop after this long")
    ap.add_argument("--end-to-end", action="store_true", help="measure new_block() of a crowded pool instead")
    ap.add_argument("--job-device", default="cpu", help="the pool's job_device in the end-to-end mode")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    doc = {"tool": "tools/bench_seal_frames.py", "device": args.device, "warmups": WARMUPS, "runs": RUNS}
    if args.end_to_end:
        doc.update(job_device=args.job_device, rows=end_to_end(args.device, args.job_device))
    else:
        rows = measure(args.device, args.reps, args.cell_seconds)
        doc.update(reps=args.reps, cell_seconds=args.cell_seconds, rows=rows, seal_min_gpu=min_gpu_default(rows))
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
