#!/usr/bin/env python3
"""Live share verification, measured (docs/KERNELS.md "Live share verification", docs/POOL.md).

(a) SHA-256d at n = 2^20 shares of the pool's own coinbase with 12 merkle branches, device time by events, the
    variants interleaved in one run:
      launch   ShareVerify.launch: otd_share_headers, the digest launch, otd_share_verdict
      chain    ShareVerify.launch followed by otd_share_pack into result records
      results  ShareVerify.launch_results: otd_share_headers, the digest launch, otd_share_pack (what ships)
    The single-launch SHA-256d kernel this table once decided about is not in the tree (docs/KERNELS.md); the run
    that measured it is recorded there.
(b) per algorithm, for n in 1, 8, 64, 512, 4096: the wall-clock round trip of ShareVerify.results (p50 and p99 over
    --reps calls after two warm-ups) beside the same host's check_shares(device=None) time for the same n shares.

Every figure of (a) and every CPU time is the median of five runs after two warm-ups, with min and max. This process
is the only one with the GPU open. Output: one JSON document (--out FILE writes it there too).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ADDR = "bc1qar0srrr7xfkvy5l643lydnw9re59gtzzwf5mdq"
SIZES = (1, 8, 64, 512, 4096)
WARMUPS, RUNS = 2, 5


def pool_share_job(n_txs: int, en_size: int = 8):
    """The parts PoolServer._make_job hands out for a template with ``n_txs`` transactions (4095 -> 12 branches)."""
    from otedama_amd.pool.batch import ShareJob
    from otedama_amd.pool.template import TemplateSource

    blk = TemplateSource(ADDR, nbits=0x1703A30C, n_txs=n_txs, seed=b"bench-verify-live").next_block()
    coinb1, coinb2 = blk.coinbase_parts(en_size)
    return ShareJob(coinb1, coinb2, en_size, blk.prev_hash, blk.nbits, blk.branches())


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def device_times(fns: dict, n: int) -> dict:
    """Event-timed ms of each callable, interleaved run by run: WARMUPS untimed rounds, then RUNS timed ones."""
    import torch

    times = {k: [] for k in fns}
    for r in range(WARMUPS + RUNS):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= WARMUPS:
                times[name].append(a.elapsed_time(b))
    return {k: {"ms": spread(v), "mshares_per_s": spread([n / ms / 1e3 for ms in v])} for k, v in times.items()}


def part_a(device: str, log2n: int) -> dict:
    import torch

    from otedama_amd.ops.verify import ShareVerify

    n = 1 << log2n
    job = pool_share_job(4095)
    op = ShareVerify("sha256d", device)
    prep = op.prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, job.branches)
    gen = torch.Generator(device=device).manual_seed(1)
    recs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=device, generator=gen)
    recs[:, 28:] = 0  # every share against target 0
    tgts = torch.full((1, 32), 0xFF, dtype=torch.uint8, device=device)
    tgts[0, 31] = 0x0F  # one hash in 16 is a share
    out = torch.empty((n, 128), dtype=torch.uint8, device=device)
    out2 = torch.empty((n, 128), dtype=torch.uint8, device=device)

    def chain():
        v, d, h = op.launch(prep, recs, tgts)
        op.native.launch_share_pack(prep.dev.data_ptr(), recs.data_ptr(), h.data_ptr(), d.data_ptr(), tgts.data_ptr(),
                                    1, n, out2.data_ptr(), torch.cuda.current_stream(op.device).cuda_stream)

    res = device_times({"launch": lambda: op.launch(prep, recs, tgts), "chain": chain,
                        "results": lambda: op.launch_results(prep, recs, tgts, out=out)}, n)
    torch.cuda.synchronize()
    same = bool(torch.equal(out, out2))
    return {"n": n, "branches": len(job.branches), "coinbase_bytes": len(job.coinb1) + job.en_size + len(job.coinb2),
            "results_equal_chain": same, **res}


def part_b(device: str, algorithm: str, reps: int, cpu_cap: int) -> list:
    from otedama_amd.ops.verify import ShareVerify
    from otedama_amd.pool.batch import check_shares

    job = pool_share_job(7)
    op = ShareVerify(algorithm, device)
    prep = op.prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, job.branches)
    targets = [bytes(31) + b"\x0f", b"\xff" * 32]
    rows = []
    for n in SIZES:
        shares = [(i.to_bytes(8, "little"), 1_700_000_000 + i, 0x9E3779B9 * (i + 1) & 0xFFFFFFFF, 0x20000000)
                  for i in range(n)]
        tidx = [i & 1 for i in range(n)]
        lat = []
        for r in range(WARMUPS + reps):
            t0 = time.perf_counter()
            got = op.results(prep, shares, targets, tidx)
            if r >= WARMUPS:
                lat.append((time.perf_counter() - t0) * 1e3)
        lat.sort()
        # nearest rank: with the default 1000 calls p99 is the 990th smallest, ten samples below the maximum
        row = {"n": n, "gpu_ms": {"p50": lat[(len(lat) - 1) // 2], "p99": lat[max(0, -(-99 * len(lat) // 100) - 1)],
                                  "min": lat[0], "max": lat[-1], "calls": len(lat)}}
        m = min(n, cpu_cap)  # a slow CPU hash is timed on the first cpu_cap shares and scaled, and marked so
        cpu = []
        for r in range(WARMUPS + RUNS):
            t0 = time.perf_counter()
            want = check_shares(algorithm, job, shares[:m], targets, tidx[:m])
            if r >= WARMUPS:
                cpu.append((time.perf_counter() - t0) * 1e3 * n / m)
        row["cpu_ms"] = dict(spread(cpu), scaled_from=m if m < n else None)
        row["equal"] = got[:m] == want
        rows.append(row)
    return rows


def min_gpu_default(rows: list):
    """The smallest measured n whose GPU p50 is at or below the CPU time, rounded up to a power of two; None = the
    GPU never won."""
    for row in rows:
        if row["gpu_ms"]["p50"] <= row["cpu_ms"]["median"]:
            return 1 << (row["n"] - 1).bit_length()
    return None


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--algos", default="sha256d,scrypt,x11")
    ap.add_argument("--log2n", type=int, default=20, help="shares of part (a)")
    ap.add_argument("--reps", type=int, default=1000, help="timed ShareVerify.results calls per size in part (b)")
    ap.add_argument("--cpu-cap", type=int, default=512, help="most shares hashed on the CPU per timing in part (b)")
    ap.add_argument("--skip-a", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    doc = {"tool": "tools/bench_verify_live.py", "device": args.device, "warmups": WARMUPS, "runs": RUNS,
           "reps": args.reps}
    if not args.skip_a:
        doc["a"] = part_a(args.device, args.log2n)
    doc["b"] = {}
    doc["verify_min_gpu"] = {}
    for algo in [a for a in args.algos.split(",") if a]:
        doc["b"][algo] = part_b(args.device, algo, args.reps, args.cpu_cap)
        doc["verify_min_gpu"][algo] = min_gpu_default(doc["b"][algo])
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
