"""Share-verification rates on one MI355X, with the digest rate of the same call for context.

python tools/bench_verify.py [--algos sha256d,scrypt,x11] [--scrypt-grid N] [--cpu-shares N]
Prints one JSON line. The job is the pool's own coinbase (``BlockTemplate.coinbase_parts(8)``) with 12 merkle
branches. Per algorithm: shares/s of ``ShareVerify.launch`` (n = 2^20 for SHA-256d and X11, one full chunk for
scrypt), the time of ``otd_share_headers`` and of ``otd_share_verdict`` alone, the digests/s of the op's own
``HeaderDigest`` over the same headers, and the shares/s of ``check_shares(device=None)`` on this host. Each GPU
figure is the median of five timed launches after two warm-ups, timed with events. Nothing is gated on the numbers.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
WARMUP, TIMED = 2, 5
BRANCHES = 12
ADDR = "bc1qar0srrr7xfkvy5l643lydnw9re59gtzzwf5mdq"


def _median_ms(launch) -> float:
    import torch

    stream = torch.cuda.current_stream(DEV)
    for _ in range(WARMUP):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(TIMED):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        launch()
        t1.record(stream)
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms)


def _job():
    from otedama_amd.pool.batch import ShareJob
    from otedama_amd.pool.template import TemplateSource

    # 2^12 - 1 other transactions: a merkle path of 12 branches
    blk = TemplateSource(ADDR, n_txs=(1 << BRANCHES) - 1, seed=b"bench-verify").next_block()
    coinb1, coinb2 = blk.coinbase_parts(8)
    branches = blk.branches()
    assert len(branches) == BRANCHES
    return ShareJob(coinb1, coinb2, 8, blk.prev_hash, blk.nbits, branches)


def _gpu_rates(name: str, n: int | None, grid: int | None, job) -> dict:
    import torch

    from otedama_amd.ops.verify import ShareVerify

    op = ShareVerify(name, DEV, capacity=n if name == "x11" else None, grid=grid)
    n = n or op.digest.capacity
    prep = op.prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, job.branches)
    g = torch.Generator(device=DEV).manual_seed(1)
    recs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=DEV, generator=g)
    recs[:, 28:] = 0  # every share against target 0 of the table
    tgts = torch.full((1, 32), 0xFF, dtype=torch.uint8, device=DEV)
    tgts[0, 31] = 0x0F
    ms = _median_ms(lambda: op.launch(prep, recs, tgts))
    verdicts, digests, headers = op.launch(prep, recs, tgts)
    s = torch.cuda.current_stream(DEV).cuda_stream
    nat, jp, rp = op.native, prep.dev.data_ptr(), recs.data_ptr()
    ms_h = _median_ms(lambda: nat.launch_share_headers(jp, rp, n, headers.data_ptr(), s))
    ms_d = _median_ms(lambda: op.digest.launch(headers, out=digests))
    ms_v = _median_ms(lambda: nat.launch_share_verdict(jp, rp, digests.data_ptr(), tgts.data_ptr(), 1, n,
                                                       verdicts.data_ptr(), s))
    torch.cuda.synchronize()
    return {"n": n, "ms": round(ms, 3), "shares_per_s": round(n / ms * 1e3),
            "share_headers_ms": round(ms_h, 3), "share_verdict_ms": round(ms_v, 4),
            "digest_ms": round(ms_d, 3), "digests_per_s": round(n / ms_d * 1e3)}


def _cpu_rate(name: str, n: int, job) -> dict:
    from otedama_amd.pool.batch import check_shares

    shares = [(i.to_bytes(8, "little"), 1_700_000_000 + i, i * 2654435761, 0x20000000) for i in range(n)]
    t0 = time.perf_counter()
    check_shares(name, job, shares, [b"\xff" * 32], [0] * n, device=None)
    dt = time.perf_counter() - t0
    return {"n": n, "ms": round(dt * 1e3, 3), "shares_per_s": round(n / dt)}


def main() -> int:
    import torch

    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--algos", default="sha256d,scrypt,x11")
    ap.add_argument("--scrypt-grid", type=int, default=None, help="ROMix blocks (default: the ops default)")
    ap.add_argument("--cpu-shares", type=int, default=2000, help="shares of the check_shares(device=None) rate")
    a = ap.parse_args()
    sizes = {"sha256d": 1 << 20, "scrypt": None, "x11": 1 << 20}
    job = _job()
    res = {"metric": "share_verify_rates", "device": torch.cuda.get_device_name(0), "branches": BRANCHES,
           "coinbase_bytes": len(job.coinb1) + job.en_size + len(job.coinb2)}
    for name in a.algos.split(","):
        grid = a.scrypt_grid if name == "scrypt" else None
        r = {"verify": _gpu_rates(name, sizes[name], grid, job)}
        torch.cuda.empty_cache()  # the scrypt pad (128 GiB at the default grid) must not outlive its algorithm
        r["cpu"] = _cpu_rate(name, a.cpu_shares, job)
        res[name] = r
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
