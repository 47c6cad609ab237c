"""Digest-op rates on one MI355X, with the search rates of the same call for context.

python tools/bench_digest.py [--algos sha256d,scrypt,x11] [--scrypt-grid N]
Prints one JSON line. Per algorithm: digests/s of ``HeaderDigest.launch`` (n = 2^22 for SHA-256d, 2^20 for X11, one
full-capacity chunk for scrypt) and hashes/s of the search op (SHA-256d: the single-header kernel over 2^32 nonces;
scrypt: one full batch on the same grid; X11: 2^20 nonces), each the median of five timed launches after two
warm-ups, timed with events. Nothing is gated on the numbers.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
WARMUP, TIMED = 2, 5


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


def _digest_rate(name: str, n: int | None, grid: int | None) -> dict:
    import torch

    from otedama_amd.ops.digest import HeaderDigest

    op = HeaderDigest(name, DEV, capacity=n if name == "x11" else None, grid=grid)
    n = n or op.capacity
    g = torch.Generator(device=DEV).manual_seed(1)
    headers = torch.randint(0, 256, (n, 80), dtype=torch.uint8, device=DEV, generator=g)
    out = torch.empty((n, 32), dtype=torch.uint8, device=DEV)
    ms = _median_ms(lambda: op.launch(headers, out=out))
    return {"n": n, "ms": round(ms, 3), "digests_per_s": round(n / ms * 1e3)}


def _search_rate(name: str, grid: int | None) -> dict:
    from otedama_amd.ops import search

    hdr, target = bytes(range(80)), bytes(32)  # target 0: no hits
    if name == "sha256d":
        s = search.Sha256dSearch(DEV)
        count = 1 << 32
        params = s.prepare(hdr, target)
    elif name == "scrypt":
        s = search.ScryptSearch(DEV, grid=grid)
        count = s.batch
        params = s.prepare(hdr, target)
    else:
        count = 1 << 20
        s = search.X11Search(DEV, batch=count)
        params = s.prepare(hdr, target)
    ms = _median_ms(lambda: s.launch(params, 0, count))
    return {"n": count, "ms": round(ms, 3), "hashes_per_s": round(count / ms * 1e3)}


def main() -> int:
    import torch

    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--algos", default="sha256d,scrypt,x11")
    ap.add_argument("--scrypt-grid", type=int, default=None, help="ROMix blocks (default: the ops default)")
    a = ap.parse_args()
    sizes = {"sha256d": 1 << 22, "scrypt": None, "x11": 1 << 20}
    res = {"metric": "digest_rates", "device": torch.cuda.get_device_name(0)}
    for name in a.algos.split(","):
        grid = a.scrypt_grid if name == "scrypt" else None
        r = {"digest": _digest_rate(name, sizes[name], grid)}
        torch.cuda.empty_cache()  # the scrypt pads (128 GiB each at the default grid) must not coexist
        r["search"] = _search_rate(name, grid)
        torch.cuda.empty_cache()
        res[name] = r
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
