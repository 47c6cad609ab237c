#!/usr/bin/env python3
"""Noise handshakes in batches, measured (docs/POOL.md "Handshakes"): where the GPU starts to win, and what a
connection storm does to the pool's event loop.

(a) The round trip of n handshakes (3n rows: e·G, e·X, s·X; three in four X ElligatorSwift, one in four x-only) for n in
    1, 8, 64, 512, 4096:
      gpu     Secp256k1Mul.mul, wall clock, p50 and p99 over --reps calls after two warm-ups
      cpu     the native secp256k1_mul_cpu on the same host, median of five after two warm-ups
      python  btccrypto.point_mul / ellswift.ecdh_x / noise.dh, the same (above 64 handshakes one run without
              warm-ups: it is linear, and 4096 take ten seconds)
(b) otd_secp256k1_mul alone, between events, at 3, 192 and 12288 rows (median of --kernel-reps launches).
(c) --storm: a pool in its own process (Noise on, one of off / cpu / cuda:0), N = 256 and 2048 Noise clients connecting
    at once from a second process that never touches the GPU (their own curve arithmetic is the native CPU twin on
    eight threads). The pool listens with a backlog of 4096, above the crowd, so that no connection waits for a TCP
    retransmission timer. Reported: the time until every client holds a channel, and the longest gap of a 1 ms
    ticker on the pool's loop.

(a) also reports one whole responder handshake in Python on this host, median of 10, per suite, with the two static·G
multiplications (before ``static_x``) and without.

``handshake_min_gpu`` is the rule of tools/bench_verify_live.py against the native CPU time. This process is the only
one with the GPU open in (a) and (b); in (c) only the pool's. Output: one JSON document (--out FILE writes it too).
"""
import argparse
import asyncio
import json
import os
import random
import struct
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_verify_live import RUNS, WARMUPS, spread  # noqa: E402

SIZES = (1, 8, 64, 512, 4096)
KERNEL_ROWS = (3, 192, 12288)
STORM = (256, 2048)
STATIC = 0x1F2E3D4C5B6A79880102030405060708090A0B0C0D0E0F101112131415161718


def handshake_rows(n: int) -> list:
    """The 3n rows of n handshakes, from a fixed seed."""
    from otedama_amd import btccrypto as ec
    from otedama_amd.ops import secp_rows as R
    from otedama_amd.ops.native import require_native

    rng = random.Random(n)
    keys = [rng.randrange(1, ec.N) for _ in range(8)]
    xs = [x for x, _p, _s in R.unpack_rows(
        require_native().secp256k1_mul_cpu(R.pack_rows([(k, R.KIND_G, b"") for k in keys])), 8)]
    rows = []
    for i in range(n):
        e = rng.randrange(1, ec.N)
        kind, point = (R.KIND_XONLY, xs[i % 8]) if i % 4 == 3 else (R.KIND_ELLSWIFT, rng.randbytes(64))
        rows += [(e, R.KIND_G, b""), (e, kind, point), (STATIC, kind, point)]
    return rows


def python_rows(rows: list) -> list:
    from otedama_amd import btccrypto as ec
    from otedama_amd.ops import secp_rows as R
    from otedama_amd.stratum import ellswift, noise

    out = []
    for scalar, kind, point in rows:
        if kind == R.KIND_G:
            out.append(ec.point_mul(ec.G, scalar)[0].to_bytes(32, "big"))
        elif kind == R.KIND_XONLY:
            out.append(noise.dh(scalar, point))
        else:
            out.append(ellswift.ecdh_x(scalar, point))
    return out


def python_handshake_ms(runs: int = 10) -> dict:
    """One whole responder handshake in Python on this host (read_message1 + write_message2), median of ``runs``:
    ``five_mul`` as before ``static_x`` existed, ``three_mul`` with it (what the pool's off path runs)."""
    import statistics

    from otedama_amd.stratum import noise as N

    out = {}
    for suite in N.SUITES:
        m1 = N.Initiator(suite=suite).write_message1()
        for name, static_x in (("five_mul", None), ("three_mul", N.static_point(STATIC))):
            times = []
            for _ in range(runs):
                t0 = time.perf_counter()
                r = N.Responder(STATIC, static_x=static_x)
                r.read_message1(m1)
                r.write_message2(b"\0" * 74)
                times.append((time.perf_counter() - t0) * 1e3)
            out[f"{suite}_{name}"] = statistics.median(times)
    return out


def timed(fn, warmups: int, runs: int) -> dict:
    times = []
    for r in range(warmups + runs):
        t0 = time.perf_counter()
        fn()
        if r >= warmups:
            times.append((time.perf_counter() - t0) * 1e3)
    return dict(spread(times), runs=runs)


def part_a(device: str, reps: int) -> list:
    from otedama_amd.ops import secp_rows as R
    from otedama_amd.ops.secp import Secp256k1Mul

    op = Secp256k1Mul(device)
    out = []
    for n in SIZES:
        rows = handshake_rows(n)
        lat = []
        for r in range(WARMUPS + reps):
            t0 = time.perf_counter()
            got = op.mul(rows)
            if r >= WARMUPS:
                lat.append((time.perf_counter() - t0) * 1e3)
        lat.sort()
        cpu = lambda: R.unpack_rows(op.native.secp256k1_mul_cpu(R.pack_rows(rows)), len(rows))  # noqa: E731
        row = {"n": n, "rows": len(rows),
               "gpu_ms": {"p50": lat[(len(lat) - 1) // 2], "p99": lat[max(0, -(-99 * len(lat) // 100) - 1)],
                          "min": lat[0], "max": lat[-1], "calls": len(lat)},
               "cpu_ms": timed(cpu, WARMUPS, RUNS),
               "python_ms": timed(lambda: python_rows(rows), *((WARMUPS, RUNS) if n <= 64 else (0, 1)))}
        row["equal"] = got == cpu() and [g[0] for g in got] == python_rows(rows)
        out.append(row)
    return out


def part_b(device: str, reps: int) -> list:
    import torch

    from otedama_amd.ops import secp_rows as R
    from otedama_amd.ops.secp import Secp256k1Mul

    op = Secp256k1Mul(device)
    out = []
    for n in KERNEL_ROWS:
        rows = handshake_rows(n // 3)
        src = torch.frombuffer(R.pack_rows(rows), dtype=torch.uint8).view(n, R.ROW_BYTES).to(device)
        dst = torch.empty((n, R.OUT_BYTES), dtype=torch.uint8, device=device)
        times = []
        for r in range(WARMUPS + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            op.launch(src, out=dst)
            b.record()
            b.synchronize()
            if r >= WARMUPS:
                times.append(a.elapsed_time(b))
        out.append({"rows": n, "kernel_ms": dict(spread(times), launches=reps)})
    return out


def min_gpu_default(rows: list):
    """The smallest measured n whose GPU p50 is at or below the native CPU time, rounded up to a power of two; None =
    the GPU never won."""
    for row in rows:
        if row["gpu_ms"]["p50"] <= row["cpu_ms"]["median"]:
            return 1 << (row["n"] - 1).bit_length()
    return None


# ---------------------------------------------------------------- (c) the storm
async def _serve(device: str) -> None:
    """The pool process: prints its address, then on a line from stdin its stats and the ticker's longest gap."""
    from otedama_amd.pool.server import PoolOptions, PoolServer

    # A listen backlog above the crowd: with asyncio's default of 100 the kernel drops what the busy loop has not
    # accepted yet, and the clients' retransmission timers (1, 3, 7, 15, 31 s) would be what the storm measures.
    start_server = asyncio.start_server
    asyncio.start_server = lambda *a, **kw: start_server(*a, **{"backlog": 4096, **kw})
    pool = PoolServer(PoolOptions(listen_v1="", job_interval=3600, block_interval=3600, fixed_difficulty=True,
                                  noise=True, handshake_device=device, handshake_min_gpu=1 if device else 0))
    await pool.start()
    gap = 0.0

    async def ticker():
        nonlocal gap
        last = time.perf_counter()
        while True:
            await asyncio.sleep(0.001)
            now = time.perf_counter()
            gap, last = max(gap, now - last), now

    tick = asyncio.ensure_future(ticker())
    loop = asyncio.get_running_loop()
    print(json.dumps({"addr": pool.addr_sv2}), flush=True)
    while True:
        line = await loop.run_in_executor(None, sys.stdin.readline)
        if not line or line.strip() == "quit":
            break
        print(json.dumps({"max_gap_ms": gap * 1e3, "handshake": pool.stats()["handshake"],
                          "rejects": pool.stats()["reject_reasons"]}), flush=True)
        gap = 0.0
    tick.cancel()
    await pool.stop()


async def _clients(addr: str, n: int) -> dict:
    """The client process: n Noise initiators (three in four ellswift) that all send message 1 first."""
    import concurrent.futures

    from otedama_amd import btccrypto as ec
    from otedama_amd.ops import secp_rows as R
    from otedama_amd.ops.native import require_native
    from otedama_amd.stratum import ellswift
    from otedama_amd.stratum import messages as M
    from otedama_amd.stratum import noise as N
    from otedama_amd.stratum.frame import FrameReader

    nat = require_native()
    threads = concurrent.futures.ThreadPoolExecutor(max_workers=8)
    loop = asyncio.get_running_loop()

    async def mul(scalar, kind, point) -> bytes:
        raw = await loop.run_in_executor(threads, nat.secp256k1_mul_cpu, R.pack_rows([(scalar, kind, point)]))
        x, _parity, status = R.unpack_rows(raw, 1)[0]
        assert status == 0
        return x

    rng = random.Random(n)
    es = [rng.randrange(1, ec.N) for _ in range(n)]
    pubs = R.unpack_rows(nat.secp256k1_mul_cpu(R.pack_rows([(e, R.KIND_G, b"") for e in es])), n)
    suites = ["legacy" if i % 4 == 3 else "ellswift" for i in range(n)]
    firsts = [ellswift.encode(int.from_bytes(x, "big")) if s == "ellswift" else x
              for (x, _p, _s), s in zip(pubs, suites)]
    h, p = addr.rsplit(":", 1)

    async def one(i: int, reader, writer) -> float:
        ell = suites[i] == "ellswift"
        k, kind = (64, R.KIND_ELLSWIFT) if ell else (32, R.KIND_XONLY)
        ss = N.SymmetricState(N.PROTOCOL_NAME_ELLSWIFT if ell else N.PROTOCOL_NAME)
        ss.mix_hash(b"")
        ss.mix_hash(firsts[i])
        ss.mix_hash(b"")
        size = struct.unpack("<H", await reader.readexactly(2))[0]
        m2 = await reader.readexactly(size)
        for key_at in (0, 1):
            if key_at == 0:
                theirs = m2[:k]
                ss.mix_hash(theirs)
            else:
                theirs = ss.decrypt_and_hash(m2[k:k + k + N.TAG])
            x = await mul(es[i], kind, theirs)
            ss.mix_key(ellswift.xdh_from_x(x, theirs, firsts[i], initiating=True) if ell else x)
        ss.decrypt_and_hash(m2[k + k + N.TAG:])
        send, recv = ss.split()
        er, ew = N.EncryptedReader(reader, recv), N.EncryptedWriter(writer, send)
        frames = FrameReader(er)
        ew.write(M.encode_message(M.SetupConnection(flags=M.FLAG_REQUIRES_VERSION_ROLLING, vendor="storm")))
        await ew.drain()
        assert isinstance(M.dispatch_frame(await frames.read_frame()), M.SetupConnectionSuccess)
        ew.write(M.encode_message(M.OpenMiningChannel(req_id=1, user="storm", nominal_hashrate=0.0)))
        await ew.drain()
        assert isinstance(M.dispatch_frame(await frames.read_frame()), M.OpenMiningChannelSuccess)
        return time.perf_counter()

    t0 = time.perf_counter()
    conns = await asyncio.gather(*(asyncio.open_connection(h, int(p)) for _ in range(n)))
    for (_r, w), m1 in zip(conns, firsts):
        w.write(struct.pack("<H", len(m1)) + m1)
    t_sent = time.perf_counter()
    done = await asyncio.gather(*(one(i, r, w) for i, (r, w) in enumerate(conns)))
    for _r, w in conns:
        w.close()
    return {"clients": n, "all_channels_ms": (max(done) - t0) * 1e3, "connect_and_send_ms": (t_sent - t0) * 1e3}


def part_c(device: str) -> list:
    me = os.path.abspath(__file__)
    out = []
    for mode in ("", "cpu", device):
        pool = subprocess.Popen([sys.executable, me, "--serve", mode or "off"], stdin=subprocess.PIPE,
                                stdout=subprocess.PIPE, text=True)
        try:
            addr = json.loads(pool.stdout.readline())["addr"]
            for n in STORM:
                res = subprocess.run([sys.executable, me, "--clients", str(n), "--addr", addr], capture_output=True,
                                     text=True, timeout=600)
                if res.returncode != 0:
                    raise RuntimeError(f"storm clients failed: {res.stderr[-2000:]}")
                row = json.loads(res.stdout.strip().splitlines()[-1])
                pool.stdin.write("stats\n")
                pool.stdin.flush()
                row.update(json.loads(pool.stdout.readline()), mode=mode or "off")
                out.append(row)
        finally:
            try:
                pool.stdin.write("quit\n")
                pool.stdin.flush()
                pool.wait(timeout=60)
            except Exception:  # noqa: BLE001 - the measurements are done; the child is ended either way
                pool.kill()
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--reps", type=int, default=1000, help="timed Secp256k1Mul.mul calls per size")
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--storm", action="store_true", help="run part (c) instead of (a) and (b)")
    ap.add_argument("--python-only", action="store_true", help="only the whole Python handshake on this host")
    ap.add_argument("--out", default="")
    ap.add_argument("--serve", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--clients", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--addr", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve is not None:
        asyncio.run(_serve("" if args.serve == "off" else args.serve))
        return 0
    if args.clients:
        print(json.dumps(asyncio.run(_clients(args.addr, args.clients))))
        return 0
    doc = {"tool": "tools/bench_handshakes.py", "device": args.device, "warmups": WARMUPS, "runs": RUNS}
    if not args.storm:
        doc["python_handshake_ms"] = python_handshake_ms()
    if args.python_only:
        pass
    elif args.storm:
        doc["storm"] = part_c(args.device)
    else:
        rows = part_a(args.device, args.reps)
        doc.update(reps=args.reps, rows=rows, handshake_min_gpu=min_gpu_default(rows),
                   kernel=part_b(args.device, args.kernel_reps))
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
