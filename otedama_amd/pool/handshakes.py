"""Batched Noise handshakes for the running pool: the secp256k1 multiplications of concurrent Stratum V2 connections
are collected and computed as one ``secp256k1_mul`` batch, off the event loop.

A connection that has read message 1 submits the three rows of ``noise.Responder.ec_requests`` (e·G, e·X, s·X) and
waits as ``(rows, future, t_received)``. A flush takes up to ``handshake_batch_max`` handshakes in arrival order when
that many are pending, or ``handshake_batch_ms`` after the oldest one arrived, and computes their rows on one dedicated
worker thread; the event loop then finishes each handshake (hashes, HKDF, AEAD, the ElligatorSwift encodings) and
writes message 2. One batch is in flight at a time; handshakes that arrive meanwhile gather for the next one.

The worker thread creates and owns the ``ops.secp.Secp256k1Mul`` op: torch and the GPU are first touched there, and
importing this module imports neither. With ``handshake_device="cpu"`` the thread runs the native
``secp256k1_mul_cpu``, which releases the GIL.

Fallbacks: a flush of fewer handshakes than ``handshake_min_gpu`` goes to the native CPU path. Any exception from the
device path sends that batch to the CPU, is logged and counted, and turns the device off in ``pool.devicepath``, the
process-wide switch the share verifier, the job fan-out and the template tree use too. A row that comes back with a
nonzero status (a message 1 key that is not on the curve) fails that one handshake in ``Responder.write_message2``;
the others of the batch go on. ``stop()`` computes what is pending on the CPU and resolves every future.

The device call has no time limit: one that never returns (a hung GPU) holds its batch, every later handshake and
``stop()``; each waiting connection still gives up after the handshake timeout. A blocked ``hipStreamSynchronize``
cannot be abandoned safely from Python, so none is attempted.
"""
from __future__ import annotations

import asyncio
import concurrent.futures
import time
from collections import deque

from otedama_amd.ops.secp_rows import MAX_ROWS, pack_rows, unpack_rows, wipe_scalars
from otedama_amd.pool.devicepath import DevicePath

ROWS_PER_HANDSHAKE = 3
NEVER = 1 << 31  # above any batch
# handshake_min_gpu = 0 resolves to this: the smallest measured number of handshakes, rounded up to a power of two, at
# which the GPU round trip (Secp256k1Mul.mul, p50) was at or below the same host's secp256k1_mul_cpu time
# (tools/bench_handshakes.py; the table is in docs/POOL.md, "Handshakes": the GPU loses at 8, 5.48 ms against 3.73 ms,
# and wins at 64, 5.38 ms against 29.7 ms). NEVER stands for "the GPU wins at no measured size".
DEFAULT_HANDSHAKE_MIN_GPU = 64


def mul_cpu(items: list) -> list:
    """The rows on the native CPU path: ``[(x, y_parity, status)]``. The packed scalars are wiped afterwards."""
    from otedama_amd.ops.native import require_native

    packed = pack_rows(items)
    try:
        return unpack_rows(require_native().secp256k1_mul_cpu(packed), len(items))
    finally:
        wipe_scalars(packed, len(items))


class HandshakeBatcher:
    def __init__(self, pool, device_mul=None):
        """``pool``: the PoolServer, whose ``opts.handshake_*`` configure the batcher. ``device_mul``: replaces the
        GPU path, ``device_mul(items)`` called on the worker thread."""
        o = pool.opts
        self.path = DevicePath("handshake_device", o.handshake_device)
        if o.handshake_batch_ms <= 0 or o.handshake_batch_max < 1 or o.handshake_min_gpu < 0:
            raise ValueError("handshake_batch_ms and handshake_batch_max must be positive, handshake_min_gpu not "
                             "negative")
        if o.handshake_batch_max * ROWS_PER_HANDSHAKE > MAX_ROWS:
            raise ValueError(f"handshake_batch_max must be at most {MAX_ROWS // ROWS_PER_HANDSHAKE}")
        self.pool = pool
        self.device = self.path.device
        self.batch_s = o.handshake_batch_ms / 1e3
        self.batch_max = int(o.handshake_batch_max)
        self.min_gpu = int(o.handshake_min_gpu) or DEFAULT_HANDSHAKE_MIN_GPU
        self._device_mul = device_mul
        self._pending: deque = deque()  # (rows, future, t_received)
        self._wake = asyncio.Event()
        self._closing = False
        self._worker = concurrent.futures.ThreadPoolExecutor(max_workers=1,
                                                             thread_name_prefix="otedama-pool-handshake")
        self._task = asyncio.ensure_future(self._run())
        self.batches = self.gpu_handshakes = self.cpu_handshakes = self.last_batch = self.max_batch = 0
        self.last_ms = 0.0

    def stats(self) -> dict:
        return {"device": self.device, "enabled": self.path.enabled, "batches": self.batches,
                "gpu_handshakes": self.gpu_handshakes, "cpu_handshakes": self.cpu_handshakes,
                "last_batch": self.last_batch, "max_batch": self.max_batch, "last_ms": self.last_ms,
                "device_errors": self.path.device_errors}

    async def submit(self, rows: list) -> list:
        """``rows``: the three rows of ``Responder.ec_requests``. Returns their ``(x, y_parity, status)`` results once
        the batch has been computed."""
        if len(rows) != ROWS_PER_HANDSHAKE:
            raise ValueError("a handshake is three rows")
        if self._closing:  # after stop(): nothing is dropped, the handshake is computed on its own
            self.cpu_handshakes += 1
            return mul_cpu(rows)
        fut = asyncio.get_running_loop().create_future()
        self._pending.append((rows, fut, time.perf_counter()))
        if len(self._pending) == 1 or len(self._pending) == self.batch_max:
            self._wake.set()  # the runner sleeps towards the oldest handshake's deadline: only these two move it
        return await fut

    async def stop(self) -> None:
        """Compute what is pending on the CPU, resolve every future, end the worker thread."""
        self._closing = True
        self._wake.set()
        await self._task
        self._worker.shutdown(wait=True)

    async def _run(self) -> None:
        while True:
            if not self._pending:
                if self._closing:
                    return
                self._wake.clear()
                await self._wake.wait()
                continue
            if len(self._pending) < self.batch_max and not self._closing:
                wait = self._pending[0][2] + self.batch_s - time.perf_counter()
                if wait > 0:
                    self._wake.clear()
                    try:
                        await asyncio.wait_for(self._wake.wait(), wait)
                    except asyncio.TimeoutError:
                        pass
                    continue
            await self._flush()

    async def _flush(self) -> None:
        batch = [self._pending.popleft() for _ in range(min(self.batch_max, len(self._pending)))]
        pool = self.pool
        t0 = time.perf_counter()
        try:
            items = [row for rows, _fut, _t in batch for row in rows]
            on_device = self.path.on and not self._closing and len(batch) >= self.min_gpu
            results, ran, error = await asyncio.get_running_loop().run_in_executor(
                self._worker, self._compute, items, on_device)
            if error is not None:  # the worker thread has already counted it and put the device on the failed list
                pool.log("error", f"pool[{pool.algo.name}]: handshake batch on {self.device} failed ({error!r}); it "
                                  f"was computed on the CPU and the device path is off for this process")
            if len(results) != len(items):
                raise RuntimeError(f"secp256k1 batch: {len(items)} rows in, {len(results)} out")
            self.batches += 1
            self.last_batch = len(batch)
            self.max_batch = max(self.max_batch, len(batch))
            self.gpu_handshakes += len(batch) if ran else 0
            self.cpu_handshakes += 0 if ran else len(batch)
            self.last_ms = (time.perf_counter() - t0) * 1e3
        except BaseException as exc:  # no future is left unresolved, whatever failed
            for _rows, fut, _t in batch:
                if not fut.done():
                    fut.set_exception(exc if isinstance(exc, Exception) else RuntimeError("handshake batcher stopped"))
            if not isinstance(exc, Exception):
                raise
            return
        for k, (_rows, fut, _t) in enumerate(batch):
            if not fut.done():  # a connection that gave up cancelled its future
                fut.set_result(results[k * ROWS_PER_HANDSHAKE:(k + 1) * ROWS_PER_HANDSHAKE])

    def _compute(self, items: list, on_device: bool):
        """On the worker thread: ``(results, ran on the device, device error)``."""
        if not on_device:
            return mul_cpu(items), False, None

        def on_dev():
            if self._device_mul is None:
                from otedama_amd.ops.secp import Secp256k1Mul  # imports torch

                self._device_mul = Secp256k1Mul(self.device).mul
            return self._device_mul(items)

        return self.path.run(on_dev, lambda: mul_cpu(items))
