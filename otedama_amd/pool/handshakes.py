"""Batched Noise handshakes for the running pool: the secp256k1 multiplications of concurrent Stratum V2 connections
are collected and computed as one ``secp256k1_mul`` batch, off the event loop.

A connection that has read message 1 submits the three rows of ``noise.Responder.ec_requests`` (e·G, e·X, s·X) and
waits for its batch (``pool.devicepath.MicroBatch``: ``handshake_batch_max`` handshakes, or ``handshake_batch_ms``
after the oldest one). The rows are computed on the worker thread; the event loop then finishes each handshake
(hashes, HKDF, AEAD, the ElligatorSwift encodings) and writes message 2. The worker thread owns the
``ops.secp.Secp256k1Mul`` op; with ``handshake_device="cpu"`` it runs the native ``secp256k1_mul_cpu``, which
releases the GIL. The loop, the thread, the threshold and the fall-back rules are ``pool.devicepath``'s.

A row that comes back with a nonzero status (a message 1 key that is not on the curve) fails that one handshake in
``Responder.write_message2``; the others of the batch go on. A device call that never returns holds its batch, every
later handshake and ``stop()``; each waiting connection still gives up after the handshake timeout.
"""
from __future__ import annotations

from otedama_amd.ops.secp_rows import MAX_ROWS, pack_rows, unpack_rows, wipe_scalars
from otedama_amd.pool.devicepath import PATHS, MicroBatch

ROWS_PER_HANDSHAKE = 3
assert PATHS["handshake"].batch_max_limit == MAX_ROWS // ROWS_PER_HANDSHAKE  # a full batch is one call of the op
# handshake_min_gpu = 0 resolves to this: the smallest measured number of handshakes, rounded up to a power of two, at
# which the GPU round trip (Secp256k1Mul.mul, p50) was at or below the same host's secp256k1_mul_cpu time
# (tools/bench_handshakes.py; the table is in docs/POOL.md, "Handshakes": the GPU loses at 8, 5.48 ms against 3.73 ms,
# and wins at 64, 5.38 ms against 29.7 ms).
DEFAULT_HANDSHAKE_MIN_GPU = 64


def mul_cpu(items: list) -> list:
    """The rows on the native CPU path: ``[(x, y_parity, status)]``. The packed scalars are wiped afterwards."""
    from otedama_amd.ops.native import require_native

    packed = pack_rows(items)
    try:
        return unpack_rows(require_native().secp256k1_mul_cpu(packed), len(items))
    finally:
        wipe_scalars(packed, len(items))


class HandshakeBatcher(MicroBatch):
    STOPPED = "handshake batcher stopped"

    def __init__(self, pool, device_mul=None):
        """``pool``: the PoolServer, whose ``opts.handshake_*`` configure the batcher. ``device_mul``: replaces the
        GPU path, ``device_mul(items)`` called on the worker thread."""
        super().__init__(pool, "handshake", DEFAULT_HANDSHAKE_MIN_GPU, "handshake batch", "it was computed")
        self._device_mul = device_mul

    async def submit(self, rows: list) -> list:
        """``rows``: the three rows of ``Responder.ec_requests``. Returns their ``(x, y_parity, status)`` results once
        the batch has been computed."""
        if len(rows) != ROWS_PER_HANDSHAKE:
            raise ValueError("a handshake is three rows")
        return await super().submit(rows)

    def _late(self, rows: list) -> list:
        self.cpu_handshakes += 1
        return mul_cpu(rows)

    async def _process(self, batch: list) -> list:
        items = [row for rows in batch for row in rows]

        def on_device():
            if self._device_mul is None:
                from otedama_amd.ops.secp import Secp256k1Mul  # imports torch

                self._device_mul = Secp256k1Mul(self.device).mul
            return self._device_mul(items)

        results, ran = await self.call_async(len(batch), on_device, lambda: mul_cpu(items), cpu_only=self._closing)
        if len(results) != len(items):
            raise RuntimeError(f"secp256k1 batch: {len(items)} rows in, {len(results)} out")
        self.batches += 1
        self.last_batch = len(batch)
        self.max_batch = max(self.max_batch, len(batch))
        self.gpu_handshakes += len(batch) if ran else 0
        self.cpu_handshakes += 0 if ran else len(batch)
        return [results[k:k + ROWS_PER_HANDSHAKE] for k in range(0, len(items), ROWS_PER_HANDSHAKE)]
