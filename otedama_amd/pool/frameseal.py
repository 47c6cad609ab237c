"""A job's Noise frames for the running pool: the ChaCha20-Poly1305 seals of every frame of one fan-out in one
``pool.batch.seal_frames`` call instead of one ``CipherState.encrypt`` per message on the event loop.

``PoolServer._make_job`` wraps its Stratum V2 fan-out in :meth:`FrameSealer.corked`. Inside, every connection's
``noise.EncryptedWriter`` queues its frames unsealed, each with its key and the counter it reserved. On the way out
the whole batch is sealed at once and each ``u16 length || sealed`` goes to its connection's transport in queue order,
so every peer sees its counters in order; then the writers are uncorked. The call is synchronous, as ``_make_job``
is: it hands the work to one dedicated worker thread and waits for it. That thread creates and owns the
``ops.seal.FrameSeal`` op: torch and the GPU are first touched there, and importing this module imports neither. With
``seal_device="cpu"`` the thread runs the native ``aead_seal_many_cpu``, which releases the GIL.

Only the job fan-out is corked. Replies to submits, ``SetTarget`` and channel opens are sealed frame by frame.

Fallbacks: a batch of fewer frames than ``seal_min_gpu`` goes to the native CPU path, a frame over the op's limit of
2048 bytes to ``utils.aead.seal`` (inside ``seal_frames``). Any exception from the device path sends that batch to
the CPU, is logged and counted, and turns the device off in ``pool.devicepath``, the process-wide switch the share
verifier, the job fan-out, the template tree and the handshakes use too. A reserved counter that is never sent
desynchronises its connection for good, so when the CPU path fails as well the connections of that batch are closed.

The device call has no time limit: one that never returns (a hung GPU) holds ``_make_job``, and with it the event
loop, for good. A blocked ``hipStreamSynchronize`` cannot be abandoned safely from Python, so none is attempted.
"""
from __future__ import annotations

import concurrent.futures
import contextlib
import struct
import time

from otedama_amd.pool.batch import seal_frames
from otedama_amd.pool.devicepath import DevicePath

NEVER = 1 << 24  # above any batch: a call takes fewer than 2^24 frames
# seal_min_gpu = 0 resolves to this: the smallest measured number of frames, rounded up to a power of two, at which the
# GPU round trip (FrameSeal.seal, p50) was at or below the same host's seal_frames(device="cpu") time
# (tools/bench_seal_frames.py; the table is in docs/POOL.md, "Frame sealing": the GPU loses at 64, 0.075 ms against
# 0.059 ms, and wins at 512, 0.279 ms against 0.422 ms). NEVER stands for "the GPU wins at no measured size".
DEFAULT_SEAL_MIN_GPU = 512


class FrameSealer:
    def __init__(self, pool, device_seal=None):
        """``pool``: the PoolServer, whose ``opts.seal_*`` configure the sealer. ``device_seal``: replaces the
        configured path, ``device_seal(frames)`` called on the worker thread: the GPU path of a ``cuda:N`` sealer (the
        fall-back stays the native call), the native call of a ``cpu`` one."""
        o = pool.opts
        self.path = DevicePath("seal_device", o.seal_device)
        if o.seal_min_gpu < 0:
            raise ValueError("seal_min_gpu must not be negative")
        self.pool = pool
        self.device = self.path.device
        self.min_gpu = int(o.seal_min_gpu) or DEFAULT_SEAL_MIN_GPU
        self._device_seal = device_seal
        self._worker = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="otedama-pool-seal")
        self.batches = self.gpu_frames = self.cpu_frames = self.last_frames = 0
        self.last_ms = 0.0

    def stats(self) -> dict:
        return {"device": self.device, "enabled": self.path.enabled, "batches": self.batches,
                "gpu_frames": self.gpu_frames, "cpu_frames": self.cpu_frames, "last_frames": self.last_frames,
                "last_ms": self.last_ms, "device_errors": self.path.device_errors}

    def close(self) -> None:
        self._worker.shutdown(wait=True)

    @contextlib.contextmanager
    def corked(self, conns):
        """Cork the Noise writer of every connection of ``conns`` (``c.writer``; a writer that is not a keyed
        ``EncryptedWriter`` is left alone) for the body; afterwards, whatever the body raised, seal what they queued
        in one call, write it out and uncork."""
        batch: list = []
        corked = []
        for c in conns:
            cork = getattr(c.writer, "cork", None)
            if cork is not None and cork(batch):
                corked.append(c.writer)
        try:
            yield batch
        finally:
            try:
                self.flush(batch)
            finally:
                for w in corked:
                    w.uncork()

    def flush(self, batch: list) -> None:
        """``batch``: ``(writer, key, counter, plaintext)`` entries in queue order. Seals them in one call and writes
        each frame to its writer's transport. If no path can seal them, their connections are closed."""
        if not batch:
            return
        try:
            sealed = self.seal([(key, counter, plain) for _w, key, counter, plain in batch])
            if len(sealed) != len(batch):
                raise RuntimeError(f"frame seal: {len(batch)} frames in, {len(sealed)} out")
        except Exception as exc:  # noqa: BLE001 - the counters are spent: these connections cannot go on
            pool = self.pool
            pool.log("error", f"pool[{pool.algo.name}]: sealing {len(batch)} job frames failed ({exc!r}); their "
                              f"connections are closed")
            for w in {id(e[0]): e[0] for e in batch}.values():
                try:
                    w.close()
                except Exception:  # noqa: BLE001
                    pass
            return
        for (w, _key, _counter, _plain), s in zip(batch, sealed):
            try:
                w.transport.write(struct.pack("<H", len(s)) + s)
            except Exception:  # noqa: BLE001 - a connection that is going away, as in _V2Conn._send
                pass

    def seal(self, frames: list) -> list:
        """``(key32, counter, plaintext)`` frames; the sealed bytes of each, in order. Waits for the worker thread."""
        if not frames:
            return []
        t0 = time.perf_counter()
        on_device = self.path.on and len(frames) >= self.min_gpu
        sealed, on_gpu, error = self._worker.submit(self._compute, frames, on_device).result()
        if error is not None:  # the worker thread has already counted it and put the device on the failed list
            pool = self.pool
            pool.log("error", f"pool[{pool.algo.name}]: frame sealing on {self.device} failed ({error!r}); the frames "
                              f"were sealed on the CPU and the device path is off for this process")
        self.batches += 1
        self.last_frames = len(frames)
        self.gpu_frames += on_gpu
        self.cpu_frames += len(frames) - on_gpu
        self.last_ms = (time.perf_counter() - t0) * 1e3
        return sealed

    def _compute(self, frames: list, on_device: bool):
        """On the worker thread: ``(sealed, frames sealed on the device, device error)``."""
        def cpu():
            return seal_frames(frames, "cpu")

        if not self.path.gpu and self._device_seal is not None:
            return self._device_seal(frames), 0, None
        if not on_device:
            return cpu(), 0, None
        device = self._device_seal or (lambda f: seal_frames(f, self.device))
        sealed, ran, error = self.path.run(lambda: device(frames), cpu)
        return sealed, len(frames) if ran else 0, error
