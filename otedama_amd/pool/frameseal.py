"""A job's Noise frames for the running pool: the ChaCha20-Poly1305 seals of every frame of one fan-out in one
``pool.batch.seal_frames`` call instead of one ``CipherState.encrypt`` per message on the event loop.

``PoolServer._make_job`` wraps its Stratum V2 fan-out in :meth:`FrameSealer.corked`. Inside, every connection's
``noise.EncryptedWriter`` queues its frames unsealed, each with its key and the counter it reserved. On the way out
the whole batch is sealed at once and each ``u16 length || sealed`` goes to its connection's transport in queue order,
so every peer sees its counters in order; then the writers are uncorked. The call is synchronous, as ``_make_job``
is: a device call that never returns holds ``_make_job``, and with it the event loop, for good. The worker thread owns
the ``ops.seal.FrameSeal`` op; with ``seal_device="cpu"`` it runs the native ``aead_seal_many_cpu``, which releases
the GIL. A frame over the op's limit of 2048 bytes goes to ``utils.aead.seal`` (inside ``seal_frames``). The thread,
the threshold and the fall-back rules are ``pool.devicepath``'s.

Only the job fan-out is corked. Replies to submits, ``SetTarget`` and channel opens are sealed frame by frame.

A reserved counter that is never sent desynchronises its connection for good, so when the CPU path fails as well the
connections of that batch are closed.
"""
from __future__ import annotations

import contextlib
import struct

from otedama_amd.pool.batch import seal_frames
from otedama_amd.pool.devicepath import DeviceWork

# seal_min_gpu = 0 resolves to this: the smallest measured number of frames, rounded up to a power of two, at which the
# GPU round trip (FrameSeal.seal, p50) was at or below the same host's seal_frames(device="cpu") time
# (tools/bench_seal_frames.py; the table is in docs/POOL.md, "Frame sealing": the GPU loses at 64, 0.075 ms against
# 0.059 ms, and wins at 512, 0.279 ms against 0.422 ms).
DEFAULT_SEAL_MIN_GPU = 512


class FrameSealer(DeviceWork):
    def __init__(self, pool, device_seal=None):
        """``pool``: the PoolServer, whose ``opts.seal_*`` configure the sealer. ``device_seal``: replaces the
        configured path, ``device_seal(frames)`` called on the worker thread: the GPU path of a ``cuda:N`` sealer (the
        fall-back stays the native call), the native call of a ``cpu`` one (counted as the CPU's)."""
        super().__init__(pool, "seal", DEFAULT_SEAL_MIN_GPU, "frame sealing", "the frames were sealed")
        self._device_seal = device_seal

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

        def on_device():
            return self._device_seal(frames) if self._device_seal else seal_frames(frames, self.device)

        def on_cpu():  # seal_frames is this module's, looked up when it is called
            return self._device_seal(frames) if self._device_seal and not self.path.gpu else seal_frames(frames, "cpu")

        sealed, ran = self.call(len(frames), on_device, on_cpu)
        self.batches += 1
        self.last_frames = len(frames)
        self.gpu_frames += len(frames) if ran else 0
        self.cpu_frames += 0 if ran else len(frames)
        return sealed
