"""Micro-batched share validation for the running pool: concurrent ``PoolServer.validate_async`` submits are
collected and judged as one ``validate_many``-style batch.

A flush (``pool.devicepath.MicroBatch``: ``verify_batch_max`` submits, or ``verify_batch_ms`` after the oldest one)
runs the three stages of ``validate_many``: the field checks and the grouping on the event loop, the headers and
hashes on the worker thread, ``_finish`` in order back on the loop. Batches finish strictly in submission order, and
``_finish`` repeats the stale and duplicate checks, so a block or job change while a batch was being hashed is judged
as sequential ``validate`` would judge it at finish time.

The worker thread owns the ``ops.verify.ShareVerify`` ops; with ``verify_device="cpu"`` it runs
``check_shares(device=None)``, as it does for a job over the job block's limits. The threshold ``verify_min_gpu``
counts a flush's survivors of the field checks. The loop, the thread and the fall-back rules are
``pool.devicepath``'s; a device call that never returns holds its batch, every later submit and ``close()``.
"""
from __future__ import annotations

from otedama_amd.pool.batch import check_shares, prepared_or_none
from otedama_amd.pool.devicepath import (NEVER, MicroBatch, device_failed, forget_device_errors,  # noqa: F401
                                         valid_device)  # re-exported

# verify_min_gpu = 0 resolves to these: the smallest measured batch, rounded up to a power of two, at which the GPU
# round trip (ShareVerify.results, p50) was at or below the same host's check_shares(device=None) time
# (tools/bench_verify_live.py; the table is in docs/POOL.md). An algorithm not measured stays on the CPU.
DEFAULT_MIN_GPU = {"sha256d": 64, "scrypt": 64, "x11": 8}


class DeviceHasher:
    """Stage 2 on a GPU: ``ShareVerify.results`` per group. Created and called on the batcher's worker thread only.
    It keeps the prepared job block of the last few groups: every job of one block is the same group."""

    KEEP_JOBS = 4

    def __init__(self, algorithm: str, device: str):
        from otedama_amd.ops.verify import ShareVerify  # imports torch

        self.algorithm = algorithm
        self.op = ShareVerify(algorithm, device)
        self._prepared: dict = {}  # group key -> PreparedJob, or None for a job over the block's limits

    def _prepare(self, job):
        key = (job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, tuple(job.branches))
        if key not in self._prepared:
            while len(self._prepared) >= self.KEEP_JOBS:
                self._prepared.pop(next(iter(self._prepared)))
            self._prepared[key] = prepared_or_none(self.op.prepare, job)
        return self._prepared[key]

    def takes(self, job) -> bool:
        """False for a job over the job block's limits: the batcher hashes that group on the CPU and counts it so."""
        return self._prepare(job) is not None

    def __call__(self, job, shares, targets, target_indices):
        prepared = self._prepare(job)
        if prepared is None:
            return check_shares(self.algorithm, job, shares, targets, target_indices)
        return self.op.results(prepared, shares, targets, target_indices)


class ShareBatcher(MicroBatch):
    STOPPED = "share batcher stopped"

    def __init__(self, pool, device_hasher=None):
        """``pool``: the PoolServer, whose ``opts.verify_*`` configure the batcher. ``device_hasher``: replaces the
        GPU path, ``hasher(job, shares, targets, target_indices)`` called on the worker thread; if it has a
        ``takes(job)`` method, a group it does not take is hashed and counted on the CPU.

        ``submit(item, t_received)`` takes ``item``: ``(worker, job_id, extranonce, ntime, nonce, version)`` and
        returns its Verdict once its batch has finished."""
        super().__init__(pool, "verify", DEFAULT_MIN_GPU.get(pool.algo.name, NEVER), "share verification",
                         "the batch was hashed")
        self._device_hasher = device_hasher

    def _late(self, item: tuple):
        return self.pool.validate(*item)

    async def _process(self, items: list) -> list:
        pool, algorithm = self.pool, self.pool.algo.name
        checked = pool._check_fields(items)
        plan = pool._group_survivors(items, checked)
        survivors = sum(len(g[1]) for g in plan)
        on_gpu = 0

        def cpu(job, shares, targets, tidx):
            return check_shares(algorithm, job, shares, targets, tidx)

        def dev(job, shares, targets, tidx):
            nonlocal on_gpu
            takes = getattr(self._device_hasher, "takes", None)
            if takes is not None and not takes(job):
                return cpu(job, shares, targets, tidx)
            res = self._device_hasher(job, shares, targets, tidx)
            on_gpu += len(shares)
            return res

        def on_device():
            if self._device_hasher is None:
                self._device_hasher = DeviceHasher(algorithm, self.device)
            return pool._hash_groups(plan, dev)

        # stage 2, on the worker thread: item index -> (header, hash)
        hashed, ran = await self.call_async(survivors, on_device, lambda: pool._hash_groups(plan, cpu),
                                            cpu_only=self._closing)
        on_gpu = on_gpu if ran else 0
        self.batches += 1
        self.last_batch = len(items)
        self.max_batch = max(self.max_batch, len(items))
        self.gpu_shares += on_gpu
        self.cpu_shares += survivors - on_gpu
        return pool._finish_many(items, checked, hashed)
