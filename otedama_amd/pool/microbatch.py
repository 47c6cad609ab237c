"""Micro-batched share validation for the running pool: concurrent ``PoolServer.validate_async`` submits are
collected and judged as one ``validate_many``-style batch.

A submit waits as ``(item, future, t_received)``. A flush takes up to ``verify_batch_max`` submits in arrival order
when that many are pending, or ``verify_batch_ms`` after the oldest one arrived, and runs the three stages of
``validate_many``: the field checks and the grouping on the event loop, the headers and hashes on one dedicated
worker thread, ``_finish`` in order back on the loop. One batch is in flight at a time; submits that arrive meanwhile
gather for the next one, so batches finish strictly in submission order, and ``_finish`` repeats the stale and
duplicate checks, so a block or job change while a batch was being hashed is judged as sequential ``validate`` would
judge it at finish time.

The worker thread creates and owns the ``ops.verify.ShareVerify`` ops: torch and the GPU are first touched there,
and importing this module imports neither. With ``verify_device="cpu"`` the thread runs
``check_shares(device=None)``.

Fallbacks: a flush with fewer survivors than ``verify_min_gpu`` and a job over the job block's limits are hashed on
the CPU. Any exception from the device path sends that batch to the CPU, is logged and counted, and turns the device
path off for the rest of the process: a GPU that has faulted is not used again, by this batcher or by any other in
the process, nor by the job fan-out (the switch is ``pool.devicepath``'s, per device; the batcher's share of it is
its :class:`~otedama_amd.pool.devicepath.DevicePath`). ``close()`` flushes what is pending on the CPU and resolves
every future.

Stage 2 has no time limit: a device call that never returns (a hung GPU) holds its batch, every later submit and
``close()``. A blocked ``hipStreamSynchronize`` cannot be abandoned safely from Python, so none is attempted.
"""
from __future__ import annotations

import asyncio
import concurrent.futures
import time
from collections import deque

from otedama_amd.pool.batch import check_shares, prepared_or_none
from otedama_amd.pool.devicepath import (DevicePath, device_failed, forget_device_errors,  # noqa: F401 - re-exported
                                         valid_device)

# verify_min_gpu = 0 resolves to these: the smallest measured batch, rounded up to a power of two, at which the GPU
# round trip (ShareVerify.results, p50) was at or below the same host's check_shares(device=None) time
# (tools/bench_verify_live.py; the table is in docs/POOL.md).
NEVER = 1 << 31  # above any batch: the GPU never won up to 4096 shares
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


class ShareBatcher:
    def __init__(self, pool, device_hasher=None):
        """``pool``: the PoolServer, whose ``opts.verify_*`` configure the batcher. ``device_hasher``: replaces the
        GPU path, ``hasher(job, shares, targets, target_indices)`` called on the worker thread; if it has a
        ``takes(job)`` method, a group it does not take is hashed and counted on the CPU."""
        o = pool.opts
        self.path = DevicePath("verify_device", o.verify_device)
        if o.verify_batch_ms <= 0 or o.verify_batch_max < 1 or o.verify_min_gpu < 0:
            raise ValueError("verify_batch_ms and verify_batch_max must be positive, verify_min_gpu not negative")
        self.pool = pool
        self.device = self.path.device
        self.batch_s = o.verify_batch_ms / 1e3
        self.batch_max = int(o.verify_batch_max)
        self.min_gpu = int(o.verify_min_gpu) or DEFAULT_MIN_GPU.get(pool.algo.name, NEVER)
        self._device_hasher = device_hasher
        self._pending: deque = deque()  # (item, future, t_received)
        self._wake = asyncio.Event()
        self._closing = False
        self._worker = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="otedama-pool-verify")
        self._task = asyncio.ensure_future(self._run())
        self.batches = self.gpu_shares = self.cpu_shares = self.last_batch = self.max_batch = 0

    def stats(self) -> dict:
        return {"device": self.device, "enabled": self.path.enabled, "batches": self.batches,
                "gpu_shares": self.gpu_shares, "cpu_shares": self.cpu_shares, "last_batch": self.last_batch,
                "max_batch": self.max_batch, "device_errors": self.path.device_errors}

    async def submit(self, item: tuple, t_received: float):
        """``item``: ``(worker, job_id, extranonce, ntime, nonce, version)``; ``t_received``: ``time.perf_counter()``
        when the submit arrived. Returns its Verdict once its batch has finished."""
        if self._closing:  # after close(): nothing is dropped, the share is judged on its own
            return self.pool.validate(*item)
        fut = asyncio.get_running_loop().create_future()
        self._pending.append((item, fut, t_received))
        if len(self._pending) == 1 or len(self._pending) == self.batch_max:
            self._wake.set()  # the runner sleeps towards the oldest submit's deadline: only these two move it
        return await fut

    async def close(self) -> None:
        """Flush what is pending on the CPU, resolve every future, end the worker thread."""
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
        items = [b[0] for b in batch]
        pool = self.pool
        try:
            checked = pool._check_fields(items)
            plan = pool._group_survivors(items, checked)
            survivors = sum(len(g[1]) for g in plan)
            on_device = self.path.on and not self._closing and survivors >= self.min_gpu
            hashed, on_gpu, error = await asyncio.get_running_loop().run_in_executor(
                self._worker, self._hash, plan, on_device)
            if error is not None:  # the worker thread has already counted it and put the device on the failed list
                pool.log("error", f"pool[{pool.algo.name}]: share verification on {self.device} failed ({error!r}); "
                                  f"the batch was hashed on the CPU and the device path is off for this process")
            self.batches += 1
            self.last_batch = len(batch)
            self.max_batch = max(self.max_batch, len(batch))
            self.gpu_shares += on_gpu
            self.cpu_shares += survivors - on_gpu
            verdicts = pool._finish_many(items, checked, hashed)
        except BaseException as exc:  # no future is left unresolved, whatever failed
            for _item, fut, _t in batch:
                if not fut.done():
                    fut.set_exception(exc if isinstance(exc, Exception) else RuntimeError("share batcher stopped"))
            if not isinstance(exc, Exception):
                raise
            return
        for (_item, fut, _t), v in zip(batch, verdicts):
            if not fut.done():  # a submitter that went away cancelled its future
                fut.set_result(v)

    def _hash(self, plan: list, on_device: bool):
        """Stage 2, on the worker thread: ``(item index -> (header, hash), shares hashed on the device, device
        error)``."""
        algorithm = self.pool.algo.name

        def cpu(job, shares, targets, tidx):
            return check_shares(algorithm, job, shares, targets, tidx)

        if not on_device:
            return self.pool._hash_groups(plan, cpu), 0, None
        on_gpu = 0

        def dev(job, shares, targets, tidx):
            nonlocal on_gpu
            takes = getattr(self._device_hasher, "takes", None)
            if takes is not None and not takes(job):
                return cpu(job, shares, targets, tidx)
            res = self._device_hasher(job, shares, targets, tidx)
            on_gpu += len(shares)
            return res

        def on_dev():
            if self._device_hasher is None:
                self._device_hasher = DeviceHasher(algorithm, self.device)
            return self.pool._hash_groups(plan, dev)

        hashed, ran, error = self.path.run(on_dev, lambda: self.pool._hash_groups(plan, cpu))
        return hashed, on_gpu if ran else 0, error
