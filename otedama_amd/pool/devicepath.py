"""The core under the pool's five CPU-or-GPU paths. Importing this module imports neither torch nor the native
extension.

=========== ====================================== ==============================================
option      path                                   built on
=========== ====================================== ==============================================
verify_*    ``microbatch.ShareBatcher``            :class:`MicroBatch`: concurrent submits
handshake_* ``handshakes.HandshakeBatcher``        :class:`MicroBatch`: concurrent handshakes
job_*       ``jobroots.JobRoots``                  :class:`DeviceWork`: one call a job
template_*  ``templatetree.TemplateTree``          :class:`DeviceWork`: one call a template
seal_*      ``frameseal.FrameSealer``              :class:`DeviceWork`: one call a job
=========== ====================================== ==============================================

:data:`PATHS` declares each path's options and stats keys once; config.py, the CLI and ``PoolServer`` read it.

The rules every path shares, stated here and nowhere else:

* Work is handed to the path's one worker thread. That thread makes and owns the op: torch and the GPU are first
  touched there.
* Work of fewer units than ``<prefix>_min_gpu`` (0 = the path's measured default) runs on the CPU.
* The event loop chooses the device; the worker thread reads the switch again before it uses it
  (:meth:`DevicePath.run`).
* Whatever the device path raises sends that work to the CPU, is logged and counted on the path that hit it, and
  turns the device off: the switch is the process's, per device, so a GPU that has faulted for one path is not used
  again by that path or by any other in the process (``otedama pool --algorithms a,b`` runs one pool per algorithm
  on the same device).
* A device call has no time limit: one that never returns (a hung GPU) holds its caller, and ``close()``. A blocked
  ``hipStreamSynchronize`` cannot be abandoned safely from Python, so none is attempted.
"""
from __future__ import annotations

import asyncio
import concurrent.futures
import re
import time
from collections import deque
from dataclasses import dataclass

_DEVICE_RE = re.compile(r"^(cpu|cuda:\d+)$")

# A min_gpu that sends every call to the CPU ("the GPU wins at no measured size"). It must exceed the units of any one
# call; the largest is a flush of verify_batch_max survivors, which has no configured bound but is a list in memory.
NEVER = 1 << 31


def valid_device(device: str) -> bool:
    """``""`` (off), ``cpu`` or ``cuda:N``. The one statement of the grammar: config.py and the CLI ask here."""
    return device == "" or bool(_DEVICE_RE.match(device))


@dataclass(frozen=True)
class PathSpec:
    prefix: str               # of its options: <prefix>_device, <prefix>_min_gpu
    api_key: str              # of its object in /api/v1/pool
    stats_keys: tuple         # of that object, in order: what a live path reports and what a pool without it reports
    batched: bool = False     # a MicroBatch: it has <prefix>_batch_ms and <prefix>_batch_max too
    batch_max_limit: int = 0  # the largest <prefix>_batch_max, 0 = unbounded
    batch_max_why: str = ""   # where that limit comes from, for the config file's message
    per_algorithm: bool = False  # <prefix>_min_gpu = 0 resolves per algorithm

    @property
    def fields(self) -> tuple:
        """The PoolOptions and ``pool_server`` fields of the path; the flags are these with ``-`` for ``_``."""
        batch = ("batch_ms", "batch_max") if self.batched else ()
        return tuple(f"{self.prefix}_{f}" for f in ("device", *batch, "min_gpu"))

    def values(self, holder) -> dict:
        """Those fields of ``holder`` without the prefix: ``device``, ``min_gpu`` and, if batched, ``batch_ms`` and
        ``batch_max``."""
        return {f[len(self.prefix) + 1:]: getattr(holder, f) for f in self.fields}

    def batch_max_ok(self, batch_max: int) -> bool:
        return batch_max >= 1 and not (self.batch_max_limit and batch_max > self.batch_max_limit)

    def off_stats(self, device: str = "") -> dict:
        """What a pool reports for a path it has not made: nothing in use, every counter zero."""
        return {"device": device, "enabled": False, **{k: 0.0 if k == "last_ms" else 0 for k in self.stats_keys[2:]}}


def _spec(prefix, api_key, counters, **kw):
    return PathSpec(prefix, api_key, ("device", "enabled", *counters.split(), "device_errors"), **kw)


PATHS = {s.prefix: s for s in (
    _spec("verify", "verify", "batches gpu_shares cpu_shares last_batch max_batch", batched=True, per_algorithm=True),
    _spec("job", "jobs", "fanouts gpu_channels cpu_channels last_channels last_ms"),
    _spec("template", "template", "trees gpu_leaves cpu_leaves last_leaves last_ms"),
    _spec("handshake", "handshake", "batches gpu_handshakes cpu_handshakes last_batch max_batch last_ms",
          batched=True, batch_max_limit=21845, batch_max_why=" (three rows a handshake, 65536 a call)"),
    _spec("seal", "seal", "batches gpu_frames cpu_frames last_frames last_ms"),
)}


# Devices whose path raised in this process. Every path looks here before it chooses the device, on the event loop
# and again on its worker thread, so after one path's device error no other path of the process starts a call on
# that device. Nothing in the package takes a device out again.
_failed_devices: set = set()


def device_failed(device: str) -> bool:
    return device in _failed_devices


def mark_failed(device: str) -> None:
    _failed_devices.add(device)


def forget_device_errors() -> None:
    """For tests that inject a failure: a later test in the same process gets its device back."""
    _failed_devices.clear()


class DevicePath:
    def __init__(self, option: str, device: str):
        """``device``: the value of the pool option ``option`` (``verify_device``, ``job_device``): ``cpu`` or
        ``cuda:N``, anything else is a ``ValueError``."""
        if not valid_device(device) or not device:
            raise ValueError(f"{option} {device!r} must be cpu or cuda:N")
        self.device = device
        self.gpu = device != "cpu"
        self.device_errors = 0

    @property
    def on(self) -> bool:
        return self.gpu and not device_failed(self.device)

    @property
    def enabled(self) -> bool:
        """For the stats: the configured path is in use (False once a device error, of this path or of another path
        of the process on the same device, has turned the GPU path off)."""
        return self.on or not self.gpu

    def run(self, on_device, on_cpu):
        """On the worker thread, for work the event loop chose the device for: ``(result, ran on the device, device
        error)``. Another path may have failed since the loop looked, so the switch is read again. Whatever
        ``on_device()`` raises is counted, turns the device off for the process, and ``on_cpu()`` answers instead."""
        if not self.on:
            return on_cpu(), False, None
        try:
            return on_device(), True, None
        except Exception as exc:  # noqa: BLE001 - whatever the device path raised, the work is still answered
            mark_failed(self.device)
            self.device_errors += 1
            return on_cpu(), False, exc


class DeviceWork:
    """One path of a pool: its options checked, its :class:`DevicePath`, its worker thread, and :meth:`call`. The
    counters of the path's ``stats_keys`` are attributes of this object, zero to begin with; the subclass bumps them."""

    def __init__(self, pool, prefix: str, default_min_gpu: int, what: str, fell_back: str):
        """``pool``: the PoolServer, whose ``opts.<prefix>_*`` configure the path. ``what`` and ``fell_back`` word the
        log line of a device error: "``what`` on cuda:0 failed (...); ``fell_back`` on the CPU and ..."."""
        self.spec = spec = PATHS[prefix]
        opt = spec.values(pool.opts)
        self.path = DevicePath(f"{prefix}_device", opt["device"])
        if spec.batched:
            if opt["batch_ms"] <= 0 or opt["batch_max"] < 1 or opt["min_gpu"] < 0:
                raise ValueError(f"{prefix}_batch_ms and {prefix}_batch_max must be positive, {prefix}_min_gpu not "
                                 f"negative")
            if not spec.batch_max_ok(opt["batch_max"]):
                raise ValueError(f"{prefix}_batch_max must be at most {spec.batch_max_limit}")
        elif opt["min_gpu"] < 0:
            raise ValueError(f"{prefix}_min_gpu must not be negative")
        self.pool = pool
        self.opt = opt
        self.device = self.path.device
        self.min_gpu = int(opt["min_gpu"]) or default_min_gpu
        self._words = (what, fell_back)
        self._worker = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix=f"otedama-pool-{prefix}")
        for key in spec.stats_keys[2:-1]:  # the counters; `enabled` and `device_errors` are the DevicePath's, below
            setattr(self, key, 0)
        self.last_ms = 0.0

    enabled = property(lambda self: self.path.enabled)
    device_errors = property(lambda self: self.path.device_errors)

    def stats(self) -> dict:
        return {k: getattr(self, k) for k in self.spec.stats_keys}

    def close(self) -> None:
        self._worker.shutdown(wait=True)

    def call(self, units: int, on_device, on_cpu, cpu_only: bool = False):
        """Run ``units`` of work on the worker thread and wait for it: ``on_device()`` from ``min_gpu`` units on
        while the device is in use, else ``on_cpu()``. Returns ``(result, ran on the device)``."""
        t0 = time.perf_counter()
        return self._done(t0, self._worker.submit(self._work, self._use(units, cpu_only), on_device, on_cpu).result())

    async def call_async(self, units: int, on_device, on_cpu, cpu_only: bool = False):
        """:meth:`call` for a coroutine: the event loop goes on while the worker thread computes."""
        t0 = time.perf_counter()
        return self._done(t0, await asyncio.get_running_loop().run_in_executor(
            self._worker, self._work, self._use(units, cpu_only), on_device, on_cpu))

    def _use(self, units: int, cpu_only: bool) -> bool:
        return self.path.on and not cpu_only and units >= self.min_gpu

    def _work(self, use_device: bool, on_device, on_cpu):
        """On the worker thread: ``(result, ran on the device, device error)``."""
        return self.path.run(on_device, on_cpu) if use_device else (on_cpu(), False, None)

    def _done(self, t0: float, outcome: tuple):
        result, ran, error = outcome
        if error is not None:  # the worker thread has already counted it and put the device on the failed list
            what, fell_back = self._words
            self.pool.log("error", f"pool[{self.pool.algo.name}]: {what} on {self.device} failed ({error!r}); "
                                   f"{fell_back} on the CPU and the device path is off for this process")
        self.last_ms = (time.perf_counter() - t0) * 1e3
        return result, ran


class MicroBatch(DeviceWork):
    """A path whose work arrives as concurrent ``submit`` calls and is computed in batches. An entry waits as ``(item,
    future, t_received)``. A flush takes up to ``batch_max`` entries in arrival order when that many are pending, or
    ``batch_ms`` after the oldest one arrived. One batch is in flight at a time; entries that arrive meanwhile gather
    for the next one, so batches finish strictly in submission order. ``close()`` flushes what is pending on the CPU.

    The subclass supplies ``async _process(items) -> one result per item`` and ``_late(item)``, the answer to a submit
    after ``close()``: nothing is dropped, it is computed on its own. ``STOPPED`` words the error of entries whose
    flush was cancelled."""

    STOPPED = "batcher stopped"

    def __init__(self, pool, prefix: str, default_min_gpu: int, what: str, fell_back: str):
        super().__init__(pool, prefix, default_min_gpu, what, fell_back)
        self.batch_s = self.opt["batch_ms"] / 1e3
        self.batch_max = int(self.opt["batch_max"])
        self._pending: deque = deque()  # (item, future, t_received)
        self._wake = asyncio.Event()
        self._closing = False
        self._task = asyncio.ensure_future(self._run())

    async def submit(self, item, t_received: float | None = None):
        """``t_received``: ``time.perf_counter()`` when the item arrived (now, if not given). Returns the item's
        result once its batch has finished."""
        if self._closing:
            return self._late(item)
        fut = asyncio.get_running_loop().create_future()
        self._pending.append((item, fut, time.perf_counter() if t_received is None else t_received))
        if len(self._pending) == 1 or len(self._pending) == self.batch_max:
            self._wake.set()  # the runner sleeps towards the oldest entry's deadline: only these two move it
        return await fut

    async def close(self) -> None:
        """Flush what is pending on the CPU, resolve every future, end the worker thread."""
        self._closing = True
        self._wake.set()
        await self._task
        super().close()

    async def stop(self) -> None:
        await self.close()

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
        try:
            results = await self._process([b[0] for b in batch])
            if len(results) != len(batch):
                raise RuntimeError(f"{len(batch)} entries in, {len(results)} results out")
        except BaseException as exc:  # no future is left unresolved, whatever failed
            for _item, fut, _t in batch:
                if not fut.done():
                    fut.set_exception(exc if isinstance(exc, Exception) else RuntimeError(self.STOPPED))
            if not isinstance(exc, Exception):
                raise
            return
        for (_item, fut, _t), result in zip(batch, results):
            if not fut.done():  # a submitter that went away cancelled its future
                fut.set_result(result)
