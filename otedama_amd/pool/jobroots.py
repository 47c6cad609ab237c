"""A job's fan-out to Stratum V2 standard channels for the running pool: every channel's merkle root of one job in
one ``pool.batch.channel_roots`` call instead of one ``PoolServer.merkle_root_for`` per channel on the event loop.

``PoolServer._make_job`` gathers the extranonce prefix of every standard channel of every connection and asks
:meth:`JobRoots.roots` once. The call is synchronous, as ``_make_job`` is: it hands the work to one dedicated worker
thread and waits for it. That thread creates and owns the ``ops.roots.ChannelRoots`` op: torch and the GPU are first
touched there, and importing this module imports neither. With ``job_device="cpu"`` the thread runs the native
``share_roots_cpu``.

Fallbacks: a fan-out of fewer channels than ``job_min_gpu`` goes to the native CPU path, a job over the job block's
limits to Python (inside ``channel_roots``). Any exception from the device path sends that fan-out to the CPU, is
logged and counted, and turns the device off in ``pool.devicepath``, the process-wide switch the share verifier
uses too: a GPU that has faulted for either path is used by neither again.

The device call has no time limit: one that never returns (a hung GPU) holds ``_make_job``, and with it the event
loop, for good. A blocked ``hipStreamSynchronize`` cannot be abandoned safely from Python, so none is attempted.
"""
from __future__ import annotations

import concurrent.futures
import time

from otedama_amd.pool.batch import channel_roots
from otedama_amd.pool.devicepath import DevicePath

# job_min_gpu = 0 resolves to this: the smallest measured fan-out, rounded up to a power of two, at which the GPU
# round trip (ChannelRoots.roots, p50) was at or below the same host's channel_roots(device="cpu") time
# (tools/bench_job_roots.py; the table is in docs/POOL.md, "Job fan-out": the GPU loses at 64, 0.121 ms against
# 0.113 ms, and wins at 512, 0.168 ms against 0.879 ms).
DEFAULT_JOB_MIN_GPU = 512


class JobRoots:
    def __init__(self, pool, device_roots=None):
        """``pool``: the PoolServer, whose ``opts.job_*`` configure the fan-out. ``device_roots``: replaces the GPU
        path, ``device_roots(job, prefixes)`` called on the worker thread."""
        o = pool.opts
        self.path = DevicePath("job_device", o.job_device)
        if o.job_min_gpu < 0:
            raise ValueError("job_min_gpu must not be negative")
        self.pool = pool
        self.device = self.path.device
        self.min_gpu = int(o.job_min_gpu) or DEFAULT_JOB_MIN_GPU
        self._device_roots = device_roots
        self._worker = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="otedama-pool-job")
        self.fanouts = self.gpu_channels = self.cpu_channels = self.last_channels = 0
        self.last_ms = 0.0

    def stats(self) -> dict:
        return {"device": self.device, "enabled": self.path.enabled, "fanouts": self.fanouts,
                "gpu_channels": self.gpu_channels, "cpu_channels": self.cpu_channels,
                "last_channels": self.last_channels, "last_ms": self.last_ms,
                "device_errors": self.path.device_errors}

    def close(self) -> None:
        self._worker.shutdown(wait=True)

    def roots(self, job, prefixes: list) -> list:
        """``job``: a ``pool.batch.ShareJob``; the root of every prefix, in order. Waits for the worker thread."""
        if not prefixes:
            return []
        t0 = time.perf_counter()
        on_device = self.path.on and len(prefixes) >= self.min_gpu
        roots, on_gpu, error = self._worker.submit(self._compute, job, prefixes, on_device).result()
        if error is not None:  # the worker thread has already counted it and put the device on the failed list
            pool = self.pool
            pool.log("error", f"pool[{pool.algo.name}]: job fan-out on {self.device} failed ({error!r}); the roots "
                              f"were computed on the CPU and the device path is off for this process")
        self.fanouts += 1
        self.last_channels = len(prefixes)
        self.gpu_channels += on_gpu
        self.cpu_channels += len(prefixes) - on_gpu
        self.last_ms = (time.perf_counter() - t0) * 1e3
        return roots

    def _compute(self, job, prefixes: list, on_device: bool):
        """On the worker thread: ``(roots, channels computed on the device, device error)``."""
        def cpu():
            return channel_roots(job, prefixes, "cpu")

        if not on_device:
            return cpu(), 0, None
        # a job over the block's limits is computed in Python inside channel_roots; it is still counted with the device
        device = self._device_roots or (lambda j, p: channel_roots(j, p, self.device))
        roots, ran, error = self.path.run(lambda: device(job, prefixes), cpu)
        return roots, len(prefixes) if ran else 0, error
