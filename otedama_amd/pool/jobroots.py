"""A job's fan-out to Stratum V2 standard channels for the running pool: every channel's merkle root of one job in
one ``pool.batch.channel_roots`` call instead of one ``PoolServer.merkle_root_for`` per channel on the event loop.

``PoolServer._make_job`` gathers the extranonce prefix of every standard channel of every connection and asks
:meth:`JobRoots.roots` once. The call is synchronous, as ``_make_job`` is: a device call that never returns holds
``_make_job``, and with it the event loop, for good. The worker thread owns the ``ops.roots.ChannelRoots`` op; with
``job_device="cpu"`` it runs the native ``share_roots_cpu``. A job over the job block's limits is computed in Python
(inside ``channel_roots``). The thread, the threshold and the fall-back rules are ``pool.devicepath``'s.
"""
from __future__ import annotations

from otedama_amd.pool.batch import channel_roots
from otedama_amd.pool.devicepath import DeviceWork

# job_min_gpu = 0 resolves to this: the smallest measured fan-out, rounded up to a power of two, at which the GPU
# round trip (ChannelRoots.roots, p50) was at or below the same host's channel_roots(device="cpu") time
# (tools/bench_job_roots.py; the table is in docs/POOL.md, "Job fan-out": the GPU loses at 64, 0.121 ms against
# 0.113 ms, and wins at 512, 0.168 ms against 0.879 ms).
DEFAULT_JOB_MIN_GPU = 512


class JobRoots(DeviceWork):
    def __init__(self, pool, device_roots=None):
        """``pool``: the PoolServer, whose ``opts.job_*`` configure the fan-out. ``device_roots``: replaces the GPU
        path, ``device_roots(job, prefixes)`` called on the worker thread."""
        super().__init__(pool, "job", DEFAULT_JOB_MIN_GPU, "job fan-out", "the roots were computed")
        self._device_roots = device_roots or (lambda job, prefixes: channel_roots(job, prefixes, self.device))

    def roots(self, job, prefixes: list) -> list:
        """``job``: a ``pool.batch.ShareJob``; the root of every prefix, in order. Waits for the worker thread."""
        if not prefixes:
            return []
        # a job over the block's limits is computed in Python inside channel_roots; it is still counted with the device
        roots, ran = self.call(len(prefixes), lambda: self._device_roots(job, prefixes),
                               lambda: channel_roots(job, prefixes, "cpu"))
        self.fanouts += 1
        self.last_channels = len(prefixes)
        self.gpu_channels += len(prefixes) if ran else 0
        self.cpu_channels += 0 if ran else len(prefixes)
        return roots
