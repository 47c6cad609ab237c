"""A block template's merkle trees for the running pool: the txid tree's coinbase path and the wtxid tree's root in
one ``pool.batch.template_tree`` call instead of ``merkle_branches`` and ``merkle_root_full`` on the event loop.

``PoolServer.new_block`` asks :meth:`TemplateTree.compute` once per template, before the first ``coinbase_parts``,
and hands the result to ``BlockTemplate.set_tree``. The call is synchronous, as ``new_block`` is: it hands the work
to one dedicated worker thread and waits for it. That thread creates and owns the ``ops.merkle.MerkleTree`` op: torch
and the GPU are first touched there, and importing this module imports neither. With ``template_device="cpu"`` the
thread runs the native ``merkle_tree_cpu``.

Fallbacks: a template of fewer leaves than ``template_min_gpu`` goes to the native CPU path, one over the op's limit
of 262144 leaves to Python (inside ``template_tree``). Any exception from the device path sends that template to the
CPU, is logged and counted, and turns the device off in ``pool.devicepath``, the process-wide switch the share
verifier and the job fan-out use too: a GPU that has faulted for any path is used by none again.

The device call has no time limit: one that never returns (a hung GPU) holds ``new_block``, and with it the event
loop, for good. A blocked ``hipStreamSynchronize`` cannot be abandoned safely from Python, so none is attempted.
"""
from __future__ import annotations

import concurrent.futures
import time

from otedama_amd.pool.batch import template_tree
from otedama_amd.pool.devicepath import DevicePath

# template_min_gpu = 0 resolves to this: the smallest measured leaf count, rounded up to a power of two, at which the
# GPU round trip (template_tree(device="cuda:0"), both trees, p50) was at or below the same host's
# template_tree(device="cpu") time (tools/bench_template_tree.py; the table is in docs/POOL.md, "Real templates and
# the template tree": the GPU loses at 512, 0.158 ms against 0.099 ms, and wins at 4096, 0.455 ms against 0.757 ms).
# Leaves are counted per tree, the coinbase slot included.
DEFAULT_TEMPLATE_MIN_GPU = 4096


class TemplateTree:
    def __init__(self, pool, device_tree=None):
        """``pool``: the PoolServer, whose ``opts.template_*`` configure the path. ``device_tree``: replaces the GPU
        path, ``device_tree(txids, wtxids)`` called on the worker thread."""
        o = pool.opts
        self.path = DevicePath("template_device", o.template_device)
        if o.template_min_gpu < 0:
            raise ValueError("template_min_gpu must not be negative")
        self.pool = pool
        self.device = self.path.device
        self.min_gpu = int(o.template_min_gpu) or DEFAULT_TEMPLATE_MIN_GPU
        self._device_tree = device_tree
        self._worker = concurrent.futures.ThreadPoolExecutor(max_workers=1,
                                                             thread_name_prefix="otedama-pool-template")
        self.trees = self.gpu_leaves = self.cpu_leaves = self.last_leaves = 0
        self.last_ms = 0.0

    def stats(self) -> dict:
        return {"device": self.device, "enabled": self.path.enabled, "trees": self.trees,
                "gpu_leaves": self.gpu_leaves, "cpu_leaves": self.cpu_leaves, "last_leaves": self.last_leaves,
                "last_ms": self.last_ms, "device_errors": self.path.device_errors}

    def close(self) -> None:
        self._worker.shutdown(wait=True)

    def compute(self, txids: list, wtxids: list) -> tuple:
        """``(branches, witness_root)`` of a template (``pool.batch.template_tree``). Waits for the worker thread.
        Leaves are counted per tree with the coinbase slot: ``1 + len(txids)``, twice with wtxids."""
        t0 = time.perf_counter()
        n = 1 + len(txids)
        leaves = n * (2 if wtxids else 1)
        on_device = self.path.on and n >= self.min_gpu
        tree, on_gpu, error = self._worker.submit(self._compute, txids, wtxids, on_device).result()
        if error is not None:  # the worker thread has already counted it and put the device on the failed list
            pool = self.pool
            pool.log("error", f"pool[{pool.algo.name}]: template tree on {self.device} failed ({error!r}); the tree "
                              f"was computed on the CPU and the device path is off for this process")
        self.trees += 1
        self.last_leaves = leaves
        self.gpu_leaves += leaves if on_gpu else 0
        self.cpu_leaves += 0 if on_gpu else leaves
        self.last_ms = (time.perf_counter() - t0) * 1e3
        return tree

    def _compute(self, txids: list, wtxids: list, on_device: bool):
        """On the worker thread: ``(tree, computed on the device, device error)``."""
        def cpu():
            return template_tree(txids, wtxids, "cpu")

        if not on_device:
            return cpu(), False, None
        # a template over the op's limit is computed in Python inside template_tree; it is still counted with the device
        device = self._device_tree or (lambda t, w: template_tree(t, w, self.device))
        return self.path.run(lambda: device(txids, wtxids), cpu)
