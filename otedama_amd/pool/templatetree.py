"""A block template's merkle trees for the running pool: the txid tree's coinbase path and the wtxid tree's root in
one ``pool.batch.template_tree`` call instead of ``merkle_branches`` and ``merkle_root_full`` on the event loop.

``PoolServer.new_block`` asks :meth:`TemplateTree.compute` once per template, before the first ``coinbase_parts``,
and hands the result to ``BlockTemplate.set_tree``. The call is synchronous, as ``new_block`` is: a device call that
never returns holds ``new_block``, and with it the event loop, for good. The worker thread owns the
``ops.merkle.MerkleTree`` op; with ``template_device="cpu"`` it runs the native ``merkle_tree_cpu``. A template over
the op's limit of 262144 leaves is computed in Python (inside ``template_tree``). The thread, the threshold and the
fall-back rules are ``pool.devicepath``'s.
"""
from __future__ import annotations

from otedama_amd.pool.batch import template_tree
from otedama_amd.pool.devicepath import DeviceWork

# template_min_gpu = 0 resolves to this: the smallest measured leaf count, rounded up to a power of two, at which the
# GPU round trip (template_tree(device="cuda:0"), both trees, p50) was at or below the same host's
# template_tree(device="cpu") time (tools/bench_template_tree.py; the table is in docs/POOL.md, "Real templates and
# the template tree": the GPU loses at 512, 0.158 ms against 0.099 ms, and wins at 4096, 0.455 ms against 0.757 ms).
# Leaves are counted per tree, the coinbase slot included.
DEFAULT_TEMPLATE_MIN_GPU = 4096


class TemplateTree(DeviceWork):
    def __init__(self, pool, device_tree=None):
        """``pool``: the PoolServer, whose ``opts.template_*`` configure the path. ``device_tree``: replaces the GPU
        path, ``device_tree(txids, wtxids)`` called on the worker thread."""
        super().__init__(pool, "template", DEFAULT_TEMPLATE_MIN_GPU, "template tree", "the tree was computed")
        self._device_tree = device_tree or (lambda txids, wtxids: template_tree(txids, wtxids, self.device))

    def compute(self, txids: list, wtxids: list) -> tuple:
        """``(branches, witness_root)`` of a template (``pool.batch.template_tree``). Waits for the worker thread.
        The threshold compares the leaves of one tree with the coinbase slot, ``1 + len(txids)``; the counters add
        those of both trees."""
        n = 1 + len(txids)
        leaves = n * (2 if wtxids else 1)
        # a template over the op's limit is computed in Python inside template_tree; it is still counted with the device
        tree, ran = self.call(n, lambda: self._device_tree(txids, wtxids), lambda: template_tree(txids, wtxids, "cpu"))
        self.trees += 1
        self.last_leaves = leaves
        self.gpu_leaves += leaves if ran else 0
        self.cpu_leaves += 0 if ran else leaves
        return tree
