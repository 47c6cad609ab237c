"""Template tree op: t merkle trees of n leaves in, every tree's root and its coinbase path out, in one enqueue.

A pool that serves a real block template owes it two trees: the txid tree, whose leftmost path is the merkle branches
of every job, and the wtxid tree, whose root goes into the coinbase's witness commitment. Both have the coinbase slot
(leaf 0) zeroed, so :class:`MerkleTree` computes them in one call with ``otd_merkle_tree``
(csrc/kernels/merkle_tree.hip): one launch up to 512 leaves, two above. ``merkle_tree_cpu`` of the native extension
writes the same rows in plain C++; ``pool.template.merkle_branches`` and ``merkle_root_full`` are the oracle.

Rows (csrc/include/otedama/merkle_tree.h): ``1 + depth`` of 32 bytes per tree, ``depth = (n - 1).bit_length()``; row 0
is the root, rows ``1..depth`` are ``merkle_branches(leaves[1:])``.
"""
from __future__ import annotations

from typing import Sequence

import torch

from otedama_amd.ops._args import ALIGN, gpu_device, launch_stream
from otedama_amd.ops._staging import Staging
from otedama_amd.ops.merkle_rows import CHUNK, MAX_LEAVES, MAX_TREES, NODE_BYTES, pack_leaves, tree_depth, unpack_rows
from otedama_amd.ops.native import require_native


def _node_rows(name: str, t, device: torch.device, trees: int | None = None, rows: int | None = None) -> tuple:
    """``ops._args.byte_rows`` for a uint8 ``[t, rows, 32]`` tensor: returns ``(t, rows)``."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError(f"{name} must be a uint8 tensor")
    if (t.dim() != 3 or t.shape[2] != NODE_BYTES or (trees is not None and t.shape[0] != trees)
            or (rows is not None and t.shape[1] != rows)):
        raise ValueError(f"{name} must have shape [{'t' if trees is None else trees}, "
                         f"{'n' if rows is None else rows}, {NODE_BYTES}]")
    if t.device != device:
        raise ValueError(f"{name} must live on {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.numel() and t.data_ptr() % ALIGN:
        raise ValueError(f"{name} must start at a {ALIGN}-byte aligned address")
    return t.shape[0], t.shape[1]


class MerkleTree:
    """Reusable tree launcher on one device. It owns the staging buffers of :meth:`tree`."""

    def __init__(self, device="cuda:0"):
        self.native = require_native()
        self.device = gpu_device(device, "MerkleTree")
        self._staging = Staging(self.device)  # in: leaves, out: rows

    def launch(self, leaves: torch.Tensor, out: torch.Tensor | None = None,
               stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Enqueue the trees of ``leaves`` (uint8 ``[t, n, 32]``, contiguous, 16-byte aligned, on the op's device;
        ``1 <= n <= 262144``, ``1 <= t <= 65535``) on ``stream`` (default: the current stream, which a given stream
        first waits for) and return their rows as uint8 ``[t, 1 + depth, 32]`` (``out`` if given: that shape,
        contiguous, 16-byte aligned, on the op's device) without synchronising: one kernel launch up to 512 leaves,
        two above, with the chunk roots between them in rows allocated on the stream. A bad argument raises
        ``ValueError`` before anything is enqueued."""
        t, n = _node_rows("leaves", leaves, self.device)
        if not 1 <= n <= MAX_LEAVES:
            raise ValueError(f"a tree has 1..{MAX_LEAVES} leaves, not {n}")
        if not 1 <= t <= MAX_TREES:
            raise ValueError(f"a launch takes 1..{MAX_TREES} trees, not {t}")
        rows = 1 + tree_depth(n)
        if out is not None:
            _node_rows("out", out, self.device, trees=t, rows=rows)
        stream = launch_stream(self.device, stream)
        scratch = None
        with torch.cuda.stream(stream):
            if out is None:
                out = torch.empty((t, rows, NODE_BYTES), dtype=torch.uint8, device=self.device)
            if n > CHUNK:
                scratch = torch.empty((t, (n + CHUNK - 1) // CHUNK, NODE_BYTES), dtype=torch.uint8,
                                      device=self.device)
        self.native.launch_merkle_tree(leaves.data_ptr(), t, n, scratch.data_ptr() if scratch is not None else 0,
                                       out.data_ptr(), stream.cuda_stream)
        return out

    def tree(self, leaf_lists: Sequence[Sequence[bytes]]) -> list[tuple[bytes, list[bytes]]]:
        """The pool's entry: ``t`` lists of ``n`` 32-byte leaves in, ``t`` tuples ``(root, path)`` out, in order;
        ``path`` is ``merkle_branches(leaves[1:])``. One pinned buffer of leaves goes to the device and one pinned
        buffer of rows comes back, both copies non-blocking on the current stream around :meth:`launch`, then one
        stream synchronise. The four buffers are the op's own and grow to the largest call seen; the call is not
        re-entrant. Lists of unequal length, a leaf that is not 32 bytes or a tree over the limits raise
        ``ValueError``."""
        packed, t, n = pack_leaves(leaf_lists)
        if n > MAX_LEAVES or t > MAX_TREES:
            raise ValueError(f"at most {MAX_TREES} trees of at most {MAX_LEAVES} leaves")
        rows = 1 + tree_depth(n)
        return unpack_rows(self._staging.round_trip(
            [packed], t * rows * NODE_BYTES,
            lambda dev_in, dev_out: self.launch(dev_in.view(t, n, NODE_BYTES), out=dev_out.view(t, rows, NODE_BYTES))),
            t, n)
