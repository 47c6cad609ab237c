"""Channel roots op: one job and n extranonce prefixes in, n merkle roots out, in one enqueue.

A pool that opens Stratum V2 standard channels owes every channel its own merkle root for every job: the channel's
extranonce prefix is fixed, so the root is ``merkle_root_from_branches(sha256d(coinb1 + prefix + coinb2), branches)``.
:class:`ChannelRoots` computes all of a job's roots with ``otd_channel_roots`` (csrc/kernels/channel_roots.hip), one
prefix per lane, against the job block that :class:`otedama_amd.ops.verify.ShareVerify` also reads
(csrc/include/otedama/share_job.h). ``share_roots_cpu`` of the native extension writes the same bytes in plain C++.
"""
from __future__ import annotations

from typing import Sequence

import torch

from otedama_amd.ops._args import byte_rows, gpu_device, launch_stream
from otedama_amd.ops._staging import Staging
from otedama_amd.ops.native import require_native
from otedama_amd.ops.share_records import PREFIX_BYTES, ROOT_BYTES, pack_prefixes, unpack_roots  # noqa: F401
from otedama_amd.ops.verify import PreparedJob, check_prepared, prepare_job


class ChannelRoots:
    """Reusable root launcher on one device. It owns the staging buffers of :meth:`roots`."""

    def __init__(self, device="cuda:0"):
        self.native = require_native()
        self.device = gpu_device(device, "ChannelRoots")
        self._staging = Staging(self.device)  # in: prefix rows, out: roots

    def prepare(self, coinb1: bytes, coinb2: bytes, en_size: int, prev_hash: bytes, nbits: int,
                branches: Sequence[bytes]) -> PreparedJob:
        """``ShareVerify.prepare``: the same arguments, the same block, the same limits (a tail of more than 32
        blocks, more than 32 branches or ``en_size`` outside 1..16 raises ``ValueError``: compute that job's roots
        on the CPU)."""
        return prepare_job(self.native, self.device, coinb1, coinb2, en_size, prev_hash, nbits, branches)

    def launch(self, job: PreparedJob, prefixes: torch.Tensor, out: torch.Tensor | None = None,
               stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Enqueue the roots of ``prefixes`` (uint8 ``[n, 16]``, contiguous, 16-byte aligned, on the op's device;
        bytes ``en_size..15`` of a row are ignored) on ``stream`` (default: the current stream, which a given
        stream first waits for) and return them as uint8 ``[n, 32]`` (``out`` if given: that shape, contiguous,
        16-byte aligned, on the op's device) without synchronising. A bad argument raises ``ValueError`` before
        anything is enqueued; an empty batch returns an empty tensor and enqueues nothing."""
        check_prepared(job, self.device, self.native.SHARE_JOB_BLOCK_SIZE)
        n = byte_rows("prefixes", prefixes, PREFIX_BYTES, self.device)
        if n >= 1 << 32:
            raise ValueError("at most 2^32 - 1 prefixes per launch")
        if out is not None:
            byte_rows("out", out, ROOT_BYTES, self.device, rows=n)
        if n == 0:
            return out if out is not None else torch.empty((0, ROOT_BYTES), dtype=torch.uint8, device=self.device)
        stream = launch_stream(self.device, stream)
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty((n, ROOT_BYTES), dtype=torch.uint8, device=self.device)
        self.native.launch_channel_roots(job.dev.data_ptr(), prefixes.data_ptr(), n, out.data_ptr(),
                                         stream.cuda_stream)
        return out

    def roots(self, job: PreparedJob, prefixes: Sequence[bytes]) -> list[bytes]:
        """The pool's entry: ``en_size``-byte prefixes in, their 32-byte roots out, in order. One pinned buffer of
        prefix rows goes to the device and one pinned buffer of roots comes back, both copies non-blocking on the
        current stream around :meth:`launch`, then one stream synchronise. The four buffers are the op's own and
        grow to the largest batch seen; the call is not re-entrant."""
        packed = pack_prefixes(prefixes, job.en_size)
        n = len(prefixes)
        if n == 0:
            return []
        return unpack_roots(self._staging.round_trip(
            [packed], n * ROOT_BYTES,
            lambda dev_in, dev_out: self.launch(job, dev_in.view(n, PREFIX_BYTES), out=dev_out.view(n, ROOT_BYTES))))
