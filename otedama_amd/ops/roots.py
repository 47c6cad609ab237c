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

from otedama_amd.ops._args import byte_rows, launch_stream
from otedama_amd.ops.native import require_native
from otedama_amd.ops.share_records import PREFIX_BYTES, ROOT_BYTES, pack_prefixes, unpack_roots  # noqa: F401
from otedama_amd.ops.verify import PreparedJob, check_prepared, prepare_job


class ChannelRoots:
    """Reusable root launcher on one device. It owns the staging buffers of :meth:`roots`."""

    def __init__(self, device="cuda:0"):
        self.native = require_native()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("ChannelRoots needs a GPU device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._pin_in: torch.Tensor | None = None   # pinned: prefix rows
        self._dev_in: torch.Tensor | None = None
        self._pin_out: torch.Tensor | None = None  # pinned: roots
        self._dev_out: torch.Tensor | None = None

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

    def _grown(self, name: str, nbytes: int, pinned: bool) -> torch.Tensor:
        buf = getattr(self, name)
        if buf is None or buf.numel() < nbytes:
            size = max(nbytes, 2 * buf.numel() if buf is not None else 4096)
            buf = (torch.empty(size, dtype=torch.uint8, pin_memory=True) if pinned
                   else torch.empty(size, dtype=torch.uint8, device=self.device))
            setattr(self, name, buf)
        return buf

    def roots(self, job: PreparedJob, prefixes: Sequence[bytes]) -> list[bytes]:
        """The pool's entry: ``en_size``-byte prefixes in, their 32-byte roots out, in order. One pinned buffer of
        prefix rows goes to the device and one pinned buffer of roots comes back, both copies non-blocking on the
        current stream around :meth:`launch`, then one stream synchronise. The four buffers are the op's own and
        grow to the largest batch seen; the call is not re-entrant."""
        packed = pack_prefixes(prefixes, job.en_size)
        n = len(prefixes)
        if n == 0:
            return []
        in_bytes, out_bytes = n * PREFIX_BYTES, n * ROOT_BYTES
        pin_in, dev_in = self._grown("_pin_in", in_bytes, True), self._grown("_dev_in", in_bytes, False)
        pin_out, dev_out = self._grown("_pin_out", out_bytes, True), self._grown("_dev_out", out_bytes, False)
        memoryview(pin_in.numpy())[:in_bytes] = packed
        stream = torch.cuda.current_stream(self.device)
        dev_in[:in_bytes].copy_(pin_in[:in_bytes], non_blocking=True)
        self.launch(job, dev_in[:in_bytes].view(n, PREFIX_BYTES), out=dev_out[:out_bytes].view(n, ROOT_BYTES))
        pin_out[:out_bytes].copy_(dev_out[:out_bytes], non_blocking=True)
        stream.synchronize()
        return unpack_roots(memoryview(pin_out.numpy())[:out_bytes])
