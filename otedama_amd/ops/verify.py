"""Share verification op: a batch of pool shares in, verdicts out, in one enqueue.

A pool never holds the 80-byte headers it has to hash. It holds a job (coinb1, coinb2, merkle branches, prev_hash,
nbits) and receives shares ``(extranonce, ntime, nonce, version)``. :class:`ShareVerify` puts a front and a back on
the digest ops (:mod:`otedama_amd.ops.digest`):

  1. ``otd_share_headers``  share records -> headers: the coinbase SHA-256d from the job's midstate and the merkle
     fold, one share per lane (csrc/kernels/share_verify.hip)
  2. the ``HeaderDigest`` launches of the op's algorithm
  3. ``otd_share_verdict``  the 256-bit little-endian compare against per-share targets and the network target

For a pool's live micro-batches, :meth:`ShareVerify.launch_results` ends the same chain with ``otd_share_pack``
(the same file) instead: one packed 128-byte record per share (header, hash, verdict), so that
:meth:`ShareVerify.results` moves one pinned buffer in and one out.

Layouts of the job block, the share record and the result record: csrc/include/otedama/share_job.h. The record
packer is torch-free (:mod:`otedama_amd.ops.share_records`) and re-exported here.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import torch

from otedama_amd.ops._args import ALIGN, byte_rows, launch_stream
from otedama_amd.ops._staging import Staging
from otedama_amd.ops.digest import DIGEST_BYTES, HEADER_BYTES, HeaderDigest
from otedama_amd.ops.share_records import (MAX_EXTRANONCE, RECORD_BYTES, RESULT_BYTES, VERDICT_BAD_INDEX,  # noqa: F401
                                           VERDICT_NETWORK, VERDICT_SHARE, pack_records, unpack_records,
                                           unpack_results)

TARGET_BYTES = 32


@dataclass
class PreparedJob:
    block: bytes          # ShareJobBlock (opaque)
    dev: torch.Tensor     # uint8 device copy of the block
    en_size: int


def check_prepared(job, device: torch.device, block_size: int) -> None:
    """``ValueError`` unless ``job`` is a :class:`PreparedJob` whose block lives on ``device`` as the kernels read
    it."""
    if not isinstance(job, PreparedJob) or not isinstance(job.dev, torch.Tensor):
        raise ValueError("job must come from prepare()")
    if job.dev.device != device:
        raise ValueError(f"job was prepared for {job.dev.device}, the op runs on {device}")
    if (job.dev.dtype != torch.uint8 or job.dev.numel() != block_size
            or not job.dev.is_contiguous() or job.dev.data_ptr() % ALIGN):
        raise ValueError("job block has the wrong size or alignment")


def prepare_job(native, device: torch.device, coinb1: bytes, coinb2: bytes, en_size: int, prev_hash: bytes,
                nbits: int, branches: Sequence[bytes]) -> PreparedJob:
    """Build the job block and upload it to ``device``; ``ValueError`` for a job over the block's limits."""
    block = native.share_job_prepare(bytes(coinb1), bytes(coinb2), int(en_size), bytes(prev_hash),
                                     int(nbits) & 0xFFFFFFFF, [bytes(b) for b in branches])
    dev = torch.frombuffer(bytearray(block), dtype=torch.uint8).to(device)
    return PreparedJob(block, dev, int(en_size))


class ShareVerify:
    """Reusable share verifier for one algorithm on one device. It owns a :class:`HeaderDigest` of the same
    algorithm and the headers buffer between the two; ``capacity`` and ``grid`` are the digest op's."""

    def __init__(self, algorithm: str, device="cuda:0", capacity: int | None = None, grid: int | None = None):
        self.digest = HeaderDigest(algorithm, device, capacity=capacity, grid=grid)
        self.algorithm = self.digest.algorithm
        self.native = self.digest.native
        self.device = self.digest.device
        self.headers: torch.Tensor | None = None  # uint8 [rows, 80], grown to the largest batch seen
        self._last_stream = None
        # the live path (launch_results / results): the digests between the chain and the pack kernel, and the
        # staging buffers of results(), all grown to the largest batch seen
        self._digests: torch.Tensor | None = None
        self._staging = Staging(self.device)  # in: records | targets, out: result records

    def prepare(self, coinb1: bytes, coinb2: bytes, en_size: int, prev_hash: bytes, nbits: int,
                branches: Sequence[bytes]) -> PreparedJob:
        """Build the job block (midstate, padded tail template, branches, network target) and upload it. A job over
        the block's limits (tail of more than 32 blocks, more than 32 branches, ``en_size`` outside 1..16) raises
        ``ValueError``: verify it on the CPU."""
        return prepare_job(self.native, self.device, coinb1, coinb2, en_size, prev_hash, nbits, branches)

    def _check(self, job: PreparedJob, records: torch.Tensor, targets: torch.Tensor) -> int:
        check_prepared(job, self.device, self.native.SHARE_JOB_BLOCK_SIZE)
        n = byte_rows("records", records, RECORD_BYTES, self.device)
        if byte_rows("targets", targets, TARGET_BYTES, self.device) < 1:
            raise ValueError("the target table is empty")
        if n >= 1 << 32 or targets.shape[0] >= 1 << 32:
            raise ValueError("at most 2^32 - 1 records and targets per launch")
        return n

    def _grow_rows(self, name: str, n: int, width: int, stream: torch.cuda.Stream) -> torch.Tensor:
        """The first ``n`` rows of the op's ``[rows, width]`` buffer ``name``, reallocated on ``stream`` when it is
        too small. The old buffer's memory stays reserved until the previous launch's stream is through with it."""
        buf = getattr(self, name)
        if buf is None or buf.shape[0] < n:
            if buf is not None and self._last_stream is not None:
                buf.record_stream(self._last_stream)
            with torch.cuda.stream(stream):
                buf = torch.empty((n, width), dtype=torch.uint8, device=self.device)
            setattr(self, name, buf)
        return buf[:n]

    def _chain(self, job: PreparedJob, records: torch.Tensor, n: int, stream: torch.cuda.Stream,
               digests: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """Enqueue ``otd_share_headers`` and the digest launches for ``n >= 1`` records on ``stream``, after whatever
        the previous launch still does with the op's buffers, and return ``(headers, digests)``: views of the op's
        buffers, the digests in the caller's tensor if it brings one."""
        if self._last_stream is not None and self._last_stream != stream:
            stream.wait_stream(self._last_stream)  # headers and digests are still in use by the previous launch
        headers = self._grow_rows("headers", n, HEADER_BYTES, stream)
        if digests is None:
            digests = self._grow_rows("_digests", n, DIGEST_BYTES, stream)
        self._last_stream = stream
        self.native.launch_share_headers(job.dev.data_ptr(), records.data_ptr(), n, headers.data_ptr(),
                                         stream.cuda_stream)
        self.digest.launch(headers, out=digests, stream=stream)
        return headers, digests

    def launch(self, job: PreparedJob, records: torch.Tensor, targets: torch.Tensor,
               stream: torch.cuda.Stream | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Enqueue headers, digests and verdicts of ``records`` (uint8 ``[n, 32]``) against ``targets`` (uint8
        ``[t, 32]``, ``t >= 1``; both contiguous, 16-byte aligned, on the op's device) on ``stream`` (default: the
        current stream, which the given stream first waits for) and return ``(verdicts uint8 [n], digests uint8
        [n, 32], headers uint8 [n, 80])`` without synchronising. ``headers`` is a view of the op's own buffer and is
        overwritten by the next launch. A bad argument raises ``ValueError`` before anything is enqueued."""
        n = self._check(job, records, targets)
        stream = launch_stream(self.device, stream)  # the caller produced `records` and `targets` on the current one
        with torch.cuda.stream(stream):
            verdicts = torch.empty(n, dtype=torch.uint8, device=self.device)
            digests = torch.empty((n, DIGEST_BYTES), dtype=torch.uint8, device=self.device)
        if n == 0:
            return verdicts, digests, torch.empty((0, HEADER_BYTES), dtype=torch.uint8, device=self.device)
        headers, _ = self._chain(job, records, n, stream, digests)
        self.native.launch_share_verdict(job.dev.data_ptr(), records.data_ptr(), digests.data_ptr(),
                                         targets.data_ptr(), targets.shape[0], n, verdicts.data_ptr(),
                                         stream.cuda_stream)
        return verdicts, digests, headers

    def launch_results(self, job: PreparedJob, records: torch.Tensor, targets: torch.Tensor,
                       out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """The live form of :meth:`launch`: the same arguments, checks and stream handling, one packed 128-byte
        result record per share (header 80 | hash 32 | verdict 1 | zeros 15; ``ShareResult`` in share_job.h) as
        uint8 ``[n, 128]`` (``out`` if given: that shape, contiguous, 16-byte aligned, on the op's device), without
        synchronising: ``otd_share_headers``, the digest launches of the algorithm, then ``otd_share_pack``, which
        compares and packs. An empty batch returns an empty tensor and enqueues nothing."""
        n = self._check(job, records, targets)
        if out is not None:
            byte_rows("out", out, RESULT_BYTES, self.device, rows=n)
        if n == 0:
            return out if out is not None else torch.empty((0, RESULT_BYTES), dtype=torch.uint8, device=self.device)
        stream = launch_stream(self.device, stream)
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty((n, RESULT_BYTES), dtype=torch.uint8, device=self.device)
        headers, digests = self._chain(job, records, n, stream)
        self.native.launch_share_pack(job.dev.data_ptr(), records.data_ptr(), headers.data_ptr(), digests.data_ptr(),
                                      targets.data_ptr(), targets.shape[0], n, out.data_ptr(), stream.cuda_stream)
        return out

    @staticmethod
    def _packed(job: PreparedJob, shares: Sequence[tuple], targets: Sequence[bytes],
                target_indices: Sequence[int] | None) -> tuple[bytes, bytes, int]:
        """The host side of both synchronous entries: ``(records, target table, number of targets)`` as bytes, with
        ``target_indices`` defaulting to target 0 for every share."""
        targets = [bytes(t) for t in targets]
        if not targets or any(len(t) != TARGET_BYTES for t in targets):
            raise ValueError(f"need at least one target, each {TARGET_BYTES} bytes")
        if target_indices is None:
            target_indices = [0] * len(shares)
        return pack_records(shares, target_indices, job.en_size), b"".join(targets), len(targets)

    def results(self, job: PreparedJob, shares: Sequence[tuple], targets: Sequence[bytes],
                target_indices: Sequence[int] | None = None) -> list[tuple[bytes, bytes, int]]:
        """The live entry: ``(extranonce, ntime, nonce, version)`` tuples and 32-byte targets in, ``(header, hash,
        verdict byte)`` per share out, the list ``pool.batch.check_shares`` returns. One pinned buffer (records |
        targets) goes to the device and one pinned buffer of result records comes back, both copies non-blocking on
        the current stream around :meth:`launch_results`, then one stream synchronise. The four buffers are the op's
        own and grow to the largest batch seen; the call is not re-entrant."""
        packed, table, n_targets = self._packed(job, shares, targets, target_indices)
        n = len(shares)
        if n == 0:
            return []
        rec_bytes = n * RECORD_BYTES

        def launch(dev_in: torch.Tensor, dev_out: torch.Tensor) -> None:
            self.launch_results(job, dev_in[:rec_bytes].view(n, RECORD_BYTES),
                                dev_in[rec_bytes:].view(n_targets, TARGET_BYTES), out=dev_out.view(n, RESULT_BYTES))

        return unpack_results(self._staging.round_trip([packed, table], n * RESULT_BYTES, launch))

    def verify(self, job: PreparedJob, shares: Sequence[tuple], targets: Sequence[bytes],
               target_indices: Sequence[int] | None = None) -> tuple[list[int], list[bytes], list[bytes]]:
        """Synchronous convenience: ``(extranonce, ntime, nonce, version)`` tuples and 32-byte targets in, the lists
        ``(verdict bytes, 32-byte hashes, 80-byte headers)`` out. ``target_indices`` defaults to target 0 for every
        share."""
        packed, table, n_targets = self._packed(job, shares, targets, target_indices)
        if not shares:
            return [], [], []
        recs = torch.frombuffer(bytearray(packed), dtype=torch.uint8).view(len(shares), RECORD_BYTES)
        tgts = torch.frombuffer(bytearray(table), dtype=torch.uint8).view(n_targets, TARGET_BYTES)
        v, d, h = self.launch(job, recs.to(self.device), tgts.to(self.device))
        torch.cuda.current_stream(self.device).synchronize()
        vb, db, hb = (t.cpu().numpy().tobytes() for t in (v, d, h))
        n = len(shares)
        return (list(vb), [db[i * DIGEST_BYTES:(i + 1) * DIGEST_BYTES] for i in range(n)],
                [hb[i * HEADER_BYTES:(i + 1) * HEADER_BYTES] for i in range(n)])
