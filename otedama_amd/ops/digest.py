"""Batch digest ops: hash a tensor of unrelated 80-byte headers on the GPU.

The search ops (:mod:`otedama_amd.ops.search`) take one prepared header and a nonce range and return the nonces
whose top word passed the filter; no digest leaves the device. :class:`HeaderDigest` is the other half: ``n``
headers in, ``n`` full 32-byte digests out, in the byte order :attr:`PowAlgorithm.hash` returns (the raw
little-endian hash, not display order).

Kernels (csrc/kernels/digest_batch.hip):
  * ``otd_sha256d_digest``                      — all 64+64+64 rounds, no midstate, no early exit
  * ``otd_scrypt_pbkdf_in_hdr`` / ``_out_hdr``  — per-lane job blocks around the search's PBKDF2 code and its ROMix
  * ``x11k::k_blake512_hdr`` + stages 1..10 + ``otd_x11_gather_digest``
"""
from __future__ import annotations

from typing import Sequence

import torch

from otedama_amd.models import algorithms
from otedama_amd.ops._args import ALIGN, byte_rows, gpu_device, launch_stream  # noqa: F401  (ALIGN: for importers)
from otedama_amd.ops.native import require_native
from otedama_amd.ops.search import default_grid
from otedama_amd.ops.tuning import SCRYPT_BLOCKS_PER_CU

HEADER_BYTES = 80
DIGEST_BYTES = 32

X11_CAPACITY = 1 << 20  # headers per chain pass: 64 MiB of stage planes


class HeaderDigest:
    """Reusable digest launcher for one algorithm on one device. It owns its scratch buffers (the scrypt state
    buffer and pad, the X11 stage planes) and shares none with a ``*Search`` instance."""

    def __init__(self, algorithm: str, device="cuda:0", capacity: int | None = None, grid: int | None = None):
        """``capacity``: headers per internal chunk (a larger batch runs as several chunks on the same stream). It
        sizes the scrypt state buffer and pad and the X11 planes; SHA-256d needs no scratch and is unchunked unless
        a capacity is given. scrypt: ``grid`` ROMix blocks of 256 lane slots, one header each, default as
        ``ScryptSearch``; a given ``capacity`` is rounded up to whole blocks."""
        self.algorithm = algorithms.get(algorithm).name
        self.native = require_native()
        self.device = gpu_device(device, "HeaderDigest")
        if capacity is not None and capacity <= 0:
            raise ValueError("capacity must be positive")
        if grid is not None and grid <= 0:
            raise ValueError("grid must be positive")
        self.grid = None
        self._last_stream = None
        if self.algorithm == "scrypt":
            if grid is None:
                grid = (capacity + 255) // 256 if capacity else default_grid(self.device, SCRYPT_BLOCKS_PER_CU)
            self.grid = int(grid)
            slots = self.grid * 256
            self.capacity = min(capacity, slots) if capacity else slots
            self.gap = self.native.SCRYPT_COOP
            self.scratch = torch.empty(self.native.scrypt_scratch_bytes(self.grid, self.gap), dtype=torch.uint8,
                                       device=self.device)
            self.xbuf = torch.empty(slots * 128, dtype=torch.uint8, device=self.device)
        elif self.algorithm == "x11":
            self.capacity = int(capacity or X11_CAPACITY)
            if self.capacity > 1 << 26:
                raise ValueError("capacity must be at most 2^26")
            self.H = torch.empty(8 * self.capacity, dtype=torch.int64, device=self.device)
        else:
            self.capacity = int(capacity) if capacity else None

    def _check(self, headers: torch.Tensor, out: torch.Tensor | None) -> int:
        n = byte_rows("headers", headers, HEADER_BYTES, self.device)
        if n >= 1 << 32:
            raise ValueError("at most 2^32 - 1 headers per launch")
        if out is not None:
            byte_rows("out", out, DIGEST_BYTES, self.device, rows=n)
        return n

    def launch(self, headers: torch.Tensor, out: torch.Tensor | None = None,
               stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Enqueue the digests of ``headers`` (uint8 ``[n, 80]``, contiguous, on the op's device) on ``stream``
        (default: the current stream) and return the uint8 ``[n, 32]`` result (``out`` if given) without
        synchronising. A bad argument raises ``ValueError`` before anything is enqueued."""
        n = self._check(headers, out)
        stream = launch_stream(self.device, stream)
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty((n, DIGEST_BYTES), dtype=torch.uint8, device=self.device)
        if n == 0:
            return out
        if self._last_stream is not None and self._last_stream != stream:
            stream.wait_stream(self._last_stream)  # the scratch buffers are still in use by the previous launch
        self._last_stream = stream
        step = self.capacity or n
        hp, op, s = headers.data_ptr(), out.data_ptr(), stream.cuda_stream
        for lo in range(0, n, step):
            m = min(step, n - lo)
            h, o = hp + lo * HEADER_BYTES, op + lo * DIGEST_BYTES  # chunk offsets keep the 16-byte alignment
            if self.algorithm == "sha256d":
                self.native.launch_sha256d_digest(h, m, o, s)
            elif self.algorithm == "scrypt":
                self.native.launch_scrypt_digest(h, m, self.xbuf.data_ptr(), self.scratch.data_ptr(), self.gap, o,
                                                 self.grid, s)
            else:
                self.native.launch_x11_digest(h, self.H.data_ptr(), self.capacity, m, o, s)
        return out

    def hash(self, headers: Sequence[bytes]) -> list[bytes]:
        """Synchronous convenience: 80-byte headers in, their 32-byte digests out."""
        headers = [bytes(h) for h in headers]
        for h in headers:
            if len(h) != HEADER_BYTES:
                raise ValueError(f"header must be {HEADER_BYTES} bytes, got {len(h)}")
        if not headers:
            return []
        host = torch.frombuffer(bytearray(b"".join(headers)), dtype=torch.uint8).view(len(headers), HEADER_BYTES)
        out = self.launch(host.to(self.device))
        torch.cuda.current_stream(self.device).synchronize()
        raw = out.cpu().numpy().tobytes()
        return [raw[i:i + DIGEST_BYTES] for i in range(0, len(raw), DIGEST_BYTES)]
