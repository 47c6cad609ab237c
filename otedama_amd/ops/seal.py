"""Frame sealing op: n plaintexts with n keys in, every frame's ChaCha20-Poly1305 ``ciphertext || tag`` out, in one
enqueue.

A new job owes every Stratum V2 channel of a Noise pool two sealed frames (``stratum/noise.py``).
:class:`FrameSeal` seals a batch of them with ``otd_aead_seal`` (csrc/kernels/aead_seal.hip), one frame per lane,
with empty associated data and the Noise transport's nonce (four zero bytes, the 64-bit counter little-endian).
``aead_seal_many_cpu`` of the native extension writes the same bytes through OpenSSL; ``utils.aead.seal`` is the
oracle.

Buffers (csrc/include/otedama/aead.h, packed by ``ops/seal_rows.py``): n 64-byte heads and the padded plaintexts in,
one region of tag and padded ciphertext per frame out.
"""
from __future__ import annotations

from typing import Sequence

import torch

from otedama_amd.ops._args import ALIGN, gpu_device, launch_stream
from otedama_amd.ops._staging import Staging
from otedama_amd.ops.native import require_native
from otedama_amd.ops.seal_rows import (HEAD_BYTES, MAX_BUFFER, MAX_FRAMES, POLY_ROW_BYTES, TAG_BYTES, pack_frames,
                                       unpack_sealed, wipe_keys)


def _flat_bytes(name: str, t, device: torch.device) -> int:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1:
        raise ValueError(f"{name} must be a one-dimensional uint8 tensor")
    if t.device != device:
        raise ValueError(f"{name} must live on {device}")
    if not t.is_contiguous() or t.numel() % ALIGN or t.numel() >= MAX_BUFFER:
        raise ValueError(f"{name} must be contiguous, a multiple of {ALIGN} bytes and below 4 GiB")
    if t.numel() and t.data_ptr() % ALIGN:
        raise ValueError(f"{name} must start at a {ALIGN}-byte aligned address")
    return t.numel()


class FrameSeal:
    """Reusable launcher on one device. It owns the staging buffers of :meth:`seal`."""

    def __init__(self, device="cuda:0"):
        self.native = require_native()
        self.device = gpu_device(device, "FrameSeal")
        self._staging = Staging(self.device)  # in: heads and plaintexts, out: regions

    def launch(self, heads_and_data: torch.Tensor, n: int, out: torch.Tensor,
               stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Enqueue the seals of the ``n`` frames of ``heads_and_data`` (uint8, one-dimensional: ``n`` heads, then the
        data region; ``1 <= n < 2^24``) into ``out`` (uint8, one-dimensional, at least the furthest region's end) on
        ``stream`` (default: the current stream, which a given stream first waits for) and return ``out`` without
        synchronising. Both tensors are contiguous, 16-byte aligned, a multiple of 16 bytes and on the op's device. A
        bad argument raises ``ValueError`` before anything is enqueued. The heads are on the device and are not
        looked at here: the kernel writes nothing for a head whose length is over the limit or whose plaintext or
        region leaves the two tensors."""
        in_bytes = _flat_bytes("heads_and_data", heads_and_data, self.device)
        out_bytes = _flat_bytes("out", out, self.device)
        if not 1 <= n <= MAX_FRAMES:
            raise ValueError(f"a launch takes 1..{MAX_FRAMES} frames, not {n}")
        if in_bytes < n * HEAD_BYTES or out_bytes < n * TAG_BYTES:
            raise ValueError(f"{n} frames are at least {n * HEAD_BYTES} bytes in and {n * TAG_BYTES} bytes out")
        stream = launch_stream(self.device, stream)
        self.native.launch_aead_seal(heads_and_data.data_ptr(), in_bytes, n, out.data_ptr(), out_bytes,
                                     stream.cuda_stream)
        return out

    def seal(self, frames: Sequence[tuple]) -> list[bytes]:
        """The pool's entry: ``(key32, counter, plaintext)`` frames in (``seal_rows.pack_frames``, which checks the
        limits), the ``ciphertext || tag`` of each out, in order. One pinned buffer of heads and plaintexts goes to
        the device and one pinned buffer of regions comes back, both copies non-blocking on the current stream
        around :meth:`launch`, then one stream synchronise. The four buffers are the op's own and grow to the
        largest batch seen; the call is not re-entrant.

        Keys are secrets and the buffers are reused: a zero fill of the device input is enqueued behind the kernel,
        before the synchronise, and the key bytes of the packed bytes and of the pinned input are overwritten after
        it, also when the device call raises."""
        n = len(frames)
        if n == 0:
            return []
        packed, out_bytes = pack_frames(frames)

        def launch(dev_in, dev_out):
            self.launch(dev_in, n, dev_out)
            dev_in.zero_()

        try:
            return unpack_sealed(packed, self._staging.round_trip([packed], out_bytes, launch), n)
        finally:
            wipe_keys(packed, n)
            if self._staging.pin_in is not None:
                wipe_keys(self._staging.pin_in.numpy(), min(n, self._staging.pin_in.numel() // HEAD_BYTES))

    def _poly1305_rows(self, rows: torch.Tensor) -> torch.Tensor:
        """Test hook: the Poly1305 tags (uint8 ``[n, 16]``) of ``rows`` (uint8 ``[n, 160]``,
        ``seal_rows.pack_poly_rows``) by the kernel's own Poly1305, synchronised."""
        from otedama_amd.ops._args import byte_rows

        n = byte_rows("rows", rows, POLY_ROW_BYTES, self.device)
        stream = launch_stream(self.device, None)
        with torch.cuda.stream(stream):
            tags = torch.empty((n, TAG_BYTES), dtype=torch.uint8, device=self.device)
        self.native._launch_poly1305_rows(rows.data_ptr(), n, tags.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        return tags
