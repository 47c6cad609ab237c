"""secp256k1 multiplication op: n scalars and n points in, the x of every product out, in one enqueue.

A Noise NX responder owes every accepted connection three multiplications: its ephemeral key's public point, and the
two Diffie-Hellman results against the initiator's key (``stratum/noise.py``). :class:`Secp256k1Mul` computes a batch
of them with ``otd_secp256k1_mul`` (csrc/kernels/secp256k1_mul.hip), one row per lane. ``secp256k1_mul_cpu`` of the
native extension writes the same bytes in plain C++; ``btccrypto.point_mul``, ``ellswift.ecdh_x`` and ``noise.dh`` are
the oracle.

Rows (csrc/include/otedama/secp256k1.h, packed by ``ops/secp_rows.py``): 128 bytes in, 48 bytes out.
"""
from __future__ import annotations

from typing import Sequence

import torch

from otedama_amd.ops._args import byte_rows, gpu_device, launch_stream
from otedama_amd.ops._staging import Staging
from otedama_amd.ops.native import require_native
from otedama_amd.ops.secp_rows import MAX_ROWS, OUT_BYTES, ROW_BYTES, pack_rows, unpack_rows, wipe_scalars


class Secp256k1Mul:
    """Reusable launcher on one device. It owns the staging buffers of :meth:`mul`."""

    def __init__(self, device="cuda:0"):
        self.native = require_native()
        self.device = gpu_device(device, "Secp256k1Mul")
        self._staging = Staging(self.device)  # in: rows, out: result rows

    def launch(self, rows: torch.Tensor, out: torch.Tensor | None = None,
               stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """Enqueue the products of ``rows`` (uint8 ``[n, 128]``, ``1 <= n <= 65536``, contiguous, 16-byte aligned,
        on the op's device) on ``stream`` (default: the current stream, which a given stream first waits for) and
        return the result rows as uint8 ``[n, 48]`` (``out`` if given: that shape, contiguous, 16-byte aligned, on
        the op's device) without synchronising. A bad argument raises ``ValueError`` before anything is enqueued."""
        n = byte_rows("rows", rows, ROW_BYTES, self.device)
        if not 1 <= n <= MAX_ROWS:
            raise ValueError(f"a launch takes 1..{MAX_ROWS} rows, not {n}")
        if out is not None:
            byte_rows("out", out, OUT_BYTES, self.device, rows=n)
        stream = launch_stream(self.device, stream)
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty((n, OUT_BYTES), dtype=torch.uint8, device=self.device)
        self.native.launch_secp256k1_mul(rows.data_ptr(), n, out.data_ptr(), stream.cuda_stream)
        return out

    def mul(self, items: Sequence[tuple]) -> list[tuple]:
        """The pool's entry: ``(scalar, kind, point)`` items in (``secp_rows.pack_rows``), ``(x, y_parity, status)``
        out, in order. One pinned buffer of rows goes to the device and one pinned buffer of results comes back,
        both copies non-blocking on the current stream around :meth:`launch`, then one stream synchronise. The four
        buffers are the op's own and grow to the largest batch seen; the call is not re-entrant.

        Scalars are secrets and the buffers are reused: a zero fill of the device input is enqueued behind the
        kernel, before the synchronise, and the scalar bytes of the pinned input are overwritten after it, also when
        the device call raises."""
        n = len(items)
        if n == 0:
            return []
        if n > MAX_ROWS:
            raise ValueError(f"at most {MAX_ROWS} rows a call")
        packed = pack_rows(items)

        def launch(dev_in, dev_out):
            self.launch(dev_in.view(n, ROW_BYTES), out=dev_out.view(n, OUT_BYTES))
            dev_in.zero_()

        try:
            return unpack_rows(self._staging.round_trip([packed], n * OUT_BYTES, launch), n)
        finally:
            wipe_scalars(packed, n)
            if self._staging.pin_in is not None:
                wipe_scalars(self._staging.pin_in.numpy(), min(n, self._staging.pin_in.numel() // ROW_BYTES))
