"""The host round trip of the ops' synchronous entries (``ShareVerify.results``, ``ChannelRoots.roots``): bytes in
through one pinned buffer, a launch, bytes out through another."""
from __future__ import annotations

from typing import Callable, Sequence

import torch


class Staging:
    """Four byte buffers on one device (pinned in, device in, pinned out, device out) that grow to the largest batch
    seen: to the size asked for or twice the old size, whichever is larger, from 4096 bytes. Not re-entrant."""

    def __init__(self, device: torch.device):
        self.device = device
        self.pin_in: torch.Tensor | None = None
        self.dev_in: torch.Tensor | None = None
        self.pin_out: torch.Tensor | None = None
        self.dev_out: torch.Tensor | None = None

    def _grown(self, name: str, nbytes: int, pinned: bool) -> torch.Tensor:
        buf = getattr(self, name)
        if buf is None or buf.numel() < nbytes:
            size = max(nbytes, 2 * buf.numel() if buf is not None else 4096)
            buf = (torch.empty(size, dtype=torch.uint8, pin_memory=True) if pinned
                   else torch.empty(size, dtype=torch.uint8, device=self.device))
            setattr(self, name, buf)
        return buf

    def round_trip(self, parts: Sequence[bytes], out_bytes: int,
                   launch: Callable[[torch.Tensor, torch.Tensor], object]) -> memoryview:
        """Write ``parts`` back to back into the pinned input, copy it to the device, call ``launch(device in,
        device out)`` with uint8 views of exactly the bytes in use, copy ``out_bytes`` back and synchronise: both
        copies non-blocking on the current stream, around whatever ``launch`` enqueues there. Returns the pinned
        output's first ``out_bytes`` bytes, valid until the next call."""
        in_bytes = sum(len(p) for p in parts)
        pin_in, dev_in = self._grown("pin_in", in_bytes, True), self._grown("dev_in", in_bytes, False)
        pin_out, dev_out = self._grown("pin_out", out_bytes, True), self._grown("dev_out", out_bytes, False)
        host, at = memoryview(pin_in.numpy()), 0
        for p in parts:
            host[at:at + len(p)] = p
            at += len(p)
        stream = torch.cuda.current_stream(self.device)
        dev_in[:in_bytes].copy_(pin_in[:in_bytes], non_blocking=True)
        launch(dev_in[:in_bytes], dev_out[:out_bytes])
        pin_out[:out_bytes].copy_(dev_out[:out_bytes], non_blocking=True)
        stream.synchronize()
        return memoryview(pin_out.numpy())[:out_bytes]
