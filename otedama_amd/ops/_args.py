"""Argument and stream rules shared by the ops that take caller-owned tensors (digest, verify, search)."""
from __future__ import annotations

import torch

ALIGN = 16  # the kernels move headers, digests, records and targets as 16-byte vectors


def gpu_device(device, who: str) -> torch.device:
    """``device`` as a CUDA ``torch.device`` with its index resolved (the current device when it names none);
    ``ValueError`` naming ``who`` for any other kind of device."""
    d = torch.device(device)
    if d.type != "cuda":
        raise ValueError(f"{who} needs a GPU device")
    return d if d.index is not None else torch.device("cuda", torch.cuda.current_device())


def byte_rows(name: str, t, width: int, device: torch.device, rows: int | None = None) -> int:
    """Check that ``t`` is a contiguous uint8 ``[n, width]`` tensor on ``device`` (``n == rows`` if given) that
    starts at a 16-byte aligned address unless it is empty, and return ``n``. Anything else raises ``ValueError``
    naming the argument."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError(f"{name} must be a uint8 tensor")
    if t.dim() != 2 or t.shape[1] != width or (rows is not None and t.shape[0] != rows):
        raise ValueError(f"{name} must have shape [{'n' if rows is None else rows}, {width}]")
    if t.device != device:
        raise ValueError(f"{name} must live on {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.shape[0] and t.data_ptr() % ALIGN:
        raise ValueError(f"{name} must start at a {ALIGN}-byte aligned address")
    return t.shape[0]


def launch_stream(device: torch.device, stream: torch.cuda.Stream | None) -> torch.cuda.Stream:
    """The stream a launch goes to: the current stream of ``device`` for ``None``; a given stream first waits for the
    current one, on which the caller produced the launch's inputs."""
    cur = torch.cuda.current_stream(device)
    if stream is None:
        return cur
    if stream != cur:
        stream.wait_stream(cur)
    return stream
