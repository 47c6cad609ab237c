"""The buffers of the batched frame seal (csrc/include/otedama/aead.h), packed and unpacked without torch:
``ops.seal.FrameSeal`` and the pool's native CPU path (``aead_seal_many_cpu``) read and write the same bytes.

Input: ``n`` heads of 64 bytes, then the data region. A head is ``key[32]``, ``counter`` u64, ``len`` u32, ``in_off``
u32, ``out_off`` u32 and 12 zero bytes, little-endian. ``in_off`` is the plaintext's byte offset from the start of the
input and ``out_off`` that of the frame's region in the output; both are multiples of 16, and every plaintext is
zero-padded to a multiple of 16 bytes. :func:`pack_frames` lays plaintexts and regions out back to back in frame
order.

Output: per frame a region of ``16 + roundup16(len)`` bytes: the tag, the ciphertext, zeros up to the next multiple
of 16. :func:`unpack_sealed` turns a region into the ``ciphertext || tag`` that ``utils.aead.seal`` returns.
"""
from __future__ import annotations

import struct
from typing import Sequence

HEAD_BYTES = 64
KEY_BYTES = 32
TAG_BYTES = 16
SEAL_MAX_PLAIN = 2048
MAX_FRAMES = (1 << 24) - 1
MAX_BUFFER = 1 << 32  # offsets are 32-bit

_HEAD = struct.Struct("<32sQIII12x")
_PLACE = struct.Struct("<40xI4xI12x")  # a head's len and out_off
_ZEROS = [bytes(i) for i in range(16)]


def pack_frames(frames: Sequence[tuple]) -> tuple[bytearray, int]:
    """``frames``: ``(key32, counter, plaintext)`` with ``counter`` in ``[0, 2^64 - 1)`` (the Noise transport never
    uses 2^64 - 1) and a plaintext of at most ``SEAL_MAX_PLAIN`` bytes. Returns the input buffer, a bytearray so
    the caller can wipe its keys, and the size of the output buffer."""
    n = len(frames)
    if not 1 <= n <= MAX_FRAMES:
        raise ValueError(f"a call takes 1..{MAX_FRAMES} frames, not {n}")
    in_off, out_off = n * HEAD_BYTES, 0
    heads, data = [], []
    pack, last_counter = _HEAD.pack, (1 << 64) - 2
    for key, counter, plain in frames:  # one pass, joined once: a job's fan-out is tens of thousands of frames
        size = len(plain)
        if len(key) != KEY_BYTES:
            raise ValueError("a key is 32 bytes")
        if not 0 <= counter <= last_counter:
            raise ValueError("a counter is in [0, 2^64 - 1)")
        if size > SEAL_MAX_PLAIN:
            raise ValueError(f"a frame is at most {SEAL_MAX_PLAIN} bytes")
        heads.append(pack(key, counter, size, in_off, out_off))
        data.append(plain)
        pad = -size & 15
        if pad:
            data.append(_ZEROS[pad])
        in_off += size + pad
        out_off += TAG_BYTES + size + pad
    if in_off >= MAX_BUFFER or out_off >= MAX_BUFFER:
        raise ValueError("a call's buffers stay below 4 GiB")
    buf = bytearray(b"".join(heads))
    buf += b"".join(data)
    return buf, out_off


def unpack_sealed(packed, out, n: int) -> list[bytes]:
    """The ``ciphertext || tag`` of each of the ``n`` frames of ``packed`` from the output buffer ``out``. Reads the
    lengths and offsets from the heads, which :func:`wipe_keys` leaves in place."""
    if len(packed) < n * HEAD_BYTES:
        raise ValueError(f"{n} heads are {n * HEAD_BYTES} bytes")
    out = bytes(out)
    sealed = []
    for size, dst in _PLACE.iter_unpack(memoryview(packed)[:n * HEAD_BYTES]):
        end = dst + TAG_BYTES + size
        if end > len(out):
            raise ValueError(f"frame {len(sealed)}'s region lies outside the {len(out)}-byte output")
        sealed.append(out[dst + TAG_BYTES:end] + out[dst:dst + TAG_BYTES])
    return sealed


def wipe_keys(buf, n: int) -> None:
    """Zero the key of each of the first ``n`` heads of a writable buffer."""
    view = memoryview(buf)
    zero = bytes(KEY_BYTES)
    for at in range(0, n * HEAD_BYTES, HEAD_BYTES):
        view[at:at + KEY_BYTES] = zero


# The Poly1305 test entry: key r | s [32], len u32, 12 zero bytes, message[112] -> a 16-byte tag.
POLY_ROW_BYTES = 160
POLY_MAX_MSG = 112


def pack_poly_rows(rows: Sequence[tuple]) -> bytearray:
    """``rows``: ``(key32, message)`` with a message of at most ``POLY_MAX_MSG`` bytes."""
    buf = bytearray(len(rows) * POLY_ROW_BYTES)
    for i, (key, msg) in enumerate(rows):
        if len(key) != KEY_BYTES or len(msg) > POLY_MAX_MSG:
            raise ValueError("a row is a 32-byte key and at most 112 bytes of message")
        at = i * POLY_ROW_BYTES
        buf[at:at + KEY_BYTES] = key
        struct.pack_into("<I", buf, at + 32, len(msg))
        buf[at + 48:at + 48 + len(msg)] = msg
    return buf
