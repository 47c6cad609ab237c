"""The rows of the batched secp256k1 multiplication (csrc/include/otedama/secp256k1.h), packed and unpacked without
torch: ``ops.secp.Secp256k1Mul`` and the pool's native CPU path (``secp256k1_mul_cpu``) read and write the same bytes.

Input row, 128 bytes: ``scalar[32]`` big-endian, ``point[64]``, ``kind`` u8, 31 zero bytes. Output row, 48 bytes:
``x[32]`` big-endian, ``status`` u8, ``y_parity`` u8, 14 zero bytes.
"""
from __future__ import annotations

from typing import Sequence

ROW_BYTES = 128
OUT_BYTES = 48
MAX_ROWS = 65536
SCALAR_BYTES = 32

KIND_G = 0         # the base point; the row's point is not read
KIND_XONLY = 1     # a 32-byte x-only key, lifted to the even y
KIND_ELLSWIFT = 2  # a 64-byte ElligatorSwift encoding

OK = 0
BAD_SCALAR = 1     # 0, or at or above the group order
BAD_POINT = 2      # a KIND_XONLY x at or above p or not on the curve
BAD_KIND = 3


def pack_rows(items: Sequence[tuple]) -> bytearray:
    """``items``: ``(scalar, kind, point)`` with ``scalar`` an int in ``[0, 2^256)``, ``kind`` in ``0..255`` and
    ``point`` up to 64 bytes (``b""`` for ``KIND_G``). A bytearray, so the caller can wipe it."""
    buf = bytearray(len(items) * ROW_BYTES)
    for i, (scalar, kind, point) in enumerate(items):
        if not 0 <= scalar < 1 << 256:
            raise ValueError("a scalar is 32 bytes")
        if len(point) > 64 or not 0 <= kind <= 255:
            raise ValueError("a point is at most 64 bytes and a kind one byte")
        at = i * ROW_BYTES
        buf[at:at + SCALAR_BYTES] = scalar.to_bytes(SCALAR_BYTES, "big")
        buf[at + 32:at + 32 + len(point)] = point
        buf[at + 96] = kind
    return buf


def unpack_rows(buf, n: int) -> list[tuple]:
    """``n`` output rows -> ``[(x, y_parity, status)]``, ``x`` 32 bytes."""
    view = memoryview(buf)
    if len(view) < n * OUT_BYTES:
        raise ValueError(f"{n} output rows are {n * OUT_BYTES} bytes")
    return [(bytes(view[at:at + 32]), view[at + 33], view[at + 32]) for at in range(0, n * OUT_BYTES, OUT_BYTES)]


def wipe_scalars(buf, n: int) -> None:
    """Zero the scalar of each of the first ``n`` input rows of a writable buffer."""
    view = memoryview(buf)
    zero = bytes(SCALAR_BYTES)
    for at in range(0, n * ROW_BYTES, ROW_BYTES):
        view[at:at + SCALAR_BYTES] = zero
