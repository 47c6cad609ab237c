"""The 32-byte share record of the share-verification op (csrc/include/otedama/share_job.h ``ShareRec``), packed
and unpacked without torch, so the pool layer (pool/batch.py) can form a batch before it decides whether a GPU is
involved at all. ``ops.verify`` re-exports these. The prefix and root rows of the channel-roots op (``ops.roots``)
are packed here too, for the same reason.

    bytes 0..15   extranonce (the first ``en_size`` bytes are used, the rest are zero)
    bytes 16..19  ntime      bytes 20..23  nonce      bytes 24..27  version (full rolled version)
    bytes 28..31  index into the target table of the launch          (all little-endian)
"""
from __future__ import annotations

import struct
from typing import Sequence

RECORD_BYTES = 32
MAX_EXTRANONCE = 16
VERDICT_SHARE = 1       # hash <= targets[index]
VERDICT_NETWORK = 2     # hash <= the network target of the job's nbits
VERDICT_BAD_INDEX = 0x80  # index outside the target table; no other bit is set

_REC = struct.Struct("<16sIIII")

# The 128-byte result record of the live path (``ShareResult``): bytes 0..79 the header, 80..111 the hash, 112 the
# verdict byte, 113..127 zero.
RESULT_BYTES = 128
_RES = struct.Struct("<80s32sB15x")

# The channel-roots op (``ops.roots``): one 16-byte row per extranonce prefix in, one 32-byte merkle root out.
PREFIX_BYTES = 16
ROOT_BYTES = 32


def pack_records(shares: Sequence[tuple], target_indices: Sequence[int], en_size: int) -> bytes:
    """``shares``: ``(extranonce, ntime, nonce, version)`` tuples, every extranonce exactly ``en_size`` bytes (a
    longer or shorter one is a different coinbase and raises ``ValueError``). Integers are taken modulo 2^32, as
    ``PoolServer.header_for`` packs them."""
    if not 1 <= en_size <= MAX_EXTRANONCE:
        raise ValueError(f"en_size must be in 1..{MAX_EXTRANONCE}")
    if len(shares) != len(target_indices):
        raise ValueError("one target index per share")
    out = bytearray(RECORD_BYTES * len(shares))
    for i, ((en, ntime, nonce, version), idx) in enumerate(zip(shares, target_indices)):
        en = bytes(en)
        if len(en) != en_size:
            raise ValueError(f"extranonce of share {i} is {len(en)} bytes, the job takes {en_size}")
        if not 0 <= idx < 1 << 32:
            raise ValueError(f"target index of share {i} does not fit 32 bits")
        _REC.pack_into(out, RECORD_BYTES * i, en, ntime & 0xFFFFFFFF, nonce & 0xFFFFFFFF, version & 0xFFFFFFFF, idx)
    return bytes(out)


def unpack_records(records: bytes, en_size: int) -> tuple[list[tuple], list[int]]:
    """Inverse of :func:`pack_records`: ``(shares, target_indices)``."""
    if not 1 <= en_size <= MAX_EXTRANONCE:
        raise ValueError(f"en_size must be in 1..{MAX_EXTRANONCE}")
    if len(records) % RECORD_BYTES:
        raise ValueError(f"records must be a multiple of {RECORD_BYTES} bytes")
    shares, indices = [], []
    for en, ntime, nonce, version, idx in _REC.iter_unpack(records):
        shares.append((en[:en_size], ntime, nonce, version))
        indices.append(idx)
    return shares, indices


def unpack_results(raw, n: int | None = None) -> list[tuple[bytes, bytes, int]]:
    """Result records (bytes, bytearray or memoryview; the first ``n`` if given) -> ``(header, hash, verdict byte)``
    per share, the list ``pool.batch.check_shares`` returns."""
    view = memoryview(raw)
    if n is not None:
        if n < 0 or n * RESULT_BYTES > len(view):
            raise ValueError(f"{n} result records do not fit {len(view)} bytes")
        view = view[:n * RESULT_BYTES]
    if len(view) % RESULT_BYTES:
        raise ValueError(f"results must be a multiple of {RESULT_BYTES} bytes")
    return list(_RES.iter_unpack(view))


def pack_prefixes(prefixes: Sequence[bytes], en_size: int) -> bytes:
    """Prefix rows as ``otd_channel_roots`` and ``share_roots_cpu`` read them: every prefix exactly ``en_size``
    bytes (anything else raises ``ValueError``), zero-padded to 16."""
    if not 1 <= en_size <= MAX_EXTRANONCE:
        raise ValueError(f"en_size must be in 1..{MAX_EXTRANONCE}")
    pad = bytes(PREFIX_BYTES - en_size)
    for i, p in enumerate(prefixes):
        if len(p) != en_size:
            raise ValueError(f"prefix {i} is {len(p)} bytes, the job takes {en_size}")
    return b"".join(bytes(p) + pad for p in prefixes)


def unpack_roots(raw) -> list[bytes]:
    """Root rows (bytes, bytearray or memoryview) -> one 32-byte root per prefix."""
    raw = bytes(raw)
    if len(raw) % ROOT_BYTES:
        raise ValueError(f"roots must be a multiple of {ROOT_BYTES} bytes")
    return [raw[i:i + ROOT_BYTES] for i in range(0, len(raw), ROOT_BYTES)]
