"""Blocks no header produces, for the ten X11 stage kernels that read the digest planes.

tests/test_x11_gpu.py feeds each stage the previous stage's output for random headers, so no stage kernel other than
BLAKE has met an all-zero block, an all-ones block, a single-bit block or a block built to push its arithmetic to its
bounds. This module builds such a set once (seeded, about 2 600 blocks of 64 bytes) and drives one stage kernel on
it; tests/test_x11_stage_inputs_cpu.py holds the set to its own conditions and tests/test_x11_stage_inputs_gpu.py
compares every position of every stage with the CPU oracle ``N.x11_stage``.

Classes (``classes()`` keeps them apart, ``all_blocks()`` is their concatenation in this order):
  constant      256  ``bytes([v]) * 64``: every LDS table index (Groestl, the AES tables of SHAvite and ECHO) in every
                     lane that holds one
  one-bit-set   512  exactly one bit set
  one-bit-clear 512  exactly one bit clear
  words          28  u64 patterns for carry chains and rotates (BMW, Skein, Keccak, JH, Luffa)
  simd-centred  512  for NTT index i and sign s: x[j] = 255 where s * centred(41^(ij) mod 257) > 0, else 0. The block
                     drives coefficient i's unreduced sum  sum_j x[j] * centred(41^(ij))  to its extreme of that sign.
  simd-table    512  the same construction on the byte the kernel's SIMD_PT table holds: x[j] = 255 where
                     (41^(ij) mod 257) - 1 >= 128 (sign +), or where it is < 128 (sign -).
  random        256  seeded random blocks, the control

41^(ij) mod 257 is never 0, and it is >= 129 exactly when its centred form is negative, so simd-table(i, s) is the
same block as simd-centred(i, -s): the two classes hold the same 512 blocks in another order. Both are kept, as two
classes, because the table form is what the kernel's dot product sees; on the GPU each of these blocks then meets four
lanes instead of two. Duplicates across classes (constant 0x00 / 0xFF also arise at i = 0) are harmless.
"""
from __future__ import annotations

import functools
import random
import struct

ALPHA = 41            # evaluation root of SIMD's message NTT over F_257 (csrc/cpu/x11_cpu.cpp simd_expand)
RANDOM_SEED = 1111
ROTATE = 37           # the second run of each stage shifts every block by this many positions
SPARE = 300           # columns past the blocks: they hold the canary
CANARY = 0x5DA7C3E1B2F49687
STAGES = ("blake", "bmw", "groestl", "skein", "jh", "keccak", "luffa", "cubehash", "shavite", "simd", "echo")
CLASS_SIZES = {"constant": 256, "one-bit-set": 512, "one-bit-clear": 512, "words": 28, "simd-centred": 512,
               "simd-table": 512, "random": 256}


def centred(p: int) -> int:
    """A residue mod 257 in [-128, 128]."""
    p %= 257
    return p if p <= 128 else p - 257


def alpha_pow(e: int) -> int:
    return pow(ALPHA, e % 256, 257)  # 41 has order 256 in F_257*


def simd_centred_block(i: int, s: int) -> bytes:
    return bytes(255 if s * centred(alpha_pow(i * j)) > 0 else 0 for j in range(64))


def simd_table_block(i: int, s: int) -> bytes:
    return bytes(255 if ((alpha_pow(i * j) - 1 >= 128) == (s > 0)) else 0 for j in range(64))


def _words(ws) -> bytes:
    return struct.pack("<8Q", *ws)


def _word_blocks() -> list[bytes]:
    ones = 0xFFFFFFFFFFFFFFFF
    out = []
    for k in range(8):
        for v in (0, 1, 0x8000000000000000):
            out.append(_words([v if w == k else ones for w in range(8)]))
    for v in (0x00000000FFFFFFFF, 0xFFFFFFFF00000000, 0x7FFFFFFFFFFFFFFF, 0x0000000100000000):
        out.append(_words([v] * 8))
    return out


def _one_bit(bit: int, clear: bool) -> bytes:
    b = bytearray(b"\xff" * 64 if clear else bytes(64))
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def classes() -> dict[str, tuple[bytes, ...]]:
    rng = random.Random(RANDOM_SEED)
    return {
        "constant": tuple(bytes([v]) * 64 for v in range(256)),
        "one-bit-set": tuple(_one_bit(b, False) for b in range(512)),
        "one-bit-clear": tuple(_one_bit(b, True) for b in range(512)),
        "words": tuple(_word_blocks()),
        "simd-centred": tuple(simd_centred_block(i, s) for i in range(256) for s in (1, -1)),
        "simd-table": tuple(simd_table_block(i, s) for i in range(256) for s in (1, -1)),
        "random": tuple(rng.randbytes(64) for _ in range(256)),
    }


@functools.lru_cache(maxsize=None)
def all_blocks() -> tuple[bytes, ...]:
    return tuple(b for name in CLASS_SIZES for b in classes()[name])


def rotated(blocks, k: int):
    """Position p holds block p - k (mod m)."""
    k %= len(blocks)
    return tuple(blocks[-k:] + blocks[:-k]) if k else tuple(blocks)


def native():
    from otedama_amd.ops.native import require_native

    return require_native()


_oracle_cache: dict[tuple[int, bytes], bytes] = {}


def oracle(N, st: int, blocks) -> list[bytes]:
    """``N.x11_stage(st, block)`` of every block, each distinct (stage, block) computed once per process. x11_stage
    holds the GIL (unlike ``N.x11``), so threads would not help: ~21 000 calls of a few microseconds each, in turn."""
    out = []
    for b in blocks:
        d = _oracle_cache.get((st, b))
        if d is None:
            d = _oracle_cache[st, b] = N.x11_stage(st, b)
        out.append(d)
    return out


def compared(st: int, digest: bytes) -> bytes:
    """The bytes a stage is held to: all 64, for ECHO (stage 10) the 32 of the chain digest."""
    return digest[:32] if st == 10 else digest


def assert_positions_equal(st: int, got, want, what: str) -> None:
    """Byte equality at every position; a failure names the first differing positions."""
    assert len(got) == len(want), (len(got), len(want))
    bad = [p for p in range(len(want)) if compared(st, got[p]) != compared(st, want[p])]
    if bad:
        p = bad[0]
        raise AssertionError(f"{what}: stage {st} ({STAGES[st]}): {len(bad)} of {len(want)} positions differ, first "
                             f"positions {bad[:8]}; position {p}: got {compared(st, got[p]).hex()}, "
                             f"want {compared(st, want[p]).hex()}")


class StageRig:
    """The planes of one ``X11Search`` with room for m blocks and SPARE canary columns, so the stride is not m."""

    def __init__(self, N, m: int, device="cuda:0"):
        from otedama_amd.ops.search import X11Search

        self.N, self.m, self.batch = N, m, m + SPARE
        self.search = X11Search(device, batch=self.batch)
        self.params = N.x11_prepare(bytes(80), bytes(32))

    def run(self, st: int, blocks) -> tuple[list[bytes], bool]:
        """Stage ``st`` (1..10) on ``blocks`` (one per position): (64 bytes per position, canary columns kept).
        Word k of block i, as a little-endian u64, goes to plane k, column i."""
        import numpy as np
        import torch

        assert 1 <= st <= 10 and len(blocks) == self.m and all(len(b) == 64 for b in blocks)
        host = np.full((8, self.batch), CANARY, dtype="<u8")
        host[:, :self.m] = np.frombuffer(b"".join(blocks), dtype="<u8").reshape(self.m, 8).T
        s = self.search
        planes = s.H.view(8, self.batch)
        planes.copy_(torch.from_numpy(host.view(np.int64)))
        stream = torch.cuda.current_stream(s.device)
        self.N.launch_x11_stage(self.params, st, 0, s.H.data_ptr(), self.batch, self.m, 0, 0, stream.cuda_stream)
        torch.cuda.synchronize(s.device)
        back = planes.cpu().numpy().view("<u8")
        raw = np.ascontiguousarray(back[:, :self.m].T).tobytes()
        kept = bool((back[:, self.m:] == np.uint64(CANARY)).all())
        return [raw[64 * i:64 * i + 64] for i in range(self.m)], kept
