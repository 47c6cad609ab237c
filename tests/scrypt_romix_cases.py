"""Cases and helpers that hold every scrypt ROMix kernel to bytes (tests/test_scrypt_romix_bytes_gpu.py).

``launch_scrypt_romix`` (csrc/kernels/scrypt_search.hip) dispatches a gap code and the environment to one of nine
kernels. Each entry of VARIANTS is one way through that dispatch: an id, the gap code (an int, or the name of the native
module's constant), the environment it needs and the allocation grid. This module needs neither a GPU nor the
extension to import: tests/test_scrypt_romix_cases_cpu.py holds the cases to their own conditions on any machine, and
tests/scrypt_romix_child.py runs the digest check in a process of its own for the one switch that is read once per
process (OTEDAMA_SCRYPT_POLL).

Two paths reach the kernels:
  * the digest path, ``N.launch_scrypt_digest`` called directly on one DigestRig per variant: n unrelated headers of
    the pool in, n digests out, each compared with ``hashlib.scrypt``;
  * the search path, ``ScryptSearch`` with the all-ones target, for what one header per lane slot cannot reach (a pad
    slot used again on a later grid-stride trip, ``coop2`` above grid * 256): every lane's post-ROMix state is read
    from ``xbuf`` and finished on the CPU with ``scrypt_digest_from_state`` (``hashlib.pbkdf2_hmac``).

Every variant sees the same headers, so the bytes a correct earlier launch left behind are the right answer of the
next one. Before every launch the state buffer, the whole pad and the result rows are therefore filled with POISON,
and the rows after the batch hold CANARY and must keep it.
"""
from __future__ import annotations

import functools
import hashlib
import os
import random
import struct
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

POOL_SIZE = 512
POOL_SEED = 2024
SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)  # wave 64, coop2 pair 128, block 256, +-1 each
SPARE_ROWS = 256   # result rows after row n: they hold the canary
POISON = 0xB6      # state buffer, pad and result rows before every launch
CANARY = 0x5D
CHILD_SIZES = (65, 512)

SEARCH_SEED = 4242
SEARCH_BASE = 0xFFFFFF00  # every search window wraps 2^32
ALL_ONES_TARGET = b"\xff" * 32

ENV_VARS = ("OTEDAMA_SCRYPT_SEGMENTS", "OTEDAMA_SCRYPT_SEG_GRID", "OTEDAMA_SCRYPT_POLL")


@dataclass(frozen=True)
class Variant:
    id: str
    gap: int | str                      # 1 / 2 / 4, or the name of the native constant
    env: dict = field(default_factory=dict)
    grid: int = 2
    child: bool = False                 # needs a fresh process (OTEDAMA_SCRYPT_POLL is read once)

    @property
    def segments(self) -> int:
        return int(self.env.get("OTEDAMA_SCRYPT_SEGMENTS", 0))


def _seg(s: int) -> Variant:
    return Variant(f"seg{s}", "SCRYPT_COOP", {"OTEDAMA_SCRYPT_SEGMENTS": str(s)})


VARIANTS = (
    Variant("lane1", 1),
    Variant("lane2", 2),
    Variant("lane4", 4),
    Variant("w8", "SCRYPT_LANE_W8"),
    Variant("coop", "SCRYPT_COOP"),
    Variant("coop2", "SCRYPT_COOP2"),
    Variant("split", "SCRYPT_COOP_SPLIT"),
    _seg(1), _seg(3), _seg(8), _seg(64),
    Variant("seg6-grid1", "SCRYPT_COOP", {"OTEDAMA_SCRYPT_SEGMENTS": "6", "OTEDAMA_SCRYPT_SEG_GRID": "1"}, grid=4),
    Variant("seg32-resident", "SCRYPT_COOP",
            {"OTEDAMA_SCRYPT_SEGMENTS": "32", "OTEDAMA_SCRYPT_SEG_GRID": "resident"}),
    Variant("coop-nopoll", "SCRYPT_COOP", {"OTEDAMA_SCRYPT_POLL": "0"}, child=True),
)


def variant(vid: str) -> Variant:
    (v,) = [v for v in VARIANTS if v.id == vid]
    return v


def gap_code(N, v: Variant) -> int:
    return v.gap if isinstance(v.gap, int) else getattr(N, v.gap)


def capacity(v: Variant) -> int:
    """Headers one digest launch of the variant takes: one per lane slot of its allocation grid."""
    return v.grid * 256


@dataclass(frozen=True)
class SearchCase:
    id: str
    kernel: str          # ScryptSearch(kernel=...)
    gap: int | str       # ScryptSearch(gap=...): 1 lets ``kernel`` choose the code
    lanes_per_slot: int
    count: int
    env: dict = field(default_factory=dict)
    grid: int = 1


SEARCH_CASES = (
    SearchCase("lane-gap2-3trips-700", "lane", 2, 3, 700),         # the third trip is ragged
    SearchCase("coop-2trips-389", "coop", 1, 2, 389),              # rounds to 448: the second trip is partial
    SearchCase("coop2-512", "coop2", 1, 1, 512),                   # both streams full
    SearchCase("coop2-321", "coop2", 1, 1, 321),                   # B stream of the last wave partly past count
    SearchCase("coop2-2trips-700", "coop2", 1, 2, 700),
    SearchCase("w8-2trips-300", "lane", "SCRYPT_LANE_W8", 2, 300),
    # the segmented kernel holds one hash per lane slot; above that the launcher must fall back to the one-launch
    # kernel, and the digests must still be exact
    SearchCase("seg4-falls-back-389", "coop", 1, 2, 389, {"OTEDAMA_SCRYPT_SEGMENTS": "4"}),
)
SEARCH_LANES = max(c.count for c in SEARCH_CASES)


def scrypt(h: bytes) -> bytes:
    return hashlib.scrypt(h, salt=h, n=1024, r=1, p=1, dklen=32)


def scrypt_many(headers) -> tuple[bytes, ...]:
    """hashlib.scrypt releases the GIL: ~3 ms per header, spread over at most 16 threads."""
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return tuple(ex.map(scrypt, headers, chunksize=16))


def known_answer_header() -> bytes | None:
    from otedama_amd.models.algorithms import KNOWN_ANSWERS

    return bytes.fromhex(KNOWN_ANSWERS["scrypt"][0]) if "scrypt" in KNOWN_ANSWERS else None


def build_headers() -> tuple[bytes, ...]:
    """POOL_SIZE headers of 80 bytes: seeded random bytes, with the all-zero header at 1, the all-0xFF header at 2
    and (if the project lists one) the scrypt known-answer header at 3."""
    rng = random.Random(POOL_SEED)
    hs = [rng.randbytes(80) for _ in range(POOL_SIZE)]
    hs[1], hs[2] = bytes(80), b"\xff" * 80
    ka = known_answer_header()
    if ka is not None:
        hs[3] = ka
    return tuple(hs)


@functools.lru_cache(maxsize=None)
def pool() -> tuple[tuple[bytes, ...], tuple[bytes, ...]]:
    """(headers, hashlib.scrypt digests), computed once per process."""
    hs = build_headers()
    return hs, scrypt_many(hs)


def search_prefix() -> bytes:
    return random.Random(SEARCH_SEED).randbytes(76)


def search_header(i: int) -> bytes:
    return search_prefix() + struct.pack("<I", (SEARCH_BASE + i) & 0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def search_oracle() -> tuple[bytes, ...]:
    """hashlib.scrypt of lanes 0..SEARCH_LANES-1 of the one window every search case runs a prefix of."""
    return scrypt_many([search_header(i) for i in range(SEARCH_LANES)])


def mismatches(got, want) -> list[int]:
    assert len(got) == len(want), (len(got), len(want))
    return [i for i in range(len(want)) if got[i] != want[i]]


def assert_digests_equal(got, want, what: str) -> None:
    """Byte equality of every digest; a failure names the first differing indices."""
    bad = mismatches(got, want)
    if bad:
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} digests differ, first indices {bad[:8]}; "
                             f"index {i}: got {bytes(got[i]).hex()}, want {bytes(want[i]).hex()}")


# ------------------------------------------------------------------------------------------------- pure-Python ROMix

# Salsa20 double round as (target, first operand, second operand, rotation): x[t] ^= rol(x[a] + x[b], r)
_SALSA_STEPS = (
    (4, 0, 12, 7), (8, 4, 0, 9), (12, 8, 4, 13), (0, 12, 8, 18),
    (9, 5, 1, 7), (13, 9, 5, 9), (1, 13, 9, 13), (5, 1, 13, 18),
    (14, 10, 6, 7), (2, 14, 10, 9), (6, 2, 14, 13), (10, 6, 2, 18),
    (3, 15, 11, 7), (7, 3, 15, 9), (11, 7, 3, 13), (15, 11, 7, 18),
    (1, 0, 3, 7), (2, 1, 0, 9), (3, 2, 1, 13), (0, 3, 2, 18),
    (6, 5, 4, 7), (7, 6, 5, 9), (4, 7, 6, 13), (5, 4, 7, 18),
    (11, 10, 9, 7), (8, 11, 10, 9), (9, 8, 11, 13), (10, 9, 8, 18),
    (12, 15, 14, 7), (13, 12, 15, 9), (14, 13, 12, 13), (15, 14, 13, 18),
)


def _salsa20_8(b: list[int]) -> list[int]:
    x = list(b)
    for _ in range(4):
        for t, p, q, r in _SALSA_STEPS:
            v = (x[p] + x[q]) & 0xFFFFFFFF
            x[t] ^= ((v << r) | (v >> (32 - r))) & 0xFFFFFFFF
    return [(x[i] + b[i]) & 0xFFFFFFFF for i in range(16)]


def _blockmix(x: list[int]) -> list[int]:
    """BlockMix_salsa20/8 at r = 1: X = B0 | B1 -> Y0 | Y1."""
    y0 = _salsa20_8([x[k] ^ x[16 + k] for k in range(16)])
    y1 = _salsa20_8([y0[k] ^ x[16 + k] for k in range(16)])
    return y0 + y1


def romix_1024(b128: bytes) -> bytes:
    """scrypt's ROMix (N = 1024, r = 1) of one 128-byte block, straight from RFC 7914. ~1 s of Python."""
    x = list(struct.unpack("<32I", b128))
    v = []
    for _ in range(1024):
        v.append(x)
        x = _blockmix(x)
    for _ in range(1024):
        t = v[x[16] & 1023]
        x = _blockmix([x[k] ^ t[k] for k in range(32)])
    return struct.pack("<32I", *x)


def post_romix_state(header80: bytes) -> bytes:
    """What a ROMix kernel must leave in xbuf for this header: ROMix of PBKDF2(header, header, 1, 128)."""
    return romix_1024(hashlib.pbkdf2_hmac("sha256", header80, header80, 1, 128))


# ------------------------------------------------------------------------------------------------------ GPU helpers

def native():
    from otedama_amd.ops.native import require_native

    return require_native()


def _fill(t, byte: int) -> None:
    t.fill_(byte)


class DigestRig:
    """The buffers of one variant's digest launches, reused for every batch size: the pool on the device, the state
    buffer and pad of ``grid`` blocks, and capacity + SPARE_ROWS result rows."""

    def __init__(self, N, gap: int, grid: int, device="cuda:0"):
        import torch

        self.N, self.gap, self.grid, self.device = N, gap, grid, torch.device(device)
        hs, _ = pool()
        self.headers = torch.frombuffer(bytearray(b"".join(hs)), dtype=torch.uint8).view(len(hs), 80).to(self.device)
        self.xbuf = torch.empty(grid * 256 * 128, dtype=torch.uint8, device=self.device)
        self.scratch = torch.empty(N.scrypt_scratch_bytes(grid, gap), dtype=torch.uint8, device=self.device)
        self.out = torch.empty((POOL_SIZE + SPARE_ROWS, 32), dtype=torch.uint8, device=self.device)

    def run(self, n: int) -> tuple[list[bytes], bool]:
        """Digests of the first n pool headers, and whether the SPARE_ROWS rows after them kept the canary."""
        import torch

        assert 0 < n <= min(POOL_SIZE, self.grid * 256), n
        for buf in (self.xbuf, self.scratch, self.out):
            _fill(buf, POISON)
        _fill(self.out[n:n + SPARE_ROWS], CANARY)
        stream = torch.cuda.current_stream(self.device)
        self.N.launch_scrypt_digest(self.headers.data_ptr(), n, self.xbuf.data_ptr(), self.scratch.data_ptr(),
                                    self.gap, self.out.data_ptr(), self.grid, stream.cuda_stream)
        stream.synchronize()
        raw = self.out[:n + SPARE_ROWS].cpu().numpy().tobytes()
        rows = [raw[32 * i:32 * i + 32] for i in range(n)]
        return rows, raw[32 * n:] == bytes([CANARY]) * (32 * SPARE_ROWS)


def check_digest_sizes(rig: DigestRig, sizes) -> dict[int, dict]:
    """Every batch size on the rig's buffers: {n: {"bad": differing indices, "canary": kept}}."""
    _, want = pool()
    res = {}
    for n in sizes:
        rows, kept = rig.run(n)
        res[n] = {"bad": mismatches(rows, want[:n]), "canary": kept, "first": rows[0].hex()}
    return res


def run_search_case(N, c: SearchCase, device="cuda:0") -> tuple[list[int], list[bytes]]:
    """The case's search with the all-ones target on poisoned buffers: (reported nonces, per-lane digests rebuilt
    from the post-ROMix states in xbuf)."""
    import torch

    from otedama_amd.ops.search import ScryptSearch
    from otedama_amd.ops.smoke_checks import scrypt_digest_from_state

    gap = c.gap if isinstance(c.gap, int) else getattr(N, c.gap)
    sc = ScryptSearch(device, cap=1024, grid=c.grid, gap=gap, lanes_per_slot=c.lanes_per_slot, kernel=c.kernel)
    assert c.count <= sc.batch and c.count <= sc.cap
    _fill(sc.xbuf, POISON)
    _fill(sc.scratch, POISON)
    hits = sc.search(search_header(0), ALL_ONES_TARGET, SEARCH_BASE, c.count)
    torch.cuda.synchronize(sc.device)
    states = sc.xbuf[:128 * c.count].cpu().numpy().tobytes()
    return hits, [scrypt_digest_from_state(search_header(i), states[128 * i:128 * i + 128]) for i in range(c.count)]


def search_window(count: int) -> list[int]:
    return sorted((SEARCH_BASE + i) & 0xFFFFFFFF for i in range(count))
