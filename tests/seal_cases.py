"""Shared cases of the frame-seal tests (test_seal_cpu.py, test_seal_gpu.py, test_noise_cork.py, test_pool_seal.py):
batches of ``(key32, counter, plaintext)`` frames with their ``utils.aead.seal`` oracle, and Poly1305 rows with a
big-integer oracle. Everything is seeded."""
import functools
import random
import struct

from otedama_amd.utils import aead

# every length 0..130, then the edges of 64-byte ChaCha blocks, of 16-byte Poly blocks and of the op's limit
LENGTHS = list(range(131)) + [191, 192, 193, 255, 256, 257, 1023, 1024, 2047, 2048]
SIZES = [1, 63, 64, 65, 257]  # one lane, a wave less one, a wave, a wave and one, a block and one
COUNTERS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 2]
JOB_BYTES = 55  # an encoded NewMiningJob


def _rnd(tag: str) -> random.Random:
    return random.Random(f"seal-cases.{tag}")


def _key(r: random.Random, i: int) -> bytes:
    return (r.randbytes(32), bytes(32), b"\xff" * 32)[0 if i % 7 < 5 else i % 7 - 4]


def _plain(r: random.Random, i: int, n: int) -> bytes:
    return (r.randbytes(n), bytes(n), b"\xff" * n)[0 if i % 5 < 3 else i % 5 - 2]


def _frames(tag: str, lengths) -> list:
    r = _rnd(tag)
    return [(_key(r, i), COUNTERS[i % len(COUNTERS)], _plain(r, i, n)) for i, n in enumerate(lengths)]


@functools.lru_cache(maxsize=None)
def batches() -> dict:
    """name -> frames. ``lengths``: one frame of every length of LENGTHS and again in reverse, so every wave mixes
    lengths; ``n<k>``: k frames of 55 bytes. Keys, counters and plaintexts cycle through random, all-zero and all-ones
    values and through COUNTERS at co-prime periods."""
    out = {"lengths": _frames("lengths", LENGTHS + LENGTHS[::-1])}
    for k in SIZES:
        out[f"n{k}"] = _frames(f"n{k}", [JOB_BYTES] * k)
    return out


def nonce(counter: int) -> bytes:
    return b"\x00" * 4 + struct.pack("<Q", counter)


def oracle(frames, bump: int = 0) -> list:
    """``ciphertext || tag`` per frame by ``utils.aead.seal``; ``bump`` is added to every counter."""
    return [aead.seal(aead.CHACHA20POLY1305, k, nonce(c + bump), p) for k, c, p in frames]


@functools.lru_cache(maxsize=None)
def expected(name: str) -> tuple:
    return tuple(oracle(batches()[name]))


@functools.lru_cache(maxsize=None)
def expected_bumped(name: str) -> tuple:
    """The oracle at counter + 1 (2^64 - 2 stays: 2^64 - 1 is no nonce), to show a comparison sees the counter."""
    return tuple(oracle([(k, c + 1 if c < 2 ** 64 - 2 else c - 1, p) for k, c, p in batches()[name]]))


# ---------------------------------------------------------------------------------------------------- Poly1305
P1305 = (1 << 130) - 5
CLAMP = 0x0ffffffc0ffffffc0ffffffc0fffffff


def poly1305(key: bytes, msg: bytes) -> bytes:
    r = int.from_bytes(key[:16], "little") & CLAMP
    s = int.from_bytes(key[16:], "little")
    h = 0
    for at in range(0, len(msg), 16):
        h = (h + int.from_bytes(msg[at:at + 16] + b"\x01", "little")) * r % P1305
    return ((h + s) % (1 << 128)).to_bytes(16, "little")


_R1 = b"\x01" + bytes(31)                                              # r = 1, s = 0
_RMAX = bytes.fromhex("ffffff0ffcffff0ffcffff0ffcffff0f") + b"\xff" * 16  # r the clamped maximum, s all ones
# (key, message, tag): h reaches p + 3, p, p - 1 and p + 1 before the final reduction; then the widest limbs
POLY_TABLE = [
    (_R1, b"\xff" * 32, bytes.fromhex("03" + "00" * 15)),
    (_R1, b"\xff" * 16 + b"\xfc" + b"\xff" * 15, bytes(16)),
    (_R1, b"\xff" * 16 + b"\xfb" + b"\xff" * 15, bytes.fromhex("fa" + "ff" * 15)),
    (_R1, b"\xff" * 16 + b"\xfd" + b"\xff" * 15, bytes.fromhex("01" + "00" * 15)),
    (_RMAX, b"\xff" * 64, bytes.fromhex("900fe32bc15fa8d7bca8efe4c7e37eb1")),
    (_RMAX, b"\xff" * 17, bytes.fromhex("7cfe7ff768f81f2763f8bf565df85f86")),
]


@functools.lru_cache(maxsize=None)
def poly_rows() -> tuple:
    """``(rows, tags)``: the table, then 300 seeded random rows of 0..100 bytes."""
    r = _rnd("poly")
    rows = [(k, m) for k, m, _t in POLY_TABLE]
    rows += [(r.randbytes(32), r.randbytes(r.randrange(101))) for _ in range(300)]
    tags = [t for _k, _m, t in POLY_TABLE] + [poly1305(k, m) for k, m in rows[len(POLY_TABLE):]]
    return rows, tags
