"""Shared rows of the batched secp256k1 multiplication tests (test_secp_cpu.py, test_secp_gpu.py,
test_pool_handshakes.py): scalars, points, bad rows, and the Python oracle's answer to each, computed once.

The oracle is the unchanged big-integer Python of otedama_amd/btccrypto.py and otedama_amd/stratum/ellswift.py:
``point_mul`` for kinds 0 and 1 (``lift_x`` for the even y), ``ellswift.decode`` then the same for kind 2."""
import functools
import random

from otedama_amd import btccrypto as ec
from otedama_amd.ops import secp_rows as R
from otedama_amd.stratum import ellswift

N, P, G = ec.N, ec.P, ec.G

_rng = random.Random(0x5EC9256)

# (n - 1) / 2 and (n + 1) / 2: the doubling after such a prefix gives -P and +P, which an add-always ladder then adds P
# to. 200 leading zero bits: the accumulator stays at infinity through 200 dropped additions.
SPECIAL_SCALARS = [1, 2, 3, N - 1, N - 2, (N - 1) // 2, (N + 1) // 2, 1 << 255, (1 << 128) - 1,
                   _rng.getrandbits(56) | (1 << 55)]
RANDOM_SCALARS = [_rng.randrange(1, N) for _ in range(32)]
SCALARS = SPECIAL_SCALARS + RANDOM_SCALARS

MULTIPLES = [ec.point_mul(G, _rng.randrange(1, N)) for _ in range(8)]


def _b32(v: int) -> bytes:
    return v.to_bytes(32, "big")


def xswiftec_case(u: int, t: int) -> str:
    """Which way ``ellswift.xswiftec`` takes for (u, t): ``x1``, ``x2`` or ``x3``, with ``+double`` when u^3 + t^2 + 7
    is zero and t is doubled first. The same arithmetic, only to name the case."""
    u, t = u % P or 1, t % P or 1
    tag = ""
    if (pow(u, 3, P) + t * t + 7) % P == 0:
        t, tag = 2 * t % P, "+double"
    X = (pow(u, 3, P) + 7 - t * t) * pow(2 * t, -1, P) % P
    Y = (X + t) * pow(ellswift.C * u, -1, P) % P
    if ellswift.is_x((u + 4 * Y * Y) % P):
        return "x1" + tag
    xy = X * pow(Y, -1, P) % P
    return ("x2" if ellswift.is_x((-xy - u) * ellswift._HALF % P) else "x3") + tag


def _case_encodings() -> dict:
    """One (u, t) per xswiftec case, found by a seeded search."""
    found: dict = {}
    rng = random.Random(324)
    while not {"x1", "x2", "x3"} <= found.keys():
        u, t = rng.randrange(1, P), rng.randrange(1, P)
        found.setdefault(xswiftec_case(u, t), _b32(u) + _b32(t))
    while not any(k.endswith("+double") for k in found):
        u = rng.randrange(1, P)
        t = ellswift._sqrt(-(pow(u, 3, P) + 7))
        if t:
            found[xswiftec_case(u, t)] = _b32(u) + _b32(t)
    return found


CASE_ENCODINGS = _case_encodings()

_enc_rng = random.Random(64)
assert ec.lift_x(1) is not None
_u, _t = _rng.randrange(1, P), _rng.randrange(1, P)
# u >= p and t >= p: only values below 2^256 - p = 2^32 + 977 have such a second spelling
_SMALL_U, _SMALL_T = 12345, 0x100000000 + 17

# (kind, point bytes)
POINTS = ([(R.KIND_G, b""), (R.KIND_XONLY, _b32(1))]
          + [(R.KIND_XONLY, _b32(m[0])) for m in MULTIPLES]
          + [(R.KIND_ELLSWIFT, ellswift.encode(m[0], rand=lambda n: _enc_rng.randbytes(n))) for m in MULTIPLES]
          + [(R.KIND_ELLSWIFT, _b32(0) + _b32(_t)),                 # u = 0
             (R.KIND_ELLSWIFT, _b32(_u) + _b32(0)),                 # t = 0
             (R.KIND_ELLSWIFT, _b32(0) + _b32(0)),
             (R.KIND_ELLSWIFT, _b32(P) + _b32(_t)),                 # u = p, reduced to 0
             (R.KIND_ELLSWIFT, _b32(_SMALL_U + P) + _b32(_t)),      # u >= p
             (R.KIND_ELLSWIFT, _b32(_u) + _b32(_SMALL_T + P)),      # t >= p
             (R.KIND_ELLSWIFT, _b32((1 << 256) - 1) + _b32((1 << 256) - 1))]
          + [(R.KIND_ELLSWIFT, enc) for _name, enc in sorted(CASE_ENCODINGS.items())])

# every scalar on G and on one other point, every point under one special and one random scalar
ROWS = ([(s, R.KIND_G, b"") for s in SCALARS]
        + [(s, *POINTS[1 + i % (len(POINTS) - 1)]) for i, s in enumerate(SCALARS)]
        + [(SPECIAL_SCALARS[i % len(SPECIAL_SCALARS)], k, p) for i, (k, p) in enumerate(POINTS)]
        + [(RANDOM_SCALARS[i % len(RANDOM_SCALARS)], k, p) for i, (k, p) in enumerate(POINTS)])

_GOOD_X = _b32(MULTIPLES[0][0])
BAD_ROWS = [((0, R.KIND_G, b""), R.BAD_SCALAR),
            ((N, R.KIND_XONLY, _GOOD_X), R.BAD_SCALAR),
            (((1 << 256) - 1, R.KIND_ELLSWIFT, POINTS[12][1]), R.BAD_SCALAR),
            ((7, R.KIND_XONLY, _b32(P)), R.BAD_POINT),
            ((7, R.KIND_XONLY, _b32(5)), R.BAD_POINT),     # x = 5 is not on the curve (test_secp_cpu asserts it)
            ((7, 9, _GOOD_X), R.BAD_KIND)]


@functools.lru_cache(maxsize=None)
def oracle(row: tuple) -> tuple:
    """``(x, y_parity, status)`` of one good row, by the Python functions."""
    scalar, kind, point = row
    if kind == R.KIND_G:
        pt = G
    elif kind == R.KIND_XONLY:
        pt = ec.lift_x(int.from_bytes(point, "big"))
    else:
        pt = ec.lift_x(ellswift.decode(point))
    x, y = ec.point_mul(pt, scalar)
    return _b32(x), y & 1, R.OK


def expected(rows) -> list:
    bad = dict(BAD_ROWS)
    return [(bytes(32), 0, bad[r]) if r in bad else oracle(r) for r in rows]


def tiled(n: int, offset: int = 0) -> list:
    """``n`` rows: the good rows in order, repeated, a bad row after every seventh, starting ``offset`` rows in."""
    cycle = []
    for i, r in enumerate(ROWS):
        cycle.append(r)
        if i % 7 == 6:
            cycle.append(BAD_ROWS[(i // 7) % len(BAD_ROWS)][0])
    return [cycle[(offset + i) % len(cycle)] for i in range(n)]
