"""Search kernels where a nonce can be lost without a wrong hash: later grid-stride trips, the compare boundary,
the two extreme targets and a full hit buffer (real MI355X).

Every comparison is exact set or byte equality against ``hashlib``, ``N.cpu_scan_sha256d`` or ``N.x11``. Headers
come from ``random.Random(seed)``; the CPU references of one window are computed once and shared by its tests.

A "key" below is what a kernel reports for one hash: the nonce, or the (nonce, variant index) pair of the
multi-variant SHA-256d kernels. "top" is the part of the digest a kernel compares with the target: its most
significant 32 bits (bytes 28..31 little-endian; SHA-256d and scrypt) or 64 bits (bytes 24..31; X11)."""
import functools
import hashlib
import os
import random
import struct
from concurrent.futures import ThreadPoolExecutor

import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL_PASS = b"\xff" * 32
ALL_ZERO = bytes(32)
EASY = ((1 << 248) - 1).to_bytes(32, "little")  # 1 hash in 256 passes
CANARY = 0x5A5AA5A5
CANARY_WORDS = 256


def _native():
    from otedama_amd.ops.native import require_native

    return require_native()


def _sha256d(h: bytes) -> bytes:
    return hashlib.sha256(hashlib.sha256(h).digest()).digest()


def _scrypt(h: bytes) -> bytes:
    return hashlib.scrypt(h, salt=h, n=1024, r=1, p=1, dklen=32)


def _x11_many(headers: list[bytes]) -> list[bytes]:
    x11 = _native().x11  # releases the GIL
    slices = [headers[i:i + 256] for i in range(0, len(headers), 256)]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return [d for part in ex.map(lambda hs: [x11(h) for h in hs], slices) for d in part]


def _prefix(seed: int) -> bytes:
    return random.Random(seed).randbytes(76)


def _nonce_hdr(prefix76: bytes, nonce: int) -> bytes:
    return prefix76[:76] + struct.pack("<I", nonce & 0xFFFFFFFF)


def _version_headers(n: int, seed: int) -> list[bytes]:
    """n BIP320 version variants of one header: they differ in the version word only."""
    tail = random.Random(seed).randbytes(72)
    return [struct.pack("<I", 0x20000000 | ((v & 0xFFFF) << 13)) + tail + bytes(4) for v in range(n)]


def _bswap(x: int) -> int:
    return int.from_bytes(x.to_bytes(4, "big"), "little")


def _window(base: int, count: int) -> list[int]:
    return [(base + i) & 0xFFFFFFFF for i in range(count)]


def _cpu_scan(hdr: bytes, target: bytes, base: int, count: int) -> list[int]:
    """N.cpu_scan_sha256d over [base, base + count), split where the window wraps 2^32."""
    N = _native()
    first = min(count, (1 << 32) - base)
    out = list(N.cpu_scan_sha256d(hdr, target, base, first))
    if count > first:
        out += list(N.cpu_scan_sha256d(hdr, target, 0, count - first))
    return sorted(out)


def _sync():
    import torch

    torch.cuda.synchronize(DEV)


# ------------------------------------------------------------------ A. many trips per lane, SHA-256d family

def test_sha256d_one_block_walks_71_trips_across_the_wrap():
    """grid=1: 256 lanes walk 256*70 + 13 nonces (71 trips, the abort-poll branch twice, a ragged last trip)
    across the 2^32 wrap."""
    from otedama_amd.ops.search import Sha256dSearch

    hdr = _prefix(4101) + bytes(4)
    base, count = 0xFFFFC000, 256 * 70 + 13
    ref = _cpu_scan(hdr, EASY, base, count)
    assert len(ref) > 50
    assert any(n >= base for n in ref) and any(n < base for n in ref)  # hits on both sides of the wrap
    got = Sha256dSearch(DEV, grid=1, cap=4096).search(hdr, EASY, base, count)
    assert sorted(got) == ref


@pytest.mark.parametrize("count", [1, 255])
def test_sha256d_fewer_nonces_than_lanes(count):
    from otedama_amd.ops.search import Sha256dSearch

    hdr = _prefix(4102) + bytes(4)
    base = 0xFFFFFFFF - 100
    got = Sha256dSearch(DEV, grid=1, cap=4096).search(hdr, ALL_PASS, base, count)
    assert sorted(got) == sorted(_window(base, count))


# The window of the K cases holds 256*9 + 5 nonces: at 1 hash in 256 that is 9 hits per variant, so these cases
# take 1 hash in 32 to have more than 50 reference hits for every variant.
K_TARGET = ((1 << 251) - 1).to_bytes(32, "little")


@pytest.mark.parametrize("k,trips", [(2, 10), (12, 10), (16, 10), (2, 17)])
def test_sha256d_k_one_block_walks_many_trips(k, trips):
    """grid=1, 256 * (trips - 1) + 5 nonces. The abort-poll period is 32 / k trips: with ten trips k=12 and k=16
    (period 2) enter the poll branch five times and k=2 (period 16) never does, so k=2 also runs 17 trips, which
    enter it once. Every variant's hits equal the CPU scan of its own header."""
    from otedama_amd.ops.search import Sha256dSearchK

    headers = _version_headers(k, 4200 + k)
    base, count = 0xFFFFFB00, 256 * (trips - 1) + 5
    got = Sha256dSearchK(DEV, k=k, grid=1, cap=4096).search(headers, K_TARGET, base, count)
    assert len(got) == len(set(got))
    for v in range(k):
        ref = _cpu_scan(headers[v], K_TARGET, base, count)
        assert len(ref) > 50
        assert sorted(n for n, vv in got if vv == v) == ref, v
    assert all(0 <= vv < k for _, vv in got)


V_BASE, V_COUNT = 0xFFFFFF00, 301


@functools.lru_cache(maxsize=None)
def _v_trip_reference() -> tuple[tuple[bytes, ...], tuple[tuple[int, ...], ...]]:
    """256 version variants and, per variant, the nonces bswap(W3), W3 in [V_BASE, V_BASE + V_COUNT), whose
    hashlib SHA-256d passes EASY."""
    hs = _version_headers(256, 4300)
    limit = int.from_bytes(EASY, "little")
    hits = []
    for h in hs:
        nonces = [_bswap(w3) for w3 in _window(V_BASE, V_COUNT)]
        hits.append(tuple(n for n in nonces if int.from_bytes(_sha256d(_nonce_hdr(h, n)), "little") <= limit))
    return tuple(hs), tuple(hits)


@pytest.mark.parametrize("grid_per_group", [1, 2])
@pytest.mark.parametrize("groups,chains,occ", [(1, 1, True), (1, 1, False), (2, 2, True), (2, 2, False),
                                                (1, 3, False), (1, 4, False)])
def test_sha256d_v_every_wave_walks_the_window(groups, chains, occ, grid_per_group):
    """One-wave blocks, one or two waves per variant group (a group is 64 * chains variants): W3 stride 1 or 2 over
    an odd window of 301 that wraps 2^32, so every wave makes 301 or about 150 trips."""
    from otedama_amd.ops.search import Sha256dSearchV

    pool, hits = _v_trip_reference()
    nvar = 64 * chains * groups
    want = sorted((n, vi) for vi in range(nvar) for n in hits[vi])
    assert len(want) > 50
    s = Sha256dSearchV(DEV, cap=4096, grid=groups * grid_per_group, block=64, chains=chains, occupancy8=occ)
    got = s.search(list(pool[:nvar]), EASY, V_BASE, V_COUNT)
    assert sorted(got) == want


# ------------------------------------------------------------------ B. later trips of the X11 table stages

def _x11_geometry(trips: int):
    """(T, n). T = CUs * 8 * 512 is one full trip of the LDS-table stages (their grid is capped at 8 blocks of 512
    per CU): position i is hashed in trip i // T + 1. n = (trips - 1) * T + T // 2 + 777 ends in the middle of trip
    `trips`: half of the lanes make `trips` trips, the others one fewer, and the last block is ragged."""
    T = _native().gpu_cu_count(0) * 8 * 512
    assert T > 0
    return T, (trips - 1) * T + T // 2 + 777


X11_CHUNK = 1 << 16
# trips=2 is the window T + T // 2 + 777 (trip 1 and half of trip 2); trips=3 adds a whole further trip, so that
# lanes also go round the loop a second time
X11_TRIPS = [2, 3]


def _x11_sample(T: int, n: int, trips: int, rng) -> list[int]:
    """64 positions: both ends, the three positions around every trip boundary, at least 20 from the last trip
    and, with three trips, at least 16 from the middle one; the rest from trip 1."""
    picks = {0, n - 1}
    for t in range(1, trips):
        picks |= {t * T - 1, t * T, t * T + 1}
    last = (trips - 1) * T
    picks |= set(rng.sample(range(last, n), 24))
    if trips == 3:
        picks |= set(rng.sample(range(T, 2 * T), 16))
    while len(picks) < 64:
        picks.add(rng.randrange(T))
    assert len(picks) == 64 and sum(i >= last for i in picks) >= 20
    return sorted(picks)


@pytest.mark.parametrize("trips", X11_TRIPS)
def test_x11_digests_past_the_first_trip(trips):
    """All eleven stages in digest mode over n nonces in one pass (the table stages go round their grid-stride
    loop up to `trips` times) equal the same range computed in chunks of 65536 (one trip each), plane by plane;
    64 sampled digests, most of them from the later trips, equal the CPU chain."""
    import torch

    N = _native()
    T, n = _x11_geometry(trips)
    prefix = _prefix(4400)
    base = 0xFFF80000  # the window wraps 2^32 inside its first trip
    params = N.x11_prepare(prefix + bytes(4), ALL_ZERO)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    H_big = torch.full((8 * n,), 0x1111111111111111, dtype=torch.int64, device=DEV)
    H_ref = torch.full((8 * n,), 0x2222222222222222, dtype=torch.int64, device=DEV)
    for st in range(N.X11_STAGES):
        N.launch_x11_stage(params, st, base, H_big.data_ptr(), n, n, 0, 0, stream)
    for off in range(0, n, X11_CHUNK):
        cnt = min(X11_CHUNK, n - off)
        for st in range(N.X11_STAGES):  # plane w of item k at H_ref[w * n + off + k]
            N.launch_x11_stage(params, st, (base + off) & 0xFFFFFFFF, H_ref.data_ptr() + 8 * off, n, cnt, 0, 0, stream)
    _sync()
    big, ref = H_big.view(8, n), H_ref.view(8, n)
    assert torch.equal(big[:4], ref[:4])  # the 32-byte chain digest
    assert torch.equal(big[4:], ref[4:])
    assert not bool(big[4:].any())  # ECHO writes zeros to planes 4..7
    picks = _x11_sample(T, n, trips, random.Random(4401))
    idx = torch.tensor(picks, dtype=torch.int64, device=DEV)
    rows = big[:4].index_select(1, idx).t().contiguous().cpu().numpy().tobytes()
    for j, i in enumerate(picks):
        want = N.x11(_nonce_hdr(prefix, base + i))
        assert rows[32 * j:32 * j + 32] == want, (i, rows[32 * j:32 * j + 32].hex(), want.hex())


@pytest.mark.parametrize("trips", X11_TRIPS)
def test_x11_search_past_the_first_trip(trips):
    """The fused ECHO compare (partial round 9) over up to `trips` trips in one launch reports exactly the union of
    the chunked searches of the same range, and every hit passes on the CPU. 1 hash in 4096 passes: about
    n / 4096 hits (384 and 640 with 256 CUs), at least 20 of them from the last trip."""
    from otedama_amd.ops.search import X11Search

    T, n = _x11_geometry(trips)
    prefix = _prefix(4410)
    hdr = prefix + bytes(4)
    base = 0xFFF80000
    top_limit = (1 << 64) // 4096 - 1
    target = b"\xff" * 24 + struct.pack("<Q", top_limit)
    small = X11Search(DEV, cap=4096, batch=X11_CHUNK)
    chunked = []
    for off in range(0, n, X11_CHUNK):
        chunked += small.search(hdr, target, (base + off) & 0xFFFFFFFF, min(X11_CHUNK, n - off))
    del small
    assert len(chunked) == len(set(chunked))
    assert 100 <= len(chunked) <= 4096
    r = X11Search(DEV, cap=4096, batch=n)
    res = r.launch(r.prepare(hdr, target), base, n)
    _sync()
    hits = res.nonces()
    assert res.count() == len(hits) == len(set(hits))
    assert sorted(hits) == sorted(chunked)
    assert sum(((h - base) & 0xFFFFFFFF) >= (trips - 1) * T for h in hits) >= 20
    for h, d in zip(hits, _x11_many([_nonce_hdr(prefix, h) for h in hits])):
        assert struct.unpack("<Q", d[24:32])[0] <= top_limit, hex(h)


# ------------------------------------------------------------------ C. the compare boundary, the extreme targets

class _Family:
    """One kernel on one small window: the CPU digest of every key, and `run(target, count)` -> (reported keys,
    device hit count) over the first `count` window positions (default: the whole window)."""

    def __init__(self, width, digests, op, job, base, count, keys_of):
        self.width = width          # compared bits: 32 or 64
        self.digests = digests      # {key: 32-byte digest}, the whole window
        self.op, self.job = op, job  # the ops object and what its prepare() takes: a header or a list of headers
        self.base, self.count = base, count
        self.keys_of = keys_of      # count -> keys of the first `count` window positions

    def run(self, target: bytes, count=None):
        r = self.op.launch(self.op.prepare(self.job, target), self.base, self.count if count is None else count)
        _sync()
        return (r.hits() if hasattr(r, "hits") else r.nonces()), r.count()

    def top(self, key) -> int:
        d = self.digests[key]
        return struct.unpack("<Q", d[24:32])[0] if self.width == 64 else struct.unpack("<I", d[28:32])[0]

    def target_with_top(self, top: int) -> bytes:
        if self.width == 64:
            return b"\xff" * 24 + struct.pack("<Q", top)
        return b"\xff" * 28 + struct.pack("<I", top)

    def median_key(self):
        ranked = sorted(self.digests, key=lambda k: (self.top(k), k))
        return ranked[len(ranked) // 2]


SHA_BASE, SHA_COUNT = 0xFFFFFC00, 2048       # wraps 2^32 half way
V_EDGE_BASE, V_EDGE_COUNT = 0x89ABCDE0, 64   # W3 values
SCRYPT_BASE, SCRYPT_COUNT, SCRYPT_ALL_PASS_COUNT = 0xFFFFFF80, 256, 200  # wraps 2^32 at position 128
X11_BASE, X11_COUNT = 0xFFFFFE00, 2048


@functools.lru_cache(maxsize=None)
def _scrypt_digests():
    prefix = _prefix(4520)
    return prefix, {n: _scrypt(_nonce_hdr(prefix, n)) for n in _window(SCRYPT_BASE, SCRYPT_COUNT)}


@functools.lru_cache(maxsize=None)
def _family(name: str) -> _Family:
    from otedama_amd.ops import search

    if name == "sha256d":
        hdr = _prefix(4500) + bytes(4)
        digests = {n: _sha256d(_nonce_hdr(hdr, n)) for n in _window(SHA_BASE, SHA_COUNT)}
        op = search.Sha256dSearch(DEV, cap=SHA_COUNT, grid=2)
        return _Family(32, digests, op, hdr, SHA_BASE, SHA_COUNT, lambda c: _window(SHA_BASE, c))
    if name == "sha256d_k4":
        hs = _version_headers(4, 4501)
        digests = {(n, v): _sha256d(_nonce_hdr(h, n)) for v, h in enumerate(hs) for n in _window(SHA_BASE, SHA_COUNT)}
        op = search.Sha256dSearchK(DEV, k=4, cap=4 * SHA_COUNT, grid=2)
        return _Family(32, digests, op, hs, SHA_BASE, SHA_COUNT,
                       lambda c: [(n, v) for v in range(4) for n in _window(SHA_BASE, c)])
    if name in ("sha256d_v1", "sha256d_v2"):
        chains, occ = (1, True) if name == "sha256d_v1" else (2, False)
        hs = _version_headers(64 * chains, 4510 + chains)
        digests = {(_bswap(w3), vi): _sha256d(_nonce_hdr(h, _bswap(w3)))
                   for vi, h in enumerate(hs) for w3 in _window(V_EDGE_BASE, V_EDGE_COUNT)}
        op = search.Sha256dSearchV(DEV, cap=len(digests), grid=4, chains=chains, occupancy8=occ)
        return _Family(32, digests, op, hs, V_EDGE_BASE, V_EDGE_COUNT,
                       lambda c: [(_bswap(w3), vi) for vi in range(len(hs)) for w3 in _window(V_EDGE_BASE, c)])
    if name.startswith("scrypt_"):
        prefix, digests = _scrypt_digests()
        op = search.ScryptSearch(DEV, cap=SCRYPT_COUNT, grid=1, kernel=name[len("scrypt_"):])
        assert op.kernel == name[len("scrypt_"):]
        return _Family(32, digests, op, prefix + bytes(4), SCRYPT_BASE, SCRYPT_COUNT,
                       lambda c: _window(SCRYPT_BASE, c))
    assert name == "x11"
    prefix = _prefix(4530)
    nonces = _window(X11_BASE, X11_COUNT)
    digests = dict(zip(nonces, _x11_many([_nonce_hdr(prefix, n) for n in nonces])))
    op = search.X11Search(DEV, cap=X11_COUNT, batch=X11_COUNT)
    return _Family(64, digests, op, prefix + bytes(4), X11_BASE, X11_COUNT, lambda c: _window(X11_BASE, c))


FAMILIES = ["sha256d", "sha256d_k4", "sha256d_v1", "sha256d_v2", "scrypt_coop", "scrypt_coop2", "scrypt_split",
            "scrypt_lane", "x11"]


@pytest.mark.parametrize("name", FAMILIES)
def test_target_equal_to_a_digest_of_the_window_reports_it(name):
    """Target = the full digest of the key whose top is the window's median: the kernel reports exactly the keys
    whose top is <= that top, the tying key among them."""
    fam = _family(name)
    star = fam.median_key()
    want = sorted(k for k in fam.digests if fam.top(k) <= fam.top(star))
    got, count = fam.run(fam.digests[star])
    assert count == len(got) == len(set(got))
    assert star in got
    assert sorted(got) == want
    assert len(fam.digests) // 2 <= len(want) <= len(fam.digests) // 2 + 2


@pytest.mark.parametrize("name", FAMILIES)
def test_target_one_below_a_digest_top_leaves_it_out(name):
    fam = _family(name)
    star = fam.median_key()
    assert fam.top(star) > 0
    want = sorted(k for k in fam.digests if fam.top(k) < fam.top(star))
    got, count = fam.run(fam.target_with_top(fam.top(star) - 1))
    assert count == len(got) == len(set(got))
    assert star not in got
    assert sorted(got) == want and want


@pytest.mark.parametrize("name", FAMILIES)
def test_all_ones_target_reports_every_key_once(name):
    fam = _family(name)
    n = SCRYPT_ALL_PASS_COUNT if name.startswith("scrypt_") else None
    got, count = fam.run(ALL_PASS) if n is None else fam.run(ALL_PASS, n)
    want = sorted(fam.keys_of(n) if n is not None else fam.digests)
    assert count == len(got) == len(set(got))
    assert sorted(got) == want


@pytest.mark.parametrize("name", FAMILIES)
def test_all_zero_target_reports_nothing(name):
    fam = _family(name)
    assert all(fam.top(k) > 0 for k in fam.digests)  # no digest of the window passes a zero top
    got, count = fam.run(ALL_ZERO)
    assert got == [] and count == 0


# ------------------------------------------------------------------ D. overflow of the ops hit buffer

OVER_CAP = 64


def _canary_out(words: int):
    """int32 [1 + words*cap + 256]: count 0, then the canary in every slot and in 256 words behind the slots."""
    import torch

    out = torch.full((1 + words * OVER_CAP + CANARY_WORDS,), CANARY, dtype=torch.int32, device=DEV)
    out[0] = 0
    return out


def _check_overflow(out, words: int, true_hits: int, valid) -> None:
    host = [x & 0xFFFFFFFF for x in out.cpu().tolist()]
    assert host[0] == true_hits  # every hit counted, kept or dropped
    body = host[1:1 + words * OVER_CAP]
    kept = body if words == 1 else list(zip(body[0::2], body[1::2]))
    assert len(set(kept)) == OVER_CAP
    assert all(valid(k) for k in kept), [k for k in kept if not valid(k)][:4]
    assert host[1 + words * OVER_CAP:] == [CANARY] * CANARY_WORDS


def test_overflow_sha256d():
    from otedama_amd.ops.search import Sha256dSearch

    base, count = 0xFFFFFE00, 1000
    window = set(_window(base, count))
    s = Sha256dSearch(DEV, cap=OVER_CAP, grid=2)
    out = _canary_out(1)
    r = s.launch(s.prepare(_prefix(4600) + bytes(4), ALL_PASS), base, count, out=out)
    _sync()
    assert r.count() == count and len(r.nonces()) == OVER_CAP
    _check_overflow(out, 1, count, lambda n: n in window)


def test_overflow_sha256d_k():
    from otedama_amd.ops.search import Sha256dSearchK

    base, count, k = 0xFFFFFE00, 1000, 4
    window = set(_window(base, count))
    s = Sha256dSearchK(DEV, k=k, cap=OVER_CAP, grid=2)
    out = _canary_out(2)
    r = s.launch(s.prepare(_version_headers(k, 4601), ALL_PASS), base, count, out=out)
    _sync()
    assert r.count() == k * count and len(r.hits()) == OVER_CAP
    _check_overflow(out, 2, k * count, lambda kv: kv[0] in window and kv[1] < k)


@pytest.mark.parametrize("chains,occ", [(1, True), (2, False)])
def test_overflow_sha256d_v(chains, occ):
    from otedama_amd.ops.search import Sha256dSearchV

    base, count, nvar = 0xFFFFFFF0, 32, 64 * chains
    nonces = {_bswap(w3) for w3 in _window(base, count)}
    s = Sha256dSearchV(DEV, cap=OVER_CAP, grid=4, chains=chains, occupancy8=occ)
    out = _canary_out(2)
    r = s.launch(s.prepare(_version_headers(nvar, 4602), ALL_PASS), base, count, out=out)
    _sync()
    assert r.count() == nvar * count and len(r.hits()) == OVER_CAP
    _check_overflow(out, 2, nvar * count, lambda kv: kv[0] in nonces and kv[1] < nvar)


def test_overflow_scrypt():
    import torch

    from otedama_amd.ops.search import ScryptSearch

    N = _native()
    base, count = 0xFFFFFE00, 1000
    window = set(_window(base, count))
    sc = ScryptSearch(DEV, cap=OVER_CAP, grid=4)  # buffers for 1024 lane slots
    assert sc.batch >= count
    out = _canary_out(1)
    N.launch_scrypt(sc.prepare(_prefix(4603) + bytes(4), ALL_PASS), base, count, sc.xbuf.data_ptr(),
                    sc.scratch.data_ptr(), sc.gap, out.data_ptr(), OVER_CAP, sc.grid,
                    torch.cuda.current_stream(DEV).cuda_stream)
    _sync()
    _check_overflow(out, 1, count, lambda n: n in window)


def test_overflow_x11():
    import torch

    from otedama_amd.ops.search import X11Search

    N = _native()
    base, count = 0xFFFFFE00, 1000
    window = set(_window(base, count))
    xs = X11Search(DEV, cap=OVER_CAP, batch=1024)
    out = _canary_out(1)
    N.launch_x11(xs.prepare(_prefix(4604) + bytes(4), ALL_PASS), base, xs.H.data_ptr(), xs.batch, count,
                 out.data_ptr(), OVER_CAP, torch.cuda.current_stream(DEV).cuda_stream)
    _sync()
    _check_overflow(out, 1, count, lambda n: n in window)
