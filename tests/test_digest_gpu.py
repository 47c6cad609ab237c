"""Batch digest ops (otedama_amd/ops/digest.py, csrc/kernels/digest_batch.hip) on a real MI355X.

Every comparison is exact byte equality: SHA-256d against ``hashlib.sha256`` twice, scrypt against
``hashlib.scrypt`` and X11 against the native C++ chain. The oracles of one header pool per algorithm are computed
once and shared; a batch of ``n`` is the first ``n`` headers of the pool (seeded random bytes with an all-zero
header, an all-0xFF header and the Bitcoin and Dash genesis headers at positions 1..4)."""
import functools
import hashlib
import os
import random
import struct
from concurrent.futures import ThreadPoolExecutor

import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOP = 0x07FFFFFF  # top word of the easy target of the search-agreement tests (1 hash in 32 passes)
SEARCH_BASE = 0x5A000000
# (header seed, nonces): seeds for which the CPU oracle alone finds >= 10 passing nonces (scrypt: 16 of 512).
AGREE = {"sha256d": (301, 1 << 16), "scrypt": (101, 512), "x11": (201, 1 << 16)}


def _native():
    from otedama_amd.ops.native import require_native

    return require_native()


def _sha256d(h: bytes) -> bytes:
    return hashlib.sha256(hashlib.sha256(h).digest()).digest()


def _scrypt(h: bytes) -> bytes:
    return hashlib.scrypt(h, salt=h, n=1024, r=1, p=1, dklen=32)


def _oracle_many(name: str, headers: list[bytes]) -> list[bytes]:
    if name == "sha256d":
        return [_sha256d(h) for h in headers]
    if name == "scrypt":
        return [_scrypt(h) for h in headers]
    x11 = _native().x11  # releases the GIL: ~0.2 ms per header, spread over the cores in slices
    slices = [headers[i:i + 512] for i in range(0, len(headers), 512)]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return [d for part in ex.map(lambda hs: [x11(h) for h in hs], slices) for d in part]


def _genesis(name: str) -> bytes:
    from otedama_amd.models.algorithms import KNOWN_ANSWERS

    return bytes.fromhex(KNOWN_ANSWERS[name][0])


@functools.lru_cache(maxsize=None)
def _pool(name: str) -> tuple[tuple[bytes, ...], tuple[bytes, ...]]:
    """(headers, oracle digests) of the algorithm's pool: 1000 headers (scrypt: 513)."""
    size = 513 if name == "scrypt" else 1000
    rng = random.Random({"sha256d": 11, "scrypt": 12, "x11": 13}[name])
    hs = [rng.randbytes(80) for _ in range(size)]
    hs[1:5] = [bytes(80), b"\xff" * 80, _genesis("sha256d"), _genesis("x11")]
    return tuple(hs), tuple(_oracle_many(name, hs))


def _to_dev(headers):
    import torch

    return torch.frombuffer(bytearray(b"".join(headers)), dtype=torch.uint8).view(len(headers), 80).to(DEV)


def _rows(t) -> list[bytes]:
    raw = t.cpu().numpy().tobytes()
    return [raw[i:i + 32] for i in range(0, len(raw), 32)]


@functools.lru_cache(maxsize=None)
def _op(name: str):
    """One op per algorithm for the whole module (scrypt: grid=2, 512 slots per chunk; X11: capacity 256), so the
    tests also cover repeated launches on reused buffers."""
    from otedama_amd.ops.digest import HeaderDigest

    if name == "scrypt":
        return HeaderDigest("scrypt", DEV, grid=2)
    if name == "x11":
        return HeaderDigest("x11", DEV, capacity=256)
    return HeaderDigest("sha256d", DEV)


def _check_prefix(name: str, n: int):
    import torch

    hs, want = _pool(name)
    out = _op(name).launch(_to_dev(hs[:n]))
    assert out.shape == (n, 32) and out.dtype == torch.uint8 and out.device == torch.device(DEV)
    torch.cuda.synchronize()
    got = _rows(out)
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, (name, n, bad[:8], got[bad[0]].hex(), want[bad[0]].hex())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sha256d_digest_equals_hashlib(n):
    """Wave edge, block edge and tail of the one-header-per-lane kernel."""
    _check_prefix("sha256d", n)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 257, 512, 513])
def test_scrypt_digest_equals_hashlib(n):
    """grid=2 (512 slots per chunk): the octet and wave granularity of the cooperative ROMix, its count rounding,
    and at 513 a batch that crosses a chunk boundary. The op always launches SCRYPT_COOP; the other ROMix kernels
    are held to bytes through the native launcher in tests/test_scrypt_romix_bytes_gpu.py."""
    assert _op("scrypt").capacity == 512
    _check_prefix("scrypt", n)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1000])
def test_x11_digest_equals_native_chain(n):
    assert _op("x11").capacity == 256
    _check_prefix("x11", n)


def test_genesis_headers_give_the_published_hashes():
    from otedama_amd.models.algorithms import KNOWN_ANSWERS

    for name in ("sha256d", "x11"):
        (d,) = _op(name).hash([_genesis(name)])
        assert d[::-1].hex() == KNOWN_ANSWERS[name][2], name


@pytest.mark.parametrize("name", ["sha256d", "scrypt", "x11"])
def test_digests_do_not_depend_on_batch_position(name):
    import torch

    hs, want = _pool(name)
    n = 257
    perm = list(range(n))
    random.Random(5).shuffle(perm)
    op = _op(name)
    a = op.launch(_to_dev(hs[:n]))
    b = op.launch(_to_dev([hs[j] for j in perm]))
    torch.cuda.synchronize()
    ra, rb = _rows(a), _rows(b)
    assert ra == list(want[:n])
    assert rb == [ra[j] for j in perm]


def _search(name: str, hdr: bytes, target: bytes, base: int, count: int) -> list[int]:
    from otedama_amd.ops import search

    if name == "sha256d":
        return search.Sha256dSearch(DEV, cap=8192).search(hdr, target, base, count)
    if name == "scrypt":
        return search.ScryptSearch(DEV, cap=1024, grid=2).search(hdr, target, base, count)
    return search.X11Search(DEV, cap=8192, batch=count).search(hdr, target, base, count)


@pytest.mark.parametrize("name", ["sha256d", "scrypt", "x11"])
def test_digest_agrees_with_the_search_kernel(name):
    """One random header, a nonce range, target top word 0x07FFFFFF (rest 0xFF): the set the search kernel reports
    equals the set read off the digests of every header of the range, and the CPU oracle gives the same digests
    (hence the same set)."""
    seed, count = AGREE[name]
    prefix = random.Random(seed).randbytes(76)
    target = b"\xff" * 28 + struct.pack("<I", TOP)
    headers = [prefix + struct.pack("<I", SEARCH_BASE + k) for k in range(count)]
    digests = _op(name).hash(headers)
    from_digest = {SEARCH_BASE + k for k, d in enumerate(digests) if struct.unpack("<I", d[28:32])[0] <= TOP}
    reported = _search(name, prefix + bytes(4), target, SEARCH_BASE, count)
    assert len(reported) == len(set(reported))
    assert set(reported) == from_digest
    cpu = _oracle_many(name, headers)
    assert cpu == digests
    assert {SEARCH_BASE + k for k, d in enumerate(cpu) if struct.unpack("<I", d[28:32])[0] <= TOP} == from_digest
    assert len(from_digest) >= 10


def test_side_stream_launch_and_out_reuse():
    import torch

    for name in ("sha256d", "scrypt", "x11"):
        hs, want = _pool(name)
        op = _op(name)
        first, second = _to_dev(hs[:100]), _to_dev(hs[100:200])
        out = torch.full((100, 32), 0xA5, dtype=torch.uint8, device=DEV)
        side = torch.cuda.Stream(DEV)
        assert op.launch(first, out=out, stream=side) is out
        side.synchronize()
        assert _rows(out) == list(want[:100]), name
        default = op.launch(first)  # the default path, after a launch on another stream
        assert op.launch(second, out=out) is out  # a second launch into the same `out` overwrites it
        torch.cuda.synchronize()
        assert _rows(default) == list(want[:100]), name
        assert _rows(out) == list(want[100:200]), name


def test_scrypt_digest_leaves_an_earlier_search_instance_alone():
    import torch

    from otedama_amd.models.header import int_to_hash
    from otedama_amd.ops.digest import HeaderDigest
    from otedama_amd.ops.search import ScryptSearch

    prefix = random.Random(77).randbytes(76)
    target_int = (1 << 254) - 1  # about 1 hash in 4 passes
    sc = ScryptSearch(DEV, grid=2, cap=1024)
    hs, want = _pool("scrypt")
    op = HeaderDigest("scrypt", DEV, grid=2)
    for buf in (op.xbuf, op.scratch):
        assert buf.data_ptr() not in (sc.xbuf.data_ptr(), sc.scratch.data_ptr())
    assert op.hash(list(hs[:130])) == list(want[:130])
    got = sorted(sc.search(prefix + bytes(4), int_to_hash(target_int), 7000, 192))
    torch.cuda.synchronize()
    ref = [n for n in range(7000, 7192)
           if int.from_bytes(_scrypt(prefix + struct.pack("<I", n)), "little") <= target_int]
    assert got == ref and 0 < len(ref) < 192


@pytest.mark.parametrize("name", ["sha256d", "scrypt", "x11"])
def test_bad_arguments_raise_and_launch_nothing(name):
    import torch

    op = _op(name)
    n = 16
    good = _to_dev(_pool(name)[0][:n])
    flat = torch.zeros(8 + 80 * n + 8, dtype=torch.uint8, device=DEV)
    assert flat.data_ptr() % 16 == 0
    bad = {
        "79 columns": torch.zeros((n, 79), dtype=torch.uint8, device=DEV),
        "int32": torch.zeros((n, 80), dtype=torch.int32, device=DEV),
        "cpu": torch.zeros((n, 80), dtype=torch.uint8),
        "transposed": torch.zeros((80, n), dtype=torch.uint8, device=DEV).t(),
        "misaligned": flat[8:8 + 80 * n].view(n, 80),
        "one dimension": torch.zeros(80 * n, dtype=torch.uint8, device=DEV),
    }
    assert bad["misaligned"].is_contiguous() and not bad["transposed"].is_contiguous()
    out = torch.full((n, 32), 0xA5, dtype=torch.uint8, device=DEV)
    for what, t in bad.items():
        with pytest.raises(ValueError):
            op.launch(t, out=out)
        with pytest.raises(ValueError):
            op.launch(t)
    for what, o in {"short out": out[:-1], "int32 out": torch.zeros((n, 8), dtype=torch.int32, device=DEV),
                    "cpu out": torch.zeros((n, 32), dtype=torch.uint8),
                    "misaligned out": torch.zeros(8 + 32 * n, dtype=torch.uint8, device=DEV)[8:].view(n, 32)}.items():
        with pytest.raises(ValueError):
            op.launch(good, out=o)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    empty = op.launch(torch.zeros((0, 80), dtype=torch.uint8, device=DEV))
    assert empty.shape == (0, 32) and empty.dtype == torch.uint8
    with pytest.raises(ValueError):
        op.hash([bytes(80), bytes(79)])
    assert op.hash([]) == []


def test_constructor_checks():
    from otedama_amd.ops.digest import HeaderDigest

    with pytest.raises(ValueError, match="unknown algorithm"):
        HeaderDigest("sha3", DEV)
    with pytest.raises(ValueError):
        HeaderDigest("sha256d", "cpu")
    assert HeaderDigest("scrypt", DEV, capacity=300).grid == 2  # rounded up to whole blocks of 256 lane slots


def test_native_launchers_refuse_before_launching():
    """n == 0, n above the capacity and misaligned arrays are HIP errors (hipErrorInvalidValue) raised by the
    launcher itself; `out` keeps its fill."""
    import torch

    N = _native()
    hdr = torch.zeros((4, 80), dtype=torch.uint8, device=DEV)
    out = torch.full((4, 32), 0xA5, dtype=torch.uint8, device=DEV)
    H = torch.empty(8 * 4, dtype=torch.int64, device=DEV)
    s = torch.cuda.current_stream(DEV).cuda_stream
    with pytest.raises(RuntimeError, match="HIP error"):
        N.launch_sha256d_digest(hdr.data_ptr() + 4, 3, out.data_ptr(), s)
    with pytest.raises(RuntimeError, match="HIP error"):
        N.launch_x11_digest(hdr.data_ptr(), H.data_ptr(), 4, 4, out.data_ptr() + 8, s)
    with pytest.raises(RuntimeError, match="HIP error"):
        N.launch_scrypt_digest(hdr.data_ptr(), 4, H.data_ptr(), H.data_ptr(), 3, out.data_ptr(), 1, s)  # bad gap
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_hash_many_on_the_device_equals_the_cpu_path():
    from otedama_amd.models.algorithms import hash_many

    for name in ("sha256d", "x11"):
        hs, want = _pool(name)
        assert hash_many(name, list(hs[:70]), device=DEV) == list(want[:70]) == hash_many(name, list(hs[:70]))
