"""``noise.Responder`` with its curve arithmetic done elsewhere (``ec_requests`` / ``write_message2(ec=)``): fed the
results of the native ``secp256k1_mul_cpu`` it writes the bytes the untouched Python path writes, and an untouched
``Initiator`` completes against it."""
import hashlib

import pytest

from otedama_amd import btccrypto as ec
from otedama_amd.ops import secp_rows as R
from otedama_amd.ops.native import require_native
from otedama_amd.stratum import ellswift
from otedama_amd.stratum import noise as N

STATIC = 0x1F2E3D4C5B6A79880102030405060708090A0B0C0D0E0F101112131415161718
PAYLOAD = b"certificate-bytes" * 4


class Stream:
    """``os.urandom`` from one fixed byte stream, read in order: the same calls get the same bytes."""

    def __init__(self, seed: bytes):
        self.seed, self.at, self.calls = seed, 0, []

    def __call__(self, n: int) -> bytes:
        out = b""
        while len(out) < n:
            block = (self.at + len(out)) // 32
            out += hashlib.sha256(self.seed + block.to_bytes(8, "big")).digest()[(self.at + len(out)) % 32:]
        self.at += n
        self.calls.append(n)
        return out[:n]


def _patch(monkeypatch, stream) -> None:
    """Every random byte of a handshake from ``stream``: ``os.urandom`` and the ``rand=os.urandom`` defaults that
    stratum/ellswift.py bound when it was imported."""
    monkeypatch.setattr(N.os, "urandom", stream)
    monkeypatch.setattr(ellswift.encode, "__defaults__", (stream,))
    monkeypatch.setattr(ellswift.create, "__defaults__", (stream,))


def _initiator(suite, monkeypatch, expected_static=None):
    _patch(monkeypatch, Stream(b"initiator/" + suite.encode()))
    i = N.Initiator(expected_static=expected_static, suite=suite)
    return i, i.write_message1()


def _mul(rows):
    return R.unpack_rows(require_native().secp256k1_mul_cpu(R.pack_rows(rows)), len(rows))


@pytest.mark.parametrize("suite", N.SUITES)
def test_batched_results_write_the_python_paths_message2(suite, monkeypatch):
    i, m1 = _initiator(suite, monkeypatch)
    assert len(m1) == (64 if suite == "ellswift" else 32)

    # the untouched path: no static_x, ec=None
    _patch(monkeypatch, Stream(b"responder"))
    plain = N.Responder(STATIC)
    plain.read_message1(m1)
    want = plain.write_message2(PAYLOAD)

    # static_x given, still in Python
    _patch(monkeypatch, Stream(b"responder"))
    known = N.Responder(STATIC, static_x=N.static_point(STATIC))
    known.read_message1(m1)
    assert known.write_message2(PAYLOAD) == want and known.s_xonly == plain.s_xonly

    # the three rows computed by the native CPU twin
    stream = Stream(b"responder")
    _patch(monkeypatch, stream)
    r = N.Responder(STATIC, static_x=N.static_point(STATIC))
    r.read_message1(m1)
    rows = r.ec_requests()
    kind = R.KIND_ELLSWIFT if suite == "ellswift" else R.KIND_XONLY
    assert [(k, p) for _s, k, p in rows] == [(R.KIND_G, b""), (kind, m1), (kind, m1)]
    assert rows[0][0] == rows[1][0] and 0 < rows[0][0] < ec.N and rows[2][0] in (STATIC, ec.N - STATIC)
    got = r.write_message2(PAYLOAD, ec=_mul(rows))
    assert got == want
    assert stream.calls.count(32) == 1 and set(stream.calls) == ({32, 33} if suite == "ellswift" else {32})
    assert len(got) == (234 - 74 + len(PAYLOAD) if suite == "ellswift" else 32 + 48 + len(PAYLOAD) + 16)
    assert r.handshake_hash == plain.handshake_hash

    # the untouched initiator completes against it, pinned to the static key, and frames pass both ways
    assert i.read_message2(got) == PAYLOAD
    assert i.remote_static == r.s_xonly == N.keypair(STATIC)[1] and i.handshake_hash == r.handshake_hash
    assert r.recv.decrypt(b"", i.send.encrypt(b"", b"to the pool")) == b"to the pool"
    assert i.recv.decrypt(b"", r.send.encrypt(b"", b"to the miner")) == b"to the miner"


@pytest.mark.parametrize("suite", N.SUITES)
def test_with_static_x_the_python_path_multiplies_three_times(suite, monkeypatch):
    i, m1 = _initiator(suite, monkeypatch)
    static_x = N.static_point(STATIC)
    calls = []
    real = ec.point_mul

    def counted(pt, k):
        calls.append(k)
        return real(pt, k)

    monkeypatch.setattr(ec, "point_mul", counted)
    r = N.Responder(STATIC, static_x=static_x)
    r.read_message1(m1)
    m2 = r.write_message2(PAYLOAD)
    assert len(calls) == 3
    del calls[:]
    old = N.Responder(STATIC)
    old.read_message1(m1)
    old.write_message2(PAYLOAD)
    assert len(calls) == 5  # the two static·G that static_x saves
    monkeypatch.setattr(ec, "point_mul", real)
    assert i.read_message2(m2) == PAYLOAD


def test_a_bad_status_or_a_missing_result_is_a_noise_error(monkeypatch):
    _i, m1 = _initiator("legacy", monkeypatch)
    r = N.Responder(STATIC, static_x=N.static_point(STATIC))
    with pytest.raises(N.NoiseError):
        r.read_message1(m1 + b"\0")
    r.read_message1((5).to_bytes(32, "big"))  # x = 5 is not on the curve: only the multiplication finds out
    rows = r.ec_requests()
    res = _mul(rows)
    assert [s for _x, _p, s in res] == [R.OK, R.BAD_POINT, R.BAD_POINT]
    with pytest.raises(N.NoiseError):
        r.write_message2(PAYLOAD, ec=res)
    with pytest.raises(N.NoiseError):
        r.write_message2(PAYLOAD, ec=res[:2])
    fresh = N.Responder(STATIC, static_x=N.static_point(STATIC))
    fresh.read_message1(m1)
    with pytest.raises(N.NoiseError):  # results without ec_requests() before them
        fresh.write_message2(PAYLOAD, ec=res)
    with pytest.raises(N.NoiseError):  # the Python path refuses the same key
        r.write_message2(PAYLOAD)
