"""The native CPU twin of the batched secp256k1 multiplication (``secp256k1_mul_cpu``, csrc/cpu/secp256k1.cpp), the
native ElligatorSwift encoder and the torch-free row packing, against the big-integer Python of btccrypto.py,
stratum/ellswift.py and stratum/noise.py. Every comparison is exact."""
import random

import pytest

import secp_cases as S
from otedama_amd import btccrypto as ec
from otedama_amd.ops import secp_rows as R
from otedama_amd.ops.native import require_native
from otedama_amd.stratum import ellswift, noise


def _mul(rows):
    out = require_native().secp256k1_mul_cpu(bytes(R.pack_rows(rows)))
    assert len(out) == len(rows) * R.OUT_BYTES
    return out, R.unpack_rows(out, len(rows))


def test_every_row_equals_the_oracle():
    rows = S.ROWS
    assert len(rows) < 513
    out, got = _mul(rows)
    want = S.expected(rows)
    for r, g, w in zip(rows, got, want):
        assert g == w, (hex(r[0]), r[1], r[2].hex())
    for i in range(len(rows)):  # the padding of every output row
        assert out[i * R.OUT_BYTES + 34:(i + 1) * R.OUT_BYTES] == bytes(14)


def test_kind_one_is_noise_dh_and_kind_two_is_ecdh_x():
    seen = set()
    for (scalar, kind, point), (x, _parity, status) in zip(S.ROWS, _mul(S.ROWS)[1]):
        assert status == R.OK
        if kind == R.KIND_XONLY:
            assert x == noise.dh(scalar, point)
        elif kind == R.KIND_ELLSWIFT:
            assert x == ellswift.ecdh_x(scalar, point)
        seen.add(kind)
    assert seen == {R.KIND_G, R.KIND_XONLY, R.KIND_ELLSWIFT}


def test_the_cases_cover_every_xswiftec_way():
    assert {"x1", "x2", "x3"} <= S.CASE_ENCODINGS.keys()
    assert any(k.endswith("+double") for k in S.CASE_ENCODINGS)
    for name, enc in S.CASE_ENCODINGS.items():
        assert S.xswiftec_case(int.from_bytes(enc[:32], "big"), int.from_bytes(enc[32:], "big")) == name


def test_bad_rows_give_their_status_and_zero_bytes():
    assert ec.lift_x(5) is None
    rows = [r for r, _s in S.BAD_ROWS]
    out, got = _mul(rows)
    assert [g[2] for g in got] == [s for _r, s in S.BAD_ROWS] == [1, 1, 1, 2, 2, 3]
    for i, (_r, status) in enumerate(S.BAD_ROWS):
        assert out[i * R.OUT_BYTES:(i + 1) * R.OUT_BYTES] == bytes(32) + bytes([status]) + bytes(15)
    # bad rows between good ones leave them alone
    mixed = S.tiled(40)
    assert any(r in dict(S.BAD_ROWS) for r in mixed)
    assert _mul(mixed)[1] == S.expected(mixed)


def test_the_row_count_limits():
    nat = require_native()
    assert (nat.SECP_ROW_BYTES, nat.SECP_OUT_BYTES, nat.SECP_MAX_ROWS) == (R.ROW_BYTES, R.OUT_BYTES, R.MAX_ROWS)
    row = bytes(R.pack_rows([S.ROWS[0]]))
    for bad in (b"", row[:-1], row + b"\0", bytes(65537 * R.ROW_BYTES)):  # n = 0, ragged, n = 65537
        with pytest.raises(ValueError):
            nat.secp256k1_mul_cpu(bad)
    assert R.unpack_rows(nat.secp256k1_mul_cpu(row), 1) == S.expected([S.ROWS[0]])


def test_pack_and_unpack_round_trip():
    rows = S.tiled(9)
    buf = R.pack_rows(rows)
    assert isinstance(buf, bytearray) and len(buf) == 9 * R.ROW_BYTES
    for i, (scalar, kind, point) in enumerate(rows):
        row = buf[i * R.ROW_BYTES:(i + 1) * R.ROW_BYTES]
        assert int.from_bytes(row[:32], "big") == scalar and row[96] == kind
        assert row[32:96] == point.ljust(64, b"\0") and row[97:] == bytes(31)
    R.wipe_scalars(buf, 9)
    for i, (_scalar, kind, point) in enumerate(rows):
        row = buf[i * R.ROW_BYTES:(i + 1) * R.ROW_BYTES]
        assert row[:32] == bytes(32) and row[96] == kind and row[32:96] == point.ljust(64, b"\0")
    out = b"".join(bytes([i]) * 32 + bytes([i % 4, i % 2]) + bytes(14) for i in range(5))
    assert R.unpack_rows(out, 5) == [(bytes([i]) * 32, i % 2, i % 4) for i in range(5)]
    with pytest.raises(ValueError):
        R.unpack_rows(out, 6)
    for bad in ((1 << 256, 0, b""), (-1, 0, b""), (1, 0, bytes(65)), (1, 256, b"")):
        with pytest.raises(ValueError):
            R.pack_rows([bad])


def test_the_native_encoder_writes_the_bytes_of_ellswift_encode():
    nat = require_native()
    rng = random.Random(200)
    tries_seen = set()
    for _ in range(200):
        x = ec.point_mul(ec.G, rng.randrange(1, ec.N))[0]
        stream = rng.randbytes(33 * 64)
        at = 0

        def rand(n):
            nonlocal at
            at += n
            return stream[at - n:at]

        want = ellswift.encode(x, rand)
        assert nat.ellswift_encode_native(x.to_bytes(32, "big"), stream) == want
        assert ellswift.decode(want) == x
        tries_seen.add(at // 33)
        # a stream that ends one try early is exhausted
        assert nat.ellswift_encode_native(x.to_bytes(32, "big"), stream[:at - 33]) is None
        assert nat.ellswift_encode_native(x.to_bytes(32, "big"), stream[:at]) == want
    assert len(tries_seen) > 3  # first-try and many-try encodings were both compared


def test_the_native_encoder_on_a_stream_that_fails_and_on_bad_input():
    nat = require_native()
    x = ec.G[0].to_bytes(32, "big")
    assert nat.ellswift_encode_native(x, bytes(33)) is None          # u = 0 is skipped
    assert nat.ellswift_encode_native(x, bytes(32)) is None          # not one whole try
    rng = random.Random(7)
    failing = next(s for s in (rng.randbytes(33) for _ in range(64))
                   if ellswift.xswiftec_inv(ec.G[0], int.from_bytes(s[:32], "big"), s[32] & 7) is None)
    assert nat.ellswift_encode_native(x, failing) is None
    with pytest.raises(ValueError):
        nat.ellswift_encode_native((5).to_bytes(32, "big"), bytes(66))  # as ellswift.encode: x not on the curve
    with pytest.raises(ValueError):
        nat.ellswift_encode_native(bytes(31), bytes(66))
