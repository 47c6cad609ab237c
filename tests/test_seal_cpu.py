"""Batched frame sealing without a GPU: the OpenSSL twin ``aead_seal_many_cpu``, the gfx950 kernel's arithmetic
compiled for the host (``_aead_seal_rows_host``, ``_poly1305_rows_host``; csrc/include/otedama/chacha_poly.h), the
packing of ops/seal_rows.py and the three paths of ``pool.batch.seal_frames``.

Every comparison is exact byte equality against ``utils.aead.seal`` (OpenSSL, pinned to RFC 8439 below) or the
big-integer Poly1305 of seal_cases.py."""
import pytest

import seal_cases as C
from otedama_amd.ops import seal_rows as R
from otedama_amd.ops.native import require_native
from otedama_amd.pool.batch import seal_frames
from otedama_amd.utils import aead


def test_the_oracle_reproduces_rfc_8439():
    sealed = aead.seal(aead.CHACHA20POLY1305, bytes(range(0x80, 0xa0)), bytes.fromhex("070000004041424344454647"),
                       b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
                       b"sunscreen would be it.", bytes.fromhex("50515253c0c1c2c3c4c5c6c7"))
    assert sealed[:16].hex() == "d31a8d34648e60db7b86afbc53ef7ec2"
    assert sealed[-16:].hex() == "1ae10b594f09e26a7e902ecbd0600691" and len(sealed) == 114 + 16


@pytest.mark.parametrize("entry", ["aead_seal_many_cpu", "_aead_seal_rows_host"])
@pytest.mark.parametrize("name", sorted(C.batches()))
def test_the_twin_and_the_host_header_equal_the_oracle(entry, name):
    frames = C.batches()[name]
    packed, out_bytes = R.pack_frames(frames)
    out = getattr(require_native(), entry)(packed, len(frames))
    assert len(out) == out_bytes
    got = R.unpack_sealed(packed, out, len(frames))
    want = C.expected(name)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(frames[i][2]), frames[i][1])
    assert len(got) == len(want) and list(got) != list(C.expected_bumped(name))
    # the padding of every region is zero, in both implementations
    at = 0
    for _k, _c, plain in frames:
        end = at + 16 + (len(plain) + 15) // 16 * 16
        assert out[at + 16 + len(plain):end] == bytes(end - at - 16 - len(plain))
        at = end
    assert at == out_bytes


def test_poly1305_rows_on_the_host_equal_the_big_integer_oracle():
    rows, tags = C.poly_rows()
    for key, msg, tag in C.POLY_TABLE:  # the table's tags are what the oracle computes
        assert C.poly1305(key, msg) == tag
    out = require_native()._poly1305_rows_host(R.pack_poly_rows(rows))
    assert len(out) == 16 * len(rows)
    for i, tag in enumerate(tags):
        assert out[16 * i:16 * i + 16] == tag, (i, rows[i])


def test_seal_frames_gives_the_same_bytes_by_all_three_paths(monkeypatch):
    frames = C.batches()["lengths"][:140] + C.batches()["n65"]
    want = C.oracle(frames)
    assert seal_frames(frames, None) == want
    assert seal_frames(frames, "cpu") == want
    assert seal_frames([], "cpu") == [] and seal_frames([], None) == []

    # the third path without a device: the process's op for that device, here one that runs the kernel's arithmetic
    # on the host in place of the launch (test_seal_gpu.py runs the real one)
    from otedama_amd.pool import batch

    class HostSeal:
        def seal(self, fr):
            packed, _ = R.pack_frames(fr)
            return R.unpack_sealed(packed, require_native()._aead_seal_rows_host(packed, len(fr)), len(fr))

    monkeypatch.setitem(batch._ops, ("seal", "", "cuda:7"), HostSeal())
    assert seal_frames(frames, "cuda:7") == want


@pytest.mark.parametrize("device", [None, "cpu"])
def test_a_frame_over_the_limit_keeps_its_place(device):
    r = C._rnd("big")
    frames = [(r.randbytes(32), 7, r.randbytes(n)) for n in (55, R.SEAL_MAX_PLAIN + 1, 0, 65519, R.SEAL_MAX_PLAIN, 54)]
    assert seal_frames(frames, device) == C.oracle(frames)
    assert seal_frames(frames[1:2], device) == C.oracle(frames[1:2])  # nothing is left for the batch


def test_pack_frames_refuses_what_the_kernel_must_not_see():
    key = bytes(range(32))
    for bad in ((key[:31], 0, b"x"), (key, 2 ** 64 - 1, b"x"), (key, -1, b"x"), (key, 0, bytes(R.SEAL_MAX_PLAIN + 1))):
        with pytest.raises(ValueError):
            R.pack_frames([(key, 0, b"ok"), bad])
    with pytest.raises(ValueError):
        R.pack_frames([])
    with pytest.raises(ValueError):
        seal_frames([(key, 2 ** 64 - 1, b"x")], None)
    native = require_native()
    packed, _ = R.pack_frames([(key, 3, b"hello")])
    for at, value in ((40, 2049), (44, 72), (44, 1 << 20), (48, 8)):  # len, in_off misaligned / outside, out_off
        broken = bytearray(packed)
        broken[at:at + 4] = value.to_bytes(4, "little")
        for entry in (native.aead_seal_many_cpu, native._aead_seal_rows_host):
            with pytest.raises(ValueError):
                entry(broken, 1)
    for entry in (native.aead_seal_many_cpu, native._aead_seal_rows_host):
        with pytest.raises(ValueError):
            entry(packed, 2)  # more heads than the buffer holds
        with pytest.raises(ValueError):
            entry(packed, 0)


def test_wipe_keys_leaves_no_key_byte():
    frames = [(bytes([0xC0 + i]) * 32, i, bytes(20 + i)) for i in range(9)]  # key bytes that occur nowhere else
    packed, out_bytes = R.pack_frames(frames)
    before = bytes(packed)
    assert all(bytes([0xC0 + i]) * 32 in before for i in range(9))
    sealed = R.unpack_sealed(packed, require_native().aead_seal_many_cpu(packed, 9), 9)
    R.wipe_keys(packed, 9)
    assert all(packed[i * 64:i * 64 + 32] == bytes(32) for i in range(9))
    assert not any(bytes([0xC0 + i]) * 2 in packed for i in range(9))  # not two bytes of a key side by side
    assert bytes(packed[9 * R.HEAD_BYTES:]) == before[9 * R.HEAD_BYTES:]  # the data region is untouched
    for i in range(9):  # and so is the rest of every head: the frames can still be unpacked
        assert packed[i * 64 + 32:(i + 1) * 64] == before[i * 64 + 32:(i + 1) * 64]
    assert sealed == C.oracle(frames)
