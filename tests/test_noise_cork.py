"""Corked Noise writers (``noise.EncryptedWriter.cork`` / ``CipherState.reserve``) and the pool's ``FrameSealer``
around them (otedama_amd/pool/frameseal.py), without a pool and without a GPU: a corked stream must be byte for byte
the stream the same writes give one frame at a time."""
import asyncio
import struct
import types

import pytest

from otedama_amd.pool import devicepath
from otedama_amd.pool.batch import seal_frames
from otedama_amd.pool.frameseal import DEFAULT_SEAL_MIN_GPU, FrameSealer
from otedama_amd.stratum import noise as N

KEY = bytes(range(1, 33))
STEP = N.MAX_FRAME - N.TAG
WRITES = [b"job " * 14, b"", b"prevhash" * 7, bytes(range(256)) * 300, b"x" * STEP, b"tail"]  # 76800 bytes: two frames


class Recorder:
    """The transport under an EncryptedWriter: keeps what is written."""

    def __init__(self):
        self.data = bytearray()
        self.closed = False

    def write(self, b):
        self.data += b

    def close(self):
        self.closed = True


def _writer(counter: int = 0):
    cs = N.CipherState(KEY)
    cs.n = counter
    rec = Recorder()
    return N.EncryptedWriter(rec, cs), rec, cs


def _flush(batch, device="cpu"):
    sealed = seal_frames([(k, c, p) for _w, k, c, p in batch], device)
    for (w, _k, _c, _p), s in zip(batch, sealed):
        w.transport.write(struct.pack("<H", len(s)) + s)


def _pool(**kw):
    logs = []
    opts = types.SimpleNamespace(**{"seal_device": "cpu", "seal_min_gpu": 0, **kw})
    pool = types.SimpleNamespace(opts=opts, algo=types.SimpleNamespace(name="sha256d"), logs=logs,
                                 log=lambda level, msg: logs.append((level, msg)))
    return pool


def test_reserve_hands_out_the_counters_encrypt_would_use():
    cs = N.CipherState(KEY)
    assert [cs.reserve(), cs.reserve()] == [0, 1] and cs.n == 2
    plain = N.CipherState(KEY)
    plain.n = 2
    assert cs.encrypt(b"", b"abc") == plain.encrypt(b"", b"abc") and cs.n == 3
    cs.n = 2 ** 64 - 2
    assert cs.reserve() == 2 ** 64 - 2
    with pytest.raises(N.NoiseError, match="exhausted"):
        cs.reserve()
    assert cs.n == 2 ** 64 - 1


def test_a_corked_stream_is_the_uncorked_stream_byte_for_byte():
    plain_w, plain_rec, plain_cs = _writer(counter=2 ** 32 - 2)
    corked_w, corked_rec, corked_cs = _writer(counter=2 ** 32 - 2)
    batch = []
    assert corked_w.cork(batch) is True
    for data in WRITES:
        plain_w.write(data)
        corked_w.write(data)
    assert corked_rec.data == b""  # nothing leaves before the flush
    assert len(batch) == 7 == corked_cs.n - (2 ** 32 - 2) and corked_cs.n == plain_cs.n  # one write gave two chunks
    assert [c for _w, _k, c, _p in batch] == list(range(2 ** 32 - 2, 2 ** 32 + 5))
    assert [len(p) for _w, _k, _c, p in batch] == [56, 0, 56, STEP, 76800 - STEP, STEP, 4]
    assert all(w is corked_w and k == KEY for w, k, _c, _p in batch)
    _flush(batch)
    corked_w.uncork()
    assert bytes(corked_rec.data) == bytes(plain_rec.data)
    plain_w.write(b"after")
    corked_w.write(b"after")  # uncorked: sealed at once again
    assert bytes(corked_rec.data) == bytes(plain_rec.data)


def test_a_reader_sees_the_writes_before_during_and_after_the_cork_in_order():
    async def body():
        w, rec, _cs = _writer()
        w.write(b"before")
        batch = []
        w.cork(batch)
        w.write(b"corked-1")
        w.write(bytes(70000))  # two frames
        w.write(b"corked-3")
        _flush(batch)
        w.uncork()
        w.write(b"after")
        stream = asyncio.StreamReader()
        stream.feed_data(bytes(rec.data))
        stream.feed_eof()
        r = N.EncryptedReader(stream, N.CipherState(KEY))
        out = [await r.readexactly(6), await r.readexactly(8), await r.readexactly(70000), await r.readexactly(8),
               await r.readexactly(5)]
        return out, await r.read()

    out, rest = asyncio.run(body())
    assert out == [b"before", b"corked-1", bytes(70000), b"corked-3", b"after"] and rest == b""


def test_an_oversize_chunk_raises_and_reserves_nothing():
    w, rec, cs = _writer(counter=5)
    batch = []
    w.cork(batch)
    with pytest.raises(N.NoiseError, match="too large"):
        w._queue(bytes(STEP + 1))
    assert cs.n == 5 and batch == [] and rec.data == b""
    w._queue(bytes(STEP))  # the largest frame
    assert cs.n == 6 and len(batch) == 1
    # as the uncorked writer's encode_frame
    with pytest.raises(N.NoiseError, match="too large"):
        N.encode_frame(cs, bytes(STEP + 1))
    assert cs.n == 6


def test_an_unkeyed_writer_is_untouched_by_cork():
    rec = Recorder()
    w = N.EncryptedWriter(rec, N.CipherState())
    batch = []
    assert w.cork(batch) is False
    w.write(b"plain")
    assert batch == [] and bytes(rec.data) == struct.pack("<H", 5) + b"plain"
    pool = _pool()
    sealer = FrameSealer(pool)
    with sealer.corked([types.SimpleNamespace(writer=w), types.SimpleNamespace(writer=rec)]) as queued:
        w.write(b"again")
    sealer.close()
    assert queued == [] and bytes(rec.data).endswith(struct.pack("<H", 5) + b"again") and sealer.batches == 0


def test_the_sealer_flushes_in_order_and_uncorks_also_when_the_body_raises():
    pool = _pool()
    sealer = FrameSealer(pool)
    (wa, ra, _), (wb, rb, _) = _writer(), _writer(counter=9)
    (pa, rpa, _), (pb, rpb, _) = _writer(), _writer(counter=9)
    conns = [types.SimpleNamespace(writer=wa), types.SimpleNamespace(writer=wb)]
    with pytest.raises(KeyError):
        with sealer.corked(conns):
            for w, p in ((wa, pa), (wb, pb), (wa, pa)):
                w.write(b"m" * 55)
                p.write(b"m" * 55)
            raise KeyError("the fan-out broke off")
    sealer.close()
    assert bytes(ra.data) == bytes(rpa.data) and bytes(rb.data) == bytes(rpb.data) and len(ra.data) == 2 * (2 + 55 + 16)
    wa.write(b"later")
    pa.write(b"later")
    assert bytes(ra.data) == bytes(rpa.data)  # uncorked
    st = sealer.stats()
    assert (st["batches"], st["cpu_frames"], st["gpu_frames"], st["last_frames"]) == (1, 3, 0, 3)
    assert set(st) == {"device", "enabled", "batches", "gpu_frames", "cpu_frames", "last_frames", "last_ms",
                       "device_errors"}
    assert DEFAULT_SEAL_MIN_GPU >= 1


def test_a_seal_fn_that_raises_falls_back_with_the_same_bytes():
    calls = []

    def broken(frames):
        calls.append(len(frames))
        raise RuntimeError("injected device failure")

    devicepath.forget_device_errors()
    try:
        pool = _pool(seal_device="cuda:0", seal_min_gpu=1)
        sealer = FrameSealer(pool, device_seal=broken)
        (w, rec, _), (p, prec, _) = _writer(), _writer()
        for _round in range(2):
            with sealer.corked([types.SimpleNamespace(writer=w)]):
                for data in (b"a" * 55, b"b" * 54):
                    w.write(data)
                    p.write(data)
        sealer.close()
        st = sealer.stats()
        failed = devicepath.device_failed("cuda:0")
        other = devicepath.DevicePath("job_device", "cuda:0").enabled
    finally:
        devicepath.forget_device_errors()
    assert bytes(rec.data) == bytes(prec.data) and len(rec.data) == 2 * (2 + 55 + 16) + 2 * (2 + 54 + 16)
    assert calls == [2]  # asked once, never again
    assert failed and other is False
    assert (st["device"], st["enabled"], st["device_errors"], st["gpu_frames"], st["cpu_frames"]) == (
        "cuda:0", False, 1, 0, 4)
    assert any(level == "error" and "frame sealing on cuda:0 failed" in msg for level, msg in pool.logs)


def test_a_fake_device_path_is_counted_as_the_gpu_above_the_threshold():
    devicepath.forget_device_errors()
    pool = _pool(seal_device="cuda:0", seal_min_gpu=3)
    sealer = FrameSealer(pool, device_seal=lambda frames: seal_frames(frames, "cpu"))
    (w, rec, _), (p, prec, _) = _writer(), _writer()
    for k in (2, 3):
        with sealer.corked([types.SimpleNamespace(writer=w)]):
            for _i in range(k):
                w.write(b"z" * 55)
                p.write(b"z" * 55)
    sealer.close()
    assert bytes(rec.data) == bytes(prec.data)
    st = sealer.stats()
    assert (st["gpu_frames"], st["cpu_frames"], st["batches"], st["device_errors"], st["enabled"]) == (3, 2, 2, 0, True)


def test_when_no_path_can_seal_the_connections_are_closed(monkeypatch):
    from otedama_amd.pool import frameseal

    def nothing_works(frames, device=None):
        raise RuntimeError("no cipher")

    monkeypatch.setattr(frameseal, "seal_frames", nothing_works)
    pool = _pool()
    sealer = FrameSealer(pool)
    (wa, ra, _), (wb, rb, _) = _writer(), _writer()
    idle, ridle, _ = _writer()
    with sealer.corked([types.SimpleNamespace(writer=w) for w in (wa, wb, idle)]):
        wa.write(b"a")
        wb.write(b"b")
    sealer.close()
    assert ra.closed and rb.closed and not ridle.closed and ra.data == rb.data == b""
    assert any(level == "error" and "connections are closed" in msg for level, msg in pool.logs)


def test_the_sealer_refuses_bad_options():
    for kw in ({"seal_device": "gpu0"}, {"seal_device": ""}, {"seal_min_gpu": -1}):
        with pytest.raises(ValueError):
            FrameSealer(_pool(**kw))
