"""Shared pieces of the batched-handshake pool tests (test_pool_handshakes.py, test_secp_gpu.py): a loopback pool
with Noise on and a crowd of Noise clients that all send message 1 before any of them reads message 2, so the pool's
batcher sees them together."""
import asyncio
import struct
import time

import channel_roots_cases as R

from otedama_amd.stratum import messages as M
from otedama_amd.stratum import noise as N

SUITES_64 = ["ellswift"] * 48 + ["legacy"] * 16
BAD_MESSAGE1 = (5).to_bytes(32, "big")  # a legacy key that is not on the curve


def noise_pool(**kw):
    return R.seeded_pool(seed=b"handshakes", noise=True, **kw)


async def _finish(pool, initiator, reader, writer):
    """Message 2 -> an open standard channel with its first job; None when the pool closed the connection."""
    try:
        n = struct.unpack("<H", await asyncio.wait_for(reader.readexactly(2), 30))[0]
        m2 = await asyncio.wait_for(reader.readexactly(n), 30)
    except (asyncio.IncompleteReadError, ConnectionError):
        return None
    if initiator is None:
        return m2
    initiator.read_message2(m2)
    assert initiator.remote_static == pool._noise_static_x[0]
    assert N.verify_certificate(initiator.payload, initiator.remote_static, pool.noise_authority_pub, int(time.time()))
    c = R.V2Client(N.EncryptedReader(reader, initiator.recv), N.EncryptedWriter(writer, initiator.send))
    await c.send(M.SetupConnection(flags=M.FLAG_REQUIRES_VERSION_ROLLING, vendor="t"))
    assert isinstance(await c.recv(30), M.SetupConnectionSuccess)
    ok, first = await c.open()
    c.close()
    return ok, first


async def crowd(pool, suites, bad_at=None):
    """``len(suites)`` Noise clients (and, at index ``bad_at`` of the sends, one that sends ``BAD_MESSAGE1``) connect,
    all send message 1, then all finish. Returns ``(channels, bad)``: per good client ``(open success, [job,
    prevhash])``, and what the bad client got (None: the pool closed it)."""
    initiators = [N.Initiator(suite=s) for s in suites]
    firsts = [i.write_message1() for i in initiators]
    if bad_at is not None:
        initiators.insert(bad_at, None)
        firsts.insert(bad_at, BAD_MESSAGE1)
    h, p = pool.addr_sv2.rsplit(":", 1)
    conns = await asyncio.gather(*(asyncio.open_connection(h, int(p)) for _ in firsts))
    for (_r, w), m1 in zip(conns, firsts):
        w.write(struct.pack("<H", len(m1)) + m1)
    done = await asyncio.gather(*(_finish(pool, i, r, w) for i, (r, w) in zip(initiators, conns)))
    for _r, w in conns:
        w.close()
    bad = done.pop(bad_at) if bad_at is not None else None
    return done, bad


def check_channels(channels, n: int) -> None:
    assert len(channels) == n and all(c is not None for c in channels)
    ids = set()
    for ok, first in channels:
        assert isinstance(ok, M.OpenMiningChannelSuccess)
        assert any(isinstance(m, M.NewMiningJob) for m in first), first
        ids.add(bytes(ok.extranonce))
    assert len(ids) == n  # every connection its own channel
