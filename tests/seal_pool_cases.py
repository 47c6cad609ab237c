"""Shared pieces of the pool's frame-sealing tests (test_pool_seal.py, test_seal_gpu.py): a loopback pool with Noise
on, Noise clients that keep their standard channel open, and the checks of a new block's fan-out."""
import asyncio
import struct

import channel_roots_cases as R
import handshake_cases as H
from otedama_amd.models.header import hash_to_int, sha256d
from otedama_amd.stratum import messages as M
from otedama_amd.stratum import noise as N


async def noise_client(pool) -> R.V2Client:
    """A Noise client with one open standard channel; its first job and SetNewPrevHash are consumed."""
    h, p = pool.addr_sv2.rsplit(":", 1)
    reader, writer = await asyncio.open_connection(h, int(p))
    er, ew, _payload, static = await N.client_handshake(reader, writer)
    assert static == pool._noise_static_x[0]
    c = R.V2Client(er, ew)
    await c.send(M.SetupConnection(flags=M.FLAG_REQUIRES_VERSION_ROLLING, vendor="t"))
    assert isinstance(await c.recv(30), M.SetupConnectionSuccess)
    await c.open()
    return c


async def pool_with_clients(k: int, body, seal_fn=None, **kw):
    pool = H.noise_pool(**kw)
    pool.seal_fn = seal_fn
    await pool.start()
    clients = []
    try:
        clients = [await noise_client(pool) for _ in range(k)]
        return await body(pool, clients)
    finally:
        for c in clients:
            c.close()
        await pool.stop()


async def take_block(pool, clients) -> None:
    """Every client decodes the NewMiningJob (with the oracle's root) and the SetNewPrevHash of the pool's new
    block."""
    taken = [await c.take(2) for c in clients]
    job = next(reversed(pool.jobs.values()))
    for c, msgs in zip(clients, taken):
        assert [type(m) for m in msgs] == [M.NewMiningJob, M.SetNewPrevHash], msgs
        assert msgs[0].job_id == job.job_int and msgs[1].prev_hash == job.block.prev_hash
        assert R.check_standard_roots({job.job_int: job}, c, msgs) == 1


async def submit_each(pool, clients) -> int:
    """Every client in turn submits a share of the pool's latest job, which the pool accepts: the counters of both
    directions stayed in step. At the test pool's easy nbits every share is a block too, so each is followed by
    the next block's two messages for every client. Returns how many blocks that were."""
    target = hash_to_int(pool.share_target(1e-6))
    for seq, c in enumerate(clients, 1):
        job = next(reversed(pool.jobs.values()))
        (channel_id, (extranonce, _extended)), = c.channels.items()
        hdr = pool.header_for(job, extranonce, job.version, job.ntime, 0)
        nonce = next(n for n in range(1 << 20) if hash_to_int(sha256d(hdr[:76] + struct.pack("<I", n))) <= target)
        await c.send(M.SubmitSharesStandard(channel_id=channel_id, sequence_number=seq, job_id=job.job_int,
                                            nonce=nonce, ntime=job.ntime, nversion=job.version))
        ok = await c.recv(30)
        assert isinstance(ok, M.SubmitSharesSuccess) and ok.new_submits_accepted == 1, ok
        await take_block(pool, clients)
    return len(clients)


async def check_new_block(pool, clients) -> int:
    """``new_block()`` and what follows from it, as above. Returns the blocks the pool made in all."""
    pool.new_block()
    await take_block(pool, clients)
    return 1 + await submit_each(pool, clients)
