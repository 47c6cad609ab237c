"""Shared pieces of the channel-roots tests (test_channel_roots_cpu.py, test_channel_roots_gpu.py): the oracle, the
prefixes, and a raw Stratum V2 client that opens channels on a loopback ``PoolServer`` and collects the job messages
the pool sends them. Everything here is deterministic."""
import asyncio

from share_verify_cases import ADDR, EASY_NBITS, rnd

from otedama_amd.models.header import sha256d
from otedama_amd.pool.server import PoolOptions, PoolServer
from otedama_amd.pool.template import TemplateSource, merkle_root_from_branches
from otedama_amd.stratum import messages as M
from otedama_amd.stratum.frame import FrameReader


def oracle_root(job, prefix: bytes) -> bytes:
    """``job``: anything with coinb1, coinb2 and branches (a ShareJob or a PoolJob)."""
    return merkle_root_from_branches(sha256d(job.coinb1 + prefix + job.coinb2), job.branches)


def make_prefixes(job, n: int, tag: str = "p") -> list:
    """n distinct prefixes of the job's extranonce size."""
    return [rnd(f"{tag}.{i}.{len(job.coinb1)}.{job.en_size}", job.en_size) for i in range(n)]


def seeded_pool(seed: bytes = b"channel-roots", n_txs: int = 7, **kw) -> PoolServer:
    """A pool whose blocks, extranonce prefixes and job ids depend on ``seed`` alone (the caller pins the clock)."""
    pool = PoolServer(PoolOptions(payout_address=ADDR, job_interval=3600, block_interval=3600, nbits=EASY_NBITS,
                                  n_txs=n_txs, initial_difficulty=1e-6, fixed_difficulty=True, **kw))
    pool.templates = TemplateSource(ADDR, nbits=EASY_NBITS, n_txs=n_txs, seed=seed)
    pool._en_counter = 0x01020000
    return pool


class V2Client:
    """One SV2 connection: ``open()`` returns the channel's success message; ``take(k)`` the next k messages."""

    def __init__(self, reader, writer):
        self.w = writer
        self.frames = FrameReader(reader)
        self.channels: dict = {}  # channel id -> (extranonce prefix, extended)

    @classmethod
    async def connect(cls, pool):
        h, p = pool.addr_sv2.rsplit(":", 1)
        c = cls(*await asyncio.open_connection(h, int(p)))
        await c.send(M.SetupConnection(flags=M.FLAG_REQUIRES_VERSION_ROLLING, vendor="t"))
        assert isinstance(await c.recv(), M.SetupConnectionSuccess)
        return c

    async def send(self, msg):
        self.w.write(M.encode_message(msg))
        await self.w.drain()

    async def recv(self, timeout=5.0):
        return M.dispatch_frame(await asyncio.wait_for(self.frames.read_frame(), timeout))

    async def take(self, k: int) -> list:
        return [await self.recv() for _ in range(k)]

    async def open(self, extended: bool = False):
        """Open a channel; returns ``(success message, [the future job, its SetNewPrevHash])``."""
        if extended:
            await self.send(M.OpenExtendedMiningChannel(req_id=7, user=ADDR, nominal_hashrate=0.0))
        else:
            await self.send(M.OpenMiningChannel(req_id=7, user=ADDR, nominal_hashrate=0.0))
        ok = await self.recv()
        assert isinstance(ok, (M.OpenMiningChannelSuccess, M.OpenExtendedMiningChannelSuccess)), ok
        self.channels[ok.channel_id] = (ok.extranonce_prefix if extended else ok.extranonce, extended)
        return ok, await self.take(2)

    def close(self):
        self.w.close()


def check_standard_roots(jobs: dict, client: V2Client, msgs: list) -> int:
    """Every NewMiningJob in ``msgs`` carries the oracle's root of its job (``jobs``: job_int -> PoolJob; a new
    block drops the pool's own) for its channel's prefix; returns how many there were."""
    n = 0
    for m in msgs:
        if isinstance(m, M.NewMiningJob):
            prefix, extended = client.channels[m.channel_id]
            assert not extended
            assert m.merkle_root == oracle_root(jobs[m.job_id], prefix), (m.channel_id, m.job_id)
            n += 1
    return n
