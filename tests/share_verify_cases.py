"""Shared cases of the share-verification tests (test_share_verify_cpu.py, test_share_verify_gpu.py): the job
grid of the block format, the Python oracle of a job's headers, and the scripted batch that drives
``PoolServer.validate_many`` against sequential ``validate``. Everything here is deterministic."""
import asyncio
import hashlib
import struct
import time

from otedama_amd.models.header import hash_to_int, sha256d, target_from_nbits
from otedama_amd.pool.batch import ShareJob, header_of
from otedama_amd.pool.server import BIP320_MASK, PoolOptions, PoolServer
from otedama_amd.pool.template import TemplateSource

ADDR = "bc1qar0srrr7xfkvy5l643lydnw9re59gtzzwf5mdq"
COINB1_LENGTHS = (1, 41, 55, 56, 63, 64, 65, 119, 120, 128, 200)
EN_SIZES = (1, 4, 8, 13, 16)
TOTAL_MOD_64 = (0, 55, 56, 63)  # padding edges: exact block, last length that fits, first that spills, one short
BRANCH_COUNTS = (0, 1, 12, 32)
# none of the lengths above puts the extranonce at byte 2 of a word; these do (one of them across a block boundary)
EXTRA_COINB1_LENGTHS = (2, 62)
EASY_NBITS = 0x2000FFFF  # target 0xffff << 232: about one hash in 256 is a block


def rnd(tag: str, n: int) -> bytes:
    out = b""
    i = 0
    while len(out) < n:
        out += hashlib.sha256(f"{tag}/{i}".encode()).digest()
        i += 1
    return out[:n]


def make_job(len1: int, en_size: int, total_mod: int, n_branches: int, extra_blocks: int = 0,
             nbits: int = EASY_NBITS) -> ShareJob:
    """A job whose coinbase (coinb1 | extranonce | coinb2) is ``total_mod`` bytes past a multiple of 64."""
    len2 = (total_mod - len1 - en_size) % 64 + 64 * extra_blocks
    tag = f"{len1}.{en_size}.{total_mod}.{n_branches}"
    return ShareJob(rnd("c1." + tag, len1), rnd("c2." + tag, len2), en_size, rnd("prev." + tag, 32), nbits,
                    [rnd(f"br{k}." + tag, 32) for k in range(n_branches)])


def full_grid():
    for len1 in COINB1_LENGTHS + EXTRA_COINB1_LENGTHS:
        for en_size in EN_SIZES:
            for i, total_mod in enumerate(TOTAL_MOD_64):
                for n_branches in BRANCH_COUNTS:
                    yield make_job(len1, en_size, total_mod, n_branches, extra_blocks=(len1 + i) % 2)


def edge_flags(job: ShareJob) -> set:
    """The edges of the issue that this job covers."""
    off = len(job.coinb1) % 64
    flags = {f"offset%4={off % 4}", f"total%64={(len(job.coinb1) + job.en_size + len(job.coinb2)) % 64}",
             f"branches={len(job.branches)}"}
    if off + job.en_size > 64:
        flags.add("straddle")
    if off == 0:
        flags.add("offset0")
    return flags


ALL_EDGES = ({f"offset%4={k}" for k in range(4)} | {f"total%64={k}" for k in TOTAL_MOD_64}
             | {f"branches={k}" for k in BRANCH_COUNTS} | {"straddle", "offset0"})


def make_shares(job: ShareJob, n: int, tag: str = "s") -> list:
    """n distinct shares; all 32 bits of every field are exercised."""
    out = []
    for i in range(n):
        r = rnd(f"{tag}.{i}.{len(job.coinb1)}.{job.en_size}", 16 + 12)
        ntime, nonce, version = struct.unpack_from("<III", r, 16)
        out.append((r[:job.en_size], ntime, nonce, version))
    return out


def oracle_headers(job: ShareJob, shares) -> list:
    return [header_of(job, en, ntime, nonce, version) for en, ntime, nonce, version in shares]


def reduced_grid() -> list:
    """At least 12 jobs that together still contain every edge of the full grid."""
    picks = [(1, 1, 0, 0), (41, 4, 55, 1), (55, 13, 56, 12), (56, 16, 63, 32), (63, 8, 0, 12), (64, 8, 55, 1),
             (65, 4, 56, 0), (119, 13, 63, 12), (120, 16, 0, 32), (128, 1, 55, 12), (200, 8, 56, 1), (63, 1, 63, 0),
             (62, 16, 56, 12), (200, 16, 63, 32)]
    jobs = [make_job(*p, extra_blocks=k % 2) for k, p in enumerate(picks)]
    covered = set().union(*(edge_flags(j) for j in jobs))
    assert covered >= ALL_EDGES, ALL_EDGES - covered
    return jobs


def pool_job(n_txs: int = 7, nbits: int = EASY_NBITS, en_size: int = 8) -> ShareJob:
    """The pool's real job: PoolServer._make_job's parts for a template with ``n_txs`` transactions."""
    blk = TemplateSource(ADDR, nbits=nbits, n_txs=n_txs, seed=b"share-verify").next_block()
    coinb1, coinb2 = blk.coinbase_parts(en_size)
    return ShareJob(coinb1, coinb2, en_size, blk.prev_hash, blk.nbits, blk.branches())


# ---------------------------------------------------------------- PoolServer.validate_many script
D0 = 1e-9           # every worker's difficulty
D_RAISED = 4e-9     # the retargeted worker's new difficulty


class ScriptedPool:
    """A PoolServer on a fixed template with two workers: ``rig`` at D0 and ``ramp``, just retargeted from D0 to
    D_RAISED (inside the grace window). Two instances built from the same template hold identical jobs."""

    def __init__(self, template, algorithm: str = "sha256d"):
        self.loop = asyncio.new_event_loop()  # a found block schedules new_block() on the loop; it never runs here
        asyncio.set_event_loop(self.loop)
        self.pool = PoolServer(PoolOptions(algorithm=algorithm, payout_address=ADDR, initial_difficulty=D0,
                                           min_difficulty=1e-12, fixed_difficulty=True))
        p = self.pool
        p.block = template
        p.jobs.clear()
        p._seen.clear()
        self.job = p._make_job(clean=True)
        self.job.ntime = template.ntime  # not the wall clock: both pools must hold the same job
        self.rig = p.new_worker("rig", BIP320_MASK)
        self.ramp = p.new_worker("ramp", BIP320_MASK)
        self.ramp.retargeted(D0, D_RAISED)
        self.ramp.vd.difficulty = D_RAISED

    def close(self):
        self.pool.journal.close()
        self.pool._hash_pool.shutdown(wait=False)
        asyncio.set_event_loop(None)
        self.loop.close()

    def state(self) -> dict:
        p = self.pool
        p.journal.flush()
        db = p.journal._db
        return {
            "accepted": p.accepted, "rejected": p.rejected, "reject_reasons": dict(p.reject_reasons),
            "blocks_found": p.blocks_found,
            "workers": [(w.name, w.accepted, w.rejected) for w in (self.rig, self.ramp)],
            "shares": db.execute("SELECT worker, algo, job_id, difficulty, accepted, reason, hash, block FROM shares "
                                 "ORDER BY id").fetchall(),
            "blocks": db.execute("SELECT height, hash, worker, reward, scheme FROM blocks ORDER BY id").fetchall(),
        }


def script_template():
    blk = TemplateSource(ADDR, nbits=EASY_NBITS, n_txs=7, seed=b"validate-many").next_block()
    blk.ntime = int(time.time()) - 60
    return blk


def build_script(sp: ScriptedPool) -> tuple[list, list]:
    """``(earlier, batch)``: ``earlier`` is validated one by one before the batch; ``batch`` is the scripted list of
    ``(worker name, job_id, extranonce, ntime, nonce, version)``. Nonces are picked by hashing with the oracle, so
    every outcome is there by construction. The labels in the comments are what sequential validate() answers."""
    p, job = sp.pool, sp.job
    assert p.algo.name == "sha256d"
    en = bytes.fromhex("0102030405060708")
    t_share = hash_to_int(p.share_target(D0))
    t_raised = hash_to_int(p.share_target(D_RAISED))
    t_net = hash_to_int(target_from_nbits(job.block.nbits))
    assert t_net < t_raised < t_share
    rolled = job.version ^ 0x00002000
    kinds: dict[str, list] = {"block": [], "raised": [], "grace": [], "low": []}
    want = {"block": 1, "raised": 5, "grace": 1, "low": 1}
    prefix = p.header_for(job, en, job.version, job.ntime, 0)[:76]
    for nonce in range(1 << 16):
        hv = hash_to_int(sha256d(prefix + struct.pack("<I", nonce)))
        kind = "block" if hv <= t_net else "raised" if hv <= t_raised else "grace" if hv <= t_share else "low"
        if len(kinds[kind]) < want[kind]:
            kinds[kind].append(nonce)
        if all(len(kinds[k]) == want[k] for k in want):
            break
    else:
        raise AssertionError(f"nonce scan incomplete: {kinds}")
    a0, a1, a2, a3, a4 = kinds["raised"]  # above the network target, under every share target in play
    jid, nt, ver = job.job_id, job.ntime, job.version
    earlier = [("rig", jid, en, nt, a0, ver)]
    batch = [
        ("rig", jid, en, nt, a1, ver),                 # accepted
        ("rig", jid, en, nt, kinds["low"][0], ver),    # low-difficulty-share
        ("rig", jid, en, nt, a2, ver),                 # accepted
        ("rig", jid, en, nt, a1, ver),                 # duplicate-share (inside the batch)
        ("rig", jid, en, nt, a0, ver),                 # duplicate-share (accepted earlier)
        ("rig", "ffff", en, nt, a3, ver),              # stale-job
        ("rig", jid, en, nt, a3, ver ^ 0x1),           # invalid-version-bits
        ("rig", jid, en, nt - 1, a3, ver),             # invalid-ntime
        ("ramp", jid, en, nt, kinds["grace"][0], ver),  # accepted at D0: the grace after ramp's retarget
        ("ramp", jid, en, nt, a3, ver),                # accepted at D_RAISED
        ("rig", jid, en, nt, kinds["block"][0], ver),  # accepted, block found
        ("rig", jid, en, nt, a4, ver),                 # accepted: the new block only starts after the batch
        ("ramp", jid, en, nt, a2, ver),                # duplicate-share (another worker, inside the batch)
        ("rig", jid, bytes(8), nt + 5, 7, rolled),     # rolled BIP320 bits, another extranonce: whatever it hashes to
    ]
    return earlier, batch


def run_sequential(sp: ScriptedPool, items: list) -> list:
    workers = {"rig": sp.rig, "ramp": sp.ramp}
    return [sp.pool.validate(workers[w], *rest) for w, *rest in items]


def run_batched(sp: ScriptedPool, items: list, device=None) -> list:
    workers = {"rig": sp.rig, "ramp": sp.ramp}
    return sp.pool.validate_many([(workers[w], *rest) for w, *rest in items], device=device)
