"""Batch share checking for the pool: shares of one job in, ``(header, hash, verdict byte)`` out.

``device=None`` is the oracle: today's Python functions, one share at a time (sha256d of the coinbase,
``merkle_root_from_branches``, the header packed as ``PoolServer.header_for`` packs it, the algorithm's CPU hash,
integer compares). With a device the whole batch is one ``ops.verify.ShareVerify.verify``: headers, hashes and
compares happen on the GPU. Both paths return the same list. Importing this module imports neither torch nor the
native extension.

:func:`channel_roots` is the same three-way choice for a job's fan-out to Stratum V2 standard channels: one job and
n extranonce prefixes in, n merkle roots out. :func:`seal_frames` is the same choice for that fan-out's Noise frames:
n plaintexts with n keys and counters in, n sealed frames out.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import Sequence

from otedama_amd.models import algorithms
from otedama_amd.models.header import hash_to_int, sha256d, target_from_nbits
from otedama_amd.ops.share_records import VERDICT_BAD_INDEX, VERDICT_NETWORK, VERDICT_SHARE
from otedama_amd.pool.template import merkle_root_from_branches


@dataclass(frozen=True)
class ShareJob:
    """What every share of one job has in common. ``en_size``: bytes of extranonce between the coinbase parts."""
    coinb1: bytes
    coinb2: bytes
    en_size: int
    prev_hash: bytes
    nbits: int
    branches: list = field(default_factory=list)


_ops: dict[tuple, object] = {}  # (kind, algorithm, device) -> the process's op of that kind on that device


def prepared_or_none(prepare, job: ShareJob):
    """``prepare`` (an op's, or the native ``share_job_prepare``) of ``job``'s block, or ``None`` for a job over the
    block's limits: that job is the CPU's."""
    try:
        return prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits & 0xFFFFFFFF, list(job.branches))
    except ValueError:
        return None


def _op(key: tuple, make_op):
    """The process's op for ``key``, made on first use."""
    op = _ops.get(key)
    if op is None:
        op = _ops[key] = make_op()
    return op


def _op_and_block(key: tuple, make_op, job: ShareJob):
    """The process's op for ``key`` and ``job``'s block prepared on its device, or ``None``."""
    op = _op(key, make_op)
    return op, prepared_or_none(op.prepare, job)


def root_of(job: ShareJob, extranonce: bytes) -> bytes:
    return merkle_root_from_branches(sha256d(job.coinb1 + extranonce + job.coinb2), job.branches)


def header_of(job: ShareJob, extranonce: bytes, ntime: int, nonce: int, version: int) -> bytes:
    root = root_of(job, extranonce)
    return (struct.pack("<I", version & 0xFFFFFFFF) + job.prev_hash + root
            + struct.pack("<III", ntime & 0xFFFFFFFF, job.nbits & 0xFFFFFFFF, nonce & 0xFFFFFFFF))


def check_shares(algorithm: str, job: ShareJob, shares: Sequence[tuple], targets: Sequence[bytes],
                 target_indices: Sequence[int], device=None) -> list[tuple[bytes, bytes, int]]:
    """``shares``: ``(extranonce, ntime, nonce, version)`` tuples against ``job``; share ``i`` is compared with
    ``targets[target_indices[i]]`` (32 bytes, little-endian) and with the network target of ``job.nbits``. Returns
    ``(header, hash, verdict)`` per share: verdict bit 0 = hash <= share target, bit 1 = hash <= network target,
    ``0x80`` alone for an index outside the table. A job over the GPU job block's limits is checked on the CPU."""
    algo = algorithms.get(algorithm)
    shares = [(bytes(en), int(ntime), int(nonce), int(version)) for en, ntime, nonce, version in shares]
    targets = [bytes(t) for t in targets]
    if not targets or any(len(t) != 32 for t in targets):
        raise ValueError("need at least one target, each 32 bytes")
    if len(target_indices) != len(shares):
        raise ValueError("one target index per share")
    if len(job.prev_hash) != 32:
        raise ValueError("prev_hash must be 32 bytes")
    for i, s in enumerate(shares):
        if len(s[0]) != job.en_size:
            raise ValueError(f"extranonce of share {i} is {len(s[0])} bytes, the job takes {job.en_size}")
    network = hash_to_int(target_from_nbits(job.nbits))
    if device is not None and shares:
        from otedama_amd.ops.verify import ShareVerify  # imports torch

        op, prepared = _op_and_block(("verify", algo.name, str(device)), lambda: ShareVerify(algo.name, device), job)
        if prepared is not None:  # else over the block's limits: the oracle path below
            verdicts, hashes, headers = op.verify(prepared, shares, targets, target_indices)
            return list(zip(headers, hashes, verdicts))
    out = []
    tints = [hash_to_int(t) for t in targets]
    for (en, ntime, nonce, version), idx in zip(shares, target_indices):
        hdr = header_of(job, en, ntime, nonce, version)
        h = algo.hash(hdr)
        if not 0 <= idx < len(tints):
            verdict = VERDICT_BAD_INDEX
        else:
            hv = hash_to_int(h)
            verdict = (VERDICT_SHARE if hv <= tints[idx] else 0) | (VERDICT_NETWORK if hv <= network else 0)
        out.append((hdr, h, verdict))
    return out


def channel_roots(job: ShareJob, prefixes: Sequence[bytes], device=None) -> list[bytes]:
    """The merkle root of ``job`` for every extranonce prefix (each ``job.en_size`` bytes), in order: the bytes
    ``PoolServer.merkle_root_for`` returns. ``device=None``: Python, one prefix at a time. ``"cpu"``: the native
    ``share_roots_cpu``. ``"cuda:N"``: one ``ops.roots.ChannelRoots.roots`` round trip on that GPU. A job over the
    job block's limits is computed in Python whatever the device."""
    prefixes = [bytes(p) for p in prefixes]
    for i, p in enumerate(prefixes):
        if len(p) != job.en_size:
            raise ValueError(f"prefix {i} is {len(p)} bytes, the job takes {job.en_size}")
    if device is not None and prefixes:
        if str(device) == "cpu":
            from otedama_amd.ops.native import require_native
            from otedama_amd.ops.share_records import pack_prefixes, unpack_roots

            native = require_native()
            block = prepared_or_none(native.share_job_prepare, job)
            if block is not None:  # else over the block's limits: the Python path below
                return unpack_roots(native.share_roots_cpu(block, pack_prefixes(prefixes, job.en_size)))
        else:
            from otedama_amd.ops.roots import ChannelRoots  # imports torch

            op, prepared = _op_and_block(("roots", "", str(device)), lambda: ChannelRoots(device), job)
            if prepared is not None:  # as above
                return op.roots(prepared, prefixes)
    return [root_of(job, p) for p in prefixes]


def seal_frames(frames: Sequence[tuple], device=None) -> list[bytes]:
    """The Noise transport's seal of every ``(key32, counter, plaintext)`` frame, in order: the bytes
    ``noise.CipherState.encrypt`` returns for that key and counter (ChaCha20-Poly1305, empty associated data, nonce
    four zero bytes and the counter little-endian). ``device=None``: ``utils.aead.seal``, one frame at a time.
    ``"cpu"``: the native ``aead_seal_many_cpu``, one call. ``"cuda:N"``: one ``ops.seal.FrameSeal.seal`` round trip
    on that GPU. A frame over ``SEAL_MAX_PLAIN`` bytes is sealed by ``utils.aead.seal`` whatever the device, in its
    place in the order."""
    from otedama_amd.ops.seal_rows import SEAL_MAX_PLAIN, pack_frames, unpack_sealed, wipe_keys
    from otedama_amd.utils import aead

    def one(key, counter, plain):
        if not 0 <= counter < (1 << 64) - 1:
            raise ValueError("a counter is in [0, 2^64 - 1)")
        return aead.seal(aead.CHACHA20POLY1305, key, b"\x00" * 4 + struct.pack("<Q", counter), plain)

    frames = list(frames)
    if device is None or not frames:
        return [one(*f) for f in frames]
    small = [i for i, f in enumerate(frames) if len(f[2]) <= SEAL_MAX_PLAIN]
    whole = len(small) == len(frames)  # the usual case: no copy of the list, no merge afterwards
    out: list = [None] * len(frames)
    if small:
        batch = frames if whole else [frames[i] for i in small]
        if str(device) == "cpu":
            from otedama_amd.ops.native import require_native

            packed, _out_bytes = pack_frames(batch)
            try:
                sealed = unpack_sealed(packed, require_native().aead_seal_many_cpu(packed, len(batch)), len(batch))
            finally:
                wipe_keys(packed, len(batch))
        else:
            from otedama_amd.ops.seal import FrameSeal  # imports torch

            sealed = _op(("seal", "", str(device)), lambda: FrameSeal(device)).seal(batch)
        if whole:
            return sealed
        for i, s in zip(small, sealed):
            out[i] = s
    for i, f in enumerate(frames):
        if out[i] is None:
            out[i] = one(*f)
    return out


def template_tree(txids: Sequence[bytes], wtxids: Sequence[bytes] = (), device=None):
    """The two trees of a block template: ``(branches, witness_root)``. ``branches`` is ``merkle_branches(txids)``,
    the coinbase's path through the txid tree; ``witness_root`` is ``merkle_root_full([bytes(32)] + wtxids)``, the
    root of the wtxid tree with the coinbase's wtxid zeroed (BIP141), or ``None`` without wtxids. Both trees get 32
    zero bytes as leaf 0: the path never depends on it. ``device=None``: those Python functions. ``"cpu"``: the
    native ``merkle_tree_cpu``. ``"cuda:N"``: one ``ops.merkle.MerkleTree.tree`` round trip on that GPU, both trees
    in it. A template over the op's limit of 262144 leaves is computed in Python whatever the device."""
    from otedama_amd.ops.merkle_rows import MAX_LEAVES, pack_leaves, unpack_rows
    from otedama_amd.pool.template import merkle_branches, merkle_root_full

    txids, wtxids = list(map(bytes, txids)), list(map(bytes, wtxids))
    if wtxids and len(wtxids) != len(txids):
        raise ValueError(f"{len(wtxids)} wtxids for {len(txids)} txids")
    for name, ids in (("txid", txids), ("wtxid", wtxids)):
        if ids and set(map(len, ids)) != {32}:
            raise ValueError(f"every {name} must be 32 bytes")
    if device is not None and 1 + len(txids) <= MAX_LEAVES:
        trees = [[bytes(32)] + txids] + ([[bytes(32)] + wtxids] if wtxids else [])
        if str(device) == "cpu":
            from otedama_amd.ops.native import require_native

            packed, t, n = pack_leaves(trees)
            out = unpack_rows(require_native().merkle_tree_cpu(packed, t, n), t, n)
        else:
            from otedama_amd.ops.merkle import MerkleTree  # imports torch

            out = _op(("tree", "", str(device)), lambda: MerkleTree(device)).tree(trees)
        return out[0][1], (out[1][0] if wtxids else None)
    return merkle_branches(txids), (merkle_root_full([bytes(32)] + wtxids) if wtxids else None)
