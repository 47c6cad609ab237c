"""Real block templates without a GPU: ``BlockTemplate.from_gbt``, the witness commitment, ``serialize_block``, the
file-based template source, the pool's template-tree path (``PoolOptions.template_device``) with a block-finding
share, a failing device path, and the options' validation.

The witness-commitment path is parity unpinned (no segwit block is available offline): these tests pin it to the
BIP141 construction written out here, and the txid tree to block 100000 (test_merkle_tree_cpu.py)."""
import asyncio
import io
import json
import struct

import pytest

import channel_roots_cases as R
import merkle_tree_cases as T
import share_verify_cases as C
from otedama_amd import btccrypto
from otedama_amd.models.header import hash_to_int, sha256d, target_from_nbits
from otedama_amd.pool import microbatch
from otedama_amd.pool.server import BIP320_MASK, PoolOptions, PoolServer
from otedama_amd.pool.template import (BlockTemplate, GbtFileSource, TemplateSource, merkle_branches,
                                       merkle_root_full, serialize_block)

PAYOUT = btccrypto.address_script_pubkey(C.ADDR)
MSG = b"/gbt-test/"


@pytest.fixture(autouse=True)
def _devices_back():
    yield
    microbatch.forget_device_errors()  # the switch is the process's: a test that tripped it hands the device back


def _commitment(wtxids: list) -> bytes:
    """BIP141: OP_RETURN, push 36, the header aa21a9ed, sha256d(witness root | witness reserved value)."""
    return bytes.fromhex("6a24aa21a9ed") + sha256d(merkle_root_full([bytes(32)] + wtxids) + bytes(32))


def gbt_result(n_txs: int = 3, bits: str = "2000ffff", commitment: bool = True) -> dict:
    """A hand-built ``getblocktemplate`` result: hashes in display order, as bitcoind prints them."""
    txids, wtxids = list(T.leaves(n_txs + 1, 2)[1:]), list(T.leaves(n_txs + 1, 3)[1:])
    res = {
        "version": 0x20000000, "height": 840_000, "curtime": 1_700_000_000, "coinbasevalue": 312_500_000 + 12_345,
        "previousblockhash": bytes(range(32))[::-1].hex(), "bits": bits, "rules": ["csv", "!segwit", "taproot"],
        "transactions": [{"txid": t[::-1].hex(), "hash": w[::-1].hex(), "data": (b"\x02\x00\x00\x00" + t + w).hex(),
                          "fee": 100 + i} for i, (t, w) in enumerate(zip(txids, wtxids))],
    }
    if commitment:
        res["default_witness_commitment"] = _commitment(wtxids).hex()
    return res


def _varint(raw: bytes, at: int) -> tuple:
    v = raw[at]
    if v < 0xFD:
        return v, at + 1
    width = {0xFD: 2, 0xFE: 4, 0xFF: 8}[v]
    return int.from_bytes(raw[at + 1:at + 1 + width], "little"), at + 1 + width


def parse_tx(raw: bytes, at: int) -> tuple:
    """A transaction at ``raw[at:]``: ``(end, non-witness serialisation, witness stacks or None)``."""
    start = at
    version = raw[at:at + 4]
    at += 4
    segwit = raw[at:at + 2] == b"\x00\x01"
    if segwit:
        at += 2
    body = at
    n_in, at = _varint(raw, at)
    for _ in range(n_in):
        at += 36
        slen, at = _varint(raw, at)
        at += slen + 4
    n_out, at = _varint(raw, at)
    for _ in range(n_out):
        at += 8
        slen, at = _varint(raw, at)
        at += slen
    body_end = at
    stacks = None
    if segwit:
        stacks = []
        for _ in range(n_in):
            items, at = _varint(raw, at)
            stack = []
            for _ in range(items):
                ilen, at = _varint(raw, at)
                stack.append(raw[at:at + ilen])
                at += ilen
            stacks.append(stack)
    locktime = raw[at:at + 4]
    at += 4
    assert at - start >= 10
    return at, version + raw[body:body_end] + locktime, stacks


# ---------------------------------------------------------------- from_gbt and the coinbase
def test_from_gbt_round_trips_a_hand_built_result():
    res = gbt_result()
    t = BlockTemplate.from_gbt(res, PAYOUT, MSG)
    assert (t.version, t.height, t.ntime, t.coinbase_value) == (0x20000000, 840_000, 1_700_000_000, 312_512_345)
    assert t.nbits == 0x2000FFFF and t.payout_script == PAYOUT and t.coinbase_message == MSG
    # display hex is reversed: the previous block hash into header order, the hashes into internal order
    assert t.prev_hash == bytes(range(32))
    assert t.txids == list(T.leaves(4, 2)[1:]) and t.wtxids == list(T.leaves(4, 3)[1:])
    assert t.tx_data == [b"\x02\x00\x00\x00" + a + b for a, b in zip(t.txids, t.wtxids)]
    assert t.branches() == merkle_branches(t.txids)
    assert BlockTemplate.from_gbt(gbt_result(commitment=False), PAYOUT, MSG).wtxids == t.wtxids
    empty = BlockTemplate.from_gbt(gbt_result(n_txs=0, commitment=False), PAYOUT, MSG)
    assert empty.txids == [] and empty.wtxids == [] and empty.witness_root() is None
    for broken in ({"height": 1}, dict(res, bits=7), dict(res, previousblockhash="00" * 31),
                   dict(res, transactions=[{"txid": "00" * 32}])):
        with pytest.raises(ValueError):
            BlockTemplate.from_gbt(broken, PAYOUT, MSG)


def test_a_wrong_default_witness_commitment_raises():
    res = gbt_result()
    good = res["default_witness_commitment"]
    for bad in (good[:-2] + ("00" if good[-2:] != "00" else "01"), good[2:], "6a24aa21a9ed" + "00" * 32):
        with pytest.raises(ValueError, match="default_witness_commitment"):
            BlockTemplate.from_gbt(dict(res, default_witness_commitment=bad), PAYOUT, MSG)
    # a template without transactions has no wtxids and builds no commitment: a node that sends one disagrees
    with pytest.raises(ValueError, match="default_witness_commitment"):
        BlockTemplate.from_gbt(dict(gbt_result(n_txs=0, commitment=False), default_witness_commitment=good), PAYOUT,
                               MSG)


def test_the_coinbase_without_wtxids_is_todays():
    """Byte for byte what ``coinbase_parts`` built before wtxids existed, written out here."""
    blk = TemplateSource(C.ADDR, nbits=C.EASY_NBITS, n_txs=7, seed=b"gbt").next_block()
    assert blk.wtxids == [] and blk.tx_data == []
    coinb1, coinb2 = blk.coinbase_parts(8)
    height = struct.pack("<I", blk.height)[:3]
    assert blk.height < 1 << 23
    script_prefix = b"\x03" + height + bytes([len(blk.coinbase_message)]) + blk.coinbase_message
    assert coinb1 == (struct.pack("<I", 1) + b"\x01" + bytes(32) + b"\xff\xff\xff\xff"
                      + bytes([len(script_prefix) + 8]) + script_prefix)
    assert coinb2 == (b"\xff\xff\xff\xff" + b"\x01" + struct.pack("<Q", blk.coinbase_value)
                      + bytes([len(blk.payout_script)]) + blk.payout_script + bytes(4))
    assert blk.branches() == merkle_branches(blk.txids)
    # a tree handed in for such a template changes nothing either
    blk.set_tree(merkle_branches(blk.txids), None)
    assert blk.coinbase_parts(8) == (coinb1, coinb2) and blk.branches() == merkle_branches(blk.txids)
    with pytest.raises(ValueError):
        blk.set_tree([], bytes(32))  # a witness root without wtxids


def test_the_coinbase_with_wtxids_carries_the_commitment():
    t = BlockTemplate.from_gbt(gbt_result(), PAYOUT, MSG)
    plain = BlockTemplate.from_gbt(gbt_result(), PAYOUT, MSG)
    plain.wtxids = []
    coinb1, coinb2 = t.coinbase_parts(8)
    p1, p2 = plain.coinbase_parts(8)
    script = _commitment(t.wtxids)
    assert len(script) == 38 and t.witness_commitment_script() == script
    assert coinb1 == p1
    payout_out = struct.pack("<Q", t.coinbase_value) + bytes([len(PAYOUT)]) + PAYOUT
    assert p2 == b"\xff\xff\xff\xff" + b"\x01" + payout_out + bytes(4)
    assert coinb2 == b"\xff\xff\xff\xff" + b"\x02" + payout_out + struct.pack("<Q", 0) + b"\x26" + script + bytes(4)
    # a tree computed elsewhere is used as handed in: the commitment follows the witness root it is given
    other_root = bytes([7]) * 32
    t.set_tree([b"\x01" * 32], other_root)
    assert t.branches() == [b"\x01" * 32]
    assert t.coinbase_parts(8)[1].endswith(bytes.fromhex("6a24aa21a9ed") + sha256d(other_root + bytes(32)) + bytes(4))
    with pytest.raises(ValueError):
        t.set_tree([], None)  # wtxids without a witness root


def test_serialize_block_parses_back():
    t = BlockTemplate.from_gbt(gbt_result(), PAYOUT, MSG)
    coinb1, coinb2 = t.coinbase_parts(8)
    coinbase = coinb1 + bytes(range(8)) + coinb2
    header = bytes(range(80))
    raw = serialize_block(header, coinbase, t)
    assert raw[:80] == header
    count, at = _varint(raw, 80)
    assert count == 4
    end, stripped, stacks = parse_tx(raw, at)
    assert raw[at + 4:at + 6] == b"\x00\x01"  # marker and flag: the witness form
    assert stacks == [[bytes(32)]]            # one input, one item: the witness reserved value
    assert stripped == coinbase and sha256d(stripped) == sha256d(coinbase)  # the txid the header's root commits to
    assert raw[end:] == b"".join(t.tx_data)
    # without wtxids the coinbase goes as it is
    t.wtxids, t.tx_data = [], []
    c1, c2 = t.coinbase_parts(8)
    raw = serialize_block(header, c1 + bytes(8) + c2, t)
    assert raw == header + b"\x01" + c1 + bytes(8) + c2
    assert parse_tx(raw, 81) == (len(raw), c1 + bytes(8) + c2, None)
    with pytest.raises(ValueError):
        serialize_block(header[:79], coinbase, t)


# ---------------------------------------------------------------- the pool over a template file
def _file_pool(tmp_path, result: dict, **kw) -> tuple:
    path = tmp_path / "gbt.json"
    path.write_text(json.dumps(result))
    src = GbtFileSource(str(path), PAYOUT, MSG)
    pool = PoolServer(PoolOptions(payout_address=C.ADDR, job_interval=3600, block_interval=3600,
                                  initial_difficulty=1e-9, min_difficulty=1e-12, fixed_difficulty=True, **kw),
                      template_source=src)
    pool._en_counter = 0x01020000
    return pool, path


def test_a_pool_over_a_template_file_serves_the_oracles_branches_and_writes_a_found_block(tmp_path):
    res = gbt_result(n_txs=5)
    res["curtime"] = 1_000_000_000  # any ntime from here to two hours ahead of the wall clock is valid

    async def body():
        pool, path = _file_pool(tmp_path, res, template_device="cpu")
        await pool.start()
        try:
            job = next(iter(pool.jobs.values()))
            c = await R.V2Client.connect(pool)
            _ok, first = await c.open(extended=True)
            sent = [m for m in first if hasattr(m, "merkle_path")]
            c.close()
            # a block-finding share: one hash in 256 is under the easy target
            worker = pool.new_worker("rig", BIP320_MASK)
            en = bytes.fromhex("0102030405060708")
            t_net = hash_to_int(target_from_nbits(job.block.nbits))
            prefix = pool.header_for(job, en, job.version, job.ntime, 0)[:76]
            nonce = next(k for k in range(1 << 16) if hash_to_int(sha256d(prefix + struct.pack("<I", k))) <= t_net)
            v = pool.validate(worker, job.job_id, en, job.ntime, nonce, job.version)
            return pool, job, sent, v, en, nonce, pool.stats()["template"], path
        finally:
            await pool.stop()

    pool, job, sent, v, en, nonce, st, path = asyncio.run(asyncio.wait_for(body(), 60))
    t = job.block
    want = merkle_branches(t.txids)
    assert len(t.txids) == 5 and job.branches == want
    assert sent and all(list(m.merkle_path) == want for m in sent)
    assert job.coinb2.endswith(_commitment(t.wtxids) + bytes(4))
    assert (st["device"], st["enabled"], st["device_errors"], st["gpu_leaves"]) == ("cpu", True, 0, 0)
    assert st["trees"] >= 1 and st["last_leaves"] == 12 and st["cpu_leaves"] == 12 * st["trees"]
    # the block file
    assert v.accepted and v.block
    out = tmp_path / f"gbt.json.block-{t.height}.hex"
    raw = bytes.fromhex(out.read_text().strip())
    header = raw[:80]
    assert header == pool.header_for(job, en, job.version, job.ntime, nonce)
    assert hash_to_int(sha256d(header)) <= hash_to_int(target_from_nbits(t.nbits))
    count, at = _varint(raw, 80)
    end, stripped, stacks = parse_tx(raw, at)
    assert count == 6 and stacks == [[bytes(32)]] and raw[end:] == b"".join(t.tx_data)
    assert stripped == job.coinb1 + en + job.coinb2
    # the header's merkle root is the root of the whole block's txids
    assert header[36:68] == merkle_root_full([sha256d(stripped)] + t.txids)


def test_the_options_off_leave_the_pool_as_it_was(tmp_path):
    """No template options: nothing is built, the synthetic source serves, no block is submitted anywhere."""
    async def body():
        pool = R.seeded_pool()
        assert isinstance(pool.templates, TemplateSource)
        job = pool.new_block()
        try:
            return pool._template_tree, job.block._tree, job.branches == merkle_branches(job.block.txids), pool.stats()
        finally:
            pool.journal.close()
            pool._hash_pool.shutdown(wait=False)

    tree, handed, same, stats = asyncio.run(body())
    assert tree is None and handed is None and same
    assert stats["template"] == {"device": "", "enabled": False, "trees": 0, "gpu_leaves": 0, "cpu_leaves": 0,
                                 "last_leaves": 0, "last_ms": 0.0, "device_errors": 0}


def test_an_injected_device_error_falls_back_counts_and_turns_the_path_off(tmp_path):
    calls = []

    def failing(txids, wtxids):
        calls.append((len(txids), len(wtxids)))
        raise RuntimeError("injected device failure")

    async def body():
        pool, _path = _file_pool(tmp_path, gbt_result(n_txs=5), template_device="cuda:0", template_min_gpu=1)
        pool.template_tree_fn = failing
        logged = []
        pool.log = lambda level, msg: logged.append((level, msg))
        try:
            first = pool.new_block()
            second = pool.new_block()
            return first, second, pool.stats()["template"], logged
        finally:
            pool._template_tree.close()
            pool.journal.close()
            pool._hash_pool.shutdown(wait=False)

    assert not microbatch.device_failed("cuda:0")
    first, second, st, logged = asyncio.run(body())
    for job in (first, second):  # still the oracle's tree, from the native CPU path
        assert job.branches == merkle_branches(job.block.txids)
        assert job.coinb2.endswith(_commitment(job.block.wtxids) + bytes(4))
    assert calls == [(5, 5)]  # the device path was tried once; after its failure no template goes there
    assert (st["device"], st["enabled"], st["device_errors"]) == ("cuda:0", False, 1)
    assert (st["trees"], st["gpu_leaves"], st["cpu_leaves"], st["last_leaves"]) == (2, 0, 24, 12)
    assert microbatch.device_failed("cuda:0")
    assert sum(level == "error" and "template tree" in msg for level, msg in logged) == 1


def test_the_device_path_is_used_from_template_min_gpu_leaves_on(tmp_path):
    from otedama_amd.pool.batch import template_tree

    seen = []

    def device(txids, wtxids):
        seen.append(len(txids))
        return template_tree(txids, wtxids)

    async def body(min_gpu):
        pool, _path = _file_pool(tmp_path, gbt_result(n_txs=5), template_device="cuda:0", template_min_gpu=min_gpu)
        pool.template_tree_fn = device
        try:
            job = pool.new_block()
            return job.branches == merkle_branches(job.block.txids), pool.stats()["template"]
        finally:
            pool._template_tree.close()
            pool.journal.close()
            pool._hash_pool.shutdown(wait=False)

    ok, st = asyncio.run(body(6))  # six leaves per tree: the coinbase slot counts
    assert ok and seen == [5] and (st["gpu_leaves"], st["cpu_leaves"], st["enabled"]) == (12, 0, True)
    ok, st = asyncio.run(body(7))
    assert ok and seen == [5] and (st["gpu_leaves"], st["cpu_leaves"]) == (0, 12)


def test_template_tree_refuses_bad_options():
    from otedama_amd.pool.templatetree import DEFAULT_TEMPLATE_MIN_GPU, TemplateTree

    for kw in ({"template_device": ""}, {"template_device": "gpu"},
               {"template_device": "cpu", "template_min_gpu": -1}):
        pool = R.seeded_pool(**kw)
        with pytest.raises(ValueError):
            TemplateTree(pool)
        pool.journal.close()
        pool._hash_pool.shutdown(wait=False)
    pool = R.seeded_pool(template_device="cpu")
    tt = TemplateTree(pool)
    assert tt.min_gpu == DEFAULT_TEMPLATE_MIN_GPU >= 1
    tt.close()
    pool.journal.close()
    pool._hash_pool.shutdown(wait=False)


def test_gbt_file_source_reads_the_file_again_for_every_block(tmp_path):
    path = tmp_path / "t.json"
    path.write_text(json.dumps({"result": gbt_result(n_txs=2), "error": None, "id": 1}))  # a whole RPC reply
    src = GbtFileSource(str(path), PAYOUT, "/msg/")
    a = src.next_block()
    assert len(a.txids) == 2 and a.coinbase_message == b"/msg/"
    path.write_text(json.dumps(dict(gbt_result(n_txs=4), height=840_001)))
    b = src.next_block()
    assert (len(b.txids), b.height) == (4, 840_001)
    assert src.submit_block(b"\x01\x02", b) == f"{path}.block-840001.hex"
    assert (tmp_path / "t.json.block-840001.hex").read_text() == "0102\n"
    path.write_text("[1, 2]")
    with pytest.raises(ValueError):
        src.next_block()


# ---------------------------------------------------------------- config and flags
def test_config_round_trip_and_validation(tmp_path):
    from otedama_amd import config as cfgmod

    ps = cfgmod.PoolServerConfig()
    assert (ps.template_file, ps.template_device, ps.template_min_gpu) == ("", "", 0)
    assert (PoolOptions().template_device, PoolOptions().template_min_gpu) == ("", 0)
    path = tmp_path / "config.yaml"
    path.write_text("bitcoin_address: " + C.ADDR + "\npool_server:\n  template_file: /tmp/gbt.json\n"
                    "  template_device: cuda:1\n  template_min_gpu: 2048\n")
    load = lambda: cfgmod.load_config_file(str(path))[0]  # noqa: E731
    cfg = load()
    assert (cfg.pool_server.template_file, cfg.pool_server.template_device, cfg.pool_server.template_min_gpu) == (
        "/tmp/gbt.json", "cuda:1", 2048)
    cfg.validate()
    assert cfg.to_dict()["pool_server"]["template_device"] == "cuda:1"
    for field, bad in (("template_device", "gpu"), ("template_device", "cuda"), ("template_device", "cuda:x"),
                       ("template_min_gpu", -1)):
        c = load()
        setattr(c.pool_server, field, bad)
        with pytest.raises(cfgmod.ConfigError, match=field):
            c.validate()
    for good in ("", "cpu", "cuda:0", "cuda:15"):
        c = load()
        c.pool_server.template_device = good
        c.validate()


def test_pool_flags_precedence_and_validation(tmp_path):
    from otedama_amd.cli import pool_cmd
    from otedama_amd.cli.main import EXIT_CONFIG

    def flags(args, file_text):
        path = tmp_path / "config.yaml"
        path.write_text(file_text)
        err = io.StringIO()
        fs = pool_cmd.pool_flags(err)
        fs.parse(["--config", str(path)] + args)
        pool_cmd.apply_config_file(fs, err)
        return dict(pool_cmd.template_options(fs), template_file=fs["template-file"])

    empty = "bitcoin_address: " + C.ADDR + "\n"
    file_text = empty + "pool_server:\n  template_file: a.json\n  template_device: cuda:1\n  template_min_gpu: 2048\n"
    assert flags([], empty) == {"template_device": "", "template_min_gpu": 0, "template_file": ""}
    assert flags([], file_text) == {"template_device": "cuda:1", "template_min_gpu": 2048, "template_file": "a.json"}
    assert flags(["--template-device", "cpu", "--template-file", "b.json"], file_text) == {
        "template_device": "cpu", "template_min_gpu": 2048, "template_file": "b.json"}  # a flag wins
    assert pool_cmd.template_options_error({"template_device": "cuda:3", "template_min_gpu": 0}) is None
    for bad in (["--template-device", "gpu0"], ["--template-min-gpu", "-2"]):
        out, err = io.StringIO(), io.StringIO()
        path = tmp_path / "empty.yaml"
        path.write_text(empty)
        assert pool_cmd.cmd_pool(["--config", str(path)] + bad, out, err) == EXIT_CONFIG, bad
        assert "template" in err.getvalue()
    # the file source the flags make pays the payout address, or burns without one
    gbt = tmp_path / "gbt.json"
    gbt.write_text(json.dumps(gbt_result()))
    fs = pool_cmd.pool_flags(io.StringIO())
    fs.parse(["--template-file", str(gbt), "--payout-address", C.ADDR])
    src = pool_cmd.template_source(fs)
    assert isinstance(src, GbtFileSource) and src.next_block().payout_script == PAYOUT
    fs = pool_cmd.pool_flags(io.StringIO())
    fs.parse([])
    assert pool_cmd.template_source(fs) is None
