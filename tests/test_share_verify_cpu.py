"""Share verification without a GPU: the job block format against the Python oracle (share_job_prepare +
share_headers_cpu, the plain C++ walker of the block the kernels read), the block's limits, the record packer, and
PoolServer.validate_many on the CPU path against sequential validate."""
import pytest

import share_verify_cases as C
from otedama_amd.ops.native import require_native
from otedama_amd.ops.share_records import RECORD_BYTES, pack_records, unpack_records
from otedama_amd.pool.batch import ShareJob, check_shares

N = require_native()


def _block(job: ShareJob) -> bytes:
    return N.share_job_prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, job.branches)


def _walk(job: ShareJob, shares) -> list:
    raw = N.share_headers_cpu(_block(job), pack_records(shares, [0] * len(shares), job.en_size))
    return [raw[i:i + 80] for i in range(0, len(raw), 80)]


def test_block_format_equals_the_oracle_over_the_whole_grid():
    covered = set()
    jobs = 0
    for job in C.full_grid():
        shares = C.make_shares(job, 3)
        assert _walk(job, shares) == C.oracle_headers(job, shares), (len(job.coinb1), job.en_size, len(job.coinb2),
                                                                    len(job.branches))
        covered |= C.edge_flags(job)
        jobs += 1
    assert jobs == (len(C.COINB1_LENGTHS) + len(C.EXTRA_COINB1_LENGTHS)) * 5 * 4 * 4
    assert covered >= C.ALL_EDGES, C.ALL_EDGES - covered


def test_reduced_grid_and_pool_job_equal_the_oracle():
    for job in C.reduced_grid() + [C.pool_job()]:
        shares = C.make_shares(job, 5)
        assert _walk(job, shares) == C.oracle_headers(job, shares)


def test_extranonce_bytes_past_en_size_are_ignored():
    job = C.make_job(55, 13, 56, 1)
    shares = C.make_shares(job, 2)
    rec = bytearray(pack_records(shares, [0, 0], job.en_size))
    rec[13:16] = b"\xff\xff\xff"
    rec[32 + 15] = 0xAA
    raw = N.share_headers_cpu(_block(job), bytes(rec))
    assert [raw[:80], raw[80:]] == C.oracle_headers(job, shares)


def test_a_tail_of_32_blocks_is_the_last_that_fits():
    ok = ShareJob(b"\x01", bytes(32 * 64 - 9 - 1 - 8), 8, bytes(32), C.EASY_NBITS, [])
    shares = C.make_shares(ok, 2)
    assert _walk(ok, shares) == C.oracle_headers(ok, shares)
    over = ShareJob(b"\x01", ok.coinb2 + b"\x00", 8, bytes(32), C.EASY_NBITS, [])
    with pytest.raises(ValueError):
        _block(over)
    whole = ShareJob(bytes(64 * 5), ok.coinb2 + b"\x00", 8, bytes(32), C.EASY_NBITS, [])  # whole blocks do not count
    assert _walk(whole, shares) == C.oracle_headers(whole, shares)


@pytest.mark.parametrize("change", [
    dict(branches=[bytes(32)] * 33), dict(en_size=0), dict(en_size=17), dict(branches=[bytes(32), bytes(31)]),
    dict(prev_hash=bytes(31)), dict(nbits=0x1D800000), dict(nbits=0x02000001), dict(nbits=0x1D000000),
    dict(nbits=0x22010000)])
def test_limits_raise_value_error(change):
    base = dict(coinb1=bytes(50), coinb2=bytes(60), en_size=8, prev_hash=bytes(32), nbits=C.EASY_NBITS,
                branches=[bytes(32)])
    _block(ShareJob(**base))
    with pytest.raises(ValueError):
        _block(ShareJob(**{**base, **change}))


def test_walker_rejects_what_prepare_cannot_have_built():
    job = C.make_job(41, 8, 0, 1)
    blk = bytearray(_block(job))
    rec = pack_records(C.make_shares(job, 1), [0], 8)
    with pytest.raises(ValueError):
        N.share_headers_cpu(bytes(blk[:-16]), rec)
    with pytest.raises(ValueError):
        N.share_headers_cpu(bytes(blk), rec[:-1])
    for offset, value in ((4, 17), (8, 33), (16, 33), (0, 0)):  # en_size, tail_blocks, n_branches, magic
        bad = bytearray(blk)
        bad[offset:offset + 4] = value.to_bytes(4, "little")
        with pytest.raises(ValueError):
            N.share_headers_cpu(bytes(bad), rec)
    assert N.share_headers_cpu(bytes(blk), b"") == b""


def test_pack_records_round_trips_and_rejects_a_wrong_extranonce():
    shares = [(bytes(range(1, 14)), 0xFFFFFFFF, 0, 0x20000000), (bytes(13), 1, 0xFFFFFFFF, 0x3FFFE000)]
    raw = pack_records(shares, [5, 0xFFFFFFFF], 13)
    assert len(raw) == 2 * RECORD_BYTES and raw[13:16] == bytes(3)
    assert raw[16:32] == bytes.fromhex("ffffffff" "00000000" "00000020" "05000000")
    assert unpack_records(raw, 13) == (shares, [5, 0xFFFFFFFF])
    assert pack_records([], [], 8) == b""
    with pytest.raises(ValueError):
        pack_records([(bytes(14), 0, 0, 0)], [0], 13)  # longer than en_size
    with pytest.raises(ValueError):
        pack_records([(bytes(12), 0, 0, 0)], [0], 13)  # a shorter one is another coinbase too
    with pytest.raises(ValueError):
        pack_records(shares, [0], 13)
    with pytest.raises(ValueError):
        pack_records(shares, [0, 1 << 32], 13)
    with pytest.raises(ValueError):
        pack_records([], [], 17)
    from otedama_amd.ops import verify  # the op re-exports the packer

    assert verify.pack_records is pack_records


def test_check_shares_oracle_verdict_bits():
    from otedama_amd.models.header import hash_to_int, int_to_hash, target_from_nbits

    job = C.pool_job()
    shares = C.make_shares(job, 40)
    probe = check_shares("sha256d", job, shares, [b"\xff" * 32], [0] * 40)
    hv = [hash_to_int(h) for _hdr, h, _v in probe]
    assert [hdr for hdr, _h, _v in probe] == C.oracle_headers(job, shares)
    targets = [int_to_hash(sorted(hv)[20]), int_to_hash(hv[0]), int_to_hash(hv[1] - 1), bytes(32)]
    idx = [1, 2] + [0] * 37 + [4]
    got = [v for _hdr, _h, v in check_shares("sha256d", job, shares, targets, idx)]
    net = hash_to_int(target_from_nbits(job.nbits))
    assert got[0] & 1 and not got[1] & 1 and got[39] == 0x80
    assert [v & 1 for v in got[2:39]] == [int(h <= sorted(hv)[20]) for h in hv[2:39]]
    assert [v >> 1 for v in got[:39]] == [int(h <= net) for h in hv[:39]]
    with pytest.raises(ValueError):
        check_shares("sha256d", job, shares, [], idx)
    with pytest.raises(ValueError):
        check_shares("sha256d", job, [(bytes(7), 0, 0, 0)], targets, [0])


def test_validate_many_equals_sequential_validate():
    tmpl = C.script_template()
    seq, bat = C.ScriptedPool(tmpl), C.ScriptedPool(tmpl)
    try:
        earlier, batch = C.build_script(seq)
        assert C.build_script(bat) == (earlier, batch)
        assert C.run_sequential(seq, earlier) == C.run_sequential(bat, earlier)
        want = C.run_sequential(seq, batch)
        got = C.run_batched(bat, batch, device=None)
        assert got == want
        # the script is what it claims to be
        assert [(v.accepted, v.reason) for v in want[:13]] == [
            (True, ""), (False, "low-difficulty-share"), (True, ""), (False, "duplicate-share"),
            (False, "duplicate-share"), (False, "stale-job"), (False, "invalid-version-bits"),
            (False, "invalid-ntime"), (True, ""), (True, ""), (True, ""), (True, ""), (False, "duplicate-share")]
        assert want[8].difficulty == C.D0 and want[9].difficulty == C.D_RAISED
        assert want[10].block and not want[11].block and want[1].hash and not want[3].hash
        s, b = seq.state(), bat.state()
        assert b == s
        assert s["blocks_found"] >= 1 and len(s["shares"]) == len(earlier) + len(batch) and len(s["blocks"]) >= 1
        assert bat.pool.validate_many([]) == []
    finally:
        seq.close()
        bat.close()
