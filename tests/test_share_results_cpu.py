"""The 128-byte result record of live share verification (csrc/include/otedama/share_job.h ``ShareResult``) without a
GPU: ``share_results_cpu`` against ``check_shares(device=None)`` on the reduced job grid, the torch-free unpacker,
and the config and flags of the pool's micro-batcher."""
import functools
import io

import pytest

import share_verify_cases as C

N_PER_JOB = 9


def _native():
    from otedama_amd.ops.native import require_native

    return require_native()


@functools.lru_cache(maxsize=None)
def grid_case(k: int):
    """(job, shares, targets, indices, oracle) of job ``k`` of the reduced grid. The table comes from the oracle's own
    hashes: for every share a tie, one under and one over; a pair differing from share 3's hash in the lowest word
    only and a pair differing from share 4's in the highest word only; then indices outside the table. Shared with
    the GPU tests and left unchanged."""
    from otedama_amd.models.header import hash_to_int, int_to_hash
    from otedama_amd.pool.batch import check_shares

    job = C.reduced_grid()[k]
    base = C.make_shares(job, N_PER_JOB, tag=f"res{k}")
    hv = [hash_to_int(h) for _hdr, h, _v in check_shares("sha256d", job, base, [b"\xff" * 32], [0] * N_PER_JOB)]
    w0 = lambda x, d: (x & ~0xFFFFFFFF) | ((x + d) & 0xFFFFFFFF)  # noqa: E731 - differs in the lowest word only
    w7 = lambda x, d: (x + (d << 224)) % (1 << 256)               # noqa: E731 - differs in the highest word only
    assert 0 < hv[3] & 0xFFFFFFFF < 0xFFFFFFFF and 0 < hv[4] >> 224 < 0xFFFFFFFF
    table, shares, indices = [], [], []
    for i, s in enumerate(base):
        for t in (hv[i], hv[i] - 1, hv[i] + 1):  # tie, one under, one over
            shares.append(s)
            indices.append(len(table))
            table.append(t % (1 << 256))
    for s, t in ((3, w0(hv[3], 1)), (3, w0(hv[3], -1)), (4, w7(hv[4], 1)), (4, w7(hv[4], -1))):
        shares.append(base[s])
        indices.append(len(table))
        table.append(t)
    for s, idx in ((5, len(table)), (6, 0xFFFFFFFF), (7, 1 << 31)):  # just past the table and far past it
        shares.append(base[s])
        indices.append(idx)
    targets = [int_to_hash(t) for t in table]
    return job, shares, targets, indices, check_shares("sha256d", job, shares, targets, indices)


def check_case_is_what_it_claims(want):
    v = [x[2] for x in want]
    for i in range(N_PER_JOB):
        assert [x & 1 for x in v[3 * i:3 * i + 3]] == [1, 0, 1], i  # a tie accepts, one under rejects, one over accepts
    p = 3 * N_PER_JOB
    assert [x & 1 for x in v[p:p + 4]] == [1, 0, 1, 0]  # lowest-word and highest-word pairs
    assert v[p + 4:p + 7] == [0x80, 0x80, 0x80]         # the guard: index t, 2^32 - 1 and 2^31


@pytest.mark.parametrize("k", range(len(C.reduced_grid())))
def test_share_results_cpu_equals_the_oracle(k):
    from otedama_amd.ops.share_records import RESULT_BYTES, pack_records, unpack_results

    n = _native()
    assert n.SHARE_RESULT_BYTES == RESULT_BYTES == 128
    job, shares, targets, indices, want = grid_case(k)
    block = n.share_job_prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, job.branches)
    raw = n.share_results_cpu(block, pack_records(shares, indices, job.en_size), b"".join(targets))
    assert len(raw) == 128 * len(shares)
    for i, (hdr, h, verdict) in enumerate(want):
        rec = raw[128 * i:128 * i + 128]
        assert rec[:80] == hdr, (k, i)
        assert rec[80:112] == h, (k, i)
        assert rec[112] == verdict, (k, i)
        assert rec[113:] == bytes(15), (k, i)
    assert unpack_results(raw) == want
    check_case_is_what_it_claims(want)


def test_share_results_cpu_rejects_bad_arguments():
    n = _native()
    job = C.make_job(41, 4, 55, 1)
    block = n.share_job_prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, job.branches)
    assert n.share_results_cpu(block, b"", b"\xff" * 32) == b""
    for args in ((block, bytes(31), b"\xff" * 32), (block, bytes(32), b""), (block, bytes(32), bytes(33)),
                 (block[:-1], bytes(32), bytes(32)), (bytes(len(block)), bytes(32), bytes(32))):
        with pytest.raises(ValueError):
            n.share_results_cpu(*args)


def test_unpack_results():
    from otedama_amd.ops.share_records import unpack_results

    rec = bytes(range(80)) + bytes(range(100, 132)) + b"\x03" + bytes(15)
    assert unpack_results(rec * 3) == [(bytes(range(80)), bytes(range(100, 132)), 3)] * 3
    assert unpack_results(bytearray(rec * 3), 2) == [(bytes(range(80)), bytes(range(100, 132)), 3)] * 2
    assert unpack_results(b"") == []
    for raw, n in ((rec[:-1], None), (rec, 2), (rec, -1)):
        with pytest.raises(ValueError):
            unpack_results(raw, n)


# ---------------------------------------------------------------- config and flags
def test_config_round_trip_and_validation(tmp_path):
    from otedama_amd import config as cfgmod

    ps = cfgmod.PoolServerConfig()
    assert (ps.verify_device, ps.verify_batch_ms, ps.verify_batch_max, ps.verify_min_gpu) == ("", 2.0, 4096, 0)
    path = tmp_path / "config.yaml"
    path.write_text("bitcoin_address: " + C.ADDR + "\npool_server:\n  verify_device: cuda:1\n  verify_batch_ms: 0.5\n"
                    "  verify_batch_max: 128\n  verify_min_gpu: 32\n")
    load = lambda: cfgmod.load_config_file(str(path))[0]  # noqa: E731
    cfg = load()
    ps = cfg.pool_server
    assert (ps.verify_device, ps.verify_batch_ms, ps.verify_batch_max, ps.verify_min_gpu) == ("cuda:1", 0.5, 128, 32)
    cfg.validate()
    assert cfg.to_dict()["pool_server"]["verify_device"] == "cuda:1"
    for field, bad in (("verify_device", "gpu"), ("verify_device", "cuda"), ("verify_device", "cuda:x"),
                       ("verify_batch_ms", 0.0), ("verify_batch_ms", -1.0), ("verify_batch_max", 0),
                       ("verify_min_gpu", -1)):
        c = load()
        setattr(c.pool_server, field, bad)
        with pytest.raises(cfgmod.ConfigError, match=field):
            c.validate()
    for good in ("", "cpu", "cuda:0", "cuda:15"):
        c = load()
        c.pool_server.verify_device = good
        c.validate()


def _pool_flags(args, tmp_path, file_text=None):
    """The options `otedama pool` would serve with: its flag set after parsing and the config file."""
    from otedama_amd.cli import pool_cmd

    if file_text is not None:
        path = tmp_path / "config.yaml"
        path.write_text(file_text)
        args = ["--config", str(path)] + args
    err = io.StringIO()
    fs = pool_cmd.pool_flags(err)
    fs.parse(args)
    pool_cmd.apply_config_file(fs, err)
    return fs, pool_cmd.verify_options(fs)


def test_pool_flags_precedence_and_validation(tmp_path):
    from otedama_amd.cli import pool_cmd
    from otedama_amd.cli.main import EXIT_CONFIG

    file_text = ("bitcoin_address: " + C.ADDR + "\npool_server:\n  verify_device: cuda:1\n  verify_batch_ms: 0.5\n"
                 "  verify_batch_max: 128\n  verify_min_gpu: 32\n")
    empty = "bitcoin_address: " + C.ADDR + "\n"
    _fs, opts = _pool_flags([], tmp_path, empty)
    assert opts == {"verify_device": "", "verify_batch_ms": 2.0, "verify_batch_max": 4096, "verify_min_gpu": 0}
    _fs, opts = _pool_flags([], tmp_path, file_text)  # the file fills what no flag gave
    assert opts == {"verify_device": "cuda:1", "verify_batch_ms": 0.5, "verify_batch_max": 128, "verify_min_gpu": 32}
    _fs, opts = _pool_flags(["--verify-device", "cpu", "--verify-batch-max", "7"], tmp_path, file_text)  # a flag wins
    assert opts == {"verify_device": "cpu", "verify_batch_ms": 0.5, "verify_batch_max": 7, "verify_min_gpu": 32}
    for bad in (["--verify-device", "gpu0"], ["--verify-batch-ms", "0"], ["--verify-batch-max", "0"],
                ["--verify-min-gpu", "-2"]):
        out, err = io.StringIO(), io.StringIO()
        path = tmp_path / "empty.yaml"
        path.write_text(empty)
        assert pool_cmd.cmd_pool(["--config", str(path)] + bad, out, err) == EXIT_CONFIG, bad
        assert "verify" in err.getvalue()
