"""Channel roots without a GPU: ``share_roots_cpu`` and ``pool.batch.channel_roots`` against the oracle
``merkle_root_from_branches(sha256d(coinb1 + prefix + coinb2), branches)``, the over-limit fall-backs, and the pool's
job fan-out (``PoolOptions.job_device``) on loopback SV2 connections: the same messages as with the option off, a
failing device path, the options' validation, the ``jobs`` API object and the per-block branch cache."""
import asyncio
import io

import pytest

import channel_roots_cases as R
import share_verify_cases as C
from otedama_amd.ops.native import require_native
from otedama_amd.ops.share_records import PREFIX_BYTES, ROOT_BYTES, pack_prefixes, unpack_roots
from otedama_amd.pool import batch, microbatch
from otedama_amd.pool import server as server_mod
from otedama_amd.pool.batch import ShareJob, channel_roots
from otedama_amd.pool.template import BlockTemplate, merkle_branches
from otedama_amd.stratum import messages as M

N = require_native()


@pytest.fixture(autouse=True)
def _devices_back():
    yield
    microbatch.forget_device_errors()  # the switch is the process's: a test that tripped it hands the device back


def _dispose(pool) -> None:
    """For a pool that was never started."""
    pool.journal.close()
    pool._hash_pool.shutdown(wait=False)


def _block(job: ShareJob) -> bytes:
    return N.share_job_prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, job.branches)


# ---------------------------------------------------------------- native walker and channel_roots
def test_share_roots_cpu_equals_the_oracle_on_the_full_grid():
    jobs = 0
    for job in C.full_grid():
        prefixes = R.make_prefixes(job, 5)
        raw = N.share_roots_cpu(_block(job), pack_prefixes(prefixes, job.en_size))
        assert unpack_roots(raw) == [R.oracle_root(job, p) for p in prefixes], (len(job.coinb1), job.en_size)
        jobs += 1
    assert jobs == 13 * 5 * 4 * 4


def test_share_roots_cpu_ignores_the_bytes_after_the_prefix_and_checks_its_arguments():
    job = C.make_job(62, 4, 56, 12)  # straddles a block boundary
    prefixes = R.make_prefixes(job, 3)
    rows = bytearray(pack_prefixes(prefixes, job.en_size))
    for i in range(3):
        rows[PREFIX_BYTES * i + job.en_size:PREFIX_BYTES * (i + 1)] = b"\xa5" * (PREFIX_BYTES - job.en_size)
    blk = _block(job)
    assert unpack_roots(N.share_roots_cpu(blk, bytes(rows))) == [R.oracle_root(job, p) for p in prefixes]
    assert N.share_roots_cpu(blk, b"") == b""
    with pytest.raises(ValueError):
        N.share_roots_cpu(blk[:-16], bytes(rows))
    with pytest.raises(ValueError):
        N.share_roots_cpu(blk, bytes(rows[:-1]))
    bad = bytearray(blk)
    bad[0] ^= 1  # the magic
    with pytest.raises(ValueError):
        N.share_roots_cpu(bytes(bad), bytes(rows))


def test_prefix_rows_pack_and_unpack():
    assert pack_prefixes([b"\x01\x02", b"\x03\x04"], 2) == b"\x01\x02" + bytes(14) + b"\x03\x04" + bytes(14)
    assert pack_prefixes([], 8) == b""
    assert unpack_roots(bytes(range(64))) == [bytes(range(32)), bytes(range(32, 64))]
    for prefixes, en_size in (([b"\x01"], 2), ([b"\x01\x02\x03"], 2), ([b""], 0), ([bytes(17)], 17)):
        with pytest.raises(ValueError):
            pack_prefixes(prefixes, en_size)
    with pytest.raises(ValueError):
        unpack_roots(bytes(ROOT_BYTES + 1))


def test_channel_roots_python_and_native_agree_with_the_oracle():
    for job in C.reduced_grid() + [C.pool_job(n_txs=4000)]:
        prefixes = R.make_prefixes(job, 9)
        want = [R.oracle_root(job, p) for p in prefixes]
        assert channel_roots(job, prefixes) == want
        assert channel_roots(job, prefixes, "cpu") == want
    job = C.pool_job()
    assert channel_roots(job, [], "cpu") == [] and channel_roots(job, []) == []
    with pytest.raises(ValueError):
        channel_roots(job, [bytes(7)], "cpu")


@pytest.mark.parametrize("what", ["33 branches", "33 tail blocks", "en_size 0", "en_size 17"])
def test_a_job_over_the_limits_falls_back_to_python(what, monkeypatch):
    if what == "33 branches":
        job = C.make_job(41, 4, 55, 33)
    elif what == "33 tail blocks":
        job = C.make_job(41, 4, 55, 1, extra_blocks=32)  # 41 + 4 + 10 + 64 * 32 bytes, then the padding
    else:
        en_size = 0 if what == "en_size 0" else 17
        base = C.make_job(41, 4, 55, 1)
        job = ShareJob(base.coinb1, base.coinb2, en_size, base.prev_hash, base.nbits, base.branches)
    with pytest.raises(ValueError):
        _block(job)
    called = []
    monkeypatch.setattr(N, "share_roots_cpu", lambda *a: called.append(a))
    prefixes = [C.rnd(f"over.{i}", job.en_size) for i in range(3)]
    assert channel_roots(job, prefixes, "cpu") == [R.oracle_root(job, p) for p in prefixes]
    assert not called


# ---------------------------------------------------------------- the pool's job fan-out
def _pin_clock(monkeypatch, t: float = 1_750_000_000.0):
    """Two pools started one after the other must stamp the same ntime."""
    monkeypatch.setattr(server_mod.time, "time", lambda: t)


async def _fanout_session(pool, late_channel: bool = False):
    """Three connections with two standard channels and one extended channel each; then a job, (a late channel,)
    another job and a new block. Returns ``(clients, every message in order per client, job_int -> PoolJob)``."""
    await pool.start()
    clients, log = [], []
    jobs = {j.job_int: j for j in pool.jobs.values()}
    for _ in range(3):
        c = await R.V2Client.connect(pool)
        msgs = []
        for extended in (False, True, False):
            ok, first = await c.open(extended)
            msgs += [ok] + first
        clients.append(c)
        log.append(msgs)
    made = [pool.new_job(clean=False)]
    for c, msgs in zip(clients, log):
        msgs += await c.take(3)
    if late_channel:  # between two jobs: its first job comes from the channel-open path, the next from the fan-out
        ok, first = await clients[1].open(False)
        log[1] += [ok] + first
    made.append(pool.new_job(clean=False))
    for c, msgs in zip(clients, log):
        msgs += await c.take(len(c.channels))
    made.append(pool.new_block())
    for c, msgs in zip(clients, log):
        msgs += await c.take(2 * len(c.channels))
    jobs.update((j.job_int, j) for j in made)
    return clients, log, jobs


def _run_session(late_channel: bool = False, **kw):
    async def body():
        pool = R.seeded_pool(**kw)
        try:
            clients, log, jobs = await _fanout_session(pool, late_channel)
            checked = sum(R.check_standard_roots(jobs, c, msgs) for c, msgs in zip(clients, log))
            for c in clients:
                c.close()
            return pool, log, checked, pool.stats()["jobs"]
        finally:
            await pool.stop()

    return asyncio.run(asyncio.wait_for(body(), 30))


def test_pool_fanout_on_the_cpu_sends_what_the_pool_sends_without_it(monkeypatch):
    _pin_clock(monkeypatch)
    _off, log_off, checked_off, jobs_off = _run_session()
    _on, log_on, checked_on, jobs_on = _run_session(job_device="cpu")
    assert log_on == log_off  # every message: the standard channels' roots, the extended channels' jobs, the rest
    # per connection: 2 standard channels x (open + job + job + block)
    assert checked_on == checked_off == 3 * 2 * 4
    extended = [m for msgs in log_on for m in msgs if isinstance(m, M.NewExtendedMiningJob)]
    assert len(extended) == 3 * 4
    assert jobs_off == {"device": "", "enabled": False, "fanouts": 0, "gpu_channels": 0, "cpu_channels": 0,
                        "last_channels": 0, "last_ms": 0.0, "device_errors": 0}
    assert jobs_on.pop("last_ms") > 0.0
    assert jobs_on == {"device": "cpu", "enabled": True, "fanouts": 3, "gpu_channels": 0, "cpu_channels": 18,
                       "last_channels": 6, "device_errors": 0}


def test_a_channel_opened_between_two_jobs_gets_the_right_roots(monkeypatch):
    _pin_clock(monkeypatch)
    _off, log_off, checked_off, _ = _run_session(late_channel=True)
    _on, log_on, checked_on, jobs = _run_session(late_channel=True, job_device="cpu")
    assert log_on == log_off
    assert checked_on == checked_off == 3 * 2 * 4 + 3  # the late channel: open, job, block
    assert (jobs["fanouts"], jobs["cpu_channels"], jobs["last_channels"]) == (3, 6 + 7 + 7, 7)


def _run_with_device_fn(device_fn, **kw):
    async def body():
        pool = R.seeded_pool(job_device="cuda:0", **kw)
        pool.job_roots_fn = device_fn
        try:
            clients, log, jobs = await _fanout_session(pool)
            checked = sum(R.check_standard_roots(jobs, c, msgs) for c, msgs in zip(clients, log))
            for c in clients:
                c.close()
            return pool, checked, pool.stats()
        finally:
            await pool.stop()

    return asyncio.run(asyncio.wait_for(body(), 30))


def test_a_failing_device_path_still_sends_the_right_roots_and_turns_the_device_off():
    calls = []

    def failing(job, prefixes):
        calls.append(len(prefixes))
        raise RuntimeError("injected device failure")

    assert not microbatch.device_failed("cuda:0")
    pool, checked, stats = _run_with_device_fn(failing, job_min_gpu=1)
    assert checked == 3 * 2 * 4  # every root is still the oracle's
    assert calls == [6]  # the device path was tried once; after its failure no fan-out goes there
    jobs = stats["jobs"]
    assert (jobs["device"], jobs["enabled"], jobs["device_errors"]) == ("cuda:0", False, 1)
    assert (jobs["fanouts"], jobs["gpu_channels"], jobs["cpu_channels"]) == (3, 0, 18)
    assert microbatch.device_failed("cuda:0")

    # the share verifier of the same process sees the device failed too
    async def verifier_view():
        vpool = R.seeded_pool(verify_device="cuda:0", verify_min_gpu=1)
        b = vpool._get_batcher()
        try:
            return b.path.on, vpool.stats()["verify"]["enabled"]
        finally:
            await b.close()
            _dispose(vpool)

    assert asyncio.run(verifier_view()) == (False, False)


def test_the_device_path_is_used_from_job_min_gpu_channels_on():
    seen = []

    def device(job, prefixes):
        seen.append(len(prefixes))
        return channel_roots(job, prefixes)

    _pool, checked, stats = _run_with_device_fn(device, job_min_gpu=6)
    assert checked == 3 * 2 * 4 and seen == [6, 6, 6]
    assert (stats["jobs"]["gpu_channels"], stats["jobs"]["cpu_channels"], stats["jobs"]["enabled"]) == (18, 0, True)
    seen.clear()
    _pool, checked, stats = _run_with_device_fn(device, job_min_gpu=7)  # never enough channels: all on the CPU
    assert checked == 3 * 2 * 4 and seen == []
    assert (stats["jobs"]["gpu_channels"], stats["jobs"]["cpu_channels"]) == (0, 18)


def test_job_roots_refuses_bad_options():
    from otedama_amd.pool.jobroots import JobRoots

    for kw in ({"job_device": ""}, {"job_device": "gpu"}, {"job_device": "cpu", "job_min_gpu": -1}):
        pool = R.seeded_pool(**kw)
        with pytest.raises(ValueError):
            JobRoots(pool)
        _dispose(pool)


# ---------------------------------------------------------------- config and flags
def test_config_round_trip_and_validation(tmp_path):
    from otedama_amd import config as cfgmod

    ps = cfgmod.PoolServerConfig()
    assert (ps.job_device, ps.job_min_gpu) == ("", 0)
    assert (server_mod.PoolOptions().job_device, server_mod.PoolOptions().job_min_gpu) == ("", 0)
    path = tmp_path / "config.yaml"
    path.write_text("bitcoin_address: " + C.ADDR + "\npool_server:\n  job_device: cuda:1\n  job_min_gpu: 512\n")
    load = lambda: cfgmod.load_config_file(str(path))[0]  # noqa: E731
    cfg = load()
    assert (cfg.pool_server.job_device, cfg.pool_server.job_min_gpu) == ("cuda:1", 512)
    cfg.validate()
    assert cfg.to_dict()["pool_server"]["job_device"] == "cuda:1"
    for field, bad in (("job_device", "gpu"), ("job_device", "cuda"), ("job_device", "cuda:x"), ("job_min_gpu", -1)):
        c = load()
        setattr(c.pool_server, field, bad)
        with pytest.raises(cfgmod.ConfigError, match=field):
            c.validate()
    for good in ("", "cpu", "cuda:0", "cuda:15"):
        c = load()
        c.pool_server.job_device = good
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
        return pool_cmd.job_options(fs)

    empty = "bitcoin_address: " + C.ADDR + "\n"
    file_text = empty + "pool_server:\n  job_device: cuda:1\n  job_min_gpu: 512\n"
    assert flags([], empty) == {"job_device": "", "job_min_gpu": 0}
    assert flags([], file_text) == {"job_device": "cuda:1", "job_min_gpu": 512}  # the file fills what no flag gave
    assert flags(["--job-device", "cpu"], file_text) == {"job_device": "cpu", "job_min_gpu": 512}  # a flag wins
    assert pool_cmd.job_options_error({"job_device": "cuda:3", "job_min_gpu": 0}) is None
    for bad in (["--job-device", "gpu0"], ["--job-min-gpu", "-2"]):
        out, err = io.StringIO(), io.StringIO()
        path = tmp_path / "empty.yaml"
        path.write_text(empty)
        assert pool_cmd.cmd_pool(["--config", str(path)] + bad, out, err) == EXIT_CONFIG, bad
        assert "job" in err.getvalue()


# ---------------------------------------------------------------- branch cache
def test_branches_are_computed_once_per_block(monkeypatch):
    calls = []
    real = BlockTemplate.branches

    def counted(self):
        calls.append(self.height)
        return real(self)

    monkeypatch.setattr(BlockTemplate, "branches", counted)
    pool = R.seeded_pool(n_txs=50)
    try:
        j1 = pool.new_block()
        j2 = pool.new_job()
        assert calls == [j1.block.height]
        uncached = merkle_branches(j1.block.txids)
        assert len(uncached) == 6
        for j in (j1, j2):
            assert j.branches == uncached
            assert (j.coinb1, j.coinb2) == j.block.coinbase_parts(server_mod.EN1_SIZE + server_mod.EN2_SIZE)
        j3 = pool.new_block()
        assert calls == [j1.block.height, j3.block.height] and j3.block is not j1.block
        assert j3.branches == merkle_branches(j3.block.txids) != uncached
        pool.new_job()
        assert len(calls) == 2
    finally:
        _dispose(pool)


def test_batch_module_stays_torch_free_at_import():
    import subprocess
    import sys

    code = ("import sys; import otedama_amd.pool.batch, otedama_amd.pool.jobroots, otedama_amd.ops.share_records; "
            "assert 'torch' not in sys.modules and 'otedama_amd._native' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
    code = ("import sys; import otedama_amd.pool.devicepath; "
            "assert 'torch' not in sys.modules and 'otedama_amd._native' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
    assert batch.root_of(C.pool_job(), bytes(8)) == R.oracle_root(C.pool_job(), bytes(8))
