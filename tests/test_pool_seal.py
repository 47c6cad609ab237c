"""The pool's batched frame sealing on the CPU (otedama_amd/pool/frameseal.py, wired in ``PoolServer._make_job``):
one seal call per job for all Noise connections, counters that stay in step in both directions, the feature off by
default, and the options' validation. The pool and its clients are in seal_pool_cases.py."""
import asyncio
import io

import pytest

import channel_roots_cases as R
from otedama_amd.pool.batch import seal_frames
from otedama_amd.pool.server import PoolOptions
from otedama_amd.stratum import messages as M
from seal_pool_cases import check_new_block, pool_with_clients, submit_each, take_block
from share_verify_cases import ADDR


def _run(coro, seconds=120):
    return asyncio.run(asyncio.wait_for(coro, seconds))


def test_one_seal_call_of_two_frames_a_channel_and_the_counters_stay_in_step():
    calls = []

    def counting(frames):
        calls.append(len(frames))
        return seal_frames(frames, "cpu")

    async def body(pool, clients):
        assert pool._sealer is None and calls == []  # channel opens and their first jobs are sealed frame by frame
        pool.new_block()
        await take_block(pool, clients)
        first = list(calls)
        pool.new_job(clean=False)  # a job on the same block: one NewMiningJob a channel
        for c in clients:
            assert isinstance(await c.recv(), M.NewMiningJob)
        second = list(calls)
        blocks = await submit_each(pool, clients)  # replies are sealed one by one; every found block is a batch
        return first, second, blocks, list(calls), pool.stats()

    k = 5
    first, second, blocks, calls_after, st = _run(pool_with_clients(k, body, seal_fn=counting, seal_device="cpu"))
    assert first == [2 * k] and second == [2 * k, k]
    assert blocks == k and calls_after == [2 * k, k] + [2 * k] * blocks
    seal = st["seal"]
    assert (seal["device"], seal["enabled"], seal["batches"], seal["cpu_frames"], seal["gpu_frames"]) == (
        "cpu", True, 2 + blocks, k + 2 * k * (1 + blocks), 0)
    assert seal["last_frames"] == 2 * k and seal["last_ms"] > 0 and seal["device_errors"] == 0
    assert st["accepted"] == k and st["rejected"] == 0 and st["blocks_found"] == k


def test_the_native_cpu_path_without_an_injection():
    async def body(pool, clients):
        await check_new_block(pool, clients)
        return pool.stats()["seal"]

    seal = _run(pool_with_clients(3, body, seal_device="cpu"))
    assert (seal["batches"], seal["cpu_frames"], seal["gpu_frames"], seal["enabled"]) == (4, 24, 0, True)


def test_off_by_default_no_sealer_exists():
    async def body(pool, clients):
        await check_new_block(pool, clients)
        return pool._sealer, pool.stats()["seal"]

    assert (PoolOptions().seal_device, PoolOptions().seal_min_gpu) == ("", 0)
    sealer, seal = _run(pool_with_clients(2, body))
    assert sealer is None
    assert seal == {"device": "", "enabled": False, "batches": 0, "gpu_frames": 0, "cpu_frames": 0, "last_frames": 0,
                    "last_ms": 0.0, "device_errors": 0}


def test_without_noise_the_option_changes_nothing():
    async def body():
        pool = R.seeded_pool(seed=b"seal-plain", seal_device="cpu")
        await pool.start()
        try:
            c = await R.V2Client.connect(pool)
            await c.open()
            pool.new_block()
            msgs = await c.take(2)
            c.close()
            return [type(m) for m in msgs], pool._sealer
        finally:
            await pool.stop()

    kinds, sealer = _run(body())
    assert kinds == [M.NewMiningJob, M.SetNewPrevHash] and sealer is None


def test_config_validate_and_the_flags(tmp_path):
    from otedama_amd import config as cfgmod
    from otedama_amd.cli import pool_cmd
    from otedama_amd.cli.main import EXIT_CONFIG

    ps = cfgmod.PoolServerConfig()
    assert (ps.seal_device, ps.seal_min_gpu) == ("", 0)
    path = tmp_path / "config.yaml"
    path.write_text("bitcoin_address: " + ADDR + "\npool_server:\n  seal_device: cuda:1\n  seal_min_gpu: 4096\n")
    load = lambda: cfgmod.load_config_file(str(path))[0]  # noqa: E731
    cfg = load()
    cfg.validate()
    assert cfg.to_dict()["pool_server"]["seal_device"] == "cuda:1"
    for field, bad in (("seal_device", "gpu0"), ("seal_min_gpu", -1)):
        c = load()
        setattr(c.pool_server, field, bad)
        with pytest.raises(cfgmod.ConfigError, match=field):
            c.validate()

    def flags(args, text):
        p = tmp_path / "flags.yaml"
        p.write_text(text)
        err = io.StringIO()
        fs = pool_cmd.pool_flags(err)
        fs.parse(["--config", str(p)] + args)
        pool_cmd.apply_config_file(fs, err)
        return pool_cmd.seal_options(fs)

    empty = "bitcoin_address: " + ADDR + "\n"
    assert flags([], empty) == {"seal_device": "", "seal_min_gpu": 0}
    assert flags([], path.read_text()) == {"seal_device": "cuda:1", "seal_min_gpu": 4096}
    assert flags(["--seal-device", "cpu"], path.read_text()) == {"seal_device": "cpu", "seal_min_gpu": 4096}
    for bad in (["--seal-device", "gpu0"], ["--seal-min-gpu", "-1"]):
        out, err = io.StringIO(), io.StringIO()
        p = tmp_path / "empty.yaml"
        p.write_text(empty)
        assert pool_cmd.cmd_pool(["--config", str(p)] + bad, out, err) == EXIT_CONFIG, bad
        assert "seal" in err.getvalue()
