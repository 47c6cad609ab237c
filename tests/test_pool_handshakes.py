"""The pool's batched Noise handshakes on the CPU (otedama_amd/pool/handshakes.py, wired in ``PoolServer._serve_v2``):
a crowd of clients of both suites, a bad key among them, a device path that raises, the secrets left in the op's
buffers, ``stop()`` with handshakes waiting, and the options' validation."""
import asyncio
import io

import pytest

import handshake_cases as H
import secp_cases as S
from otedama_amd.ops import secp_rows as R
from otedama_amd.ops.native import require_native
from otedama_amd.pool import devicepath
from otedama_amd.pool.handshakes import DEFAULT_HANDSHAKE_MIN_GPU, HandshakeBatcher, mul_cpu
from otedama_amd.pool.server import PoolOptions
from share_verify_cases import ADDR


def _run(coro, seconds=120):
    return asyncio.run(asyncio.wait_for(coro, seconds))


async def _with_pool(pool, body):
    await pool.start()
    try:
        return await body(pool)
    finally:
        await pool.stop()


def test_sixty_four_clients_of_both_suites_on_the_cpu_path():
    async def body(pool):
        channels, _bad = await H.crowd(pool, H.SUITES_64)
        return channels, pool.stats()

    channels, st = _run(_with_pool(H.noise_pool(handshake_device="cpu"), body))
    H.check_channels(channels, 64)
    hs = st["handshake"]
    assert hs["cpu_handshakes"] == 64 and hs["gpu_handshakes"] == 0 and hs["device_errors"] == 0
    assert (hs["device"], hs["enabled"]) == ("cpu", True)
    assert hs["max_batch"] > 1 and 1 <= hs["batches"] < 64 and hs["last_batch"] >= 1 and hs["last_ms"] > 0
    assert set(hs) == {"device", "enabled", "batches", "gpu_handshakes", "cpu_handshakes", "last_batch", "max_batch",
                       "last_ms", "device_errors"}
    assert "noise-handshake" not in st["reject_reasons"]


def test_a_key_off_the_curve_is_rejected_alone():
    async def body(pool):
        channels, bad = await H.crowd(pool, ["ellswift"] * 6 + ["legacy"] * 2, bad_at=3)
        return channels, bad, pool.stats()

    # a long flush delay and a flush size of all nine: the bad key is in the same flush as the others
    pool = H.noise_pool(handshake_device="cpu", handshake_batch_ms=5000.0, handshake_batch_max=9)
    channels, bad, st = _run(_with_pool(pool, body))
    assert bad is None  # closed without a message 2
    H.check_channels(channels, 8)
    assert st["reject_reasons"].get("noise-handshake") == 1
    assert (st["handshake"]["batches"], st["handshake"]["max_batch"], st["handshake"]["cpu_handshakes"]) == (1, 9, 9)


def test_a_device_error_falls_back_and_turns_the_shared_switch():
    calls = []

    def broken(items):
        calls.append(len(items))
        raise RuntimeError("injected device failure")

    async def body(pool):
        first, _ = await H.crowd(pool, ["ellswift"] * 3 + ["legacy"])
        second, _ = await H.crowd(pool, ["legacy", "ellswift"] * 2)
        return first, second, pool.stats(), devicepath.DevicePath("verify_device", "cuda:0").enabled

    devicepath.forget_device_errors()
    try:
        pool = H.noise_pool(handshake_device="cuda:0", handshake_min_gpu=1, handshake_batch_ms=5000.0,
                            handshake_batch_max=4)
        pool.handshake_mul_fn = broken
        logs = []
        pool.log = lambda level, msg: logs.append((level, msg))
        assert devicepath.DevicePath("verify_device", "cuda:0").enabled
        first, second, st, verify_enabled = _run(_with_pool(pool, body))
    finally:
        devicepath.forget_device_errors()
    H.check_channels(first, 4)
    H.check_channels(second, 4)
    hs = st["handshake"]
    assert calls == [12]  # asked once, never again
    assert hs["device_errors"] == 1 and hs["enabled"] is False and hs["device"] == "cuda:0"
    assert hs["gpu_handshakes"] == 0 and hs["cpu_handshakes"] == 8
    assert verify_enabled is False  # the share verifier's path for that device is off too
    assert any(level == "error" and "handshake batch on cuda:0 failed" in msg for level, msg in logs)


def test_a_fake_device_path_is_counted_as_the_gpu():
    async def body(pool):
        channels, _ = await H.crowd(pool, ["ellswift", "legacy", "ellswift"])
        return channels, pool.stats()["handshake"]

    devicepath.forget_device_errors()
    pool = H.noise_pool(handshake_device="cuda:0", handshake_min_gpu=3, handshake_batch_ms=5000.0,
                        handshake_batch_max=3)
    pool.handshake_mul_fn = mul_cpu
    channels, hs = _run(_with_pool(pool, body))
    H.check_channels(channels, 3)
    assert (hs["gpu_handshakes"], hs["cpu_handshakes"], hs["device_errors"], hs["enabled"]) == (3, 0, 0, True)


def test_the_op_leaves_no_scalar_in_its_pinned_buffer():
    import torch

    from otedama_amd.ops.secp import Secp256k1Mul

    class FakeStaging:
        """``ops._staging.Staging`` without a device: the 'device' computes with the native CPU twin."""

        def __init__(self):
            self.pin_in = torch.zeros(8192, dtype=torch.uint8)
            self.seen = b""

        def round_trip(self, parts, out_bytes, launch):
            raw = b"".join(bytes(p) for p in parts)
            self.pin_in[:len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
            self.seen = raw
            return memoryview(require_native().secp256k1_mul_cpu(raw))[:out_bytes]

    op = Secp256k1Mul("cuda:0")  # no device is touched before the first launch
    op._staging = FakeStaging()
    rows = S.tiled(20)
    assert op.mul(rows) == S.expected(rows)
    assert op._staging.seen == bytes(R.pack_rows(rows))  # the scalars did go in
    left = op._staging.pin_in.numpy().tobytes()
    for i, (_scalar, kind, point) in enumerate(rows):
        row = left[i * R.ROW_BYTES:(i + 1) * R.ROW_BYTES]
        assert row[:32] == bytes(32) and row[32:96] == point.ljust(64, b"\0") and row[96] == kind
    assert op.mul([]) == []
    with pytest.raises(ValueError):
        op.mul([S.ROWS[0]] * (R.MAX_ROWS + 1))


def test_stop_resolves_the_handshakes_that_wait():
    async def body():
        pool = H.noise_pool(handshake_device="cpu", handshake_batch_ms=60000.0)
        batcher = HandshakeBatcher(pool)
        groups = [S.ROWS[3 * i:3 * i + 3] for i in range(5)]
        tasks = [asyncio.ensure_future(batcher.submit(g)) for g in groups]
        await asyncio.sleep(0)
        assert not any(t.done() for t in tasks) and batcher.batches == 0
        await batcher.stop()
        got = [t.result() for t in tasks]
        late = await batcher.submit(groups[0])  # after stop(): answered on its own
        pool.journal.close()
        return groups, got, late, batcher.stats()

    groups, got, late, st = _run(body())
    assert got == [S.expected(g) for g in groups] and late == S.expected(groups[0])
    assert st["cpu_handshakes"] == 6 and st["batches"] == 1 and st["max_batch"] == 5


def test_off_by_default_no_batcher_exists():
    async def body(pool):
        channels, _ = await H.crowd(pool, ["ellswift", "legacy"])
        return channels, pool._handshakes, pool.stats()["handshake"]

    assert PoolOptions().handshake_device == "" and DEFAULT_HANDSHAKE_MIN_GPU >= 1
    assert (PoolOptions().handshake_batch_ms, PoolOptions().handshake_batch_max, PoolOptions().handshake_min_gpu) == (
        2.0, 4096, 0)
    channels, batcher, hs = _run(_with_pool(H.noise_pool(), body))
    H.check_channels(channels, 2)
    assert batcher is None
    assert hs == {"device": "", "enabled": False, "batches": 0, "gpu_handshakes": 0, "cpu_handshakes": 0,
                  "last_batch": 0, "max_batch": 0, "last_ms": 0.0, "device_errors": 0}


def test_the_batcher_refuses_bad_options():
    async def body():
        out = []
        for kw in ({"handshake_device": "gpu0"}, {"handshake_device": ""}, {"handshake_batch_ms": 0.0},
                   {"handshake_batch_max": 0}, {"handshake_batch_max": 21846}, {"handshake_min_gpu": -1}):
            pool = H.noise_pool(**{"handshake_device": "cpu", **kw})
            try:
                HandshakeBatcher(pool)
                out.append(kw)
            except ValueError:
                pass
            pool.journal.close()
        return out

    assert _run(body()) == []


def test_config_validate_and_the_flags(tmp_path):
    from otedama_amd import config as cfgmod
    from otedama_amd.cli import pool_cmd
    from otedama_amd.cli.main import EXIT_CONFIG

    ps = cfgmod.PoolServerConfig()
    assert (ps.handshake_device, ps.handshake_batch_ms, ps.handshake_batch_max, ps.handshake_min_gpu) == (
        "", 2.0, 4096, 0)
    path = tmp_path / "config.yaml"
    path.write_text("bitcoin_address: " + ADDR + "\npool_server:\n  handshake_device: cuda:1\n"
                    "  handshake_batch_ms: 0.5\n  handshake_batch_max: 128\n  handshake_min_gpu: 32\n")
    load = lambda: cfgmod.load_config_file(str(path))[0]  # noqa: E731
    cfg = load()
    cfg.validate()
    assert cfg.to_dict()["pool_server"]["handshake_device"] == "cuda:1"
    for field, bad in (("handshake_device", "gpu0"), ("handshake_batch_ms", 0), ("handshake_min_gpu", -1),
                       ("handshake_batch_max", 0), ("handshake_batch_max", 21846)):
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
        return pool_cmd.handshake_options(fs)

    empty = "bitcoin_address: " + ADDR + "\n"
    assert flags([], empty) == {"handshake_device": "", "handshake_batch_ms": 2.0, "handshake_batch_max": 4096,
                                "handshake_min_gpu": 0}
    assert flags([], path.read_text()) == {"handshake_device": "cuda:1", "handshake_batch_ms": 0.5,
                                           "handshake_batch_max": 128, "handshake_min_gpu": 32}
    assert flags(["--handshake-device", "cpu", "--handshake-batch-max", "7"], path.read_text()) == {
        "handshake_device": "cpu", "handshake_batch_ms": 0.5, "handshake_batch_max": 7, "handshake_min_gpu": 32}
    for bad in (["--handshake-device", "gpu0"], ["--handshake-batch-ms", "0"], ["--handshake-batch-max", "0"],
                ["--handshake-min-gpu", "-1"]):
        out, err = io.StringIO(), io.StringIO()
        p = tmp_path / "empty.yaml"
        p.write_text(empty)
        assert pool_cmd.cmd_pool(["--config", str(p)] + bad, out, err) == EXIT_CONFIG, bad
        assert "handshake" in err.getvalue()
