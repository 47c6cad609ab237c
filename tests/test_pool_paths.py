"""The core under the pool's five CPU-or-GPU paths (otedama_amd/pool/devicepath.py) without a GPU: the one table of
the paths against what the pool, the CLI and the config file make of it, the micro-batch loop with a trivial
processor, and the synchronous core with fake callables."""
import asyncio
import threading
import time
import types

import channel_roots_cases as R
import pytest

from otedama_amd import config as cfgmod
from otedama_amd.cli import pool_cmd
from otedama_amd.pool import devicepath
from otedama_amd.pool.server import PoolOptions

# prefix -> (key in /api/v1/pool, PoolServer's stats method, its keys in order)
STATS = {
    "verify": ("verify", "verify_stats", ["device", "enabled", "batches", "gpu_shares", "cpu_shares", "last_batch",
                                          "max_batch", "device_errors"]),
    "job": ("jobs", "jobs_stats", ["device", "enabled", "fanouts", "gpu_channels", "cpu_channels", "last_channels",
                                   "last_ms", "device_errors"]),
    "template": ("template", "template_stats", ["device", "enabled", "trees", "gpu_leaves", "cpu_leaves",
                                                "last_leaves", "last_ms", "device_errors"]),
    "handshake": ("handshake", "handshake_stats", ["device", "enabled", "batches", "gpu_handshakes", "cpu_handshakes",
                                                   "last_batch", "max_batch", "last_ms", "device_errors"]),
    "seal": ("seal", "seal_stats", ["device", "enabled", "batches", "gpu_frames", "cpu_frames", "last_frames",
                                    "last_ms", "device_errors"]),
}

# (field, bad value, what `otedama pool` says, what the config file's validation says), recorded before the five
# paths shared one implementation
MESSAGES = [
    ("verify_device", "gpu", "--verify-device 'gpu' must be empty (off), cpu or cuda:N",
     'pool_server.verify_device \'gpu\' is not one of "", cpu, cuda:N'),
    ("verify_device", "cuda", "--verify-device 'cuda' must be empty (off), cpu or cuda:N",
     'pool_server.verify_device \'cuda\' is not one of "", cpu, cuda:N'),
    ("verify_device", "cuda:x", "--verify-device 'cuda:x' must be empty (off), cpu or cuda:N",
     'pool_server.verify_device \'cuda:x\' is not one of "", cpu, cuda:N'),
    ("verify_min_gpu", -1, "--verify-min-gpu must not be negative (0 = the algorithm's measured default)",
     "pool_server.verify_min_gpu must be >= 0 (0 = the algorithm's default)"),
    ("verify_batch_ms", 0, "--verify-batch-ms and --verify-batch-max must be positive",
     "pool_server.verify_batch_ms must be > 0"),
    ("verify_batch_max", 0, "--verify-batch-ms and --verify-batch-max must be positive",
     "pool_server.verify_batch_max must be > 0"),
    ("job_device", "gpu", "--job-device 'gpu' must be empty (off), cpu or cuda:N",
     'pool_server.job_device \'gpu\' is not one of "", cpu, cuda:N'),
    ("job_device", "cuda", "--job-device 'cuda' must be empty (off), cpu or cuda:N",
     'pool_server.job_device \'cuda\' is not one of "", cpu, cuda:N'),
    ("job_device", "cuda:x", "--job-device 'cuda:x' must be empty (off), cpu or cuda:N",
     'pool_server.job_device \'cuda:x\' is not one of "", cpu, cuda:N'),
    ("job_min_gpu", -1, "--job-min-gpu must not be negative (0 = the measured default)",
     "pool_server.job_min_gpu must be >= 0 (0 = the measured default)"),
    ("template_device", "gpu", "--template-device 'gpu' must be empty (off), cpu or cuda:N",
     'pool_server.template_device \'gpu\' is not one of "", cpu, cuda:N'),
    ("template_device", "cuda", "--template-device 'cuda' must be empty (off), cpu or cuda:N",
     'pool_server.template_device \'cuda\' is not one of "", cpu, cuda:N'),
    ("template_device", "cuda:x", "--template-device 'cuda:x' must be empty (off), cpu or cuda:N",
     'pool_server.template_device \'cuda:x\' is not one of "", cpu, cuda:N'),
    ("template_min_gpu", -1, "--template-min-gpu must not be negative (0 = the measured default)",
     "pool_server.template_min_gpu must be >= 0 (0 = the measured default)"),
    ("handshake_device", "gpu", "--handshake-device 'gpu' must be empty (off), cpu or cuda:N",
     'pool_server.handshake_device \'gpu\' is not one of "", cpu, cuda:N'),
    ("handshake_device", "cuda", "--handshake-device 'cuda' must be empty (off), cpu or cuda:N",
     'pool_server.handshake_device \'cuda\' is not one of "", cpu, cuda:N'),
    ("handshake_device", "cuda:x", "--handshake-device 'cuda:x' must be empty (off), cpu or cuda:N",
     'pool_server.handshake_device \'cuda:x\' is not one of "", cpu, cuda:N'),
    ("handshake_min_gpu", -1, "--handshake-min-gpu must not be negative (0 = the measured default)",
     "pool_server.handshake_min_gpu must be >= 0 (0 = the measured default)"),
    ("handshake_batch_ms", 0, "--handshake-batch-ms must be positive and --handshake-batch-max in 1..21845",
     "pool_server.handshake_batch_ms must be > 0"),
    ("handshake_batch_max", 0, "--handshake-batch-ms must be positive and --handshake-batch-max in 1..21845",
     "pool_server.handshake_batch_max must be in 1..21845 (three rows a handshake, 65536 a call)"),
    ("handshake_batch_max", 21846, "--handshake-batch-ms must be positive and --handshake-batch-max in 1..21845",
     "pool_server.handshake_batch_max must be in 1..21845 (three rows a handshake, 65536 a call)"),
    ("seal_device", "gpu", "--seal-device 'gpu' must be empty (off), cpu or cuda:N",
     'pool_server.seal_device \'gpu\' is not one of "", cpu, cuda:N'),
    ("seal_device", "cuda", "--seal-device 'cuda' must be empty (off), cpu or cuda:N",
     'pool_server.seal_device \'cuda\' is not one of "", cpu, cuda:N'),
    ("seal_device", "cuda:x", "--seal-device 'cuda:x' must be empty (off), cpu or cuda:N",
     'pool_server.seal_device \'cuda:x\' is not one of "", cpu, cuda:N'),
    ("seal_min_gpu", -1, "--seal-min-gpu must not be negative (0 = the measured default)",
     "pool_server.seal_min_gpu must be >= 0 (0 = the measured default)"),
]


def _dispose(pool) -> None:
    """For a pool that was never started."""
    pool.journal.close()
    pool._hash_pool.shutdown(wait=False)


def _fake_pool(**opts):
    logs = []
    return types.SimpleNamespace(opts=types.SimpleNamespace(**opts), algo=types.SimpleNamespace(name="sha256d"),
                                 logs=logs, log=lambda level, msg: logs.append((level, msg)))


# ---------------------------------------------------------------- the table
def test_the_table_names_the_five_paths_their_api_keys_and_their_stats_keys():
    assert list(devicepath.PATHS) == list(STATS)
    for prefix, (api_key, _method, keys) in STATS.items():
        spec = devicepath.PATHS[prefix]
        assert (spec.prefix, spec.api_key, list(spec.stats_keys)) == (prefix, api_key, keys)
    assert [p for p, s in devicepath.PATHS.items() if s.batched] == ["verify", "handshake"]
    assert (devicepath.PATHS["verify"].batch_max_limit, devicepath.PATHS["handshake"].batch_max_limit) == (0, 21845)


@pytest.mark.parametrize("prefix", list(STATS))
def test_a_pool_without_the_path_reports_the_keys_of_a_live_one_all_zero(prefix):
    api_key, method, keys = STATS[prefix]

    async def live_stats():
        pool = R.seeded_pool(**{f"{prefix}_device": "cpu"})
        path = pool._path(prefix)
        try:
            return path.stats(), getattr(pool, method)(), pool._path(prefix) is path
        finally:
            closed = path.close()
            if closed is not None:
                await closed
            _dispose(pool)

    live, through_pool, made_once = asyncio.run(live_stats())
    pool = R.seeded_pool()
    try:
        off = getattr(pool, method)()
        pool.new_block()
        assert pool.stats()[api_key] == off
    finally:
        _dispose(pool)
    assert list(off) == list(live) == list(through_pool) == keys and made_once
    assert off == {k: "" if k == "device" else False if k == "enabled" else 0 for k in keys}
    assert all(type(off[k]) is type(live[k]) for k in keys)
    assert (live["device"], live["enabled"]) == ("cpu", True) and all(live[k] == 0 for k in keys[2:])


# ---------------------------------------------------------------- the CLI and the config file
@pytest.mark.parametrize("field,bad,cli,cfg", MESSAGES, ids=[f"{m[0]}={m[1]}" for m in MESSAGES])
def test_bad_values_get_the_recorded_messages(field, bad, cli, cfg):
    prefix = field.split("_")[0]
    defaults = {f: getattr(PoolOptions(), f) for f in devicepath.PATHS[prefix].fields}
    assert field in defaults
    assert getattr(pool_cmd, f"{prefix}_options_error")(defaults) is None
    assert getattr(pool_cmd, f"{prefix}_options_error")({**defaults, field: bad}) == cli
    c = cfgmod.Config()
    c.bitcoin_address = R.ADDR
    c.validate()
    setattr(c.pool_server, field, bad)
    with pytest.raises(cfgmod.ConfigError) as err:
        c.validate()
    assert str(err.value) == "config validation failed:\n  - " + cfg


def test_the_flags_of_every_path_reach_the_options_and_the_config_file():
    fs = pool_cmd.pool_flags(None)
    for prefix, spec in devicepath.PATHS.items():
        opts = getattr(pool_cmd, f"{prefix}_options")(fs)
        assert opts == {f: getattr(PoolOptions(), f) for f in spec.fields}
        assert all(pool_cmd._FILE_FIELD[f.replace("_", "-")] == f and hasattr(cfgmod.PoolServerConfig(), f)
                   for f in spec.fields)


# ---------------------------------------------------------------- the micro-batch loop
class Doubler(devicepath.MicroBatch):
    """The loop with a trivial processor: twice the item. ``gate`` holds a batch in flight; ``"boom"`` breaks one."""

    def __init__(self, batch_ms: float, batch_max: int):
        super().__init__(_fake_pool(verify_device="cpu", verify_batch_ms=batch_ms, verify_batch_max=batch_max,
                                    verify_min_gpu=0), "verify", 1, "doubling", "it was doubled")
        self.seen: list = []
        self.gate = None

    async def _process(self, items: list) -> list:
        self.seen.append(list(items))
        if self.gate is not None:
            await self.gate.wait()
        if "boom" in items:
            raise RuntimeError("the processor broke")
        return [2 * i for i in items]

    def _late(self, item):
        return ("late", item)


def _loop_test(body, batch_ms: float, batch_max: int):
    async def run():
        b = Doubler(batch_ms, batch_max)
        try:
            return await asyncio.wait_for(body(b), 20)
        finally:
            await b.close()

    return asyncio.run(run())


def test_the_loop_flushes_at_batch_max_without_waiting_out_batch_ms():
    async def body(b):
        t0 = time.perf_counter()
        got = await asyncio.gather(*(b.submit(i) for i in (1, 2, 3)))
        return got, b.seen, time.perf_counter() - t0

    got, seen, took = _loop_test(body, batch_ms=60000.0, batch_max=3)
    assert got == [2, 4, 6] and seen == [[1, 2, 3]] and took < 10.0


def test_the_loop_flushes_a_lone_entry_after_batch_ms():
    async def body(b):
        t0 = time.perf_counter()
        got = await b.submit(7)
        return got, b.seen, time.perf_counter() - t0

    got, seen, took = _loop_test(body, batch_ms=5.0, batch_max=64)
    assert got == 14 and seen == [[7]] and 0.005 <= took < 10.0


def test_the_loop_counts_batch_ms_from_the_arrival_time_it_is_given():
    async def body(b):
        t0 = time.perf_counter()
        got = await b.submit(7, t0 - 3600.0)  # it arrived an hour ago: due at once
        return got, time.perf_counter() - t0

    got, took = _loop_test(body, batch_ms=60000.0, batch_max=64)
    assert got == 14 and took < 10.0


def test_entries_that_arrive_while_a_batch_is_in_flight_come_out_in_the_next_one_in_order():
    async def body(b):
        b.gate = asyncio.Event()
        first = [asyncio.ensure_future(b.submit(i)) for i in (1, 2)]
        while not b.seen:
            await asyncio.sleep(0)
        later = [asyncio.ensure_future(b.submit(i)) for i in (5, 4, 3)]
        await asyncio.sleep(0.01)
        assert b.seen == [[1, 2]] and len(b._pending) == 3 and not any(t.done() for t in first + later)
        b.gate.set()
        return await asyncio.gather(*first, *later), b.seen

    got, seen = _loop_test(body, batch_ms=5.0, batch_max=2)
    assert got == [2, 4, 10, 8, 6] and seen == [[1, 2], [5, 4], [3]]


def test_a_processor_that_raises_fails_every_entry_of_that_batch_and_the_loop_goes_on():
    async def body(b):
        broken = await asyncio.gather(b.submit(1), b.submit("boom"), return_exceptions=True)
        return broken, await asyncio.gather(b.submit(2), b.submit(3)), b.seen

    broken, after, seen = _loop_test(body, batch_ms=60000.0, batch_max=2)
    assert [type(e) for e in broken] == [RuntimeError, RuntimeError] and broken[0] is broken[1]
    assert str(broken[0]) == "the processor broke"
    assert after == [4, 6] and seen == [[1, "boom"], [2, 3]]


def test_a_result_short_of_the_batch_fails_it_instead_of_leaving_a_future_unresolved():
    class Short(Doubler):
        async def _process(self, items):
            return [0] * (len(items) - 1)

    async def run():
        b = Short(60000.0, 2)
        try:
            return await asyncio.wait_for(asyncio.gather(b.submit(1), b.submit(2), return_exceptions=True), 20)
        finally:
            await b.close()

    assert [type(e) for e in asyncio.run(run())] == [RuntimeError, RuntimeError]


def test_a_cancelled_future_is_skipped():
    async def body(b):
        gone = asyncio.ensure_future(b.submit(1))
        await asyncio.sleep(0)
        gone.cancel()
        await asyncio.sleep(0)
        assert gone.cancelled() and len(b._pending) == 1  # it still takes its place in the batch
        stayed = await b.submit(2)
        return stayed, await asyncio.gather(b.submit(3), b.submit(4)), b.seen

    stayed, after, seen = _loop_test(body, batch_ms=60000.0, batch_max=2)
    assert stayed == 4 and after == [6, 8] and seen == [[1, 2], [3, 4]]


def test_close_drains_what_is_pending_and_answers_later_submits_on_their_own():
    async def run():
        b = Doubler(60000.0, 2)
        tasks = [asyncio.ensure_future(b.submit(i)) for i in (1, 2, 3)]
        await asyncio.sleep(0.01)  # 1 and 2 are done, 3 waits for a deadline a minute away
        assert [t.done() for t in tasks] == [True, True, False]
        t0 = time.perf_counter()
        await b.stop()  # close() under its other name
        await asyncio.sleep(0)
        assert all(t.done() for t in tasks)
        return [t.result() for t in tasks], b.seen, await b.submit(9), b._worker._shutdown, time.perf_counter() - t0

    got, seen, late, worker_ended, took = asyncio.run(asyncio.wait_for(run(), 20))
    assert got == [2, 4, 6] and seen == [[1, 2], [3]] and late == ("late", 9) and worker_ended and took < 10.0


def test_the_loop_refuses_bad_options():
    async def run():
        for kw in ({"batch_ms": 0.0}, {"batch_max": 0}):
            with pytest.raises(ValueError, match="verify_batch_ms and verify_batch_max must be positive, "
                                                 "verify_min_gpu not negative"):
                Doubler(**{"batch_ms": 1.0, "batch_max": 1, **kw})

    asyncio.run(run())


# ---------------------------------------------------------------- the synchronous core
class Work(devicepath.DeviceWork):
    """As thin as the real users: ``do(n)`` is n units of work, counted by where they ran."""

    def __init__(self, pool, on_device, on_cpu):
        super().__init__(pool, "job", 512, "fake work", "it was done")
        self.on_device, self.on_cpu = on_device, on_cpu

    def do(self, n: int):
        result, ran = self.call(n, lambda: self.on_device(n), lambda: self.on_cpu(n))
        self.fanouts += 1
        self.last_channels = n
        self.gpu_channels += n if ran else 0
        self.cpu_channels += 0 if ran else n
        return result


@pytest.fixture
def fresh_switch():
    devicepath.forget_device_errors()
    yield
    devicepath.forget_device_errors()


def _recording(tag: str, calls: list, fail: bool = False):
    def fn(n):
        calls.append((tag, n, threading.current_thread().name))
        if fail:
            raise RuntimeError("injected device failure")
        return (tag, n)

    return fn


def test_the_core_sends_work_below_min_gpu_to_the_cpu_and_from_min_gpu_on_to_the_device(fresh_switch):
    calls: list = []
    pool = _fake_pool(job_device="cuda:0", job_min_gpu=4)
    w = Work(pool, _recording("gpu", calls), _recording("cpu", calls))
    try:
        assert w.min_gpu == 4 and w.do(3) == ("cpu", 3) and [c[:2] for c in calls] == [("cpu", 3)]
        assert w.do(4) == ("gpu", 4) and w.do(9) == ("gpu", 9)
    finally:
        w.close()
    assert [c[:2] for c in calls] == [("cpu", 3), ("gpu", 4), ("gpu", 9)]
    assert all(c[2].startswith("otedama-pool-job") for c in calls)  # on the path's own worker thread
    st = w.stats()
    assert list(st) == STATS["job"][2] and st["last_ms"] > 0.0
    assert {k: v for k, v in st.items() if k != "last_ms"} == {
        "device": "cuda:0", "enabled": True, "fanouts": 3, "gpu_channels": 13, "cpu_channels": 3, "last_channels": 9,
        "device_errors": 0}
    assert pool.logs == []


def test_min_gpu_zero_is_the_paths_default_and_a_cpu_path_never_calls_the_device(fresh_switch):
    calls: list = []
    w = Work(_fake_pool(job_device="cuda:0", job_min_gpu=0), _recording("gpu", calls), _recording("cpu", calls))
    c = Work(_fake_pool(job_device="cpu", job_min_gpu=1), _recording("gpu", calls), _recording("cpu", calls))
    try:
        assert w.min_gpu == 512 and w.do(511) == ("cpu", 511) and w.do(512) == ("gpu", 512)
        assert c.do(1 << 20) == ("cpu", 1 << 20) and c.stats()["enabled"] is True
    finally:
        w.close()
        c.close()


def test_a_device_error_is_tried_once_answered_by_the_cpu_and_turns_the_device_off_for_every_path(fresh_switch):
    calls: list = []
    pool = _fake_pool(job_device="cuda:0", job_min_gpu=1)
    w = Work(pool, _recording("gpu", calls, fail=True), _recording("cpu", calls))
    try:
        assert w.do(5) == ("cpu", 5) and w.do(6) == ("cpu", 6)
    finally:
        w.close()
    assert [c[:2] for c in calls] == [("gpu", 5), ("cpu", 5), ("cpu", 6)]
    st = w.stats()
    assert (st["enabled"], st["device_errors"], st["gpu_channels"], st["cpu_channels"]) == (False, 1, 0, 11)
    assert pool.logs == [("error", "pool[sha256d]: fake work on cuda:0 failed (RuntimeError('injected device "
                                   "failure')); it was done on the CPU and the device path is off for this process")]
    assert devicepath.device_failed("cuda:0") and not devicepath.device_failed("cuda:1")

    calls.clear()
    other_pool = _fake_pool(job_device="cuda:0", job_min_gpu=1)
    other = Work(other_pool, _recording("gpu", calls), _recording("cpu", calls))
    elsewhere = Work(_fake_pool(job_device="cuda:1", job_min_gpu=1), _recording("gpu", calls), _recording("cpu", calls))
    try:
        assert other.stats()["enabled"] is False and other.do(7) == ("cpu", 7)
        assert elsewhere.stats()["enabled"] is True and elsewhere.do(7) == ("gpu", 7)
    finally:
        other.close()
        elsewhere.close()
    assert [c[:2] for c in calls] == [("cpu", 7), ("gpu", 7)]
    assert other.stats()["device_errors"] == 0 and other_pool.logs == []  # counted on the path that hit it


def test_the_switch_is_read_again_on_the_worker_thread(fresh_switch):
    calls: list = []
    w = Work(_fake_pool(job_device="cuda:0", job_min_gpu=1), _recording("gpu", calls), _recording("cpu", calls))
    try:
        # the loop chose the device; another path's error arrives before the worker thread starts the call
        assert w._use(5, False) is True
        devicepath.mark_failed("cuda:0")
        result, ran, error = w._worker.submit(w._work, True, lambda: w.on_device(5), lambda: w.on_cpu(5)).result()
    finally:
        w.close()
    assert (result, ran, error) == (("cpu", 5), False, None) and [c[:2] for c in calls] == [("cpu", 5)]
    assert w.stats()["device_errors"] == 0


def test_the_core_refuses_bad_options():
    for kw, text in (({"job_device": ""}, "job_device '' must be cpu or cuda:N"),
                     ({"job_device": "gpu"}, "job_device 'gpu' must be cpu or cuda:N"),
                     ({"job_min_gpu": -1}, "job_min_gpu must not be negative")):
        with pytest.raises(ValueError) as err:
            Work(_fake_pool(**{"job_device": "cpu", "job_min_gpu": 0, **kw}), None, None)
        assert str(err.value) == text


def test_never_is_above_any_batch_and_is_the_one_definition():
    from otedama_amd.pool import frameseal, handshakes, microbatch

    assert microbatch.NEVER is devicepath.NEVER and devicepath.NEVER > 1 << 24
    assert not hasattr(frameseal, "NEVER") and not hasattr(handshakes, "NEVER")
