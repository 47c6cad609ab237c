"""The pool's micro-batcher (otedama_amd/pool/microbatch.py) without a GPU: concurrent ``validate_async`` submits
through ``verify_device="cpu"`` against sequential ``validate`` on a twin pool, item by item and row by row."""
import asyncio
import time

import pytest

import share_verify_cases as C


def _pools(**opts):
    """(A, B, earlier, batch): twin scripted pools, B with the batcher options; ``earlier`` validated on both."""
    tmpl = C.script_template()
    a, b = C.ScriptedPool(tmpl), C.ScriptedPool(tmpl)
    for k, v in opts.items():
        setattr(b.pool.opts, k, v)
    b.pool.new_block = lambda: None  # a found block schedules it on the running loop; A's loop never runs
    earlier, batch = C.build_script(a)
    assert C.run_sequential(a, earlier) == C.run_sequential(b, earlier)
    return a, b, earlier, batch


def _close(*pools):
    from otedama_amd.pool.microbatch import forget_device_errors

    for sp in pools:
        sp.close()
    forget_device_errors()  # the switch is the process's: a test that tripped it hands the device back


def _submit_all(sp, items):
    """One asyncio.gather of validate_async over ``items`` on the pool's own loop, then the batcher closed."""
    workers = {"rig": sp.rig, "ramp": sp.ramp}

    async def go():
        try:
            return await asyncio.gather(*(sp.pool.validate_async(workers[w], *rest) for w, *rest in items))
        finally:
            if sp.pool._batcher is not None:
                await sp.pool._batcher.close()

    asyncio.set_event_loop(sp.loop)
    return sp.loop.run_until_complete(go())


@pytest.mark.parametrize("cap,flushes", [(5, 3), (1, 14), (64, 1)])
def test_batched_submits_equal_sequential_validation(cap, flushes):
    a, b, _earlier, batch = _pools(verify_device="cpu", verify_batch_max=cap, verify_min_gpu=1)
    try:
        want = C.run_sequential(a, batch)
        got = _submit_all(b, batch)
        assert len(got) == len(batch) == 14
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, i
        assert sum(v.accepted for v in got) >= 6 and any(v.block for v in got)
        assert b.state() == a.state()
        vs = b.pool.stats()["verify"]
        assert vs["device"] == "cpu" and vs["enabled"] and vs["batches"] == flushes
        assert vs["max_batch"] == min(cap, 14) and vs["gpu_shares"] == 0 and vs["device_errors"] == 0
        assert vs["cpu_shares"] == 11  # 14 less the stale job, the version bits and the ntime
        assert len(b.pool._validate_ms) == 14
    finally:
        _close(a, b)


def test_a_lone_submit_is_flushed_by_time():
    a, b, _earlier, batch = _pools(verify_device="cpu", verify_batch_max=64, verify_batch_ms=20.0, verify_min_gpu=1)
    try:
        want = C.run_sequential(a, batch[:1])
        t0 = time.perf_counter()
        got = _submit_all(b, batch[:1])
        dt = time.perf_counter() - t0
        assert got == want
        # liveness, not a timing claim: answered without a second submit, not before the delay, far inside 5 s
        assert 0.015 <= dt < 5.0, dt
        assert b.pool.stats()["verify"]["batches"] == 1
        assert b.pool.validation_ms(0.5) >= 15.0  # submit received -> verdict includes the wait
    finally:
        _close(a, b)


def test_a_device_error_falls_back_to_the_cpu_and_disables_the_device():
    a, b, _earlier, batch = _pools(verify_device="cuda:0", verify_batch_max=5, verify_min_gpu=1)
    calls = []

    def failing(job, shares, targets, indices):
        calls.append(len(shares))
        raise RuntimeError("injected device failure")

    logged = []
    b.pool.verify_hasher = failing
    b.pool.log = lambda level, msg: logged.append((level, msg))
    try:
        want = C.run_sequential(a, batch)
        got = _submit_all(b, batch)
        assert got == want
        assert b.state() == a.state()
        vs = b.pool.stats()["verify"]
        assert vs["device"] == "cuda:0" and vs["device_errors"] == 1 and vs["enabled"] is False
        assert vs["batches"] == 3 and vs["gpu_shares"] == 0 and vs["cpu_shares"] == 11
        assert len(calls) == 1  # the first batch only: the next batches never call the hasher
        assert any(level == "error" and "injected device failure" in msg for level, msg in logged)
    finally:
        _close(a, b)


def test_a_device_error_in_one_pool_disables_the_device_for_every_pool_of_the_process():
    """`otedama pool --algorithms a,b --verify-device cuda:0` runs one pool and one batcher per algorithm on the same
    device. Two pools share one failing hasher here: after the first pool's error the second never calls it."""
    a, b, _earlier, batch = _pools(verify_device="cuda:0", verify_batch_max=5, verify_min_gpu=1)
    a2, c, _earlier2, _batch2 = _pools(verify_device="cuda:0", verify_batch_max=5, verify_min_gpu=1)
    calls = []

    def failing(job, shares, targets, indices):
        calls.append(len(shares))
        raise RuntimeError("injected device failure")

    b.pool.verify_hasher = c.pool.verify_hasher = failing
    try:
        want = C.run_sequential(a, batch)
        assert c.pool.stats()["verify"]["enabled"] is False  # no batcher yet
        assert _submit_all(b, batch) == want
        assert len(calls) == 1 and b.pool.stats()["verify"]["device_errors"] == 1
        from otedama_amd.pool.microbatch import device_failed

        assert device_failed("cuda:0") and not device_failed("cuda:1")
        assert _submit_all(c, batch) == C.run_sequential(a2, batch) == want
        assert len(calls) == 1  # the second pool never reached the hasher
        vs = c.pool.stats()["verify"]
        assert vs["enabled"] is False and vs["device_errors"] == 0 and vs["gpu_shares"] == 0 and vs["cpu_shares"] == 11
        assert c.state() == a2.state() == a.state()
    finally:
        _close(a, b, a2, c)


def test_a_group_the_device_hasher_does_not_take_is_counted_on_the_cpu():
    from otedama_amd.pool.batch import check_shares

    a, b, _earlier, batch = _pools(verify_device="cuda:0", verify_batch_max=64, verify_min_gpu=1)
    calls = []

    class Hasher:
        def takes(self, job):  # as DeviceHasher for a job over the job block's limits
            return False

        def __call__(self, job, shares, targets, indices):
            calls.append(len(shares))
            return check_shares("sha256d", job, shares, targets, indices)

    b.pool.verify_hasher = Hasher()
    try:
        assert _submit_all(b, batch) == C.run_sequential(a, batch) and b.state() == a.state()
        vs = b.pool.stats()["verify"]
        assert calls == [] and vs["gpu_shares"] == 0 and vs["cpu_shares"] == 11 and vs["enabled"]
    finally:
        _close(a, b)


def test_an_injected_device_hasher_is_used_at_and_above_the_threshold_only():
    from otedama_amd.pool.batch import check_shares

    a, b, _earlier, batch = _pools(verify_device="cuda:0", verify_batch_max=5, verify_min_gpu=4)
    calls = []

    def device(job, shares, targets, indices):
        calls.append(len(shares))
        return check_shares("sha256d", job, shares, targets, indices)

    b.pool.verify_hasher = device
    try:
        want = C.run_sequential(a, batch)
        assert _submit_all(b, batch) == want and b.state() == a.state()
        vs = b.pool.stats()["verify"]
        # survivors per flush: 5, then 2 (the stale job and the two field rejects leave before hashing), then 4
        assert calls == [5, 4] and vs["gpu_shares"] == 9 and vs["cpu_shares"] == 2 and vs["enabled"]
    finally:
        _close(a, b)


def test_close_with_submits_pending_resolves_every_future():
    a, b, _earlier, batch = _pools(verify_device="cpu", verify_batch_max=64, verify_batch_ms=60000.0, verify_min_gpu=1)
    workers = {"rig": b.rig, "ramp": b.ramp}

    async def go():
        tasks = [asyncio.ensure_future(b.pool.validate_async(workers[w], *rest)) for w, *rest in batch]
        await asyncio.sleep(0)  # every submit is pending; the flush delay is a minute away
        assert b.pool._batcher is not None and len(b.pool._batcher._pending) == len(batch)
        assert not any(t.done() for t in tasks)
        await b.pool._batcher.close()
        await asyncio.sleep(0)
        assert all(t.done() for t in tasks)
        return [t.result() for t in tasks]

    try:
        want = C.run_sequential(a, batch)
        asyncio.set_event_loop(b.loop)
        t0 = time.perf_counter()
        got = b.loop.run_until_complete(go())
        assert time.perf_counter() - t0 < 30.0
        assert got == want and b.state() == a.state()
    finally:
        _close(a, b)


def test_feature_off_never_constructs_a_batcher(monkeypatch):
    import otedama_amd.pool.microbatch as mb

    def boom(*a, **kw):
        raise AssertionError("a batcher was constructed with the feature off")

    monkeypatch.setattr(mb, "ShareBatcher", boom)
    a, b, _earlier, batch = _pools()
    try:
        assert b.pool.opts.verify_device == ""
        want = C.run_sequential(a, batch)
        assert _submit_all(b, batch) == want and b.state() == a.state()
        assert b.pool._batcher is None
        vs = b.pool.stats()["verify"]
        assert vs == {"device": "", "enabled": False, "batches": 0, "gpu_shares": 0, "cpu_shares": 0,
                      "last_batch": 0, "max_batch": 0, "device_errors": 0}
    finally:
        _close(a, b)
