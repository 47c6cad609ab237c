"""Channel roots on a real MI355X: ``ChannelRoots.launch`` / ``roots`` (otedama_amd/ops/roots.py;
``otd_channel_roots`` of csrc/kernels/channel_roots.hip) and the pool's job fan-out on the GPU.

Every comparison is exact byte equality against the Python oracle
``merkle_root_from_branches(sha256d(coinb1 + prefix + coinb2), branches)``."""
import asyncio
import functools

import pytest

import channel_roots_cases as R
import share_verify_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID_N = 257  # a whole block and a tail of one
CANARY = 0xA5


@functools.lru_cache(maxsize=None)
def _op():
    from otedama_amd.ops.roots import ChannelRoots

    return ChannelRoots(DEV)


def _prepare(op, job):
    return op.prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, job.branches)


def _dev(raw: bytes, width: int):
    import torch

    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(-1, width).to(DEV)


def _rows(prefixes, en_size: int, fill: int = 0) -> bytes:
    """Prefix rows with ``fill`` in the bytes the kernel must ignore."""
    return b"".join(p + bytes([fill]) * (16 - en_size) for p in prefixes)


def _host(t) -> list:
    raw = t.cpu().numpy().tobytes()
    return [raw[i:i + 32] for i in range(0, len(raw), 32)]


@functools.lru_cache(maxsize=None)
def _case(k: int):
    """Job ``k`` of the reduced grid with 257 prefixes and the oracle's roots, computed once."""
    job = C.reduced_grid()[k]
    prefixes = R.make_prefixes(job, GRID_N, tag=f"g{k}")
    return job, prefixes, [R.oracle_root(job, p) for p in prefixes]


@functools.lru_cache(maxsize=None)
def _straddle_case():
    """A job whose extranonce lies across a 64-byte block boundary at byte 2 of a word, 513 prefixes."""
    job = C.make_job(62, 16, 56, 12)
    assert "straddle" in C.edge_flags(job) and "offset%4=2" in C.edge_flags(job)
    prefixes = R.make_prefixes(job, 513, tag="straddle")
    return job, prefixes, [R.oracle_root(job, p) for p in prefixes]


def test_the_grid_covers_every_edge():
    assert set().union(*(C.edge_flags(j) for j in C.reduced_grid())) >= C.ALL_EDGES


@pytest.mark.parametrize("k", range(len(C.reduced_grid())))
def test_roots_equal_the_oracle_on_the_grid(k):
    import torch

    job, prefixes, want = _case(k)
    op = _op()
    r = op.launch(_prepare(op, job), _dev(_rows(prefixes, job.en_size), 16))
    torch.cuda.synchronize()
    assert r.shape == (GRID_N, 32) and r.dtype == torch.uint8 and r.device == torch.device(DEV)
    assert _host(r) == want
    assert op.roots(_prepare(op, job), prefixes) == want


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_the_tail_guard_leaves_the_rows_after_n_alone(n):
    import torch

    job, prefixes, want = _straddle_case()
    op = _op()
    buf = torch.full((n + 3, 32), CANARY, dtype=torch.uint8, device=DEV)
    r = op.launch(_prepare(op, job), _dev(_rows(prefixes[:n], job.en_size), 16), out=buf[:n])
    torch.cuda.synchronize()
    assert r.data_ptr() == buf.data_ptr()
    assert _host(buf[:n]) == want[:n]
    assert buf[n:].cpu().numpy().tobytes() == bytes([CANARY]) * (3 * 32)


def test_garbage_after_the_prefix_does_not_change_a_root():
    import torch

    op = _op()
    for k in (0, 1, 4, 7):  # en_size 1, 4, 8 and 13
        job, prefixes, want = _case(k)
        assert job.en_size < 16
        prep = _prepare(op, job)
        for fill in (0xFF, 0x80):
            r = op.launch(prep, _dev(_rows(prefixes[:70], job.en_size, fill), 16))
            torch.cuda.synchronize()
            assert _host(r) == want[:70], (k, fill)


def test_a_32_block_tail_with_32_branches():
    import torch

    job = C.make_job(63, 8, 55, 32, extra_blocks=30)  # 63 + 8 + 48 + 64 * 30 = 2039 bytes: 32 blocks with the padding
    op = _op()
    prep = _prepare(op, job)
    assert int.from_bytes(prep.block[8:12], "little") == 32 and int.from_bytes(prep.block[16:20], "little") == 32
    prefixes = R.make_prefixes(job, 70, tag="big")
    want = [R.oracle_root(job, p) for p in prefixes]
    r = op.launch(prep, _dev(_rows(prefixes, job.en_size), 16))
    torch.cuda.synchronize()
    assert _host(r) == want
    assert op.roots(prep, prefixes) == want


def test_two_launches_back_to_back_on_another_stream():
    import torch

    job, prefixes, want = _straddle_case()
    op = _op()
    prep = _prepare(op, job)
    a, b = _dev(_rows(prefixes[:257], job.en_size), 16), _dev(_rows(prefixes[256:], job.en_size), 16)
    s = torch.cuda.Stream(DEV)
    ra = op.launch(prep, a, stream=s)
    rb = op.launch(prep, b, stream=s)
    s.synchronize()
    assert _host(ra) == want[:257] and _host(rb) == want[256:]


def test_out_given_and_not_given_and_an_empty_batch():
    import torch

    job, prefixes, want = _case(5)
    op = _op()
    prep = _prepare(op, job)
    rows = _dev(_rows(prefixes[:9], job.en_size), 16)
    out = torch.zeros((9, 32), dtype=torch.uint8, device=DEV)
    assert op.launch(prep, rows, out=out) is out
    fresh = op.launch(prep, rows)
    torch.cuda.synchronize()
    assert _host(out) == _host(fresh) == want[:9]
    r = op.launch(prep, rows[:0])
    assert r.shape == (0, 32) and r.dtype == torch.uint8 and r.device == torch.device(DEV)
    assert op.launch(prep, rows[:0], out=out[:0]).shape == (0, 32)
    assert op.roots(prep, []) == []
    # the staging buffers of roots() are pinned, reused, and grow
    assert op.roots(prep, prefixes[:3]) == want[:3]
    pin = op._staging.pin_in
    assert pin.is_pinned() and op._staging.pin_out.is_pinned()
    assert op.roots(prep, prefixes[:5]) == want[:5] and op._staging.pin_in is pin
    assert op.roots(prep, prefixes) == want
    with pytest.raises(ValueError):
        op.roots(prep, [bytes(job.en_size + 1)])


def test_launch_rejects_bad_arguments_with_nothing_enqueued():
    import torch

    from otedama_amd.ops.verify import PreparedJob

    op = _op()
    job, prefixes, _want = _case(5)
    prep = _prepare(op, job)
    rows = _dev(_rows(prefixes[:4], job.en_size), 16)
    raw = torch.zeros(4 * 32 + 16, dtype=torch.uint8, device=DEV)
    wide = torch.zeros((4, 64), dtype=torch.uint8, device=DEV)
    good_out = torch.zeros((4, 32), dtype=torch.uint8, device=DEV)
    bad_rows = [rows.to(torch.int32), rows.view(-1), rows.view(8, 8), rows.view(2, 32), rows.cpu(), wide[:, :16],
                raw[8:8 + 64].view(4, 16), rows.cpu().numpy()]
    bad_out = [raw[8:8 + 128].view(4, 32), good_out[:3], good_out.view(8, 16), wide[:, :32], good_out.cpu(),
               good_out.to(torch.int8), good_out.view(-1), good_out.cpu().numpy()]
    for r in bad_rows:
        with pytest.raises(ValueError):
            op.launch(prep, r, out=good_out)
    for o in bad_out:
        with pytest.raises(ValueError):
            op.launch(prep, rows, out=o)
    for bad_job in (PreparedJob(prep.block, prep.dev.cpu(), prep.en_size),
                    PreparedJob(prep.block, prep.dev[:-16], prep.en_size), prep.block):
        with pytest.raises(ValueError):
            op.launch(bad_job, rows, out=good_out)
    n = op.native
    okp = (prep.dev.data_ptr(), rows.data_ptr(), 4, good_out.data_ptr())
    for pos, bad in ((0, 0), (1, 0), (3, 0), (2, 0), (0, prep.dev.data_ptr() + 8), (1, raw.data_ptr() + 8),
                     (3, good_out.data_ptr() + 8)):
        args = list(okp)
        args[pos] = bad
        with pytest.raises(ValueError):
            n.launch_channel_roots(*args)
    torch.cuda.synchronize()
    assert good_out.cpu().numpy().tobytes() == bytes(128)  # nothing was written by a rejected call
    with pytest.raises(ValueError):
        type(op)("cpu")


def test_channel_roots_on_the_device_and_its_fall_back():
    from otedama_amd.pool.batch import channel_roots

    job, prefixes, want = _case(9)
    assert channel_roots(job, prefixes, DEV) == want
    assert channel_roots(job, [], DEV) == []
    over = C.make_job(41, 4, 55, 33)  # 33 branches: Python, whatever the device
    pre = R.make_prefixes(over, 3)
    assert channel_roots(over, pre, DEV) == [R.oracle_root(over, p) for p in pre]


def test_the_pool_fans_a_job_out_on_the_gpu():
    async def body():
        pool = R.seeded_pool(job_device=DEV, job_min_gpu=1)
        await pool.start()
        try:
            clients = [await R.V2Client.connect(pool) for _ in range(2)]
            jobs = {j.job_int: j for j in pool.jobs.values()}
            checked = 0
            for c in clients:
                for _ in range(4):
                    _ok, first = await c.open()
                    checked += R.check_standard_roots(jobs, c, first)
            job = pool.new_job(clean=False)
            jobs[job.job_int] = job
            received = 0
            for c in clients:
                msgs = await c.take(4)
                received += R.check_standard_roots(jobs, c, msgs)
                for m in msgs:  # the issue's statement of the same check
                    assert m.merkle_root == pool.merkle_root_for(job, c.channels[m.channel_id][0])
                c.close()
            return checked, received, pool.stats()["jobs"]
        finally:
            await pool.stop()

    checked, received, jobs = asyncio.run(asyncio.wait_for(body(), 60))
    assert (checked, received) == (8, 8)
    assert jobs["gpu_channels"] == 8 and jobs["cpu_channels"] == 0 and jobs["device_errors"] == 0
    assert (jobs["device"], jobs["enabled"], jobs["fanouts"], jobs["last_channels"]) == (DEV, True, 1, 8)
