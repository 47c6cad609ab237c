"""Live share verification on a real MI355X: ``ShareVerify.launch_results`` / ``results`` (otedama_amd/ops/verify.py;
``otd_share_headers``, the digest launches and ``otd_share_pack`` of csrc/kernels/share_verify.hip, for every
algorithm) and the pool's micro-batcher on the GPU.

Every comparison is exact byte equality against the Python oracle ``check_shares(device=None)``; the target tables
are built from the oracle's own hashes (``grid_case`` of test_share_results_cpu.py), so every outcome is there by
construction."""
import functools

import pytest

import share_verify_cases as C
from test_share_batcher_cpu import _close, _pools, _submit_all
from test_share_results_cpu import check_case_is_what_it_claims, grid_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 255, 256, 257)  # one lane, one short of a block, a whole block, a block and a tail of one


@functools.lru_cache(maxsize=None)
def _op(algorithm="sha256d", capacity=None, grid=None):
    from otedama_amd.ops.verify import ShareVerify

    return ShareVerify(algorithm, DEV, capacity=capacity, grid=grid)


def _prepare(op, job):
    return op.prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, job.branches)


def _dev(raw: bytes, width: int):
    import torch

    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(-1, width).to(DEV)


def _records(raw: bytes) -> list:
    """128-byte records -> (header, hash, verdict), with the pad bytes checked to be zero."""
    assert len(raw) % 128 == 0
    out = []
    for i in range(0, len(raw), 128):
        assert raw[i + 113:i + 128] == bytes(15), i // 128
        out.append((raw[i:i + 80], raw[i + 80:i + 112], raw[i + 112]))
    return out


def _launch_results(op, job, shares, targets, indices, **kw) -> list:
    import torch

    from otedama_amd.ops.verify import pack_records

    r = op.launch_results(_prepare(op, job), _dev(pack_records(shares, indices, job.en_size), 32),
                          _dev(b"".join(targets), 32), **kw)
    torch.cuda.synchronize()
    assert r.shape == (len(shares), 128) and r.dtype == torch.uint8
    return _records(r.cpu().numpy().tobytes())


@functools.lru_cache(maxsize=None)
def _sized_case(k: int):
    """Job ``k`` of the grid with 257 shares: the 34 of ``grid_case`` (ties, word pairs, bad indices), then distinct
    shares cycling through its table. The oracle is computed once."""
    from otedama_amd.pool.batch import check_shares

    job, shares, targets, indices, want = grid_case(k)
    more = C.make_shares(job, max(SIZES) - len(shares), tag=f"fill{k}")
    more_idx = [i % len(targets) for i in range(len(more))]
    return (job, shares + more, targets, indices + more_idx,
            want + check_shares("sha256d", job, more, targets, more_idx))


@pytest.mark.parametrize("k", range(len(C.reduced_grid())))
def test_sha256d_records_equal_the_oracle_and_the_three_launch_path(k):
    import torch

    from otedama_amd.ops.verify import pack_records

    job, shares, targets, indices, want = _sized_case(k)
    check_case_is_what_it_claims(want)
    op = _op()
    for n in SIZES:
        got = _launch_results(op, job, shares[:n], targets, indices[:n])
        for i, (g, w) in enumerate(zip(got, want[:n])):
            assert g == w, (k, n, i)
        assert len(got) == n
    # the same inputs through ShareVerify.launch: header, digest and verdict
    v, d, h = op.launch(_prepare(op, job), _dev(pack_records(shares, indices, job.en_size), 32),
                        _dev(b"".join(targets), 32))
    torch.cuda.synchronize()
    vb, db, hb = (t.cpu().numpy().tobytes() for t in (v, d, h))
    assert [(hb[80 * i:80 * i + 80], db[32 * i:32 * i + 32], vb[i]) for i in range(len(shares))] == got


def test_extranonce_bytes_past_en_size_are_ignored():
    import torch

    from otedama_amd.ops.verify import pack_records
    from otedama_amd.pool.batch import check_shares

    job = C.make_job(55, 13, 56, 1)
    shares = C.make_shares(job, 65)
    rec = bytearray(pack_records(shares, [0] * 65, job.en_size))
    for i in range(65):
        rec[32 * i + 13:32 * i + 16] = b"\xff\xa5\x5a"
    op = _op()
    r = op.launch_results(_prepare(op, job), _dev(bytes(rec), 32), _dev(bytes(31) + b"\x40", 32))
    torch.cuda.synchronize()
    assert _records(r.cpu().numpy().tobytes()) == check_shares("sha256d", job, shares, [bytes(31) + b"\x40"], [0] * 65)


@pytest.mark.parametrize("algorithm,kw", [("sha256d", {}), ("x11", {"capacity": 256})])
def test_no_store_past_the_last_record(algorithm, kw):
    import torch

    from otedama_amd.ops.verify import pack_records

    job, shares, targets, indices, want = _sized_case(4)
    op = _op(algorithm, **kw)
    prep = _prepare(op, job)
    for n in (1, 257):
        buf = torch.full((n + 1, 128), 0xA5, dtype=torch.uint8, device=DEV)
        r = op.launch_results(prep, _dev(pack_records(shares[:n], indices[:n], job.en_size), 32),
                              _dev(b"".join(targets), 32), out=buf[:n])
        torch.cuda.synchronize()
        assert r.data_ptr() == buf.data_ptr()
        raw = buf.cpu().numpy().tobytes()
        assert raw[128 * n:] == b"\xa5" * 128, n
        if algorithm == "sha256d":
            assert _records(raw[:128 * n]) == want[:n]
        else:
            assert [x[0] for x in _records(raw[:128 * n])] == [x[0] for x in want[:n]]


@pytest.mark.parametrize("algorithm,n,kw", [("scrypt", 65, {"grid": 2}), ("x11", 33, {"capacity": 256})])
def test_chain_and_pack_equal_the_oracle(algorithm, n, kw):
    from otedama_amd.models.header import hash_to_int, int_to_hash
    from otedama_amd.pool.batch import check_shares

    op = _op(algorithm, **kw)
    job = C.make_job(119, 13, 63, 12)
    shares = C.make_shares(job, n, tag="pack")
    probe = check_shares(algorithm, job, shares, [b"\xff" * 32], [0] * n)
    hv = sorted(hash_to_int(x[1]) for x in probe)
    # the median, a tie with the smallest hash, everything, nothing; the last share points past the table
    targets = [int_to_hash(hv[n // 2]), int_to_hash(hv[0]), b"\xff" * 32, bytes(32)]
    indices = [i % 4 for i in range(n - 1)] + [4]
    want = check_shares(algorithm, job, shares, targets, indices)
    assert want[-1][2] == 0x80 and {x[2] & 1 for x in want[:-1]} == {0, 1}
    assert _launch_results(op, job, shares, targets, indices) == want
    assert op.results(_prepare(op, job), shares, targets, indices) == want
    assert op.results(_prepare(op, job), shares[:3], targets, indices[:3]) == want[:3]  # the buffers are reused


def test_results_equals_the_oracle_and_reuses_its_buffers():
    op = _op()
    for k in (11, 3):  # a small batch, then a larger one: the staging buffers grow
        job, shares, targets, indices, want = _sized_case(k)
        prep = _prepare(op, job)
        assert op.results(prep, shares[:34], targets, indices[:34]) == want[:34]
        assert op.results(prep, shares, targets, indices) == want
        assert op.results(prep, shares[:1], targets[:1], None) == want[:1]
    assert op.results(prep, [], targets) == []
    pin = op._staging.pin_in
    assert pin.is_pinned() and op._staging.pin_out.is_pinned()
    job, shares, targets, indices, want = _sized_case(0)
    assert op.results(_prepare(op, job), shares[:5], targets, indices[:5]) == want[:5]
    assert op._staging.pin_in is pin  # no new staging buffer for a batch that fits
    with pytest.raises(ValueError):
        op.results(prep, shares[:1], [], [0])


def test_launch_results_rejects_bad_arguments_and_takes_an_empty_batch():
    import torch

    from otedama_amd.ops.verify import PreparedJob, pack_records

    op = _op()
    job = C.pool_job(n_txs=7)
    prep = _prepare(op, job)
    recs = _dev(pack_records(C.make_shares(job, 4), [0] * 4, 8), 32)
    tgts = _dev(b"\xff" * 64, 32)
    raw = torch.zeros(4 * 128 + 16, dtype=torch.uint8, device=DEV)
    wide = torch.zeros((4, 256), dtype=torch.uint8, device=DEV)
    bad_records = [recs.to(torch.int32), recs.view(-1), recs.view(8, 16), recs.cpu(), wide[:, :32],
                   raw[8:8 + 128].view(4, 32), recs.cpu().numpy()]
    bad_targets = [tgts.to(torch.int8), tgts.view(-1), tgts.view(4, 16), tgts.cpu(), wide[:2, :32],
                   raw[8:8 + 64].view(2, 32), tgts[:0]]
    good_out = torch.zeros((4, 128), dtype=torch.uint8, device=DEV)
    bad_out = [raw[8:8 + 512].view(4, 128), good_out[:3], good_out.view(8, 64), wide[:, :128], good_out.cpu(),
               good_out.to(torch.int8), good_out.view(-1), good_out.cpu().numpy()]
    for r in bad_records:
        with pytest.raises(ValueError):
            op.launch_results(prep, r, tgts)
    for t in bad_targets:
        with pytest.raises(ValueError):
            op.launch_results(prep, recs, t)
    for o in bad_out:
        with pytest.raises(ValueError):
            op.launch_results(prep, recs, tgts, out=o)
    with pytest.raises(ValueError):
        op.launch_results(PreparedJob(prep.block, prep.dev.cpu(), prep.en_size), recs, tgts)
    with pytest.raises(ValueError):
        op.launch_results(PreparedJob(prep.block, prep.dev[:-16], prep.en_size), recs, tgts)
    with pytest.raises(ValueError):
        op.launch_results(prep.block, recs, tgts)
    with pytest.raises(ValueError):
        op.launch_results(prep, recs[:0], tgts[:0])  # an empty table is an error even for an empty batch
    torch.cuda.synchronize()
    assert good_out.cpu().numpy().tobytes() == bytes(512)  # nothing was written by a rejected call
    r = op.launch_results(prep, recs[:0], tgts)
    assert r.shape == (0, 128) and r.device == torch.device(DEV)
    assert op.launch_results(prep, recs[:0], tgts, out=good_out[:0]).shape == (0, 128)
    assert op.results(prep, [], [b"\xff" * 32]) == []
    n = op.native
    okp = (prep.dev.data_ptr(), recs.data_ptr(), raw.data_ptr(), raw.data_ptr(), tgts.data_ptr(), 2, 4,
           good_out.data_ptr())
    for pos, bad in ((0, 0), (2, 0), (3, 0), (7, 0), (5, 0), (6, 0), (2, raw.data_ptr() + 8),
                     (7, good_out.data_ptr() + 8)):
        args = list(okp)
        args[pos] = bad
        with pytest.raises(ValueError):
            n.launch_share_pack(*args)
    torch.cuda.synchronize()
    assert good_out.cpu().numpy().tobytes() == bytes(512)


def test_an_empty_batch_enqueues_nothing():
    """launch_results returns the empty tensor before it looks at a stream: the side stream stays idle."""
    import torch

    op = _op()
    prep = _prepare(op, C.pool_job(n_txs=7))
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    r = op.launch_results(prep, torch.empty((0, 32), dtype=torch.uint8, device=DEV), _dev(b"\xff" * 32, 32),
                          stream=side)
    assert r.shape == (0, 128) and side.query()


def test_launch_results_on_a_side_stream_matches():
    import torch

    from otedama_amd.ops.verify import pack_records

    job, shares, targets, indices, want = _sized_case(7)
    for op in (_op(), _op("x11", capacity=256)):
        ref = _launch_results(op, job, shares[:65], targets, indices[:65])
        side = torch.cuda.Stream(DEV)
        r = op.launch_results(_prepare(op, job), _dev(pack_records(shares[:65], indices[:65], job.en_size), 32),
                              _dev(b"".join(targets), 32), stream=side)
        side.synchronize()
        assert _records(r.cpu().numpy().tobytes()) == ref
        # and back on the current stream: the op waits for its previous launch's stream
        assert _launch_results(op, job, shares[:65], targets, indices[:65]) == ref
    assert _launch_results(_op(), job, shares[:65], targets, indices[:65]) == want[:65]


@functools.lru_cache(maxsize=None)
def _oracle(algorithm: str):
    from otedama_amd.pool.batch import check_shares

    job, shares, targets, indices, want = _sized_case(7)
    return want if algorithm == "sha256d" else check_shares(algorithm, job, shares, targets, indices)


@pytest.mark.parametrize("algorithm,kw", [("sha256d", {}), ("x11", {"capacity": 256})])
def test_launch_and_launch_results_interleaved_on_one_op(algorithm, kw):
    """Both entries share the op's headers buffer and ``_last_stream``: alternate them across two streams on a fresh
    op, with a batch that outgrows the buffer while the side stream's launch was the last to use it."""
    import torch

    from otedama_amd.ops.verify import ShareVerify, pack_records

    job, shares, targets, indices, _ = _sized_case(7)
    want = _oracle(algorithm)
    op = ShareVerify(algorithm, DEV, **kw)
    prep = _prepare(op, job)
    tgts = _dev(b"".join(targets), 32)
    side = torch.cuda.Stream(DEV)
    cur = torch.cuda.current_stream(DEV)

    def packed(n):
        return _dev(pack_records(shares[:n], indices[:n], job.en_size), 32)

    def launch_results(n, stream):
        r = op.launch_results(prep, packed(n), tgts, stream=stream)
        (stream or cur).synchronize()
        assert _records(r.cpu().numpy().tobytes()) == want[:n], n

    def launch(n, stream):
        v, d, h = op.launch(prep, packed(n), tgts, stream=stream)
        (stream or cur).synchronize()
        assert h.data_ptr() == op.headers.data_ptr() and h.shape == (n, 80)
        vb, db, hb = (t.cpu().numpy().tobytes() for t in (v, d, h))
        assert [(hb[80 * i:80 * i + 80], db[32 * i:32 * i + 32], vb[i]) for i in range(n)] == want[:n], n

    launch_results(65, side)
    assert op.headers.shape[0] == 65 and op._last_stream == side
    launch(257, None)  # the headers buffer grows while the side stream's launch was its last user
    assert op.headers.shape[0] == 257 and op._last_stream == cur
    launch_results(1, None)
    launch(64, side)
    assert op.headers.shape[0] == 257 and op._last_stream == side


@pytest.mark.parametrize("min_gpu,gpu_shares", [(1, 11), (64, 0)])
def test_pool_batcher_on_the_gpu_equals_sequential_cpu_validation(min_gpu, gpu_shares):
    a, b, _earlier, batch = _pools(verify_device=DEV, verify_batch_max=5, verify_min_gpu=min_gpu)
    try:
        want = C.run_sequential(a, batch)
        got = _submit_all(b, batch)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, i
        assert len(got) == 14 and sum(v.accepted for v in got) >= 6 and any(v.block for v in got)
        assert b.state() == a.state()
        vs = b.pool.stats()["verify"]
        assert vs["device"] == DEV and vs["enabled"] and vs["device_errors"] == 0 and vs["batches"] == 3
        assert vs["gpu_shares"] == gpu_shares and vs["cpu_shares"] == 11 - gpu_shares
    finally:
        _close(a, b)
