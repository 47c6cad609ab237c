"""Share verification op (otedama_amd/ops/verify.py, csrc/kernels/share_verify.hip) on a real MI355X.

Every comparison is exact byte equality against the Python oracle, ``check_shares(device=None)`` or its parts
(share_verify_cases.py). The target tables of the verdict tests are built from the oracle's own hashes, so every
outcome is there by construction."""
import functools

import pytest

import share_verify_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 63, 64, 65, 257)  # wave edge, block edge and tail


@functools.lru_cache(maxsize=None)
def _op(algorithm="sha256d", capacity=None, grid=None):
    from otedama_amd.ops.verify import ShareVerify

    return ShareVerify(algorithm, DEV, capacity=capacity, grid=grid)


def _prepare(op, job):
    return op.prepare(job.coinb1, job.coinb2, job.en_size, job.prev_hash, job.nbits, job.branches)


def _dev(raw: bytes, width: int):
    import torch

    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(-1, width).to(DEV)


def _launch(op, job, shares, targets, indices):
    """One launch, synchronised: (verdict list, digest list, header list)."""
    import torch

    from otedama_amd.ops.verify import pack_records

    v, d, h = op.launch(_prepare(op, job), _dev(pack_records(shares, indices, job.en_size), 32),
                        _dev(b"".join(targets), 32))
    torch.cuda.synchronize()
    n = len(shares)
    assert v.shape == (n,) and d.shape == (n, 32) and h.shape == (n, 80)
    db, hb = d.cpu().numpy().tobytes(), h.cpu().numpy().tobytes()
    return (list(v.cpu().numpy().tobytes()), [db[32 * i:32 * i + 32] for i in range(n)],
            [hb[80 * i:80 * i + 80] for i in range(n)])


_JOBS = C.reduced_grid() + [C.pool_job(n_txs=7)]


@pytest.mark.parametrize("k", range(len(_JOBS)))
def test_headers_equal_the_oracle(k):
    job = _JOBS[k]
    shares = C.make_shares(job, max(SIZES))
    want = C.oracle_headers(job, shares)
    for n in SIZES:
        _v, _d, got = _launch(_op(), job, shares[:n], [b"\xff" * 32], [0] * n)
        assert got == want[:n], (k, n)


def test_extranonce_bytes_past_en_size_are_ignored():
    import torch

    from otedama_amd.ops.verify import pack_records

    job = C.make_job(55, 13, 56, 1)
    shares = C.make_shares(job, 65)
    rec = bytearray(pack_records(shares, [0] * 65, job.en_size))
    for i in range(65):
        rec[32 * i + 13:32 * i + 16] = b"\xff\xa5\x5a"
    op = _op()
    _v, _d, h = op.launch(_prepare(op, job), _dev(bytes(rec), 32), _dev(b"\xff" * 32, 32))
    torch.cuda.synchronize()
    assert h.cpu().numpy().tobytes() == b"".join(C.oracle_headers(job, shares))


def _verdict_case():
    """(job, shares, targets, indices): the table and the network target come from the oracle's own hashes."""
    from otedama_amd.models.header import hash_to_int, int_to_hash, nbits_from_target
    from otedama_amd.pool.batch import ShareJob, check_shares

    base = C.pool_job(n_txs=7)
    shares = C.make_shares(base, 257, tag="verdict")
    probe = sorted(hash_to_int(h) for _hdr, h, _v in check_shares("sha256d", base, shares, [b"\xff" * 32], [0] * 257))
    nbits = nbits_from_target(int_to_hash(probe[128]))  # about the median: both network outcomes occur
    job = ShareJob(base.coinb1, base.coinb2, base.en_size, base.prev_hash, nbits, base.branches)
    hv = [hash_to_int(h) for _hdr, h, _v in check_shares("sha256d", job, shares, [b"\xff" * 32], [0] * 257)]
    w0 = lambda x, d: (x & ~0xFFFFFFFF) | ((x + d) & 0xFFFFFFFF)  # noqa: E731 - differs in the lowest word only
    w7 = lambda x, d: (x + (d << 224)) % (1 << 256)               # noqa: E731 - differs in the highest word only
    assert 0 < hv[3] & 0xFFFFFFFF < 0xFFFFFFFF and 0 < hv[4] >> 224 < 0xFFFFFFFF
    table = [sorted(hv)[128], hv[0], hv[1] - 1, hv[2] + 1, (1 << 256) - 1, 0,
             w0(hv[3], 1), w0(hv[3], -1), w7(hv[4], 1), w7(hv[4], -1)]
    targets = [int_to_hash(t) for t in table]
    # shares 0..2 meet their own entries; every other share cycles through the table; then the word pairs, and
    # indices just past the table and far past it
    indices = [1, 2, 3] + [i % len(table) for i in range(3, 257)]
    extra = [(3, 6), (3, 7), (4, 8), (4, 9), (5, len(table)), (6, 0xFFFFFFFF), (7, 1 << 31)]
    all_shares = shares + [shares[s] for s, _t in extra]
    indices += [t for _s, t in extra]
    return job, all_shares, targets, indices


def test_verdicts_equal_the_oracle_on_a_table_built_from_its_hashes():
    from otedama_amd.pool.batch import check_shares

    job, shares, targets, indices = _verdict_case()
    want = check_shares("sha256d", job, shares, targets, indices)
    v, d, h = _launch(_op(), job, shares, targets, indices)
    assert h == [x[0] for x in want] and d == [x[1] for x in want]
    assert v == [x[2] for x in want]
    # the cases are what they claim to be
    assert v[0] & 1 and not v[1] & 1 and v[2] & 1              # a tie accepts; one under rejects; one over accepts
    assert [x & 1 for x in v[257:261]] == [1, 0, 1, 0]          # lowest-word and highest-word pairs
    assert v[261:264] == [0x80, 0x80, 0x80]                     # the guard: index t, 2^32 - 1 and 2^31
    assert {x >> 1 for x in v[:257]} == {0, 1}                  # both network outcomes
    cyc = [(i, x) for i, x in enumerate(v[3:257], 3)]
    assert all(x & 1 for i, x in cyc if i % 10 == 4) and not any(x & 1 for i, x in cyc if i % 10 == 5)
    assert {x & 1 for i, x in cyc if i % 10 == 0} == {0, 1}     # the median splits


@pytest.mark.parametrize("algorithm,n,kw", [("sha256d", 257, {}), ("scrypt", 65, {"grid": 2}),
                                            ("x11", 65, {"capacity": 256})])
def test_end_to_end_equals_check_shares(algorithm, n, kw):
    from otedama_amd.models.header import hash_to_int, int_to_hash
    from otedama_amd.pool.batch import check_shares

    op = _op(algorithm, **kw)
    for round_, job in enumerate((C.pool_job(n_txs=7), C.make_job(119, 13, 63, 12))):  # the second reuses the buffers
        shares = C.make_shares(job, n, tag=f"e2e{round_}")
        probe = check_shares(algorithm, job, shares, [b"\xff" * 32], [0] * n)
        hv = sorted(hash_to_int(x[1]) for x in probe)
        targets = [int_to_hash(hv[n // 2]), int_to_hash(hv[0]), b"\xff" * 32, bytes(32)]
        indices = [i % 4 for i in range(n - 1)] + [4]
        want = check_shares(algorithm, job, shares, targets, indices)
        v, d, h = _launch(op, job, shares, targets, indices)
        assert h == [x[0] for x in want]
        assert d == [x[1] for x in want]
        assert v == [x[2] for x in want] and v[-1] == 0x80 and {x & 1 for x in v[:-1]} == {0, 1}


def test_check_shares_on_the_device_equals_the_oracle():
    from otedama_amd.pool.batch import ShareJob, check_shares

    job = C.pool_job(n_txs=7)
    shares = C.make_shares(job, 70, tag="cs")
    targets, indices = [bytes(31) + b"\x40", b"\xff" * 32], [i % 3 for i in range(70)]
    assert check_shares("sha256d", job, shares, targets, indices, device=DEV) == \
        check_shares("sha256d", job, shares, targets, indices)
    assert check_shares("sha256d", job, [], targets, [], device=DEV) == []
    # over the block's limits (33 branches): the oracle path, not an error
    big = ShareJob(job.coinb1, job.coinb2, 8, job.prev_hash, job.nbits, [bytes(32)] * 33)
    assert check_shares("sha256d", big, shares[:3], targets, [0, 1, 2], device=DEV) == \
        check_shares("sha256d", big, shares[:3], targets, [0, 1, 2])


def test_launch_rejects_bad_arguments_and_takes_an_empty_batch():
    import torch

    from otedama_amd.ops.verify import PreparedJob, pack_records

    op = _op()
    job = C.pool_job(n_txs=7)
    prep = _prepare(op, job)
    recs = _dev(pack_records(C.make_shares(job, 4), [0] * 4, 8), 32)
    tgts = _dev(b"\xff" * 64, 32)
    raw = torch.zeros(4 * 32 + 16, dtype=torch.uint8, device=DEV)
    wide = torch.zeros((4, 64), dtype=torch.uint8, device=DEV)
    bad_records = [recs.to(torch.int32), recs.view(-1), recs.view(8, 16), recs.cpu(), wide[:, :32],
                   raw[8:8 + 128].view(4, 32), recs.cpu().numpy()]
    bad_targets = [tgts.to(torch.int8), tgts.view(-1), tgts.view(4, 16), tgts.cpu(), wide[:2, :32],
                   raw[8:8 + 64].view(2, 32), tgts[:0]]
    for r in bad_records:
        with pytest.raises(ValueError):
            op.launch(prep, r, tgts)
    for t in bad_targets:
        with pytest.raises(ValueError):
            op.launch(prep, recs, t)
    with pytest.raises(ValueError):
        op.launch(PreparedJob(prep.block, prep.dev.cpu(), prep.en_size), recs, tgts)  # prepared for another device
    with pytest.raises(ValueError):
        op.launch(PreparedJob(prep.block, prep.dev[:-16], prep.en_size), recs, tgts)
    with pytest.raises(ValueError):
        op.launch(prep.block, recs, tgts)
    with pytest.raises(ValueError):
        op.launch(prep, recs[:0], tgts[:0])  # an empty table is an error even for an empty batch
    with pytest.raises(ValueError):
        op.prepare(job.coinb1, job.coinb2, 17, job.prev_hash, job.nbits, job.branches)
    v, d, h = op.launch(prep, recs[:0], tgts)
    assert v.shape == (0,) and d.shape == (0, 32) and h.shape == (0, 80)
    assert op.verify(prep, [], [b"\xff" * 32]) == ([], [], [])
    n = op.native
    for args in ((0, recs.data_ptr(), 4, raw.data_ptr()), (prep.dev.data_ptr(), 0, 4, raw.data_ptr()),
                 (prep.dev.data_ptr(), recs.data_ptr(), 0, raw.data_ptr()),
                 (prep.dev.data_ptr(), recs.data_ptr() + 8, 4, raw.data_ptr())):
        with pytest.raises(ValueError):
            n.launch_share_headers(*args)
    torch.cuda.synchronize()


def test_launch_on_a_side_stream_matches():
    import torch

    from otedama_amd.ops.verify import pack_records

    op = _op()
    job = C.make_job(63, 8, 0, 12)
    shares = C.make_shares(job, 65, tag="side")
    side = torch.cuda.Stream(DEV)
    v, d, h = op.launch(_prepare(op, job), _dev(pack_records(shares, [0] * 65, 8), 32), _dev(b"\xff" * 32, 32),
                        stream=side)
    side.synchronize()
    assert h.cpu().numpy().tobytes() == b"".join(C.oracle_headers(job, shares))
    assert set(v.cpu().numpy().tobytes()) <= {1, 3}
    # and back on the current stream: the op waits for its previous launch's stream
    _v, _d, h2 = _launch(op, job, shares, [b"\xff" * 32], [0] * 65)
    assert h2 == C.oracle_headers(job, shares)


def test_validate_many_on_the_device_equals_the_cpu_path():
    tmpl = C.script_template()
    cpu, gpu = C.ScriptedPool(tmpl), C.ScriptedPool(tmpl)
    try:
        earlier, batch = C.build_script(cpu)
        assert C.run_sequential(cpu, earlier) == C.run_sequential(gpu, earlier)
        want = C.run_batched(cpu, batch, device=None)
        got = C.run_batched(gpu, batch, device=DEV)
        assert got == want and sum(v.accepted for v in got) >= 6 and any(v.block for v in got)
        assert gpu.state() == cpu.state()
    finally:
        cpu.close()
        gpu.close()
