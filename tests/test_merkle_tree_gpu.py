"""The template tree on a real MI355X: ``MerkleTree.launch`` / ``tree`` (otedama_amd/ops/merkle.py; ``otd_merkle_tree``
of csrc/kernels/merkle_tree.hip), ``template_tree`` on the device and the pool's template path on the GPU.

Every comparison is exact byte equality against the Python oracle ``merkle_branches`` / ``merkle_root_full``."""
import asyncio
import functools

import pytest

import channel_roots_cases as R
import merkle_tree_cases as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5


@functools.lru_cache(maxsize=None)
def _op():
    from otedama_amd.ops.merkle import MerkleTree

    return MerkleTree(DEV)


def _dev(raw: bytes, t: int, n: int):
    import torch

    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(t, n, 32).to(DEV)


def _host(rows, t: int, n: int) -> list:
    return T.rows_of(rows.cpu().numpy().tobytes(), t, n)


@pytest.mark.parametrize("n", T.SIZES)
def test_launch_and_tree_equal_the_oracle(n):
    import torch

    op = _op()
    one = op.launch(_dev(T.packed(n), 1, n))
    two = op.launch(_dev(T.packed(n, (0, 1)), 2, n))  # two trees of different leaves
    torch.cuda.synchronize()
    assert one.shape == (1, 1 + T.depth(n), 32) and one.dtype == torch.uint8 and one.device == torch.device(DEV)
    assert two.shape == (2, 1 + T.depth(n), 32)
    assert _host(one, 1, n) == [T.oracle(n)]
    assert _host(two, 2, n) == [T.oracle(n, 0), T.oracle(n, 1)]
    assert op.tree([T.leaves(n)]) == [T.oracle(n)]
    assert op.tree([T.leaves(n, 1), T.leaves(n, 0)]) == [T.oracle(n, 1), T.oracle(n, 0)]


@pytest.mark.parametrize("n", [1, 2, 257, 513, 1025])
def test_the_rows_after_out_and_after_the_leaves_stay_untouched(n):
    import torch

    op = _op()
    rows = 1 + T.depth(n)
    for t, trees in ((1, (0,)), (2, (0, 1))):
        # the leaves end exactly where canary rows begin: a read past node n would fold them in
        src = torch.full((t * n + 4, 32), CANARY, dtype=torch.uint8, device=DEV)
        src[:t * n] = _dev(T.packed(n, trees), t, n).view(t * n, 32)
        buf = torch.full((t * rows + 4, 32), CANARY, dtype=torch.uint8, device=DEV)
        out = buf[:t * rows].view(t, rows, 32)
        r = op.launch(src[:t * n].view(t, n, 32), out=out)
        torch.cuda.synchronize()
        assert r.data_ptr() == buf.data_ptr()
        assert _host(out, t, n) == [T.oracle(n, y) for y in trees]
        assert buf[t * rows:].cpu().numpy().tobytes() == bytes([CANARY]) * (4 * 32)
        assert src[t * n:].cpu().numpy().tobytes() == bytes([CANARY]) * (4 * 32)
        assert src[:t * n].cpu().numpy().tobytes() == T.packed(n, trees)  # the leaves themselves are only read


def test_out_given_and_not_given_and_the_staging_buffers():
    import torch

    op = _op()
    n = 9
    leaves = _dev(T.packed(n), 1, n)
    out = torch.zeros((1, 1 + T.depth(n), 32), dtype=torch.uint8, device=DEV)
    assert op.launch(leaves, out=out) is out
    fresh = op.launch(leaves)
    torch.cuda.synchronize()
    assert _host(out, 1, n) == _host(fresh, 1, n) == [T.oracle(n)]
    # the staging buffers of tree() are pinned, reused, and grow (a fresh op: the shared one has seen 262144 leaves)
    op = type(op)(DEV)
    assert op.tree([T.leaves(3)]) == [T.oracle(3)]
    pin = op._staging.pin_in
    assert pin.is_pinned() and op._staging.pin_out.is_pinned()
    assert op.tree([T.leaves(5)]) == [T.oracle(5)] and op._staging.pin_in is pin
    assert op.tree([T.leaves(4001)]) == [T.oracle(4001)]
    assert op._staging.pin_in is not pin and op._staging.pin_in.numel() >= 4001 * 32
    assert op.tree([T.leaves(3)]) == [T.oracle(3)]  # a small call after a large one
    for bad in ([], [[]], [T.leaves(3), T.leaves(4)], [[bytes(31)]], [[bytes(32), bytes(33)]]):
        with pytest.raises(ValueError):
            op.tree(bad)


def test_two_launches_back_to_back_on_another_stream():
    import torch

    op = _op()
    a, b = _dev(T.packed(1025, (0, 1)), 2, 1025), _dev(T.packed(513), 1, 513)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    ra = op.launch(a, stream=s)
    rb = op.launch(b, stream=s)
    s.synchronize()
    assert _host(ra, 2, 1025) == [T.oracle(1025, 0), T.oracle(1025, 1)]
    assert _host(rb, 1, 513) == [T.oracle(513)]


def test_launch_rejects_bad_arguments_with_nothing_enqueued():
    import torch

    op = _op()
    n, rows = 5, 1 + T.depth(5)
    leaves = _dev(T.packed(n), 1, n)
    raw = torch.zeros(n * 32 + 16, dtype=torch.uint8, device=DEV)
    wide = torch.zeros((1, n, 64), dtype=torch.uint8, device=DEV)
    good_out = torch.zeros((1, rows, 32), dtype=torch.uint8, device=DEV)
    bad_leaves = [leaves.to(torch.int32), leaves.view(-1), leaves.view(n, 32), leaves.view(1, n * 2, 16), leaves.cpu(),
                  wide[:, :, :32], raw[8:8 + n * 32].view(1, n, 32), leaves.cpu().numpy(),
                  leaves[:, :0],                                                       # n = 0
                  leaves[:0]]                                                          # t = 0
    bad_out = [raw[8:8 + rows * 32].view(1, rows, 32), good_out[:, :rows - 1], good_out.view(rows, 32),
               good_out.cpu(), good_out.to(torch.int8), good_out.view(-1), good_out.cpu().numpy(),
               torch.zeros((2, rows, 32), dtype=torch.uint8, device=DEV)]
    for x in bad_leaves:
        with pytest.raises(ValueError):
            op.launch(x, out=good_out)
        with pytest.raises(ValueError):
            op.launch(x)
    for o in bad_out:
        with pytest.raises(ValueError):
            op.launch(leaves, out=o)
    # n over the limit: a view with stride 0 stands for 262145 leaves without their memory; it is not contiguous,
    # so the size check is asked through the raw binding below as well
    with pytest.raises(ValueError):
        op.launch(leaves[:, :1].expand(1, T.LIMIT + 1, 32), out=good_out)
    nat = op.native
    scratch = torch.zeros((4, 32), dtype=torch.uint8, device=DEV)
    ok = (leaves.data_ptr(), 1, n, scratch.data_ptr(), good_out.data_ptr())
    for pos, bad in ((0, 0), (4, 0), (1, 0), (2, 0), (2, T.LIMIT + 1), (1, nat.MERKLE_TREE_MAX_TREES + 1),
                     (0, leaves.data_ptr() + 8), (3, scratch.data_ptr() + 8), (4, good_out.data_ptr() + 8)):
        args = list(ok)
        args[pos] = bad
        with pytest.raises(ValueError):
            nat.launch_merkle_tree(*args)
    with pytest.raises(ValueError):  # more than one chunk needs the scratch rows
        nat.launch_merkle_tree(leaves.data_ptr(), 1, 513, 0, good_out.data_ptr())
    torch.cuda.synchronize()
    assert good_out.cpu().numpy().tobytes() == bytes(rows * 32)  # nothing was written by a rejected call
    with pytest.raises(ValueError):
        type(op)("cpu")


def test_template_tree_on_the_device_equals_the_oracle():
    from otedama_amd.pool.batch import template_tree
    from otedama_amd.pool.template import merkle_root_from_branches, merkle_root_full

    for n in (1, 2, 8, 513, 4001):
        txids, wtxids = list(T.leaves(n, 0)[1:]), list(T.leaves(n, 1)[1:])
        want_root = merkle_root_full([bytes(32)] + wtxids) if wtxids else None
        assert template_tree(txids, wtxids, DEV) == (T.oracle(n, 0)[1], want_root), n
        assert template_tree(txids, [], DEV) == (T.oracle(n, 0)[1], None), n
    coinbase_txid, others, root = T.block_100000()
    branches, witness_root = template_tree(others, [], DEV)
    assert witness_root is None and merkle_root_from_branches(coinbase_txid, branches) == root
    assert _op().tree([[coinbase_txid] + others])[0][0] == root


def test_the_pool_computes_its_template_tree_on_the_gpu():
    from otedama_amd.pool.template import merkle_branches

    async def body():
        pool = R.seeded_pool(n_txs=600, template_device=DEV, template_min_gpu=1)
        await pool.start()
        try:
            c = await R.V2Client.connect(pool)
            _ok, first = await c.open(extended=True)
            job = next(iter(pool.jobs.values()))
            sent = [m for m in first if hasattr(m, "merkle_path")]
            c.close()
            return job.branches, pool.block.txids, [list(m.merkle_path) for m in sent], pool.stats()["template"]
        finally:
            await pool.stop()

    branches, txids, sent, st = asyncio.run(asyncio.wait_for(body(), 60))
    want = merkle_branches(txids)
    assert len(txids) == 600 and branches == want
    assert sent and all(path == want for path in sent)  # the branches on the wire are the oracle's
    assert st["gpu_leaves"] == 601 and st["cpu_leaves"] == 0 and st["device_errors"] == 0
    assert (st["device"], st["enabled"], st["trees"], st["last_leaves"]) == (DEV, True, 1, 601)
