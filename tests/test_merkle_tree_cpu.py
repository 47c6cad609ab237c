"""The template tree without a GPU: the native ``merkle_tree_cpu`` and ``pool.batch.template_tree(device="cpu")``
against the oracle ``merkle_branches`` / ``merkle_root_full`` (exact byte equality), block 100000, the limits, the
over-limit fall-back to Python, and the torch-free imports."""
import subprocess
import sys

import pytest

import merkle_tree_cases as T
from otedama_amd.models.header import sha256d
from otedama_amd.ops.native import require_native
from otedama_amd.pool import batch
from otedama_amd.pool.batch import template_tree
from otedama_amd.pool.template import merkle_branches, merkle_root_from_branches, merkle_root_full

N = require_native()


@pytest.mark.parametrize("n", T.SIZES)
def test_merkle_tree_cpu_equals_the_oracle(n):
    assert T.rows_of(N.merkle_tree_cpu(T.packed(n), 1, n), 1, n) == [T.oracle(n)]
    # two trees of different leaves in one call
    assert T.rows_of(N.merkle_tree_cpu(T.packed(n, (0, 1)), 2, n), 2, n) == [T.oracle(n, 0), T.oracle(n, 1)]


@pytest.mark.parametrize("n", T.SIZES)
def test_template_tree_on_the_cpu_equals_the_oracle(n):
    txids, wtxids = list(T.leaves(n, 0)[1:]), list(T.leaves(n, 1)[1:])
    want_branches = T.oracle(n, 0)[1]  # merkle_branches(txids): the path never depends on leaf 0
    # t = 1: no wtxids, no witness root
    assert template_tree(txids, [], "cpu") == (want_branches, None)
    # t = 2: the witness root is the root of the tree whose leaf 0 is 32 zero bytes
    branches, witness_root = template_tree(txids, wtxids, "cpu")
    assert branches == want_branches
    if wtxids:
        assert witness_root == merkle_root_full([bytes(32)] + wtxids)
    else:
        assert witness_root is None
    if n <= 4001:
        assert template_tree(txids, wtxids) == (branches, witness_root)  # the Python path says the same


def test_block_100000_folds_to_the_published_root():
    coinbase_txid, others, root = T.block_100000()
    assert merkle_root_full([coinbase_txid] + others) == root  # the oracle itself
    for device in (None, "cpu"):
        branches, witness_root = template_tree(others, [], device)
        assert witness_root is None and len(branches) == 2
        assert merkle_root_from_branches(coinbase_txid, branches) == root
    rows = T.rows_of(N.merkle_tree_cpu(coinbase_txid + b"".join(others), 1, 4), 1, 4)
    assert rows[0][0] == root  # with the real coinbase txid as leaf 0, row 0 is the block's merkle root


def test_a_duplicated_last_leaf_gives_the_same_root():
    a, b, c = T.leaves(3)
    three = T.rows_of(N.merkle_tree_cpu(a + b + c, 1, 3), 1, 3)[0]
    four = T.rows_of(N.merkle_tree_cpu(a + b + c + c, 1, 4), 1, 4)[0]
    assert three[0] == four[0] == sha256d(sha256d(a + b) + sha256d(c + c))
    assert three[1] == four[1] == [b, sha256d(c + c)]


def test_limits_and_bad_lengths_raise():
    leaf = bytes(32)
    assert N.MERKLE_TREE_MAX_LEAVES == T.LIMIT
    for leaves, t, n in ((b"", 1, 0), (b"", 0, 1), (leaf, 0, 1), (leaf, 1, 0), (leaf * 2, 1, 1), (leaf * 2, 2, 2),
                         (leaf[:31], 1, 1), (leaf + b"\x00", 1, 1), (leaf * 3, 2, 2), (leaf, 1, T.LIMIT + 1),
                         (leaf, N.MERKLE_TREE_MAX_TREES + 1, 1)):
        with pytest.raises(ValueError):
            N.merkle_tree_cpu(leaves, t, n)
    with pytest.raises(ValueError):
        N.merkle_tree_cpu(bytes(32 * (T.LIMIT + 1)), 1, T.LIMIT + 1)  # the right length, over the limit
    assert N.merkle_tree_cpu(leaf, 1, 1) == leaf  # one leaf: the root is the leaf, no path
    for txids, wtxids in (([leaf[:31]], []), ([leaf], [leaf[:31]]), ([leaf, leaf], [leaf])):
        for device in (None, "cpu"):
            with pytest.raises(ValueError):
                template_tree(txids, wtxids, device)
    assert template_tree([], [], "cpu") == ([], None) == template_tree([], [])


def test_over_the_limit_template_tree_falls_back_to_python(monkeypatch):
    """One leaf over the op's limit: the native call would raise, ``template_tree`` answers in Python whatever the
    device. (The native extension is made unreachable, so the answer provably comes from the Python path; a GPU
    device string never reaches torch either.)"""
    n = T.LIMIT + 1
    txids = [bytes([i & 0xFF, (i >> 8) & 0xFF, i >> 16]) + bytes(29) for i in range(n - 1)]
    want = merkle_branches(txids)
    assert len(want) == 19

    def unreachable():
        raise AssertionError("the native path must not be asked for a tree over the limit")

    import otedama_amd.ops.native as native_mod

    monkeypatch.setattr(native_mod, "require_native", unreachable)
    for device in ("cpu", "cuda:0"):
        assert template_tree(txids, [], device) == (want, None)
    assert ("tree", "", "cuda:0") not in batch._ops  # no op was made for it


def test_importing_the_pool_modules_does_not_import_torch():
    code = ("import sys; import otedama_amd.pool.batch, otedama_amd.pool.templatetree, otedama_amd.ops.merkle_rows; "
            "assert 'torch' not in sys.modules and 'otedama_amd._native' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
