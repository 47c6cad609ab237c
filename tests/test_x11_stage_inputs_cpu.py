"""tests/x11_stage_inputs.py held to its own conditions, without a GPU."""
import random

import numpy as np
import pytest

import x11_stage_inputs as X


def test_the_set_is_deterministic_and_has_the_stated_classes():
    a = X.all_blocks()
    X.classes.cache_clear()
    X.all_blocks.cache_clear()
    b = X.all_blocks()
    assert a == b
    cl = X.classes()
    assert list(cl) == list(X.CLASS_SIZES)
    assert {k: len(v) for k, v in cl.items()} == X.CLASS_SIZES
    assert len(a) == sum(X.CLASS_SIZES.values()) == 2588
    assert all(type(blk) is bytes and len(blk) == 64 for blk in a)
    for name, blocks in cl.items():
        assert len(set(blocks)) == len(blocks), name  # no duplicates within a class
    assert X.SPARE == 300 and X.ROTATE == 37 and X.ROTATE % 64 and X.ROTATE % 8


def test_the_classes_are_what_their_names_say():
    cl = X.classes()
    assert cl["constant"] == tuple(bytes([v]) * 64 for v in range(256))
    ones = (1 << 512) - 1
    assert sorted(int.from_bytes(b, "little") for b in cl["one-bit-set"]) == [1 << k for k in range(512)]
    assert sorted(int.from_bytes(b, "little") ^ ones for b in cl["one-bit-clear"]) == [1 << k for k in range(512)]
    words = [tuple(int.from_bytes(b[8 * k:8 * k + 8], "little") for k in range(8)) for b in cl["words"]]
    full = 0xFFFFFFFFFFFFFFFF
    for k in range(8):
        for v in (0, 1, 0x8000000000000000):
            assert tuple(v if w == k else full for w in range(8)) in words
    for v in (0x00000000FFFFFFFF, 0xFFFFFFFF00000000, 0x7FFFFFFFFFFFFFFF, 0x0000000100000000):
        assert (v,) * 8 in words
    assert all(set(b) <= {0, 255} for name in ("simd-centred", "simd-table") for b in cl[name])


def test_rotation_moves_every_block_by_37_positions():
    blocks = X.all_blocks()
    rot = X.rotated(blocks, X.ROTATE)
    m = len(blocks)
    assert len(rot) == m and all(rot[p] == blocks[(p - X.ROTATE) % m] for p in range(m))
    assert X.rotated(blocks, 0) == blocks


def test_the_table_form_is_the_centred_form_with_the_other_sign():
    """41^(ij) mod 257 is in [1, 256]; the SIMD_PT byte (that value minus 1) is >= 128 exactly where the centred value
    is negative. So the two constructions give the same 512 blocks."""
    assert X.alpha_pow(256) == 1 and X.alpha_pow(128) == 256 and len({X.alpha_pow(e) for e in range(256)}) == 256
    assert [X.centred(p) for p in (1, 128, 129, 256)] == [1, 128, -128, -1]
    for e in range(256):
        p = X.alpha_pow(e)
        assert 1 <= p <= 256 and (p - 1 >= 128) == (X.centred(p) < 0)
    for i in range(256):
        for s in (1, -1):
            assert X.simd_table_block(i, s) == X.simd_centred_block(i, -s)
    assert set(X.classes()["simd-table"]) == set(X.classes()["simd-centred"])


def test_each_sign_matched_block_reaches_the_extreme_unreduced_sum():
    """For index i the unreduced sum  sum_j x[j] * centred(41^(ij))  over bytes x[j] in [0, 255] is largest when x is
    255 on the positive coefficients and 0 elsewhere, smallest the other way round. The blocks reach those values
    exactly, and none of 1000 seeded random blocks passes them."""
    coef = np.array([[X.centred(X.alpha_pow(i * j)) for j in range(64)] for i in range(256)], dtype=np.int64)
    upper = 255 * np.where(coef > 0, coef, 0).sum(axis=1)
    lower = 255 * np.where(coef < 0, coef, 0).sum(axis=1)
    rng = random.Random(77)
    rnd = np.frombuffer(b"".join(rng.randbytes(64) for _ in range(1000)), dtype=np.uint8).reshape(1000, 64)
    rnd_sums = rnd.astype(np.int64) @ coef.T  # [1000, 256]
    blocks = X.classes()["simd-centred"]
    for i in range(256):
        plus = np.frombuffer(blocks[2 * i], dtype=np.uint8).astype(np.int64)
        minus = np.frombuffer(blocks[2 * i + 1], dtype=np.uint8).astype(np.int64)
        assert blocks[2 * i] == X.simd_centred_block(i, 1) and blocks[2 * i + 1] == X.simd_centred_block(i, -1)
        assert int(plus @ coef[i]) == upper[i] >= rnd_sums[:, i].max(), i
        assert int(minus @ coef[i]) == lower[i] <= rnd_sums[:, i].min(), i
    # far below the bound the kernel's lazy reduction is justified by (centre257: |x| < 2^27)
    assert max(upper.max(), -lower.min()) < 1 << 27


def test_the_comparison_names_position_zero_against_the_next_stage():
    from otedama_amd.ops.native import load

    N = load(build_if_missing=False)
    if N is None:
        pytest.skip("the native extension is not built")
    blocks = X.all_blocks()[:64]
    for st in (1, 9):
        got = X.oracle(N, st, blocks)
        X.assert_positions_equal(st, got, X.oracle(N, st, blocks), "self")
        with pytest.raises(AssertionError, match=r"64 of 64 positions differ, first positions \[0, 1, 2"):
            X.assert_positions_equal(st, got, X.oracle(N, st + 1, blocks), "wrong stage")


def test_the_cpu_oracle_gives_64_bytes_for_every_block_at_every_stage():
    from otedama_amd.ops.native import load

    N = load(build_if_missing=False)
    if N is None:
        pytest.skip("the native extension is not built")
    blocks = X.all_blocks()
    for st in range(1, 11):
        out = X.oracle(N, st, blocks)
        assert len(out) == len(blocks) and all(type(d) is bytes and len(d) == 64 for d in out), st
        assert out[0] != out[1], st
    assert X.compared(10, bytes(range(64))) == bytes(range(32)) and X.compared(9, bytes(64)) == bytes(64)
