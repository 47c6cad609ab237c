"""Every X11 stage kernel on blocks no header produces, every position compared (MI355X).

tests/test_x11_gpu.py runs the stage kernels on the chain's own pseudo-random intermediates and samples 32 of 1000
positions. Here each of the ten kernels that read the digest planes runs alone (``N.launch_x11_stage`` on planes
written by the test) on the set of tests/x11_stage_inputs.py: constant blocks (every table index in every lane),
single-bit blocks, carry and rotate patterns, and 0/255 blocks that drive one SIMD-512 NTT coefficient's unreduced sum
to its extreme, which pins the hardware form (``v_dot4_u32_u8``, byte permutes, the packed 16-bit multiply, lazy
reduction mod 257) of arithmetic that a host model otherwise only vouches for.

All m blocks sit on the planes at once with 300 canary columns after them (so the stride is not m, and a store past
the batch is seen), each stage runs the set twice, the second time shifted by 37 positions (another lane, another SIMD
8-lane slot, another AES lane offset for every block), and every position is compared with ``N.x11_stage`` by byte
equality (ECHO: the 32 bytes of the chain digest, as in tests/test_x11_gpu.py). BLAKE (stage 0) has its own input
path and gets extreme job blocks over a window that wraps 2^32.
"""
import functools
import struct

import pytest

import x11_stage_inputs as X

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _rig():
    return X.StageRig(X.native(), len(X.all_blocks()), DEV)


@pytest.mark.parametrize("st", range(1, 11), ids=[f"{st}-{X.STAGES[st]}" for st in range(1, 11)])
def test_stage_kernel_equals_cpu_at_every_position(st):
    N = X.native()
    rig = _rig()
    assert rig.batch == rig.m + 300 and rig.m == len(X.all_blocks())
    for shift in (0, X.ROTATE):
        blocks = X.rotated(X.all_blocks(), shift)
        got, canary_kept = rig.run(st, blocks)
        want = X.oracle(N, st, blocks)
        X.assert_positions_equal(st, got, want, f"shift {shift}")
        assert canary_kept, f"stage {st} shift {shift}: the columns past the batch were written"
    # the comparison can fail: the kernel's output against the oracle of another stage is refused at position 0
    other = st % 10 + 1
    with pytest.raises(AssertionError, match=r"first positions \[0, "):
        X.assert_positions_equal(st, got, X.oracle(N, other, blocks), "another stage's oracle")


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_blake_on_extreme_job_blocks_over_a_wrapping_window(fill):
    from otedama_amd.ops.search import X11Search

    N = X.native()
    prefix = bytes([fill]) * 76
    base, count = 0xFFFFFF00, 512
    s = X11Search(DEV, batch=count + 300)
    got = s.trace(prefix + bytes(4), base, count)[0].numpy().tobytes()
    headers = [prefix + struct.pack("<I", (base + i) & 0xFFFFFFFF) for i in range(count)]
    X.assert_positions_equal(0, [got[64 * i:64 * i + 64] for i in range(count)],
                             [N.x11_stage(0, h) for h in headers], f"prefix {fill:#04x}")


def test_constant_headers_end_to_end_equal_the_cpu_chain():
    from otedama_amd.ops.digest import HeaderDigest

    N = X.native()
    headers = [b + bytes(16) for b in X.classes()["constant"]]
    assert len(headers) == 256 and all(len(h) == 80 for h in headers)
    got = HeaderDigest("x11", DEV, capacity=256).hash(headers)
    want = [N.x11(h) for h in headers]
    bad = [i for i in range(256) if got[i] != want[i]]
    assert not bad, (bad[:8], got[bad[0]].hex(), want[bad[0]].hex())
