"""The batched secp256k1 multiplication on a real MI355X: ``Secp256k1Mul.launch`` / ``mul`` (otedama_amd/ops/secp.py;
``otd_secp256k1_mul`` of csrc/kernels/secp256k1_mul.hip) and the pool's handshake batcher on the GPU.

Every comparison is exact byte equality against the Python oracle of secp_cases.py."""
import asyncio
import functools

import pytest

import handshake_cases as H
import secp_cases as S
from otedama_amd.ops import secp_rows as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5
POISON = 0x5C


@functools.lru_cache(maxsize=None)
def _op():
    from otedama_amd.ops.secp import Secp256k1Mul

    return Secp256k1Mul(DEV)


def _dev(rows):
    import torch

    return torch.frombuffer(R.pack_rows(rows), dtype=torch.uint8).view(len(rows), R.ROW_BYTES).to(DEV)


def _expected_bytes(rows) -> bytes:
    return b"".join(x + bytes([status, parity]) + bytes(14) for x, parity, status in S.expected(rows))


# one lane, a wave less one, a wave, a wave and one, a block and one, two blocks and one (a tail of one lane)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 513])
def test_launch_equals_the_oracle_and_keeps_inside_out(n):
    import torch

    assert len(S.ROWS) + len(S.BAD_ROWS) < 513  # at 513 every row of the cases has been through the kernel
    rows = S.tiled(n, offset=n)  # another stretch of the cases at every size
    src = _dev(rows)
    buf = torch.full((n + 64, R.OUT_BYTES), CANARY, dtype=torch.uint8, device=DEV)
    out = buf[:n]
    out.fill_(POISON)
    r = _op().launch(src, out=out)
    torch.cuda.synchronize()
    assert r.data_ptr() == buf.data_ptr()
    got = out.cpu().numpy().tobytes()
    want = _expected_bytes(rows)
    for i in range(n):
        assert got[i * R.OUT_BYTES:(i + 1) * R.OUT_BYTES] == want[i * R.OUT_BYTES:(i + 1) * R.OUT_BYTES], (i, rows[i])
    assert buf[n:].cpu().numpy().tobytes() == bytes([CANARY]) * (64 * R.OUT_BYTES)
    assert src.cpu().numpy().tobytes() == bytes(R.pack_rows(rows))  # the rows are only read


def test_bad_rows_between_good_ones_in_one_wave():
    import torch

    good = S.ROWS[:58]
    rows = list(good)
    for k, (bad, _status) in enumerate(S.BAD_ROWS):
        rows.insert(3 + 9 * k, bad)
    assert len(rows) == 64
    out = _op().launch(_dev(rows))
    torch.cuda.synchronize()
    assert out.shape == (64, R.OUT_BYTES) and out.dtype == torch.uint8 and out.device == torch.device(DEV)
    got = R.unpack_rows(out.cpu().numpy().tobytes(), 64)
    assert got == S.expected(rows)
    assert [g for g, r in zip(got, rows) if r in good] == S.expected(good)
    assert sorted(g[2] for g in got if g[2]) == [1, 1, 1, 2, 2, 3]


def test_mul_equals_the_cpu_twin_and_wipes_the_device_input():
    import torch

    op = type(_op())(DEV)  # its own staging buffers
    for n in (3, 192):
        rows = S.tiled(n, offset=5)
        want = R.unpack_rows(op.native.secp256k1_mul_cpu(R.pack_rows(rows)), n)
        assert op.mul(rows) == want == S.expected(rows)
        st = op._staging
        assert st.pin_in.is_pinned() and st.pin_out.is_pinned()
        torch.cuda.synchronize()
        assert st.dev_in[:n * R.ROW_BYTES].cpu().numpy().tobytes() == bytes(n * R.ROW_BYTES)
        left = st.pin_in.numpy().tobytes()
        assert all(left[i * R.ROW_BYTES:i * R.ROW_BYTES + 32] == bytes(32) for i in range(n))
    assert op.mul([]) == []


def test_launch_rejects_bad_arguments_with_nothing_enqueued():
    import torch

    op = _op()
    rows = _dev(S.tiled(4))
    raw = torch.zeros(4 * R.ROW_BYTES + 16, dtype=torch.uint8, device=DEV)
    good_out = torch.zeros((4, R.OUT_BYTES), dtype=torch.uint8, device=DEV)
    for x in (rows.to(torch.int32), rows.view(-1), rows.view(8, 64), rows.cpu(), rows[:, :64], rows[:0],
              raw[8:8 + 4 * R.ROW_BYTES].view(4, R.ROW_BYTES), rows[:1].expand(R.MAX_ROWS + 1, R.ROW_BYTES)):
        with pytest.raises(ValueError):
            op.launch(x)
    for o in (good_out[:3], good_out.cpu(), good_out.view(-1), raw[8:8 + 4 * R.OUT_BYTES].view(4, R.OUT_BYTES)):
        with pytest.raises(ValueError):
            op.launch(rows, out=o)
    nat = op.native
    ok = (rows.data_ptr(), 4, good_out.data_ptr())
    for pos, bad in ((0, 0), (2, 0), (1, 0), (1, R.MAX_ROWS + 1), (0, rows.data_ptr() + 8),
                     (2, good_out.data_ptr() + 8)):
        args = list(ok)
        args[pos] = bad
        with pytest.raises(ValueError):
            nat.launch_secp256k1_mul(*args)
    torch.cuda.synchronize()
    assert good_out.cpu().numpy().tobytes() == bytes(4 * R.OUT_BYTES)  # nothing was written by a rejected call
    with pytest.raises(ValueError):
        type(op)("cpu")


def test_the_pool_computes_sixty_four_handshakes_on_the_gpu():
    async def body():
        pool = H.noise_pool(handshake_device=DEV, handshake_min_gpu=1)
        await pool.start()
        try:
            channels, _ = await H.crowd(pool, H.SUITES_64)
            return channels, pool.stats()["handshake"]
        finally:
            await pool.stop()

    channels, hs = asyncio.run(asyncio.wait_for(body(), 120))
    H.check_channels(channels, 64)
    assert hs["gpu_handshakes"] == 64 and hs["cpu_handshakes"] == 0 and hs["device_errors"] == 0
    assert (hs["device"], hs["enabled"]) == (DEV, True) and hs["max_batch"] > 1
