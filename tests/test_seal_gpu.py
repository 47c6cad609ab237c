"""Batched frame sealing on a real MI355X: ``FrameSeal.launch`` / ``seal`` (otedama_amd/ops/seal.py; ``otd_aead_seal``
and ``otd_poly1305_rows`` of csrc/kernels/aead_seal.hip) and the pool's frame sealer on the GPU.

Every comparison is exact byte equality against ``utils.aead.seal`` or the big-integer Poly1305 of seal_cases.py."""
import asyncio
import functools

import pytest

import seal_cases as C
import seal_pool_cases as P
from otedama_amd.ops import seal_rows as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xA5
CANARY = 0x5C
GUARD = 256  # canary bytes before the first region and after the last


@functools.lru_cache(maxsize=None)
def _op():
    from otedama_amd.ops.seal import FrameSeal

    return FrameSeal(DEV)


def _launch(packed, n, out_bytes, in_slack=0):
    """One launch into a filled output between two canaries; returns ``(output bytes, canaries intact)``."""
    import torch

    src = torch.zeros(len(packed) + in_slack, dtype=torch.uint8, device=DEV)
    src[:len(packed)] = torch.frombuffer(bytearray(packed), dtype=torch.uint8).to(DEV)
    buf = torch.full((GUARD + out_bytes + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    out = buf[GUARD:GUARD + out_bytes]
    out.fill_(FILL)
    r = _op().launch(src[:len(packed)], n, out)
    torch.cuda.synchronize()
    assert r.data_ptr() == out.data_ptr()
    raw = buf.cpu().numpy().tobytes()
    intact = raw[:GUARD] == bytes([CANARY]) * GUARD and raw[GUARD + out_bytes:] == bytes([CANARY]) * GUARD
    assert src[:len(packed)].cpu().numpy().tobytes() == bytes(packed)  # the input is only read
    return raw[GUARD:GUARD + out_bytes], intact


@pytest.mark.parametrize("name", sorted(C.batches()))
def test_launch_equals_the_oracle_and_keeps_inside_its_regions(name):
    frames = C.batches()[name]
    n = len(frames)
    packed, out_bytes = R.pack_frames(frames)
    out, intact = _launch(packed, n, out_bytes)
    assert intact
    got = R.unpack_sealed(packed, out, n)
    want = C.expected(name)
    at = 0
    for i, (g, w) in enumerate(zip(got, want)):
        size = len(frames[i][2])
        assert g == w, (i, size, frames[i][1])
        assert g[-16:] != bytes([FILL]) * 16 and (size < 8 or g[:size] != bytes([FILL]) * size)  # written, not left
        end = at + 16 + (size + 15) // 16 * 16
        assert out[at + 16 + size:end] == bytes(end - at - 16 - size)  # the padding of its own region: zeros
        at = end
    assert at == out_bytes and len(got) == len(want) == n
    bumped = C.expected_bumped(name)
    assert all(g != b for g, b in zip(got, bumped))  # the comparison does see a wrong counter, in every frame


def test_seal_equals_the_oracle_and_the_twin_and_wipes_the_keys():
    import torch

    op = type(_op())(DEV)  # its own staging buffers
    for name in ("n1", "lengths", "n257"):
        frames = C.batches()[name]
        n = len(frames)
        packed, _ = R.pack_frames(frames)
        twin = R.unpack_sealed(packed, op.native.aead_seal_many_cpu(packed, n), n)
        assert op.seal(frames) == twin == list(C.expected(name))
        st = op._staging
        assert st.pin_in.is_pinned() and st.pin_out.is_pinned()
        torch.cuda.synchronize()
        assert st.dev_in[:len(packed)].cpu().numpy().tobytes() == bytes(len(packed))  # the device input: all zero
        left = st.pin_in.numpy().tobytes()
        heads = left[:n * R.HEAD_BYTES]
        for i in range(n):  # the heads did go in, and only their keys are gone
            assert heads[i * 64:i * 64 + 32] == bytes(32)
            assert heads[i * 64 + 32:(i + 1) * 64] == packed[i * 64 + 32:(i + 1) * 64]
        assert left[n * R.HEAD_BYTES:len(packed)] == packed[n * R.HEAD_BYTES:]
    assert op.seal([]) == []
    with pytest.raises(ValueError):
        op.seal([(bytes(32), 0, bytes(R.SEAL_MAX_PLAIN + 1))])
    with pytest.raises(ValueError):
        op.seal([(bytes(32), 2 ** 64 - 1, b"")])


def test_poly1305_rows_on_the_device_equal_the_table_and_the_random_rows():
    import torch

    rows, tags = C.poly_rows()
    packed = R.pack_poly_rows(rows)
    src = torch.frombuffer(packed, dtype=torch.uint8).view(len(rows), R.POLY_ROW_BYTES).to(DEV)
    out = _op()._poly1305_rows(src).cpu().numpy().tobytes()
    for i, tag in enumerate(tags):
        assert out[16 * i:16 * i + 16] == tag, (i, rows[i])
    assert len(out) == 16 * len(tags) and len(tags) > 256  # more than one block


def test_a_head_that_breaks_the_rules_writes_nothing():
    frames = C.batches()["n65"][:6]
    packed, out_bytes = R.pack_frames(frames)
    region = out_bytes // 6
    broken = bytearray(packed)
    # frame 1: a length over the limit; frame 2: a region that ends past the output (it would land in the canary,
    # still inside the allocation); frame 3: a plaintext that ends past the input (inside the allocation's slack);
    # frame 4: offsets that are no multiples of 16
    broken[1 * 64 + 40:1 * 64 + 44] = (R.SEAL_MAX_PLAIN + 1).to_bytes(4, "little")
    broken[2 * 64 + 48:2 * 64 + 52] = (out_bytes - 16).to_bytes(4, "little")
    broken[3 * 64 + 44:3 * 64 + 48] = (len(packed) - 16).to_bytes(4, "little")
    broken[4 * 64 + 48:4 * 64 + 52] = (4 * region + 8).to_bytes(4, "little")
    out, intact = _launch(broken, 6, out_bytes, in_slack=256)
    assert intact
    want = C.expected("n65")
    for i in range(6):
        got = out[i * region:(i + 1) * region]
        if i in (0, 5):
            assert got[16:16 + 55] + got[:16] == want[i]
        else:
            assert got == bytes([FILL]) * region, i


def test_launch_rejects_bad_arguments_with_nothing_enqueued():
    import torch

    op = _op()
    packed, out_bytes = R.pack_frames(C.batches()["n1"])
    src = torch.frombuffer(bytearray(packed), dtype=torch.uint8).to(DEV)
    raw = torch.zeros(1024, dtype=torch.uint8, device=DEV)
    good = torch.zeros(out_bytes, dtype=torch.uint8, device=DEV)
    for x in (src.to(torch.int32), src.view(2, -1), src.cpu(), src[:56], raw[8:8 + len(packed)], src[::2]):
        with pytest.raises(ValueError):
            op.launch(x, 1, good)
    for o in (good.cpu(), good.view(1, -1), good[:8], raw[8:8 + out_bytes]):
        with pytest.raises(ValueError):
            op.launch(src, 1, o)
    for n in (0, 3, R.MAX_FRAMES + 1):  # 3: more heads than the input holds
        with pytest.raises(ValueError):
            op.launch(src, n, good)
    nat = op.native
    ok = (src.data_ptr(), len(packed), 1, good.data_ptr(), out_bytes)
    for pos, bad in ((0, 0), (3, 0), (2, 0), (2, R.MAX_FRAMES + 1), (0, src.data_ptr() + 8), (3, good.data_ptr() + 8),
                     (1, 48), (1, len(packed) + 8), (4, out_bytes + 8), (1, 1 << 32), (4, 1 << 32)):
        args = list(ok)
        args[pos] = bad
        with pytest.raises(ValueError):
            nat.launch_aead_seal(*args)
    with pytest.raises(ValueError):
        nat._launch_poly1305_rows(0, 1, good.data_ptr())
    torch.cuda.synchronize()
    assert good.cpu().numpy().tobytes() == bytes(out_bytes)  # nothing was written by a rejected call
    with pytest.raises(ValueError):
        type(op)("cpu")


def test_the_pool_seals_three_channels_on_the_gpu():
    async def body(pool, clients):
        pool.new_block()
        await P.take_block(pool, clients)
        first = pool.stats()["seal"]
        blocks = await P.submit_each(pool, clients)
        return first, blocks, pool.stats()["seal"]

    first, blocks, last = asyncio.run(asyncio.wait_for(
        P.pool_with_clients(3, body, seal_device=DEV, seal_min_gpu=1), 120))
    assert first["gpu_frames"] == 6 and first["cpu_frames"] == 0 and first["batches"] == 1
    assert (first["device"], first["enabled"], first["device_errors"]) == (DEV, True, 0)
    assert blocks == 3 and last["gpu_frames"] == 6 * (1 + blocks) and last["cpu_frames"] == 0
    assert last["device_errors"] == 0 and last["enabled"] is True
