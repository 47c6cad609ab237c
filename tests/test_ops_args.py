"""``ops._args.byte_rows``: the one tensor check of the digest and share-verification ops, on CPU tensors. Its stream
companion ``launch_stream`` needs a GPU and is exercised in test_share_results_gpu.py."""
import pytest
import torch

from otedama_amd.ops._args import ALIGN, byte_rows

CPU = torch.device("cpu")
W = 32


def _aligned(n: int, width: int = W) -> torch.Tensor:
    """A zeroed uint8 [n, width] tensor that starts at a 16-byte aligned address, with 16 spare bytes behind it."""
    raw = torch.zeros(n * width + 2 * ALIGN, dtype=torch.uint8)
    off = -raw.data_ptr() % ALIGN
    t = raw[off:off + n * width].view(n, width)
    assert t.data_ptr() % ALIGN == 0
    return t


def test_a_good_tensor_gives_its_row_count():
    assert byte_rows("records", _aligned(5), W, CPU) == 5
    assert byte_rows("records", _aligned(5), W, CPU, rows=5) == 5
    assert byte_rows("headers", _aligned(3, 80), 80, CPU) == 3


def test_an_empty_tensor_may_be_unaligned():
    base = _aligned(4)
    empty = base.view(-1)[8:8].view(0, W)
    assert empty.storage_offset() - base.storage_offset() == 8  # torch reports no address for an empty tensor
    assert byte_rows("records", empty, W, CPU) == 0
    assert byte_rows("records", empty, W, CPU, rows=0) == 0


def test_each_bad_tensor_raises_a_value_error_naming_the_argument():
    good = _aligned(4)
    wide = _aligned(4, 2 * W)
    shifted = _aligned(5).view(-1)[8:8 + 4 * W].view(4, W)  # starts 8 bytes into a buffer
    assert shifted.data_ptr() % ALIGN == 8 and shifted.is_contiguous()
    assert not wide[:, :W].is_contiguous()
    bad = {
        "wrong dtype": good.to(torch.int32),
        "1-D": good.view(-1),
        "wrong width": good.view(8, 16),
        "non-contiguous column slice": wide[:, :W],
        "8 bytes into a buffer": shifted,
        "a numpy array": good.numpy(),
    }
    for what, t in bad.items():
        with pytest.raises(ValueError, match="^some_arg must "):
            byte_rows("some_arg", t, W, CPU)
            pytest.fail(what)
    with pytest.raises(ValueError, match="^some_arg must "):
        byte_rows("some_arg", good, W, CPU, rows=3)
    with pytest.raises(ValueError, match="^out must "):
        byte_rows("out", good, W, torch.device("meta"))  # another device
