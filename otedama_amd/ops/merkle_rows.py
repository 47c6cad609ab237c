"""The rows of the template tree op (csrc/include/otedama/merkle_tree.h), packed and unpacked for
``ops.merkle.MerkleTree`` and the native ``merkle_tree_cpu``. Importing this module imports neither torch nor the
native extension."""
from __future__ import annotations

from typing import Sequence

NODE_BYTES = 32
CHUNK = 512          # nodes one workgroup folds
MAX_LEAVES = 262144  # CHUNK squared: two launches at most
MAX_TREES = 65535    # the tree is the launch grid's y


def tree_depth(n: int) -> int:
    return (n - 1).bit_length()


def pack_leaves(leaf_lists: Sequence[Sequence[bytes]]) -> tuple[bytes, int, int]:
    """``t`` lists of ``n`` 32-byte leaves as the ``[t, n, 32]`` bytes of the op and of ``merkle_tree_cpu``, with
    ``t`` and ``n``. Lists of unequal length, an empty list or a leaf that is not 32 bytes raise ``ValueError``."""
    t = len(leaf_lists)
    if t == 0:
        raise ValueError("need at least one tree")
    n = len(leaf_lists[0])
    if n == 0 or any(len(ls) != n for ls in leaf_lists):
        raise ValueError("every tree needs the same number of leaves, at least one")
    # a full template is tens of thousands of leaves: the lengths and the join go through C-level loops
    if any(set(map(len, ls)) != {NODE_BYTES} for ls in leaf_lists):
        raise ValueError("every leaf must be 32 bytes")
    try:
        packed = b"".join(b"".join(ls) for ls in leaf_lists)
    except TypeError as exc:
        raise ValueError("every leaf must be a bytes-like object") from exc
    return packed, t, n


def unpack_rows(rows, t: int, n: int) -> list[tuple[bytes, list[bytes]]]:
    """The ``[t, 1 + depth, 32]`` bytes of the op as ``t`` tuples ``(root, path)``."""
    per = 1 + tree_depth(n)
    raw = bytes(rows)
    out = []
    for y in range(t):
        r = [raw[(y * per + k) * NODE_BYTES:(y * per + k + 1) * NODE_BYTES] for k in range(per)]
        out.append((r[0], r[1:]))
    return out
