"""Shared pieces of the template-tree tests (test_merkle_tree_cpu.py, test_merkle_tree_gpu.py, test_template_gbt.py):
deterministic leaves, the size list, the oracle's rows computed once per size, and block 100000 of Bitcoin.

The oracle is the unchanged pair ``merkle_branches`` / ``merkle_root_full`` of otedama_amd/pool/template.py: row 0 of
a tree is ``merkle_root_full(leaves)``, rows ``1..depth`` are ``merkle_branches(leaves[1:])``."""
import functools
import hashlib

from otedama_amd.pool.template import merkle_branches, merkle_root_full

# Small: the level count changes at every power of two, an odd count at every level (7), a node paired with itself at
# one level only (5, 9), one wave and more (255..257). Chunk edges: one workgroup exactly (512), a last chunk of one
# node that is still folded nine times (513), of two and three (514, 515), a half (767), two chunks exactly and one
# more node (1023..1025), an odd number of chunk roots with a last chunk of one (1537). Larger: a Bitcoin-sized
# template (4001), 129 chunk roots with a last chunk of one (65537), the op's limit (262144).
SMALL = [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257]
CHUNK_EDGES = [511, 512, 513, 514, 515, 767, 1023, 1024, 1025, 1537]
LARGER = [4001, 65537, 262144]
SIZES = SMALL + CHUNK_EDGES + LARGER
LIMIT = 262144


def depth(n: int) -> int:
    return (n - 1).bit_length()


@functools.lru_cache(maxsize=None)
def leaves(n: int, tree: int = 0) -> tuple:
    """``n`` leaves from a SHA-256 counter; ``tree`` selects another stream. Never mutated."""
    seed = b"merkle-tree-cases/%d/" % tree
    return tuple(hashlib.sha256(seed + i.to_bytes(4, "little")).digest() for i in range(n))


@functools.lru_cache(maxsize=None)
def oracle(n: int, tree: int = 0) -> tuple:
    """``(root, path)`` of ``leaves(n, tree)`` by the pool's Python functions, computed once."""
    ls = list(leaves(n, tree))
    path = merkle_branches(ls[1:])
    assert len(path) == depth(n)
    return merkle_root_full(ls), path


def packed(n: int, trees=(0,)) -> bytes:
    return b"".join(b"".join(leaves(n, y)) for y in trees)


def rows_of(raw: bytes, t: int, n: int) -> list:
    """``[t, 1 + depth, 32]`` bytes as ``t`` tuples ``(root, path)``."""
    per = 1 + depth(n)
    assert len(raw) == t * per * 32
    out = []
    for y in range(t):
        r = [raw[(y * per + k) * 32:(y * per + k + 1) * 32] for k in range(per)]
        out.append((r[0], r[1:]))
    return out


# Block 100000 of Bitcoin: its four txids and its merkle root, in display order (the coinbase first).
BLOCK_100000_TXIDS = [
    "8c14f0db3df150123e6f3dbbf30f8b955a8249b62ac1d1ff16284aefa3d06d87",
    "fff2525b8931402dd09222c50775608f75787bd2b87e56995a7bdd30f79702c4",
    "6359f0868171b1d194cbee1af2f16ea598ae8fad666d9b012c8ed2b79a236ec4",
    "e9a66845e05d5abc0ad04ec80f774a7e585c6e8db975962d069a522137b80c1d",
]
BLOCK_100000_ROOT = "f3e94742aca4b5ef85488dc37c06c3282295ffec960994b2c0d5ac2a25a95766"


def block_100000() -> tuple:
    """``(coinbase txid, the other txids, merkle root)`` in internal byte order."""
    ids = [bytes.fromhex(h)[::-1] for h in BLOCK_100000_TXIDS]
    return ids[0], ids[1:], bytes.fromhex(BLOCK_100000_ROOT)[::-1]
