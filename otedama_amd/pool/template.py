"""Block templates, coinbase construction and merkle branches for the local pool.

[NO REFERENCE CODE] — v3 of the reference removed pool operator mode
(CHANGELOG.md:6623-6624) and its V1 client never builds a coinbase
(poolproto/stratumv1/parse.go:52-54,91). This module is the pool half of the
coinbase / merkle work: a BIP34 coinbase paying the operator's
address, split around the extranonce for Stratum V1 (coinb1 | en1 | en2 | coinb2),
and fixed merkle roots for Stratum V2 standard channels (one extranonce prefix
per channel).

No bitcoind is available offline, so the default templates are synthetic: a
random or chained prev-hash, a configurable nBits, and optional fake
transaction ids (to exercise merkle branches of realistic depth).

A real template comes from a ``getblocktemplate`` result
(:meth:`BlockTemplate.from_gbt`, :class:`GbtFileSource`): txids for the coinbase
branches, wtxids for the BIP141 witness commitment in the coinbase, and the raw
transactions for :func:`serialize_block`. Both trees can be computed elsewhere
(``pool.batch.template_tree``, on the native CPU path or a GPU) and handed in
with :meth:`BlockTemplate.set_tree`. The witness-commitment path is parity
unpinned: no segwit block is available offline, only the txid tree is pinned
(block 100000, tests/merkle_tree_cases.py).
"""
from __future__ import annotations

import hashlib
import json
import os
import struct
import time
from dataclasses import dataclass, field

from otedama_amd import btccrypto
from otedama_amd.models.header import sha256d


WITNESS_COMMITMENT_HEADER = bytes.fromhex("6a24aa21a9ed")  # OP_RETURN, push 36, the BIP141 commitment header


def varint(n: int) -> bytes:
    if n < 0xFD:
        return bytes([n])
    if n <= 0xFFFF:
        return b"\xfd" + struct.pack("<H", n)
    if n <= 0xFFFFFFFF:
        return b"\xfe" + struct.pack("<I", n)
    return b"\xff" + struct.pack("<Q", n)


def script_num(n: int) -> bytes:
    """Minimal CScriptNum push (BIP34 height)."""
    if n == 0:
        return b"\x00"
    out = bytearray()
    v = abs(n)
    while v:
        out.append(v & 0xFF)
        v >>= 8
    if out[-1] & 0x80:
        out.append(0x80 if n < 0 else 0)
    elif n < 0:
        out[-1] |= 0x80
    return bytes([len(out)]) + bytes(out)


def merkle_branches(txids: list[bytes]) -> list[bytes]:
    """Branches for the coinbase (index 0) given the other txids (internal byte order)."""
    branches = []
    level = [None] + list(txids)  # None = coinbase placeholder (always index 0)
    while len(level) > 1:
        if len(level) % 2:
            level.append(level[-1])
        branches.append(level[1])
        level = [None] + [sha256d(level[i] + level[i + 1]) for i in range(2, len(level), 2)]
    return branches


def merkle_root_from_branches(coinbase_txid: bytes, branches: list[bytes]) -> bytes:
    root = coinbase_txid
    for b in branches:
        root = sha256d(root + b)
    return root


def merkle_root_full(txids: list[bytes]) -> bytes:
    level = list(txids)
    while len(level) > 1:
        if len(level) % 2:
            level.append(level[-1])
        level = [sha256d(level[i] + level[i + 1]) for i in range(0, len(level), 2)]
    return level[0]


@dataclass
class BlockTemplate:
    height: int
    prev_hash: bytes            # header byte order
    version: int
    nbits: int
    ntime: int
    coinbase_value: int         # satoshis
    payout_script: bytes
    txids: list[bytes] = field(default_factory=list)
    coinbase_message: bytes = b"/otedama-mi355x/"
    wtxids: list[bytes] = field(default_factory=list)   # internal byte order, one per txid; empty = no commitment
    tx_data: list[bytes] = field(default_factory=list)  # the raw transactions, for serialize_block
    _tree: tuple | None = field(default=None, repr=False, compare=False)

    def set_tree(self, branches: list[bytes], witness_root: bytes | None) -> None:
        """Hand in the trees computed elsewhere (``pool.batch.template_tree(self.txids, self.wtxids, device)``):
        ``branches()`` and ``coinbase_parts()`` use them instead of hashing in Python."""
        if bool(self.wtxids) != (witness_root is not None):
            raise ValueError("a witness root goes with wtxids, and only with them")
        self._tree = (list(branches), witness_root)

    def witness_root(self) -> bytes | None:
        """The root of the wtxid tree with the coinbase's wtxid zeroed (BIP141), or None without wtxids."""
        if not self.wtxids:
            return None
        if self._tree is not None:
            return self._tree[1]
        return merkle_root_full([bytes(32)] + self.wtxids)

    def witness_commitment_script(self) -> bytes | None:
        """The 38-byte scriptPubKey of the commitment output (witness reserved value: 32 zero bytes), or None."""
        root = self.witness_root()
        return None if root is None else WITNESS_COMMITMENT_HEADER + sha256d(root + bytes(32))

    def coinbase_parts(self, extranonce_size: int) -> tuple[bytes, bytes]:
        """(coinb1, coinb2) around an `extranonce_size`-byte extranonce (en1 + en2)."""
        script_prefix = script_num(self.height) + bytes([len(self.coinbase_message)]) + self.coinbase_message
        script_len = len(script_prefix) + extranonce_size
        if script_len > 100:
            raise ValueError("coinbase scriptSig too long")
        coinb1 = (struct.pack("<I", 1)            # tx version
                  + b"\x01"                        # 1 input
                  + bytes(32) + b"\xff\xff\xff\xff"  # null prevout
                  + varint(script_len) + script_prefix)
        commitment = self.witness_commitment_script()
        outputs = struct.pack("<Q", self.coinbase_value) + varint(len(self.payout_script)) + self.payout_script
        if commitment is not None:                 # BIP141: value 0, OP_RETURN 0x24 0xaa21a9ed <32 bytes>
            outputs += struct.pack("<Q", 0) + varint(len(commitment)) + commitment
        coinb2 = (b"\xff\xff\xff\xff"              # sequence
                  + (b"\x01" if commitment is None else b"\x02")  # outputs
                  + outputs
                  + b"\x00\x00\x00\x00")           # locktime
        return coinb1, coinb2

    def branches(self) -> list[bytes]:
        if self._tree is not None:
            return list(self._tree[0])
        return merkle_branches(self.txids)

    def merkle_root(self, coinbase: bytes) -> bytes:
        return merkle_root_from_branches(sha256d(coinbase), self.branches())


    @classmethod
    def from_gbt(cls, result: dict, payout_script: bytes,
                 coinbase_message: bytes = b"/otedama-mi355x/") -> "BlockTemplate":
        """A template from a ``getblocktemplate`` result (segwit rules): ``version``, ``height``, ``curtime``,
        ``coinbasevalue``, ``previousblockhash`` (display hex, reversed into header order), ``bits`` (hex) and every
        transaction's ``txid``, ``hash`` (the wtxid) and ``data``; the hashes are reversed into internal order. A
        ``default_witness_commitment`` that differs from the script built here is a ``ValueError``: the node and the
        pool would disagree about the block."""
        try:
            txs = list(result.get("transactions", []))
            t = cls(height=int(result["height"]), prev_hash=bytes.fromhex(result["previousblockhash"])[::-1],
                    version=int(result["version"]), nbits=int(result["bits"], 16), ntime=int(result["curtime"]),
                    coinbase_value=int(result["coinbasevalue"]), payout_script=bytes(payout_script),
                    txids=[bytes.fromhex(tx["txid"])[::-1] for tx in txs],
                    coinbase_message=bytes(coinbase_message),
                    wtxids=[bytes.fromhex(tx["hash"])[::-1] for tx in txs],
                    tx_data=[bytes.fromhex(tx["data"]) for tx in txs])
        except (KeyError, TypeError, AttributeError) as exc:
            raise ValueError(f"not a getblocktemplate result: {exc!r}") from exc
        if len(t.prev_hash) != 32 or any(len(x) != 32 for x in t.txids + t.wtxids):
            raise ValueError("getblocktemplate result: a hash is not 32 bytes")
        theirs = result.get("default_witness_commitment")
        if theirs is not None:
            ours = t.witness_commitment_script() or b""
            if bytes.fromhex(theirs) != ours:
                raise ValueError(f"default_witness_commitment {theirs} differs from the commitment built from the "
                                 f"template's wtxids ({ours.hex()})")
        return t


def serialize_block(header80: bytes, coinbase: bytes, template: BlockTemplate) -> bytes:
    """The block for ``submitblock``: the 80-byte header, the transaction count, the coinbase (``coinb1 + extranonce
    + coinb2``, whose sha256d is the txid the header commits to) and every ``tx_data`` of the template. With wtxids
    the coinbase goes in witness form: marker and flag after the version, and before the locktime a witness stack of
    one item, the 32 zero bytes of the witness reserved value."""
    if len(header80) != 80:
        raise ValueError("the header is 80 bytes")
    if template.wtxids:
        coinbase = coinbase[:4] + b"\x00\x01" + coinbase[4:-4] + b"\x01\x20" + bytes(32) + coinbase[-4:]
    return header80 + varint(1 + len(template.tx_data)) + coinbase + b"".join(template.tx_data)


class GbtFileSource:
    """Templates from a JSON file that holds a ``getblocktemplate`` result (or the whole RPC reply, with the result
    under ``"result"``): read again on every :meth:`next_block`, so an operator keeps it fresh with ``bitcoin-cli
    getblocktemplate '{"rules": ["segwit"]}'`` in a loop. A found block is written as hex next to it."""

    def __init__(self, path: str, payout_script: bytes, message: bytes | str = b"/otedama-mi355x/"):
        self.path = str(path)
        self.payout_script = bytes(payout_script)
        self.msg = (message.encode() if isinstance(message, str) else bytes(message))[:40]

    def next_block(self) -> BlockTemplate:
        with open(self.path, "r", encoding="utf-8") as f:
            result = json.load(f)
        if isinstance(result, dict) and isinstance(result.get("result"), dict):
            result = result["result"]
        if not isinstance(result, dict):
            raise ValueError(f"{self.path}: not a getblocktemplate result")
        return BlockTemplate.from_gbt(result, self.payout_script, self.msg)

    def submit_block(self, raw: bytes, template: BlockTemplate) -> str:
        """Write the block as hex to ``<path>.block-<height>.hex`` (for ``bitcoin-cli submitblock``); the path."""
        out = f"{self.path}.block-{template.height}.hex"
        with open(out, "w", encoding="ascii") as f:
            f.write(raw.hex() + "\n")
        return out


class TemplateSource:
    """Synthetic chain: each new block gets a fresh prev-hash and height."""

    def __init__(self, payout_address: str | None, nbits: int = 0x1703A30C, n_txs: int = 0,
                 coinbase_message: str = "/otedama-mi355x/", seed: bytes | None = None):
        if payout_address:
            self.payout_script = btccrypto.address_script_pubkey(payout_address)
        else:
            self.payout_script = b"\x6a"  # OP_RETURN (burn) when no operator address is configured
        self.nbits = nbits
        self.n_txs = n_txs
        self.msg = coinbase_message.encode()[:40]
        self.height = 900_000
        self._prev = hashlib.sha256(seed or os.urandom(32)).digest()

    def next_block(self) -> BlockTemplate:
        self.height += 1
        self._prev = sha256d(self._prev + struct.pack("<I", self.height))
        txids = [sha256d(self._prev + struct.pack("<I", i)) for i in range(self.n_txs)]
        subsidy = 312_500_000  # 3.125 BTC (provider/mining.go:84)
        return BlockTemplate(height=self.height, prev_hash=self._prev, version=0x20000000, nbits=self.nbits,
                             ntime=int(time.time()), coinbase_value=subsidy, payout_script=self.payout_script,
                             txids=txids, coinbase_message=self.msg)
