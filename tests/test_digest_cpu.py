"""The batch digest entry points that need no GPU: ``models.algorithms.hash_many`` on the CPU oracle, the native
module's digest launchers being present, and the torch-free imports the engine and the pool rely on."""
import os
import random
import subprocess
import sys

import pytest

from otedama_amd.models import algorithms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _headers(seed: int, n: int) -> list[bytes]:
    rng = random.Random(seed)
    return [bytes(rng.getrandbits(8) for _ in range(80)) for _ in range(n)]


@pytest.mark.parametrize("name,n", [("sha256d", 33), ("scrypt", 5), ("x11", 9)])
def test_hash_many_equals_the_oracle_one_by_one(name, n):
    hs = _headers(20 + n, n)
    got = algorithms.hash_many(name, hs)
    assert got == [algorithms.get(name).hash(h) for h in hs]
    assert all(len(d) == 32 for d in got) and len(set(got)) == n


def test_hash_many_accepts_any_sequence_of_bytes_like_headers():
    hs = _headers(3, 4)
    want = algorithms.hash_many("sha256d", hs)
    assert algorithms.hash_many("SHA256D", tuple(bytearray(h) for h in hs)) == want
    assert algorithms.hash_many("sha256d", []) == []


@pytest.mark.parametrize("name", ["sha256d", "x11"])
def test_hash_many_returns_the_genesis_hashes(name):
    hdr_hex, _nonce, display = algorithms.KNOWN_ANSWERS[name]
    hdr = bytes.fromhex(hdr_hex)
    got = algorithms.hash_many(name, [bytes(80), hdr, hdr])
    assert got[1][::-1].hex() == display and got[2] == got[1] and got[0] != got[1]


@pytest.mark.parametrize("name", ["sha256d", "scrypt", "x11"])
def test_hash_many_refuses_a_short_header(name):
    with pytest.raises(ValueError):
        algorithms.hash_many(name, [bytes(80), bytes(79)])
    with pytest.raises(ValueError):
        algorithms.hash_many(name, [bytes(81)])


def test_hash_many_refuses_an_unknown_algorithm():
    with pytest.raises(ValueError, match="unknown algorithm"):
        algorithms.hash_many("sha3", [bytes(80)])
    with pytest.raises(ValueError, match="unknown algorithm"):
        algorithms.hash_many("sha3", [])


def test_native_module_has_the_digest_launchers():
    from otedama_amd.ops.native import require_native

    n = require_native()
    for name in ("launch_sha256d_digest", "launch_scrypt_digest", "launch_x11_digest"):
        assert callable(getattr(n, name)), name


def test_digest_bindings_refuse_null_and_empty_launches_on_the_host():
    """The argument checks of the bindings run before any HIP call, so they hold on a machine without a GPU."""
    from otedama_amd.ops.native import require_native

    n = require_native()
    with pytest.raises(ValueError):
        n.launch_sha256d_digest(0, 1, 16, 0)
    with pytest.raises(ValueError):
        n.launch_sha256d_digest(16, 0, 16, 0)
    with pytest.raises(ValueError):
        n.launch_scrypt_digest(16, 513, 16, 16, n.SCRYPT_COOP, 16, 2, 0)  # n above grid * 256
    with pytest.raises(ValueError):
        n.launch_x11_digest(16, 16, 4, 5, 16, 0)  # n above stride


@pytest.mark.parametrize("module", ["otedama_amd.ops", "otedama_amd.models.algorithms"])
def test_import_stays_torch_free(module):
    code = (f"import sys; import {module}; from otedama_amd.models.algorithms import hash_many; "
            "assert len(hash_many('sha256d', [bytes(80)])[0]) == 32; print('torch' in sys.modules)")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "False"
