"""Every scrypt ROMix kernel, every lane, byte for byte against hashlib (MI355X).

tests/test_digest_gpu.py compares one of the nine kernels ``launch_scrypt_romix`` can launch with ``hashlib.scrypt``
(``HeaderDigest`` hard-wires SCRYPT_COOP); the others were only seen through hit sets at a 1-in-4 target, one bit per
nonce. Here every variant of tests/scrypt_romix_cases.py goes through ``N.launch_scrypt_digest`` at the batch sizes
around the wave (64), ``coop2`` pair (128) and block (256) granularities, all n digests compared; and the search path
(``ScryptSearch``, all-ones target, a window that wraps 2^32) covers what one header per lane slot cannot reach: pad
slots used again on later grid-stride trips, ``coop2`` above grid * 256, and the launcher's fall-back from the
segmented kernel. There every lane's state is read from ``xbuf`` and finished with ``hashlib.pbkdf2_hmac``.

Every comparison is byte or set equality; there is no tolerance. All variants hash the same headers, so before each
launch the state buffer, the whole pad and the result rows are filled with a fixed byte: a ROMix that does nothing
leaves PBKDF2-out to hash the fill, one that skips its write phase or looks up an entry it never stored mixes the fill
into X, and either gives digests that differ from hashlib's with all but negligible probability. The 256 result rows
after the batch hold a canary and must keep it.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import scrypt_romix_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHILD = str(Path(__file__).resolve().parent / "scrypt_romix_child.py")
# An upper bound, not a wait: the child imports torch and the extension, hashes the pool on the CPU (~0.2-1.5 s) and
# runs two digest launches (tens of ms).
CHILD_TIMEOUT_S = 60


def _set_env(monkeypatch, env):
    """Exactly ``env`` of the ROMix variables; the once-per-process poll switch must be at its default here."""
    for var in C.ENV_VARS:
        if var in env:
            monkeypatch.setenv(var, env[var])
        else:
            monkeypatch.delenv(var, raising=False)
    assert "OTEDAMA_SCRYPT_POLL" not in env


def _assert_mode(N, segments):
    mode = N._scrypt_romix_mode()
    assert mode["segments"] == segments and mode["write_polls"] is True, mode


@pytest.mark.parametrize("vid", [v.id for v in C.VARIANTS if not v.child])
def test_digest_path_every_size_equals_hashlib(monkeypatch, vid):
    """One set of buffers per variant, every size of C.SIZES on it in turn (so the buffers are reused, poisoned anew
    each time): all n digests equal hashlib.scrypt's and the rows after row n keep the canary."""
    N = C.native()
    v = C.variant(vid)
    _set_env(monkeypatch, v.env)
    _assert_mode(N, v.segments)
    _, want = C.pool()
    rig = C.DigestRig(N, C.gap_code(N, v), v.grid, DEV)
    assert rig.scratch.numel() == N.scrypt_scratch_bytes(v.grid, C.gap_code(N, v))
    for n in C.SIZES:
        assert n <= C.capacity(v)
        rows, canary_kept = rig.run(n)
        C.assert_digests_equal(rows, want[:n], f"{vid} n={n}")
        assert canary_kept, f"{vid} n={n}: the rows after the batch were written"
    _assert_mode(N, v.segments)


def test_digest_path_names_a_flipped_oracle_bit(monkeypatch):
    """The comparison above can fail: the kernel's own output against a pool in which bit 4 of byte 17 of digest 130
    is flipped is refused, and the message names index 130."""
    N = C.native()
    _set_env(monkeypatch, {})
    _assert_mode(N, 0)
    _, want = C.pool()
    rows, canary_kept = C.DigestRig(N, N.SCRYPT_COOP2, 2, DEV).run(257)
    assert canary_kept
    C.assert_digests_equal(rows, want[:257], "coop2 n=257")
    wrong = list(want[:257])
    wrong[130] = wrong[130][:17] + bytes([wrong[130][17] ^ 0x10]) + wrong[130][18:]
    with pytest.raises(AssertionError, match=r"1 of 257 digests differ, first indices \[130\]"):
        C.assert_digests_equal(rows, wrong, "flipped")


def test_digest_path_without_write_polls_in_a_child():
    """OTEDAMA_SCRYPT_POLL=0 selects ``otd_scrypt_romix_coop<2, 1024>``; the switch is read once per process, so the
    check runs in one fresh child, which reports the mode it ran in and the differing indices per size."""
    v = C.variant("coop-nopoll")
    env = {k: val for k, val in os.environ.items() if k not in C.ENV_VARS}
    env.update(v.env)
    proc = subprocess.run([sys.executable, CHILD, v.id], env=env, capture_output=True, text=True,
                          timeout=CHILD_TIMEOUT_S)
    assert proc.returncode == 0, f"child exit {proc.returncode}:\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}"
    r = json.loads(proc.stdout.strip().splitlines()[-1])
    assert r["variant"] == v.id and r["write_polls"] is False and r["segments"] == 0, r
    assert sorted(r["sizes"]) == sorted(str(n) for n in C.CHILD_SIZES), r
    _, want = C.pool()
    for n in C.CHILD_SIZES:
        got = r["sizes"][str(n)]
        assert got["bad"] == [] and got["canary"] is True, (n, got["bad"][:8], got["canary"])
        assert got["first"] == want[0].hex()  # the child hashed this pool


@pytest.mark.parametrize("cid", [c.id for c in C.SEARCH_CASES])
def test_search_path_every_lane_equals_hashlib(monkeypatch, cid):
    """All-ones target over a window that wraps 2^32: the hit list is exactly the window, and the digest rebuilt from
    every lane's post-ROMix state equals hashlib.scrypt of that lane's header."""
    N = C.native()
    (c,) = [c for c in C.SEARCH_CASES if c.id == cid]
    _set_env(monkeypatch, c.env)
    _assert_mode(N, int(c.env.get("OTEDAMA_SCRYPT_SEGMENTS", 0)))
    hits, digests = C.run_search_case(N, c, DEV)
    assert len(hits) == c.count and sorted(hits) == C.search_window(c.count), (cid, len(hits))
    C.assert_digests_equal(digests, C.search_oracle()[:c.count], cid)
