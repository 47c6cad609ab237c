"""The pause / resume / switch scenario of tests/test_miner_modes_gpu.py in a process of its own.

``python tests/miner_mode_child.py <algo> <out.json>``

OTEDAMA_SCRYPT_POLL and OTEDAMA_X11_MIDPOLL are read once per process, so a test cannot flip them after its process
has launched anything: it starts this script with the variable in the environment instead, one at a time and while it
holds no miner and no search object itself. The script runs the scenario (miner_exact_cases.run_scenario) and writes
the polls, the stats snapshots and what the launch files say about their mode as JSON; the parent, whose environment
is the default, computes the reference and asserts. With OTEDAMA_SCRYPT_POLL=0 the miner launches another ROMix
template instance (no scalar polls in the write loop), so a scrypt child first holds the ops-API search, which launches
the same instance in this process, to hashlib.scrypt.

Exit status: 0 = the scenario ran and the file is written; non-zero = a failed check, a wait that ran out, or a miner
that reports ``faulted``.
"""
import hashlib
import json
import os
import struct
import sys
import time
from pathlib import Path

ROOT = str(Path(__file__).resolve().parent.parent)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import miner_exact_cases as C  # noqa: E402 - this file's directory is sys.path[0]


def _off(var):
    return os.environ.get(var, "")[:1] == "0"


def launch_modes():
    N = C._native()
    mode = N._scrypt_romix_mode()
    return {"write_polls": mode["write_polls"], "segments": mode["segments"],
            "x11_midstage_polls": N.x11_midstage_polls()}


def scrypt_ops_equal_hashlib():
    """The comparison tests/test_gpu_kernels.py makes for the default instance, here for whichever instance this
    process's environment selects: every hit of a 1-in-4 target over n nonces against hashlib.scrypt. n = 200 is not
    a multiple of 64; 512 nonces on one block of 256 lane slots use every pad slot twice."""
    from otedama_amd.models.header import int_to_hash
    from otedama_amd.ops.search import ScryptSearch

    target_int = (1 << 254) - 1
    checked = []
    for n, base, kw in ((192, 5000, {}), (200, 5000, {}), (512, 0, {"lanes_per_slot": 2})):
        hdr = (hashlib.sha256(f"modes-child-ops-{n}".encode()).digest() * 3)[:76] + bytes(4)
        sc = ScryptSearch("cuda:0", grid=1, cap=1024, kernel="coop", **kw)
        assert sc.kernel == "coop"
        got = sorted(sc.search(hdr, int_to_hash(target_int), base, n))
        del sc
        ref = []
        for nonce in range(base, base + n):
            h80 = hdr[:76] + struct.pack("<I", nonce)
            if int.from_bytes(hashlib.scrypt(h80, salt=h80, n=1024, r=1, p=1, dklen=32), "little") <= target_int:
                ref.append(nonce)
        assert got == ref and 0 < len(ref) < n, (n, len(got), len(ref), sorted(set(got) ^ set(ref))[:8])
        checked.append([n, len(ref)])
    return checked


def main(argv):
    if len(argv) != 3 or argv[1] not in C.SCENARIO:
        print(__doc__, file=sys.stderr)
        return 2
    algo, out = argv[1], argv[2]
    t0 = time.monotonic()
    modes = launch_modes()
    assert modes["write_polls"] is not _off("OTEDAMA_SCRYPT_POLL"), modes
    assert modes["x11_midstage_polls"] is not _off("OTEDAMA_X11_MIDPOLL"), modes
    ops = scrypt_ops_equal_hashlib() if algo == "scrypt" else None
    t1 = time.monotonic()
    try:
        r = C.run_scenario(algo, "child", evidence=launch_modes)
    except BaseException as e:  # a wait that ran out or a faulted miner (pytest.fail): say it and leave
        print(f"scenario failed: {e!r}", file=sys.stderr)
        return 1
    if any(r[st]["faulted"] for st in ("st1", "st2", "st_a", "st3")):
        print(f"the miner faulted: {r['st3']}", file=sys.stderr)
        return 1
    assert r["evidence"] == modes, (r["evidence"], modes)
    r = C.scenario_to_json(r)
    r["ops_checked"] = ops
    r["seconds"] = {"ops": round(t1 - t0, 3), "scenario": round(time.monotonic() - t1, 3)}
    Path(out).write_text(json.dumps(r))
    print(json.dumps({"algo": algo, "modes": modes, "ops_checked": ops, "seconds": r["seconds"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
