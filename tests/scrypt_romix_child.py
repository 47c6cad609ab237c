"""The digest-path check of tests/test_scrypt_romix_bytes_gpu.py in a process of its own.

``python tests/scrypt_romix_child.py <variant id>``

OTEDAMA_SCRYPT_POLL is read once per process, so the parent cannot reach ``otd_scrypt_romix_coop<2, 1024>`` after it
has launched anything: it starts this script with the variant's environment instead, one child at a time. The script
asserts that the launch file reports the mode the environment asks for, runs the variant's digest launches at
scrypt_romix_cases.CHILD_SIZES on poisoned buffers and prints one JSON line with, per size, the indices whose digest
differs from hashlib.scrypt and whether the canary rows were kept. The parent asserts on that line.

Exit status: 0 = the line is printed (whatever it says); non-zero = the mode check failed or a launch raised.
"""
import json
import os
import sys
from pathlib import Path

ROOT = str(Path(__file__).resolve().parent.parent)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import scrypt_romix_cases as C  # noqa: E402 - this file's directory is sys.path[0]


def main(argv):
    if len(argv) != 2 or argv[1] not in [v.id for v in C.VARIANTS]:
        print(__doc__, file=sys.stderr)
        return 2
    v = C.variant(argv[1])
    for var in C.ENV_VARS:
        assert os.environ.get(var) == v.env.get(var), (var, os.environ.get(var))
    N = C.native()
    mode = N._scrypt_romix_mode()
    assert mode["write_polls"] is (v.env.get("OTEDAMA_SCRYPT_POLL", "")[:1] != "0"), mode
    assert mode["segments"] == v.segments, mode
    rig = C.DigestRig(N, C.gap_code(N, v), v.grid)
    res = C.check_digest_sizes(rig, C.CHILD_SIZES)
    print(json.dumps({"variant": v.id, "write_polls": mode["write_polls"], "segments": mode["segments"],
                      "sizes": {str(n): r for n, r in res.items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
