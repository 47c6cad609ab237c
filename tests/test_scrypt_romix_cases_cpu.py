"""tests/scrypt_romix_cases.py held to its own conditions, without a GPU.

The GPU module trusts four things of the cases module: that the header pool is what it says, that no batch is larger
than the buffers it runs on, that the variant table reaches every ``case`` of ``launch_scrypt_romix``, and that the
helper which finishes a digest from a post-ROMix state (``scrypt_digest_from_state``) is right. The last is shown on
one header with a ROMix written out in plain Python, so the search-path tests do not take the helper on trust. The
comparison itself is shown to be able to fail: against a pool with one bit of one digest flipped it names that index.
"""
import hashlib
import re
from pathlib import Path

import pytest

import scrypt_romix_cases as C

ROOT = Path(__file__).resolve().parent.parent


def _native_or_skip():
    from otedama_amd.ops.native import load

    N = load(build_if_missing=False)
    if N is None:
        pytest.skip("the native extension is not built")
    return N


def test_the_pool_is_deterministic_and_holds_the_special_headers():
    a, b = C.build_headers(), C.build_headers()
    assert a == b and len(a) == C.POOL_SIZE == 512
    assert all(len(h) == 80 for h in a) and len(set(a)) == len(a)
    assert a[1] == bytes(80) and a[2] == b"\xff" * 80
    ka = C.known_answer_header()
    if ka is not None:
        assert a[3] == ka
    hs, digests = C.pool()
    assert hs == a and len(digests) == len(hs)
    for i in (0, 1, 2, 3, 511):
        assert digests[i] == hashlib.scrypt(hs[i], salt=hs[i], n=1024, r=1, p=1, dklen=32)
    assert C.pool() is C.pool()  # computed once


def test_every_size_fits_the_grid_it_runs_on():
    assert C.SIZES == (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)
    for g in (64, 128, 256):  # each granularity with both neighbours
        assert {g - 1, g, g + 1} <= set(C.SIZES)
    for v in C.VARIANTS:
        sizes = C.CHILD_SIZES if v.child else C.SIZES
        assert max(sizes) <= C.capacity(v) and max(sizes) <= C.POOL_SIZE, v.id
        assert v.grid == (4 if v.id == "seg6-grid1" else 2), v.id
    assert set(C.CHILD_SIZES) <= set(C.SIZES)
    assert C.POISON != 0 and C.CANARY not in (0, C.POISON)


def test_search_cases_fit_their_buffers_and_leave_the_first_trip():
    assert C.SEARCH_BASE == 0xFFFFFF00 and C.SEARCH_LANES == 700
    ids = [c.id for c in C.SEARCH_CASES]
    assert len(set(ids)) == len(ids)
    for c in C.SEARCH_CASES:
        per_trip = c.grid * 256 * (2 if c.kernel == "coop2" else 1)
        assert c.count <= per_trip * c.lanes_per_slot <= 1024, c.id  # the batch, and the hit buffer of 1024
        assert c.count > 256 and C.SEARCH_BASE + c.count > 1 << 32, c.id  # past the first trip; wraps
    by_id = {c.id: c for c in C.SEARCH_CASES}
    assert by_id["lane-gap2-3trips-700"].count > 2 * 256          # a third, ragged trip
    assert by_id["coop-2trips-389"].count > 256 and (389 + 63) // 64 * 64 == 448
    assert by_id["coop2-321"].count % 128 > 64                    # the B stream of the last wave is partial
    assert by_id["coop2-2trips-700"].count > 512
    fb = by_id["seg4-falls-back-389"]                             # above one hash per lane slot: no segments
    assert fb.env == {"OTEDAMA_SCRYPT_SEGMENTS": "4"} and (fb.count + 63) // 64 * 64 > fb.grid * 256
    assert C.search_window(3) == [0xFFFFFF00, 0xFFFFFF01, 0xFFFFFF02]
    assert C.search_window(300)[0] == 0 and len(set(C.search_window(700))) == 700


def _switch_cases() -> list[str]:
    """The ``case`` labels of the switch in launch_scrypt_romix, as written in the source."""
    src = (ROOT / "csrc" / "kernels" / "scrypt_search.hip").read_text()
    body = src[src.index("hipError_t launch_scrypt_romix("):src.index("hipError_t launch_scrypt_search(")]
    return re.findall(r"^\s*case\s+(\w+)\s*:", body, flags=re.M)


def test_the_variants_cover_every_case_of_the_launcher():
    N = _native_or_skip()
    ids = [v.id for v in C.VARIANTS]
    assert len(set(ids)) == len(ids)
    assert set(ids) == {"lane1", "lane2", "lane4", "w8", "coop", "coop2", "split", "seg1", "seg3", "seg8", "seg64",
                        "seg6-grid1", "seg32-resident", "coop-nopoll"}
    labels = _switch_cases()
    assert len(labels) == 7, labels

    def code(label):  # kScryptLaneW8 -> SCRYPT_LANE_W8
        return int(label) if label.isdigit() else getattr(N, re.sub(r"(?<=[a-z0-9])(?=[A-Z])", "_", label[1:]).upper())

    assert {code(x) for x in labels} == {C.gap_code(N, v) for v in C.VARIANTS}
    assert {code(x) for x in labels} == {1, 2, 4, N.SCRYPT_LANE_W8, N.SCRYPT_COOP, N.SCRYPT_COOP2, N.SCRYPT_COOP_SPLIT}
    # inside `case kScryptCoop` the environment chooses among four kernels: each choice has a variant
    coop = [v for v in C.VARIANTS if C.gap_code(N, v) == N.SCRYPT_COOP]
    assert {v.segments for v in coop} >= {0, 1, 3, 6, 8, 32, 64}
    assert {v.env.get("OTEDAMA_SCRYPT_SEG_GRID") for v in coop} == {None, "1", "resident"}
    assert [v.id for v in C.VARIANTS if v.child] == ["coop-nopoll"]
    assert C.variant("coop-nopoll").env == {"OTEDAMA_SCRYPT_POLL": "0"}
    assert all(N.scrypt_scratch_bytes(v.grid, C.gap_code(N, v)) <= 128 << 20 for v in C.VARIANTS)


def test_digest_from_state_inverts_a_plain_python_romix():
    from otedama_amd.ops.smoke_checks import scrypt_digest_from_state

    h = C.build_headers()[0]
    state = C.post_romix_state(h)
    assert len(state) == 128
    assert scrypt_digest_from_state(h, state) == C.pool()[1][0]
    flipped = bytes([state[0] ^ 1]) + state[1:]
    assert scrypt_digest_from_state(h, flipped) != C.pool()[1][0]
    assert scrypt_digest_from_state(h, bytes([C.POISON]) * 128) != C.pool()[1][0]


def test_the_comparison_names_a_flipped_digest():
    _, want = C.pool()
    C.assert_digests_equal(list(want), want, "self")
    k = 389
    wrong = list(want)
    wrong[k] = wrong[k][:17] + bytes([wrong[k][17] ^ 0x10]) + wrong[k][18:]
    assert C.mismatches(list(want), wrong) == [k]
    with pytest.raises(AssertionError, match=r"1 of 512 digests differ, first indices \[389\]"):
        C.assert_digests_equal(list(want), wrong, "one bit flipped")
