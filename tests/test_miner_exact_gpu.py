"""The native GpuMiner loop searches its stripe exactly once, hit for hit (MI355X).

The other miner tests re-hash some shares and count them statistically, so a loop that silently loses or repeats hits
passes them. Here the loop is held to a set equality. ``stats()`` gives the search cursor (``cursor_k``,
``cursor_nonce_off``) and ``idle``, the loop's own observation that nothing is in flight and nothing is left to queue
(docs/RUNTIME.md). After a pause (``set_job(None)`` lets the batches in flight run to their end) or at the end of the
stripe, everything before the cursor has been searched, so the shares polled from the miner must equal, as a set of
``(version, ntime, extranonce2, nonce)``, the reference hits of exactly that region: two launches in flight on two
streams and two buffer halves, the hit ring drained while the kernel runs, the per-launch variant table, the cached
group, the layout fallback, the cursor, pause / resume and the job switch are all inside that equality.

The reference hits come from the ops-API search kernels, which tests/test_gpu_kernels.py, test_search_edges_gpu.py
and test_digest_gpu.py pin to hashlib, the CPU scan and the native X11 chain. Where there is one, it is another
kernel than the miner's: the one-chain version-parallel build for the miner's two-chain groups, the single-header
kernel for its K-variant groups (a single-header group has only that kernel). Every reference candidate is then
filtered by a full 256-bit compare of a host digest (hashlib for SHA-256d and scrypt, the native CPU X11 chain), and
every miner share is re-hashed on the host from its own version, ntime, extranonce2 and nonce. The reference runs
after the miner is stopped and released, so two scrypt pads never coexist.

With every equality go the counters: no duplicate, ``shares`` = shares polled, nothing overflowed or dropped,
``candidates == shares + rejected_candidates``, no aborted launch, and ``hashes`` = the size of the region. The job
switch case cannot check ``hashes`` and ``aborted_launches``: the old work's last launches are aborted by design and
credited an estimate.

Sensitivity, checked once on scratch builds of gpu_miner.hip / launch_plan.h (host-side, in-bounds changes):
  * drain_ring handles a record only once the next one is published and stops one short of the final count (the last
    record of every launch is lost): the single-header and stride cases fail, the single-header one by exactly its
    four launches' last hits. The same change in the pass after completion alone is not observable: every record
    was consumed while its launch ran (``ring_hits == candidates``, also at 130 launches of 0.2 ms each), so that
    pass is a safety net that sees no record in practice.
  * SearchCursor::advance starts the next group one launch in: the layout-fallback and stride cases fail. (Adding
    ``count + 1`` instead of ``count`` on a group's last launch changes nothing: the offset is reset to 0 there.)
  * launch_scrypt gives both slots the X buffer of slot 0: the scrypt case fails (216 reference hits lost, none extra).
"""
import time

import pytest

from miner_exact_cases import (NONCES, QUEUE_CAP, _assert_both_slots, _job, _key, _native, _pause, _wait, assert_exact,
                               check_shares, reference_hits, region_hashes, searched_region)

pytestmark = pytest.mark.gpu


def _bswap(x: int) -> int:
    return int.from_bytes(x.to_bytes(4, "little"), "big")


def run_to_exhaustion(job, target_int, sha_variants, batch_nonces=1 << 30):
    """Run `job` until the loop reports its stripe exhausted and idle; a further 200 ms must add nothing. Returns
    (shares, stats, region, reference hits); the reference runs after the miner is gone."""
    N = _native()
    m = N.GpuMiner(0, "gpu-0", batch_nonces=batch_nonces, queue_cap=QUEUE_CAP, sha_variants=sha_variants)
    try:
        m.set_job(job)
        m.start()
        st = _wait(m, lambda st: st["idle"], "stripe exhausted")
        shares = m.poll(QUEUE_CAP)
        time.sleep(0.2)
        later, late_shares = m.stats(), m.poll(QUEUE_CAP)
    finally:
        m.stop()
    del m
    assert late_shares == [] and later["idle"], later
    for f in ("launches", "shares", "candidates", "hashes", "cursor_k", "cursor_nonce_off", "inflight"):
        assert later[f] == st[f], (f, st, later)
    assert st["inflight"] == 0 and st["cursor_nonce_off"] == 0, st
    region = searched_region(job, st, sha_variants)
    check_shares(job, shares, target_int)
    return shares, st, region, reference_hits(region, target_int)


# ------------------------------------------------------------------- 1, 2: two-chain SHA-256d, pause / resume / pause

V2_BATCH = 1 << 28
V2_PER = V2_BATCH // 128            # W3 positions per launch of a 128-variant group
V2_TARGET = (1000 << 224) - 1       # ~1000 candidates per 2^32 hashes: the launch cap (2^31) stays above the batch
# Pause after 32 launches, not the minimum of 16: the reference must hold every one of the 128 variant indices, and at
# ~17 expected hits per variant the chance that one has none is 128 * e^-17 < 1e-5 (at 16 launches, ~8 per variant,
# it would be 5%).
V2_FIRST, V2_MORE = 32, 8


@pytest.fixture(scope="module")
def two_chain_run():
    """One miner: run, pause, poll, resume the same work, pause, poll. The reference of the larger region is computed
    once; the first region's reference is its part below the first pause's cursor."""
    N = _native()
    job = _job("exact-v2", V2_TARGET, 1, "v2", version_mask=0x1FFFE000)
    m = N.GpuMiner(0, "gpu-0", batch_nonces=V2_BATCH, queue_cap=QUEUE_CAP)
    try:
        m.set_job(job)
        m.start()
        _wait(m, lambda st: st["cursor_nonce_off"] >= V2_FIRST * V2_PER, "first 32 launches")
        st1 = _pause(m)
        poll1 = m.poll(QUEUE_CAP)
        m.set_job(dict(job))  # the same work again: a resume, not new work
        _wait(m, lambda st: st["cursor_nonce_off"] >= st1["cursor_nonce_off"] + V2_MORE * V2_PER, "8 more launches")
        st2 = _pause(m)
        poll2 = m.poll(QUEUE_CAP)
    finally:
        m.stop()
    del m
    region2 = searched_region(job, st2, 128)
    assert [(kind, len(v)) for kind, v, _ in region2] == [("v", 128)], st2
    check_shares(job, poll1 + poll2, V2_TARGET)
    index_of = {v[1]: i for i, v in enumerate(region2[0][1])}  # version -> variant index
    return {"job": job, "st1": st1, "st2": st2, "poll1": poll1, "poll2": poll2, "index_of": index_of,
            "ref2": reference_hits(region2, V2_TARGET)}


def test_two_chain_pause_shares_equal_the_reference(two_chain_run):
    r = two_chain_run
    st1, off1 = r["st1"], r["st1"]["cursor_nonce_off"]
    assert st1["cursor_k"] == 0 and off1 >= V2_FIRST * V2_PER and off1 % V2_PER == 0 and st1["inflight"] == 0, st1
    assert st1["variant_launches"] == st1["launches"] == off1 // V2_PER, st1
    ref1 = {k for k in r["ref2"] if _bswap(k[3]) < off1}
    assert len(ref1) >= 500, len(ref1)
    assert {r["index_of"][k[0]] for k in ref1} == set(range(128))
    assert_exact(r["poll1"], ref1, st1, hashes=128 * off1)


def test_resume_neither_restarts_nor_skips(two_chain_run):
    r = two_chain_run
    st1, st2 = r["st1"], r["st2"]
    off1, off2 = st1["cursor_nonce_off"], st2["cursor_nonce_off"]
    assert st2["cursor_k"] == 0 and off2 >= off1 + V2_MORE * V2_PER and st2["inflight"] == 0, st2
    assert st2["job_switches"] == st1["job_switches"] == 1, st2  # the same work: no new generation, no cursor reset
    k1, k2 = {_key(s) for s in r["poll1"]}, {_key(s) for s in r["poll2"]}
    assert not k1 & k2
    assert not [k for k in k2 if _bswap(k[3]) < off1]  # nothing of the first region is searched again
    assert len(r["ref2"]) > len(k1)
    assert_exact(r["poll1"] + r["poll2"], r["ref2"], st2, hashes=128 * off2)


# ------------------------------------------------------------------------------- 3, 4, 5: stripes run to exhaustion

SHA_TARGET = (500 << 224) - 1  # ~500 candidates per 2^32 hashes


def test_layout_fallback_across_groups_to_exhaustion():
    """Variants 2..7 of a (2 version bits) x (2 ntimes) space with sha_variants 3: positions 0-1 share an ntime (K=2),
    2-4 the next (K=3), position 5 is left over (single)."""
    job = _job("exact-fallback", SHA_TARGET, 1, "fb", version_mask=0x00006000, ntime_roll=1, variant_start=2)
    shares, st, region, ref = run_to_exhaustion(job, SHA_TARGET, sha_variants=3)
    assert [(kind, len(v), w) for kind, v, w in region] == [("k", 2, NONCES), ("k", 3, NONCES), ("single", 1, NONCES)]
    assert st["cursor_k"] == 6 and 0 < st["variant_launches"] < st["launches"], st
    assert len({(v[1], v[2]) for _, vs, _ in region for v in vs}) == 6
    assert len(ref) >= 1500, len(ref)
    assert_exact(shares, ref, st, hashes=6 << 32)


def test_stride_two_stripe_to_exhaustion():
    """variant_start 1, stride 2 over 3 version bits: the four odd version variants, one K=4 group."""
    N = _native()
    job = _job("exact-stride", SHA_TARGET, 1, "st", version_mask=0x0000E000, variant_start=1, variant_stride=2)
    shares, st, region, ref = run_to_exhaustion(job, SHA_TARGET, sha_variants=4)
    assert [(kind, len(v), w) for kind, v, w in region] == [("k", 4, NONCES)]
    versions = {N.variant_header(job, v)[1] for v in (1, 3, 5, 7)}
    assert len(versions) == 4 and {s["version"] for s in shares} == versions
    assert st["cursor_k"] == 4 and st["variant_launches"] == st["launches"], st
    assert len(ref) >= 1000, len(ref)
    assert_exact(shares, ref, st, hashes=4 << 32)


def test_single_header_to_exhaustion():
    job = _job("exact-single", SHA_TARGET, 1, "sg")
    shares, st, region, ref = run_to_exhaustion(job, SHA_TARGET, sha_variants=1)
    assert [(kind, len(v), w) for kind, v, w in region] == [("single", 1, NONCES)]
    assert st["cursor_k"] == 1 and st["variant_launches"] == 0 and st["launches"] >= 4, st
    assert len(ref) >= 250, len(ref)
    assert_exact(shares, ref, st, hashes=NONCES)


# -------------------------------------------------------------- 6, 7: scrypt halves and X11 planes, both slots checked

def _paused_run(job, target_int, min_launches):
    """Run `job` for at least `min_launches` launches, pause, and return (shares, stats, region, reference hits)."""
    N = _native()
    m = N.GpuMiner(0, "gpu-0", batch_nonces=1 << 23, queue_cap=QUEUE_CAP)
    try:
        m.set_job(job)
        m.start()
        _wait(m, lambda st: st["launch_hashes"] > 0 and st["cursor_nonce_off"] >= min_launches * st["launch_hashes"],
              f"{min_launches} launches")
        st = _pause(m)
        shares = m.poll(QUEUE_CAP)
    finally:
        m.stop()
    del m
    assert st["cursor_k"] == 0 and st["inflight"] == 0 and st["launches"] >= min_launches, st
    assert st["cursor_nonce_off"] == st["launches"] * st["launch_hashes"], st
    region = searched_region(job, st, 128)
    check_shares(job, shares, target_int)
    return shares, st, region, reference_hits(region, target_int)


def test_scrypt_both_halves_pause_shares_equal_the_reference():
    target = (1 << 244) - 1  # 1 hash in 4096
    job = _job("exact-scrypt", target, 1, "sc", algo="scrypt")
    shares, st, region, ref = _paused_run(job, target, 4)
    assert [(kind, len(v)) for kind, v, _ in region] == [("scrypt", 1)]
    _assert_both_slots(ref, st)
    assert_exact(shares, ref, st, hashes=st["cursor_nonce_off"])


def test_x11_both_planes_pause_shares_equal_the_reference():
    target = (20 << 233) - 1  # ~20 hits per 2^23-nonce launch
    job = _job("exact-x11", target, 1, "x", algo="x11")
    shares, st, region, ref = _paused_run(job, target, 4)
    assert [(kind, len(v)) for kind, v, _ in region] == [("x11", 1)]
    assert st["launch_hashes"] == 1 << 23, st
    _assert_both_slots(ref, st)
    assert_exact(shares, ref, st, hashes=st["cursor_nonce_off"])


# ------------------------------------------------------------------------------------ 8: new work resets the cursor

def test_new_work_resets_the_cursor():
    """Job A (a 128-variant group) runs, job B (single header) replaces it and is paused. B's shares equal the
    reference of B's region from the cursor. A's last launches were aborted, so A's shares are held sound, unique and
    inside the furthest region A can have reached: its cursor just before the switch plus two launches."""
    N = _native()
    batch = 1 << 30
    per_a = batch // 128
    target_a, target_b = (1000 << 224) - 1, (4000 << 224) - 1  # B's launches are capped to 2^29 nonces
    job_a = _job("exact-switch-a", target_a, 1, "a", version_mask=0x1FFFE000)
    job_b = _job("exact-switch-b", target_b, 2, "b")
    m = N.GpuMiner(0, "gpu-0", batch_nonces=batch, queue_cap=QUEUE_CAP)
    try:
        m.set_job(job_a)
        m.start()
        st_a = _wait(m, lambda st: st["variant_epoch"] == 1 and st["cursor_nonce_off"] >= 4 * per_a, "4 launches of A")
        m.set_job(job_b)
        _wait(m, lambda st: st["variant_epoch"] == 2 and (st["cursor_k"] >= 1 or st["cursor_nonce_off"] >= 4 << 29),
              "4 launches of B")
        st = _pause(m)
        shares = m.poll(QUEUE_CAP)
    finally:
        m.stop()
    del m
    assert st_a["cursor_k"] == 0 and st["inflight"] == 0, (st_a, st)
    assert st["job_switches"] == 2 and st["launch_hashes"] == 1 << 29, st
    a = [s for s in shares if s["job_id"] == "a"]
    b = [s for s in shares if s["job_id"] == "b"]
    assert len(a) + len(b) == len(shares) and a and b
    check_shares(job_a, a, target_a)
    check_shares(job_b, b, target_b)
    region_b = searched_region(job_b, st, 128)
    assert [(kind, len(v)) for kind, v, _ in region_b] == [("single", 1)] and region_hashes(region_b) >= 4 << 29, st
    ref_b = reference_hits(region_b, target_b)
    assert len(ref_b) >= 1000, len(ref_b)
    furthest_a = dict(st_a, cursor_nonce_off=st_a["cursor_nonce_off"] + 2 * per_a)
    ref_a = reference_hits(searched_region(job_a, furthest_a, 128), target_a)
    keys_a = [_key(s) for s in a]
    assert len(set(keys_a)) == len(keys_a) and set(keys_a) <= ref_a, (len(keys_a), len(ref_a), st_a, st)
    assert_exact(b, ref_b, st, other_shares=len(a))
