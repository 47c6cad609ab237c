"""Shared helpers of the miner exactness tests (test_miner_exact_gpu.py, test_miner_modes_gpu.py, and the child
process miner_mode_child.py): jobs from seeds, waiting on ``stats()``, the region a cursor stands for, its reference
hits from the ops-API search kernels filtered by host digests, and the one assertion that holds the polled shares to
that reference. The second half is the pause / resume / switch scenario that the mode tests run once per mode, and its
checks. Everything here is deterministic: headers come from hashlib."""
import hashlib
import os
import struct
import time

import pytest

DEADLINE_S = 40.0  # every wait; a miss fails the test with the stats in its message
NONCES = 1 << 32
QUEUE_CAP = 1 << 20

# The variables that select the miner and launch modes under test. The reference must run with none of them set.
MODE_VARS = ("OTEDAMA_SEARCH_STREAMS", "OTEDAMA_HOST_ABORT", "OTEDAMA_RESERVE_CUS", "OTEDAMA_SCRYPT_HALVES",
             "OTEDAMA_SCRYPT_SEGMENTS", "OTEDAMA_SCRYPT_SEG_GRID", "OTEDAMA_SCRYPT_POLL", "OTEDAMA_X11_OVERLAP",
             "OTEDAMA_X11_MIDPOLL")


def _native():
    from otedama_amd.ops.native import require_native

    return require_native()


def _header(seed: str) -> bytes:
    body = hashlib.sha256(seed.encode()).digest() * 3
    return struct.pack("<I", 0x20000000) + body[:72] + bytes(4)


def _job(seed, target_int, epoch, job_id, algo="sha256d", **kw):
    from otedama_amd.models.header import int_to_hash

    return dict({"header": _header(seed), "target": int_to_hash(target_int), "epoch": epoch, "job_id": job_id,
                 "algo": algo}, **kw)


def _wait(m, pred, what):
    end = time.monotonic() + DEADLINE_S
    while True:
        st = m.stats()
        if st["faulted"]:
            pytest.fail(f"{what}: the miner faulted: {st}")
        if pred(st):
            return st
        if time.monotonic() > end:
            pytest.fail(f"{what}: not reached within {DEADLINE_S} s: {st}")
        time.sleep(0.001)


def _pause(m):
    """Pause and wait until the loop itself reports the batches in flight finished and their hits handed on."""
    m.set_job(None)
    return _wait(m, lambda st: st["idle"] and st["candidates"] == st["shares"] + st["rejected_candidates"], "pause")


def _key(s):
    return (s["version"], s["ntime"], s["extranonce2"], s["nonce"])


# ---------------------------------------------------------------------------------------------- the searched region

def searched_region(job, stats, sha_variants):
    """Per stripe group the miner has searched: (kind, [(header80, version, ntime, extranonce2)], window). The groups
    before stripe position cursor_k in full, then [0, cursor_nonce_off) of the group at cursor_k. kind "v" (version-
    parallel: the window counts W3, the nonces are bswap(W3)), "k", "single", "scrypt" or "x11" (the nonce itself)."""
    N = _native()
    algo = job.get("algo", "sha256d")
    start, stride = job.get("variant_start", 0), job.get("variant_stride", 1)
    space = N.variant_space(job)
    widest = N._launch_plan_rules(sha_variants=sha_variants, run=128)["layout"][0] if algo == "sha256d" else 1
    groups, k = [], 0
    while k < stats["cursor_k"] or (k == stats["cursor_k"] and stats["cursor_nonce_off"] > 0):
        assert start + k * stride < space, (k, stats)  # the cursor never passes the end of the stripe by a group
        run = [N.variant_header(job, start + k * stride)]
        while len(run) < widest and start + (k + len(run)) * stride < space:
            nxt = N.variant_header(job, start + (k + len(run)) * stride)
            if nxt[0][64:76] != run[0][0][64:76]:
                break
            run.append(nxt)
        nvar, use_v = (N._launch_plan_rules(sha_variants=sha_variants, run=len(run))["layout"] if algo == "sha256d"
                       else (1, False))
        kind = algo if algo != "sha256d" else "v" if use_v else "k" if nvar > 1 else "single"
        groups.append((kind, run[:nvar], NONCES if k < stats["cursor_k"] else stats["cursor_nonce_off"]))
        k += nvar
    assert k == stats["cursor_k"] or (k > stats["cursor_k"] and groups[-1][2] < NONCES), (k, stats)  # a group boundary
    return groups


def region_hashes(region):
    return sum(len(variants) * window for _, variants, window in region)


def _digest(algo, h80):
    if algo == "scrypt":
        return hashlib.scrypt(h80, salt=h80, n=1024, r=1, p=1, dklen=32)
    if algo == "x11":
        return _native().x11(h80)
    return hashlib.sha256(hashlib.sha256(h80).digest()).digest()


def _chunk(window, per_position, target_int, cap):
    """Positions per reference launch: the kernels pass a hash whose top word is <= the target's, so at most
    cap / 8 expected candidates per launch (every launch's count is still asserted against cap)."""
    p = ((target_int >> 224) + 1) / 2.0 ** 32
    c = NONCES
    while c > 1 and c * per_position * p > cap / 8:
        c >>= 1
    return min(c, window) if window else c


def assert_default_modes():
    """The reference is the ops API as it is by default: with a mode variable still set it would take the path under
    test too (OTEDAMA_SCRYPT_SEGMENTS is read at every launch) and the comparison would hold the code to itself."""
    left = {v: os.environ[v] for v in MODE_VARS if v in os.environ}
    assert not left, f"mode variables still set when the reference starts: {left}"
    assert _native()._scrypt_romix_mode()["segments"] == 0


def reference_hits(region, target_int):
    """{(version, ntime, extranonce2, nonce)} of the region: candidates from the ops-API search kernels, each kept only
    if its host digest passes the full 256-bit compare."""
    import torch

    from otedama_amd.models.header import int_to_hash
    from otedama_amd.ops.search import ScryptSearch, Sha256dSearch, Sha256dSearchV, X11Search

    assert_default_modes()
    tgt = int_to_hash(target_int)
    cap = 1 << 14
    made = {}

    def searcher(kind):
        if kind not in made:
            made[kind] = (Sha256dSearchV("cuda:0", cap=cap, chains=1, occupancy8=False) if kind == "v"
                          else ScryptSearch("cuda:0", cap=cap, grid=1024) if kind == "scrypt"
                          else X11Search("cuda:0", cap=cap) if kind == "x11"
                          else Sha256dSearch("cuda:0", cap=cap))
        return made[kind]

    cands, s = [], None  # (algo, header80, version, ntime, extranonce2, nonce)
    for kind, variants, window in region:
        s = searcher(kind)
        if kind == "v":
            assert len(variants) % 64 == 0
            for lo in range(0, len(variants), 64):
                part = variants[lo:lo + 64]
                prep = s.prepare([v[0] for v in part], tgt)
                step = _chunk(window, 64, target_int, cap)
                for base in range(0, window, step):
                    r = s.launch(prep, base, min(step, window - base))
                    torch.cuda.synchronize()
                    assert r.count() <= cap, r.count()
                    cands += [("sha256d",) + part[vi] + (nonce,) for nonce, vi in r.hits()]
            continue
        algo = kind if kind in ("scrypt", "x11") else "sha256d"
        for v in variants:
            params = s.prepare(v[0], tgt)
            step = _chunk(window, 1, target_int, cap)
            if algo != "sha256d":
                step = min(step, s.batch)
            for base in range(0, window, step):
                r = s.launch(params, base, min(step, window - base))
                torch.cuda.synchronize()
                assert r.count() <= cap, r.count()
                cands += [(algo,) + v + (nonce,) for nonce in r.nonces()]
    del s
    made.clear()
    torch.cuda.empty_cache()  # the reference's scrypt pad (32 GiB) and digest planes do not outlive it
    ref = set()
    for algo, hdr, version, ntime, en2, nonce in cands:
        d = _digest(algo, hdr[:76] + struct.pack("<I", nonce))
        if int.from_bytes(d, "little") <= target_int:
            ref.add((version, ntime, en2, nonce))
    return ref


def check_shares(job, shares, target_int):
    """Re-hash every share on the host from its own fields (the jobs here have no coinbase: extranonce2 is 0)."""
    hdr, algo = job["header"], job.get("algo", "sha256d")
    for s in shares:
        assert s["extranonce2"] == 0 and s["job_id"] == job["job_id"], s
        h80 = (struct.pack("<I", s["version"]) + hdr[4:68] + struct.pack("<I", s["ntime"]) + hdr[72:76]
               + struct.pack("<I", s["nonce"]))
        d = _digest(algo, h80)
        assert d == s["hash"] and int.from_bytes(d, "little") <= target_int, s


def assert_exact(shares, ref, st, hashes=None, other_shares=0):
    """The one assertion of every case: the polled shares are the reference set, each once, and the counters agree.
    `hashes`: the size of the region, for a miner that ran this work only (no launch aborted); `other_shares`: shares
    of the same miner that belong to other work."""
    keys = [_key(s) for s in shares]
    got = set(keys)
    lost, extra = ref - got, got - ref  # got == ref, said so that a failure names a few keys instead of both sets
    assert not lost and not extra, {"n_ref": len(ref), "n_lost": len(lost), "lost": sorted(lost)[:8],
                                    "n_extra": len(extra), "extra": sorted(extra)[:8], "stats": st}
    assert len(shares) == len(got) == st["shares"] - other_shares, (len(shares), len(got), other_shares, st)
    assert st["ring_overflow"] == st["dropped"] == st["verify_dropped"] == 0, st
    assert st["candidates"] == st["shares"] + st["rejected_candidates"], st
    if hashes is not None:
        assert st["aborted_launches"] == 0, st
        assert st["hashes"] == hashes, (st["hashes"], hashes)


def _assert_both_slots(ref, st):
    """Launch i covers nonces [i * launch_hashes, (i + 1) * launch_hashes) and the two slots take turns: the reference
    alone must put hits into launches of either parity, so the buffers of both slots are held to it."""
    by_parity = [0, 0]
    for k in ref:
        by_parity[(k[3] // st["launch_hashes"]) % 2] += 1
    assert min(by_parity) >= 20, (by_parity, st)


# ------------------------------------------------------------- the pause / resume / switch scenario of the mode tests
#
# Every job of the scenario is one header variant (no version mask, no ntime roll), so a cursor is one number: the
# position cursor_k * 2^32 + cursor_nonce_off in a stripe of variant_space * 2^32 nonces.

SCENARIO = {  # algo -> (target, batch_nonces). SHA-256d: launches capped to 2^29 nonces by the target.
    "scrypt": ((1 << 244) - 1, 1 << 23),
    "x11": ((20 << 233) - 1, 1 << 23),
    "sha256d": ((4000 << 224) - 1, 1 << 30),
}


def position(st):
    return st["cursor_k"] * NONCES + st["cursor_nonce_off"]


def at_position(st, pos, job):
    """`st` with its cursor moved to `pos`, at most the end of the job's stripe (one variant per stripe position)."""
    pos = min(pos, _native().variant_space(job) * NONCES)
    return dict(st, cursor_k=pos // NONCES, cursor_nonce_off=pos % NONCES)


def _queued(st, epoch, launches, beyond=0):
    """At least `launches` launches of the work with control-plane epoch `epoch` queued past position `beyond`."""
    return (st["variant_epoch"] == epoch and st["launch_hashes"] > 0
            and position(st) >= beyond + launches * st["launch_hashes"])


def run_scenario(algo, tag, evidence=None):
    """Jobs A and B of `algo` on one miner: run A, pause, poll; resume A, pause, poll; resume A, switch to B the moment
    A's cursor has moved, run B, pause, poll. `evidence()` is called while the miner lives and its result returned with
    the polls and the stats snapshots. No reference is computed here: the miner's mode may still be in the
    environment."""
    N = _native()
    target, batch = SCENARIO[algo]
    job_a = _job(f"modes-{tag}-a", target, 1, "a", algo=algo)
    job_b = _job(f"modes-{tag}-b", target, 2, "b", algo=algo)
    m = N.GpuMiner(0, "gpu-0", batch_nonces=batch, queue_cap=QUEUE_CAP)
    try:
        m.set_job(job_a)
        m.start()
        _wait(m, lambda st: _queued(st, 1, 4), "4 launches of A")
        st1 = _pause(m)
        poll1 = m.poll(QUEUE_CAP)
        m.set_job(dict(job_a))  # the same work again: a resume, not new work
        _wait(m, lambda st: _queued(st, 1, 2, position(st1)), "2 more launches of A")
        st2 = _pause(m)
        poll2 = m.poll(QUEUE_CAP)
        m.set_job(dict(job_a))
        # (a SHA-256d stripe is 8 launches: if the pauses came late and it is all queued already, nothing can move)
        end = N.variant_space(job_a) * NONCES
        st_a = _wait(m, lambda st: position(st) > position(st2) or position(st2) == end,
                     "A's cursor past the second pause")
        m.set_job(job_b)
        _wait(m, lambda st: _queued(st, 2, 4), "4 launches of B")
        st3 = _pause(m)
        poll3 = m.poll(QUEUE_CAP)
        seen = evidence() if evidence else None
    finally:
        m.stop()
    del m
    return {"algo": algo, "tag": tag, "cus": N.gpu_cu_count(0), "evidence": seen, "st1": st1, "st2": st2, "st_a": st_a,
            "st3": st3, "poll1": poll1, "poll2": poll2, "poll3": poll3}


def check_scenario(r, expect):
    """Every assertion on one run of run_scenario; `expect` maps stats fields to the values the mode must show (with
    `launch_hashes` given per CU count by the caller). Computes the references, so the miner is gone and the
    environment is the default by now. Returns the reference counts, for the record."""
    algo, tag = r["algo"], r["tag"]
    target, _ = SCENARIO[algo]
    job_a = _job(f"modes-{tag}-a", target, 1, "a", algo=algo)
    job_b = _job(f"modes-{tag}-b", target, 2, "b", algo=algo)
    st1, st2, st_a, st3 = r["st1"], r["st2"], r["st_a"], r["st3"]
    poll1, poll2, poll3 = r["poll1"], r["poll2"], r["poll3"]
    for st in (st1, st2, st_a, st3):
        assert not st["faulted"], st
        for field, want in expect.items():
            assert st[field] == want and type(st[field]) is type(want), (field, want, st)
    lh = st2["launch_hashes"]
    assert st1["launch_hashes"] == st3["launch_hashes"] == lh, (st1, st3)

    # A, first and second pause: exact, nothing twice, the counters of a miner that ran this work only
    p1, p2 = position(st1), position(st2)
    assert p1 >= 4 * lh and p1 % lh == 0 and st1["inflight"] == 0 and st1["aborted_launches"] == 0, st1
    assert p2 >= p1 + 2 * lh and p2 % lh == 0 and st2["inflight"] == 0, (st1, st2)
    assert st1["job_switches"] == st2["job_switches"] == 1, (st1, st2)
    assert st2["launches"] * lh == p2, st2
    assert all(s["job_id"] == "a" for s in poll1 + poll2)
    check_shares(job_a, poll1 + poll2, target)
    furthest_a = at_position(st_a, position(st_a) + 2 * lh, job_a)
    region_a = searched_region(job_a, furthest_a, 128)
    assert {kind for kind, _, _ in region_a} == {"single" if algo == "sha256d" else algo}, region_a
    ref_a = reference_hits(region_a, target)
    assert position(furthest_a) <= NONCES  # one variant: a share's nonce is its position

    def of(ref, lo, hi):
        return {k for k in ref if lo <= k[3] < hi}


    ref1, ref2 = of(ref_a, 0, p1), of(ref_a, 0, p2)
    k1, k2 = {_key(s) for s in poll1}, {_key(s) for s in poll2}
    assert not k1 & k2
    assert_exact(poll1, ref1, st1, hashes=p1)
    assert st2["hashes"] == p2 and st2["aborted_launches"] == 0, st2
    assert_exact(poll1 + poll2, ref2, st2, hashes=p2)
    _assert_both_slots(ref2, st2)

    # the switch: B exact from nonce 0; A's last shares sound, new, and inside what A can have reached
    a3 = [s for s in poll3 if s["job_id"] == "a"]
    b3 = [s for s in poll3 if s["job_id"] == "b"]
    assert len(a3) + len(b3) == len(poll3) and b3, (len(a3), len(b3), len(poll3))
    check_shares(job_a, a3, target)
    check_shares(job_b, b3, target)
    assert st3["job_switches"] == 2 and st3["inflight"] == 0 and st3["variant_epoch"] == 2, st3
    p3 = position(st3)
    assert p3 >= 4 * lh and p3 % lh == 0, st3
    ref_b = reference_hits(searched_region(job_b, st3, 128), target)
    _assert_both_slots(ref_b, st3)
    keys_a3 = [_key(s) for s in a3]
    assert len(set(keys_a3)) == len(keys_a3), len(keys_a3)
    assert not set(keys_a3) & (k1 | k2)
    late = set(keys_a3) - of(ref_a, p2, position(furthest_a))
    assert not late, (sorted(late)[:8], st2, st_a)
    assert_exact(b3, ref_b, st3, other_shares=len(poll1) + len(poll2) + len(a3))
    return {"ref_a_st2": len(ref2), "ref_b": len(ref_b), "launches_a_st2": p2 // lh, "launches_b": p3 // lh,
            "a_after_st2": len(a3)}


def scenario_to_json(r):
    """The result of run_scenario with the shares' hashes as hex (for the child process)."""
    out = dict(r)
    for p in ("poll1", "poll2", "poll3"):
        out[p] = [dict(s, hash=s["hash"].hex()) for s in r[p]]
    return out


def scenario_from_json(r):
    out = dict(r)
    for p in ("poll1", "poll2", "poll3"):
        out[p] = [dict(s, hash=bytes.fromhex(s["hash"])) for s in r[p]]
    return out
