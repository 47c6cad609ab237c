"""Job switches of scrypt and X11, and the miner modes docs/ENVIRONMENT.md offers, held to exact hits (MI355X).

tests/test_miner_exact_gpu.py holds the GpuMiner loop to a set equality with reference hits, but its only exact job
switch is SHA-256d to SHA-256d and every case runs the default mode. Here one scenario (miner_exact_cases.run_scenario)
runs once per algorithm and mode on one miner: job A runs, is paused and polled, resumed, paused and polled again,
resumed and then replaced by job B of the same algorithm the moment its cursor has moved; B runs and is paused. The
two pauses of A must each equal the reference of A's region at that cursor (nothing lost, nothing twice, ``hashes`` =
the cursor, no aborted launch); B's shares must equal the reference of B's region from nonce 0; and A's shares after
the second pause must be sound, new, and inside the region from the second pause's cursor to the cursor read just
before the switch plus the two launches that can be in flight. Both launch parities hold at least 20 reference hits
in A's and in B's region, so both slots' buffers are held to the reference.

A mode counts only if the run shows it was on: ``stats()`` carries ``search_streams``, ``scrypt_halves``,
``x11_overlap``, ``host_abort`` and ``reserved_cus``, ``launch_hashes`` follows from the layout, and the launch files
report their own switches (``_scrypt_romix_mode()``, ``x11_midstage_polls()``). The environment is set for the miner's
lifetime only; the reference runs afterwards and refuses to start with one of the variables still set.

The cross-algorithm case runs SHA-256d, scrypt, X11 and SHA-256d again on one miner (the pad and the planes are
allocated on first use while the other algorithm's batches retire), by default and with two CUs masked out of the
search streams. OTEDAMA_SCRYPT_POLL=0 and OTEDAMA_X11_MIDPOLL=0 are read once per process, so their scenario runs in
a child (miner_mode_child.py), one at a time, and the parent checks what the child wrote.

Reference hits on the first MI355X run (256 CUs; every case paused A after 6 launches and B after 4), A's region at
the second pause / B's region: scrypt default 794 / 508, HALVES=0 1611 / 1023, HALVES=0 with SEGMENTS=32 1535 / 991,
SEARCH_STREAMS=1 791 / 515, SCRYPT_POLL=0 782 / 554; X11 default 133 / 80, X11_OVERLAP=0 108 / 86, SEARCH_STREAMS=1
127 / 72, X11_MIDPOLL=0 99 / 70; SHA-256d HOST_ABORT=0 2917 / 2109, SEARCH_STREAMS=1 3004 / 2002. Cross-algorithm
(shares polled / reference of the job's furthest region): 1267 / 2988, 264 / 754, 50 / 134, and the last job exact at
2008; with two CUs reserved 1537 / 3123, 272 / 736, 55 / 139, 1954. The smallest parity count is X11's: B's four
launches of ~20 hits. In the scrypt and X11 cases A published nothing after the second pause (its relaunched batches
are aborted within the first millisecond; an aborted ROMix or X11 chain publishes nothing); SHA-256d published ~50.

Sensitivity, checked once on a scratch build of gpu_miner.hip (host-side, in-bounds changes; all 13 cases ran under
each):
  (a) Run::enqueue without the hipStreamWaitEvent(stream, prev->done, 0) of the shared-buffer chain: exactly the
      three shared-buffer cases fail, all at A's first pause, by lost hits and none extra: HALVES=0 770 of 1037,
      HALVES=0 with SEGMENTS=32 1034 of 1034, X11_OVERLAP=0 67 of 67. The other ten pass.
  (b) launch_x11 gives both slots plane 0 while overlap is on: X11 default (92 of 92 lost at the first pause), the
      X11_MIDPOLL=0 child (64 of 64) and both cross-algorithm cases (the X11 job yields no share at all) fail.
      X11_OVERLAP=0 (one plane anyway) and SEARCH_STREAMS=1 (one queue serialises the two batches) pass, as they must.
  (c) new work keeps the old cursor's nonce offset (only the stripe position is reset): every scrypt and X11 switch
      case, both children and both cross-algorithm cases fail on B (scrypt 876 of 1003, 2055 of 2332, 2035 of 2538,
      945 of 1090, child 945 of 1085; X11 166 of 197, 157 of 198, 161 of 191, child 154 of 176 lost; in the cross
      case scrypt, starting at SHA-256d's offset 2^31, is switched away before it publishes). The two SHA-256d cases
      pass, and cannot do otherwise under this mutation: the single-header stripe is 8 launches of 2^29, a resume
      queues two at once, so after pauses at 4 and 6 launches A's cursor has wrapped to offset 0 when B arrives, and
      keeping 0 is resetting. A SHA-256d cursor that is not 0 at the switch is in the cross-algorithm case (2^31, which
      failed) and in test_miner_exact_gpu.py::test_new_work_resets_the_cursor.
"""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import pytest

import miner_exact_cases as C

pytestmark = pytest.mark.gpu

CHILD = str(Path(__file__).resolve().parent / "miner_mode_child.py")
# The child's limit: three times its own default run (same scenario, no variable set: a fresh process that imports
# the extension, for scrypt runs the ops-level comparison and allocates the pad), rounded up to 10 s. Measured on
# the MI355X: scrypt 3.41 s (4.40 s in a second run: the same limit), X11 2.48 s (2.64 s).
CHILD_TIMEOUT_S = {"scrypt": 20, "x11": 10}

MODES = [  # (algo, environment, what every stats() snapshot must show besides launch_hashes)
    ("scrypt", {}, {"search_streams": 2, "scrypt_halves": True, "x11_overlap": True, "reserved_cus": 0}),
    ("scrypt", {"OTEDAMA_SCRYPT_HALVES": "0"}, {"search_streams": 2, "scrypt_halves": False}),
    ("scrypt", {"OTEDAMA_SCRYPT_HALVES": "0", "OTEDAMA_SCRYPT_SEGMENTS": "32"},
     {"search_streams": 2, "scrypt_halves": False}),
    ("scrypt", {"OTEDAMA_SEARCH_STREAMS": "1"}, {"search_streams": 1, "scrypt_halves": True}),
    ("x11", {}, {"search_streams": 2, "scrypt_halves": True, "x11_overlap": True, "reserved_cus": 0}),
    ("x11", {"OTEDAMA_X11_OVERLAP": "0"}, {"search_streams": 2, "x11_overlap": False}),
    ("x11", {"OTEDAMA_SEARCH_STREAMS": "1"}, {"search_streams": 1, "x11_overlap": True}),
    ("sha256d", {"OTEDAMA_HOST_ABORT": "0"}, {"search_streams": 2, "host_abort": False}),
    ("sha256d", {"OTEDAMA_SEARCH_STREAMS": "1"}, {"search_streams": 1}),
]


def _mode_id(env):
    return ",".join(f"{k[len('OTEDAMA_'):]}={v}" for k, v in env.items()) or "default"


def launch_hashes(algo, cus, scrypt_halves=True):
    """Hashes per launch of the scenario's jobs: the scrypt grid is 16 blocks of 256 lane slots per CU, split between
    the slots with halves on; X11 batches are 2^23; the SHA-256d target caps launches to 2^29."""
    if algo == "scrypt":
        return cus * 16 * 256 // (2 if scrypt_halves else 1)
    return 1 << 23 if algo == "x11" else 1 << 29


def _report(name, counts, seconds):
    print(f"\n[miner modes] {name}: {counts} in {seconds:.1f} s")


@pytest.mark.parametrize("algo,env,expect", MODES, ids=[f"{a}-{_mode_id(e)}" for a, e, _ in MODES])
def test_mode_pause_resume_switch_exact(monkeypatch, algo, env, expect):
    t0 = time.monotonic()
    N = C._native()
    for var in C.MODE_VARS:
        assert var not in os.environ, var
    with monkeypatch.context() as mp:
        for var, val in env.items():
            mp.setenv(var, val)
        r = C.run_scenario(algo, _mode_id(env), evidence=N._scrypt_romix_mode)
    assert r["evidence"]["segments"] == int(env.get("OTEDAMA_SCRYPT_SEGMENTS", 0)), r["evidence"]
    want = dict(expect, launch_hashes=launch_hashes(algo, N.gpu_cu_count(0), expect.get("scrypt_halves", True)))
    counts = C.check_scenario(r, want)
    _report(f"{algo} {_mode_id(env)}", counts, time.monotonic() - t0)


# -------------------------------------------------------------------------------------- one miner, three algorithms

@pytest.mark.parametrize("reserve", [None, "0,32"], ids=["default", "RESERVE_CUS=0,32"])
def test_cross_algorithm_switches(monkeypatch, reserve):
    """SHA-256d, scrypt, X11, SHA-256d on one miner, each for at least 4 launches, the last one paused: the last job
    exact from its cursor, every earlier one sound, free of duplicates and inside its last cursor plus two launches."""
    t0 = time.monotonic()
    N = C._native()
    tag = f"cross-{reserve or 'default'}"
    plan = [("sha256d", "1"), ("scrypt", "2"), ("x11", "3"), ("sha256d", "4")]
    jobs = [C._job(f"modes-{tag}-{jid}", C.SCENARIO[algo][0], i + 1, jid, algo=algo)
            for i, (algo, jid) in enumerate(plan)]
    for var in C.MODE_VARS:
        assert var not in os.environ, var
    before = []  # per job: the stats read just before the next set_job (the last: after the pause)
    with monkeypatch.context() as mp:
        if reserve:
            mp.setenv("OTEDAMA_RESERVE_CUS", reserve)
        m = N.GpuMiner(0, "gpu-0", batch_nonces=1 << 30, queue_cap=C.QUEUE_CAP)
        try:
            m.set_job(jobs[0])
            m.start()
            for i in range(len(jobs)):
                st = C._wait(m, lambda st: C._queued(st, i + 1, 4), f"4 launches of job {i + 1}")
                if i + 1 < len(jobs):
                    m.set_job(jobs[i + 1])
                before.append(st)
            before[-1] = C._pause(m)
            shares = m.poll(C.QUEUE_CAP)
        finally:
            m.stop()
        del m
    final = before[-1]
    cus = N.gpu_cu_count(0)
    assert not final["faulted"] and final["job_switches"] == 4 and final["inflight"] == 0, final
    assert final["reserved_cus"] == (2 if reserve else 0) and type(final["reserved_cus"]) is int, final
    assert final["search_streams"] == 2 and final["scrypt_halves"] is True and final["x11_overlap"] is True, final
    by_job = {jid: [s for s in shares if s["job_id"] == jid] for _, jid in plan}
    assert sum(len(v) for v in by_job.values()) == len(shares)
    counts = {}
    for (algo, jid), job, st in zip(plan, jobs, before):
        target, mine = C.SCENARIO[algo][0], by_job[jid]
        assert st["launch_hashes"] == launch_hashes(algo, cus), (algo, st)
        assert C.position(st) >= 4 * st["launch_hashes"] and C.position(st) % st["launch_hashes"] == 0, st
        C.check_shares(job, mine, target)
        keys = [C._key(s) for s in mine]
        assert mine and len(set(keys)) == len(keys), (jid, len(keys))
        if job is jobs[-1]:
            ref = C.reference_hits(C.searched_region(job, st, 128), target)
            C.assert_exact(mine, ref, st, other_shares=len(shares) - len(mine))
        else:
            furthest = C.at_position(st, C.position(st) + 2 * st["launch_hashes"], job)
            ref = C.reference_hits(C.searched_region(job, furthest, 128), target)
            assert set(keys) <= ref, (jid, sorted(set(keys) - ref)[:8], st)
        counts[jid] = (len(mine), len(ref))
    _report(tag, counts, time.monotonic() - t0)


# ------------------------------------------------------------- the switches that are read once per process: a child

_child_trouble = []  # a child that died on a signal or ran into its limit: no further child is started


def _run_child(tmp_path, algo, env):
    if _child_trouble:
        pytest.fail(f"not started: an earlier child did not end by itself ({_child_trouble[0]})")
    out = tmp_path / "child.json"
    child_env = {k: v for k, v in os.environ.items() if k not in C.MODE_VARS}
    child_env.update(env)
    t0 = time.monotonic()
    try:
        proc = subprocess.run([sys.executable, CHILD, algo, str(out)], env=child_env, capture_output=True, text=True,
                              timeout=CHILD_TIMEOUT_S[algo])
    except subprocess.TimeoutExpired as e:
        _child_trouble.append(f"{algo} {env}: limit of {CHILD_TIMEOUT_S[algo]} s")
        pytest.fail(f"the child reached its limit of {CHILD_TIMEOUT_S[algo]} s:\n{e.stdout}\n{e.stderr}")
    if proc.returncode < 0:
        _child_trouble.append(f"{algo} {env}: signal {-proc.returncode}")
    assert proc.returncode == 0, f"child exit {proc.returncode}:\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}"
    r = json.loads(out.read_text())
    return C.scenario_from_json(r), time.monotonic() - t0


def test_scrypt_without_write_polls_in_a_child(tmp_path):
    """OTEDAMA_SCRYPT_POLL=0: the ROMix instance without scalar polls in its write loop, first against hashlib at the
    ops level (in the child), then under the miner's pause / resume / switch."""
    t0 = time.monotonic()
    r, child_s = _run_child(tmp_path, "scrypt", {"OTEDAMA_SCRYPT_POLL": "0"})
    assert r["evidence"]["write_polls"] is False and r["evidence"]["segments"] == 0, r["evidence"]
    assert [n for n, _ in r["ops_checked"]] == [192, 200, 512] and all(h > 0 for _, h in r["ops_checked"]), r
    want = {"search_streams": 2, "scrypt_halves": True, "launch_hashes": launch_hashes("scrypt", r["cus"])}
    counts = C.check_scenario(r, want)
    _report(f"scrypt SCRYPT_POLL=0 (child {child_s:.1f} s: {r['seconds']})", counts, time.monotonic() - t0)


def test_x11_without_midstage_polls_in_a_child(tmp_path):
    """OTEDAMA_X11_MIDPOLL=0: only BLAKE and the compare stage see the abort word."""
    t0 = time.monotonic()
    r, child_s = _run_child(tmp_path, "x11", {"OTEDAMA_X11_MIDPOLL": "0"})
    assert r["evidence"]["x11_midstage_polls"] is False, r["evidence"]
    want = {"search_streams": 2, "x11_overlap": True, "launch_hashes": launch_hashes("x11", r["cus"])}
    counts = C.check_scenario(r, want)
    _report(f"x11 X11_MIDPOLL=0 (child {child_s:.1f} s: {r['seconds']})", counts, time.monotonic() - t0)
