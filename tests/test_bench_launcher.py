"""bench.py as the driver runs it: ``python bench.py --gpus N`` with no torchrun env spawns N ranks itself.

The CPU rehearsal (``--cpu-rehearsal``: gloo + the native CPU scanner in place of the kernels) drives the same
launcher, rank bootstrap, R1/R2/R3 collectives, hit de-duplication and JSON contract as the MI355X run, at the
world sizes the 8-GPU node uses. On a host with fewer GPUs than ``--gpus`` the GPU run must refuse instead of
silently reporting a smaller node.
"""
import os
import subprocess
import sys
import tempfile

import pytest

from benchjson import detail_env, result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _bench(*args, env=None, timeout=240):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    denv, detail = detail_env(tempfile.mkdtemp(prefix="otd-bench-"))
    e.update(denv)
    e.update(env or {})
    res = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=timeout, env=e,
                         cwd=ROOT)
    res.detail = detail
    return res


def _json(res) -> dict:
    return result(res, res.detail)


@pytest.mark.parametrize("n", [4, 8])
def test_launcher_runs_n_ranks(n):
    res = _bench("--gpus", str(n), "--steps", "3", "--warmup", "1", "--cpu-rehearsal")
    assert res.returncode == 0, res.stderr[-3000:]
    d = _json(res)
    assert KEYS <= set(d)
    assert d["n_gpus"] == n and d["world_size"] == n
    assert d["rccl_ranks_seen"] == list(range(n))
    assert d["dist_backend"] == "gloo" and d["rehearsal"] == "cpu-gloo"
    assert len(d["per_rank_hashes_per_sec"]) == n and all(r > 0 for r in d["per_rank_hashes_per_sec"])
    # whole-job value = total hashes / max rank time; each rank scans its own stripe
    assert d["value"] == pytest.approx(d["config"]["global_batch"] * d["steps"] / (d["ms_per_step"] * d["steps"] / 1e3))
    # every hit found is unique and verifies; R2 delivered every rank's hits to rank 0
    assert d["hits_duplicate"] == 0 and d["hits_outside_window"] == 0
    assert d["hits_verified"] == d["hits_found"] > 0
    assert d["hits_r2_gathered"] == d["hits_found"]
    assert abs(d["hits_z"]) < 6


def test_single_rank_rehearsal_keeps_the_json_contract():
    res = _bench("--steps", "2", "--warmup", "1", "--cpu-rehearsal")
    assert res.returncode == 0, res.stderr[-3000:]
    d = _json(res)
    assert KEYS <= set(d) and d["n_gpus"] == 1 and d["rccl_ranks_seen"] == [0]
    assert d["higher_is_better"] is True and d["scaling"] == "weak"
    assert "REHEARSAL" in d["data"]


def test_plain_run_is_the_headline_alone_and_dumps_what_the_last_step_returned(tmp_path):
    """Without --full a run measures the SHA-256d headline and nothing else (no other section starts, their keys are
    null). --dump-outputs writes the last timed step's hits and every timed step's hits as float64 .npy: each row
    verifies against hashlib under the run's target, the counts are the line's, and a second run with the same
    arguments writes the same arrays."""
    import hashlib

    import numpy as np

    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    from otedama_amd.ops import native
    from otedama_amd.parallel import stripe_for

    dumps = []
    for name in ("a", "b"):
        res = _bench("--steps", "3", "--warmup", "1", "--cpu-rehearsal", "--dump-outputs", str(tmp_path / name))
        assert res.returncode == 0, res.stderr[-3000:]
        d = _json(res)
        assert set(d["sections"]) == {"preflight", "sha256d"} and d["errors"] is None
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["comm"] is None and d["cpu"] is None
        assert d.line["summary"]["cfg1_cpu_1t_hps"] is None
        assert sorted(os.listdir(tmp_path / name)) == ["hit_count.npy", "hits.npy", "hits_timed.npy", "r2_hits.npy"]
        dumps.append({f[:-4]: np.load(tmp_path / name / f) for f in os.listdir(tmp_path / name)})
    a, b = dumps
    assert all(a[k].dtype == np.float64 and np.array_equal(a[k], b[k]) for k in a)
    assert a["hits"].shape == (int(a["hit_count"][0]), 2) and len(a["hits"]) > 0
    assert len(a["hits_timed"]) == d["hits_found"] == int(a["r2_hits"][0])
    assert np.array_equal(a["hits_timed"][a["hits_timed"][:, 0] == 2][:, 1:], a["hits"])  # the last of 3 steps
    # every row is a hit: the rehearsal's step i scans nonces [i % 2 * 4096, +4096) of variants 4 * (i // 2) .. + 3
    N = native.require_native()
    job, stripe = bench.synthetic_job(1), stripe_for(0, 1)
    for step, nonce, vi in a["hits_timed"].astype(np.int64).tolist():
        hdr = N.variant_header(job, stripe.start + (4 * (step // 2) + vi) * stripe.stride)[0]
        h = hashlib.sha256(hashlib.sha256(hdr[:76] + nonce.to_bytes(4, "little")).digest()).digest()
        assert int.from_bytes(h, "little") < 1 << 244 and (step % 2) * 4096 <= nonce < (step % 2 + 1) * 4096


def test_refuses_more_gpus_than_visible():
    res = _bench("--gpus", "2", "--steps", "1", "--warmup", "0", env={"HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""})
    assert res.returncode != 0
    assert "visible GPUs" in res.stderr
    assert not [ln for ln in res.stdout.splitlines() if ln.startswith("{")]


def test_torchrun_world_size_must_match_gpus():
    res = _bench("--gpus", "2", "--cpu-rehearsal", env={"WORLD_SIZE": "3", "RANK": "0"})
    assert res.returncode == 2 and "WORLD_SIZE=3" in res.stderr


def test_driver_torchrun_invocation():
    """Exactly the driver's multi-GPU command line (torchrun, its agent TCPStore, 127.0.0.1), with the CPU
    rehearsal in place of the GPUs: ranks join the agent's store, run R1/R2/R3, and rank 0 prints one JSON line."""
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    e.update(detail_env(tempfile.mkdtemp(prefix="otd-bench-"))[0])
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2",
                          "--steps", "2", "--warmup", "1", "--cpu-rehearsal"],
                         capture_output=True, text=True, timeout=240, env=e, cwd=ROOT)
    res.detail = e["OTEDAMA_BENCH_DETAIL"]
    assert res.returncode == 0, res.stderr[-3000:]
    d = _json(res)
    assert d["n_gpus"] == 2 and d["world_size"] == 2 and d["rccl_ranks_seen"] == [0, 1]
    assert d["hits_duplicate"] == 0 and d["hits_verified"] == d["hits_found"]


@pytest.mark.timeout(300)
def test_driver_torchrun_invocation_on_the_native_data_plane():
    """The driver's N>1 command line (torchrun, its agent's store) with the native data plane the GPU run uses: the
    probe children form a native group through the agent's store, every rank's R1 / R2 / R3 and the comm section run
    on the native module's API (its CPU stand-in, tests/loopback_rccl.py), and the line says rccl-native."""
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    e.update(detail_env(tempfile.mkdtemp(prefix="otd-bench-"))[0])
    e.update(OTEDAMA_RCCL_MODULE="loopback_rccl", PYTHONPATH=os.path.join(ROOT, "tests"))
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "4",
                          "--steps", "2", "--warmup", "1", "--cpu-rehearsal", "--full", "--cpu-seconds", "0", "--comm-ops",
                          "20"],
                         capture_output=True, text=True, timeout=240, env=e, cwd=ROOT)
    res.detail = e["OTEDAMA_BENCH_DETAIL"]
    assert res.returncode == 0, res.stderr[-3000:]
    d = _json(res)
    assert d.line["summary"]["data_plane"] == "rccl-native" and d["dist_backend"] == "rccl"
    assert d["rccl_ranks_seen"] == [0, 1, 2, 3] and d["hits_r2_gathered"] == d["hits_found"] > 0
    assert d["comm"]["idle"]["R2_dev"]["samples"] == 20 and d["comm"]["busbw"]["blocks_ok"]


@pytest.mark.timeout(400)
def test_driver_torchrun_invocation_with_the_node_section():
    """The driver's N>1 command line end to end, node section included: torchrun's ranks run the kernel sections,
    then rank 0 (still a torchrun worker, its agent's store on MASTER_PORT) starts `otedama node --gpus N` with its
    own supervisor store, and the JSON carries that node's object."""
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    e.update(detail_env(tempfile.mkdtemp(prefix="otd-bench-"))[0])
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "4",
                          "--steps", "2", "--warmup", "1", "--cpu-rehearsal", "--full", "--node-seconds", "3",
                          "--node-warmup", "2", "--cpu-seconds", "0"],
                         capture_output=True, text=True, timeout=360, env=e, cwd=ROOT)
    res.detail = e["OTEDAMA_BENCH_DETAIL"]
    assert res.returncode == 0, res.stderr[-3000:]
    d = _json(res)
    assert d["n_gpus"] == 4 and d["rccl_ranks_seen"] == [0, 1, 2, 3]
    node = d["node"]
    assert "error" not in node, node
    assert node["n_ranks"] == 4 and node["ranks_seen"] == [0, 1, 2, 3] and node["exit_code"] == 0
    assert all(r > 0 for r in node["per_rank_hashes_per_sec"]) and node["accepted_remote_in_window"] > 0
    assert node["rejected"] == 0 and node["pool_rejected"] == node["job_switch"]["stale_rejects"]


def test_bench_ranks_get_a_long_collective_bound(monkeypatch):
    """The bench is not the fault-tolerant node: its ranks run with a 600 s collective bound (a cold rank start on
    a fresh 8-GPU node must not trip the node's 30 s default), unless the caller set one."""
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    monkeypatch.delenv("OTEDAMA_PG_TIMEOUT", raising=False)
    assert bench.main(["--gpus", "0"]) == 2  # refused before any rank starts, after the bound is set
    assert os.environ["OTEDAMA_PG_TIMEOUT"] == bench.BENCH_PG_TIMEOUT_S
    monkeypatch.setenv("OTEDAMA_PG_TIMEOUT", "45")
    bench.main(["--gpus", "0"])
    assert os.environ["OTEDAMA_PG_TIMEOUT"] == "45"


NODE_KEYS = {"total_hashes_per_sec", "per_rank_hashes_per_sec", "accepted", "rejected", "pool_accepted",
             "pool_rejected", "ranks_seen", "dist_backend", "collectives", "collectives_total",
             "hit_to_accept_rank0", "hit_to_accept_remote", "host_verify_to_accept_rank0",
             "host_verify_to_accept_remote", "share_difficulty"}


@pytest.mark.timeout(540)
@pytest.mark.parametrize("n", [4, 8])
def test_node_section_json_contract(n):
    """after the kernel sections, bench.py runs the production node (`otedama node --gpus N`:
    supervisor, N ranks, a device process per rank, rank 0 on the pool session) against the local pool and reports
    it. The CPU rehearsal runs the same processes over gloo with CPU miners.
    At world 8 the pool and CPU sections run too: the worst case of the printed line (missing #1: node
    objects for 3 algorithms x 8 ranks, the pool's) must still fit bench.LINE_CAP (checked in _json)."""
    extra = ("--pool-seconds", "3", "--cpu-seconds", "0.3") if n == 8 else ("--cpu-seconds", "0")
    res = _bench("--gpus", str(n), "--steps", "2", "--warmup", "1", "--cpu-rehearsal", "--full", "--node-seconds",
                 "3", "--node-warmup", "2", *extra, timeout=480)
    assert res.returncode == 0, res.stderr[-3000:]
    d = _json(res)
    s = d.line["summary"]
    assert s["world_size"] == n and s["ranks_seen"] == list(range(n)) and len(s["per_rank_hps"]) == n
    assert set(s["node_hps"]) == {"sha256d", "x11", "scrypt"} and s["lost_ranks"] == [] and s["reforms"] == 0
    assert 0 < s["rank_rate_min_max"] <= 1 and s["rank_efficiency"] > 0
    assert s["shares_via_preview"] + s["shares_via_r2"] > 0 and s["node_op_p99_ms"] > 0
    if n == 8:
        assert s["cfg1_cpu_1t_hps"] > 0 and set(s["cfg5_pool_validations"]) == {"sha256d", "scrypt"}
    node = d["node"]
    assert "error" not in node, node
    assert NODE_KEYS <= set(node), sorted(node)
    assert node["n_ranks"] == n and node["ranks_seen"] == list(range(n)) and node["dist_backend"] == "gloo"
    assert len(node["per_rank_hashes_per_sec"]) == n and all(r > 0 for r in node["per_rank_hashes_per_sec"])
    assert node["total_hashes_per_sec"] == pytest.approx(sum(node["per_rank_hashes_per_sec"]))
    assert d["node_hashes_per_sec"] == node["total_hashes_per_sec"]
    # no reject while mining; the forced new blocks of the job-switch phase may catch a share in flight (stale only)
    assert node["rejected"] == 0 and node["pool_accepted"] > 0
    assert set(node["pool_reject_reasons"] or {}) <= {"stale-job"}
    js = node["job_switch"]
    assert node["pool_rejected"] == js["stale_rejects"]
    assert js["missing"] == 0 and all(v["samples"] == js["blocks"] for v in js["per_rank"].values())
    assert set(node["collectives"]) == {"rank0", *(f"rank{r}" for r in range(1, n))}
    assert all(c > 0 for c in node["collectives"].values())
    # remote ranks' shares crossed R2 and were accepted; CPU miners carry no kernel clock, so the host timeline is used
    assert node["host_verify_to_accept_remote"]["samples"] > 0 and node["accepted_remote_in_window"] > 0
    assert node["share_difficulty"] == pytest.approx(node["share_difficulty_requested"], rel=1e-6)
    assert node["exit_code"] == 0


@pytest.mark.timeout(300)
def test_pool_and_cpu_sections_json_contract():
    """BASELINE configs 1 and 5 in the bench JSON: the native CPU miner (single thread, all cores) and the mixed
    SHA-256d + scrypt pool with vardiff (here CPU miners for both algorithms), windowed once every worker converged
    (VERDICT r4 item 5), with the pool's flood capacity beside it."""
    res = _bench("--steps", "2", "--warmup", "1", "--cpu-rehearsal", "--full", "--pool-seconds", "3", "--cpu-seconds",
                 "0.5", timeout=280)
    assert res.returncode == 0, res.stderr[-3000:]
    d = _json(res)
    assert d["cpu_single_thread_hashes_per_sec"] > 0 and d["cpu_all_cores_hashes_per_sec"] > 0
    assert d["cpu"]["threads"] >= 1 and d["cpu"]["sha_ni"] in (True, False)
    pool = d["pool"]
    assert "error" not in pool, pool
    assert set(pool["algorithms"]) == {"sha256d", "scrypt"}
    for algo, a in pool["algorithms"].items():
        assert a["accepted_total"] > 0 and a["rejected_total"] == 0, (algo, a)
        # validation quantiles over the window only (the pool's timed log), the whole run's beside them
        assert a["validate_ms"]["p50"] is not None and abs(a["validate_ms"]["samples"] - a["accepted"]) <= 3
        assert a["validate_ms_whole_run"]["samples"] == a["accepted_total"]
        assert a["workers"] and all(w["difficulty"] > 0 for w in a["workers"])
        for w in a["workers"]:  # convergence and window timing per worker (the CPU miners' rates are too noisy
            # on a shared container to pin the window after convergence here; the GPU run records it)
            assert w["converged_after_s"] >= 0 and w["window_opened_after_s"] > 0, w
            assert w["share_interval_s"] and w["interval_vs_target"] > 0
        assert all(m["exit_code"] == 0 for m in a["miners"])
        assert pool["flood"][algo]["validated_shares_per_sec"] > 100 and pool["flood"][algo]["rejected"] == 0
    assert pool["time_to_steady_s"] >= pool["time_to_first_accept_s"] > 0


def test_compact_line_caps_a_pathological_result():
    """compact_line keeps the driver contract and the summary's headline keys within LINE_CAP even when every
    section failed with a long error and the per-rank lists are long (a 64-rank world)."""
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    from benchjson import check_line

    full = {k: 1 for k in bench.CONTRACT_KEYS}
    full["config"] = {"model": "sha256d", "global_batch": 1, "seq_len": 80, "parallelism": "dp64", "kernel": "k" * 500,
                      "variants_per_step": 128, "nonce_split": "x" * 5000}
    full["node"] = {"big": "y" * 100_000}
    full["summary"] = {"cfg2_version_rolled_hps": 1.9e10, "per_rank_hps": [1.0e9] * 64,
                       "ranks_seen": list(range(64)), "errors": {f"s{i}": "e" * 160 for i in range(40)},
                       "sections_s": {f"s{i}": 1.0 for i in range(40)},
                       "rank_phases": {f"p{i}" * 10: list(range(64)) for i in range(20)}}
    line = bench.compact_line(full, "/x/bench_detail.json")
    d = check_line(line)
    assert d["summary"]["cfg2_version_rolled_hps"] == 1.9e10 and d["detail"] == "bench_detail.json"
    assert "dropped" in d["summary"] and "node" not in d and len(d["config"]["kernel"]) <= 60
