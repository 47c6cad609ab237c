"""``otedama pool`` — run the local validating Stratum pool [NO REFERENCE CODE].

One process can serve several algorithms (``--algorithms sha256d,scrypt``):
each gets its own SV2 + V1 listener pair (ports increment per algorithm), its
own vardiff / diff1 constant and share journal, and all publish into one
/metrics registry — the "mixed SHA-256d + scrypt workers" pool of BASELINE.json
config 5.

Settings come from flags, then the config file's ``pool_server`` section (plus ``http_addr``), then the flag
defaults: an explicitly given flag always wins.
"""
from __future__ import annotations

import asyncio
import json
import signal
from typing import TextIO

from otedama_amd.cli.flags import FlagSet
from otedama_amd.cli.main import EXIT_CONFIG, EXIT_OK, EXIT_RUNTIME, parse_subcommand


def _bump(addr: str, k: int) -> str:
    if not addr:
        return ""
    h, _, p = addr.rpartition(":")
    return f"{h}:{int(p) + k}" if p and int(p) else addr


def apply_config_file(fs: FlagSet, stderr: TextIO) -> None:
    """Fill every flag the user did not give from the config file's pool_server section."""
    from otedama_amd.cli.main import load_config

    cfg = load_config(fs, stderr)
    ps = cfg.pool_server
    pairs = (("algorithms", ps.algorithm), ("listen-sv2", ps.listen_sv2), ("listen-v1", ps.listen_v1),
             ("difficulty", ps.initial_difficulty), ("share-seconds", ps.target_share_seconds),
             ("retarget-seconds", ps.vardiff_retarget_seconds), ("journal", ps.journal_path),
             ("verify-device", ps.verify_device), ("verify-batch-ms", ps.verify_batch_ms),
             ("verify-batch-max", ps.verify_batch_max), ("verify-min-gpu", ps.verify_min_gpu),
             ("job-device", ps.job_device), ("job-min-gpu", ps.job_min_gpu),
             ("template-file", ps.template_file), ("template-device", ps.template_device),
             ("template-min-gpu", ps.template_min_gpu), ("handshake-device", ps.handshake_device),
             ("handshake-batch-ms", ps.handshake_batch_ms), ("handshake-batch-max", ps.handshake_batch_max),
             ("handshake-min-gpu", ps.handshake_min_gpu), ("seal-device", ps.seal_device),
             ("seal-min-gpu", ps.seal_min_gpu), ("http-addr", cfg.http_addr))
    default = type(ps)()
    for flag, value in pairs:
        unset_in_file = flag != "http-addr" and value == getattr(default, _FILE_FIELD[flag])
        if flag in fs.set_flags or unset_in_file or value in ("", None):
            continue
        fs.values[flag] = value
    fs.values["coinbase-message"] = ps.coinbase_message


_FILE_FIELD = {"algorithms": "algorithm", "listen-sv2": "listen_sv2", "listen-v1": "listen_v1",
               "difficulty": "initial_difficulty", "share-seconds": "target_share_seconds",
               "retarget-seconds": "vardiff_retarget_seconds", "journal": "journal_path",
               "verify-device": "verify_device", "verify-batch-ms": "verify_batch_ms",
               "verify-batch-max": "verify_batch_max", "verify-min-gpu": "verify_min_gpu",
               "job-device": "job_device", "job-min-gpu": "job_min_gpu",
               "template-file": "template_file", "template-device": "template_device",
               "template-min-gpu": "template_min_gpu", "handshake-device": "handshake_device",
               "handshake-batch-ms": "handshake_batch_ms", "handshake-batch-max": "handshake_batch_max",
               "handshake-min-gpu": "handshake_min_gpu", "seal-device": "seal_device",
               "seal-min-gpu": "seal_min_gpu"}


def verify_options(fs: FlagSet) -> dict:
    """The micro-batcher's PoolOptions fields from the (file-filled) flags."""
    return {"verify_device": fs["verify-device"], "verify_batch_ms": fs["verify-batch-ms"],
            "verify_batch_max": fs["verify-batch-max"], "verify_min_gpu": fs["verify-min-gpu"]}


def verify_options_error(opts: dict) -> str | None:
    from otedama_amd.pool.devicepath import valid_device

    if not valid_device(opts["verify_device"]):
        return f"--verify-device {opts['verify_device']!r} must be empty (off), cpu or cuda:N"
    if opts["verify_batch_ms"] <= 0 or opts["verify_batch_max"] <= 0:
        return "--verify-batch-ms and --verify-batch-max must be positive"
    if opts["verify_min_gpu"] < 0:
        return "--verify-min-gpu must not be negative (0 = the algorithm's measured default)"
    return None


def job_options(fs: FlagSet) -> dict:
    """The job fan-out's PoolOptions fields from the (file-filled) flags."""
    return {"job_device": fs["job-device"], "job_min_gpu": fs["job-min-gpu"]}


def job_options_error(opts: dict) -> str | None:
    from otedama_amd.pool.devicepath import valid_device

    if not valid_device(opts["job_device"]):
        return f"--job-device {opts['job_device']!r} must be empty (off), cpu or cuda:N"
    if opts["job_min_gpu"] < 0:
        return "--job-min-gpu must not be negative (0 = the measured default)"
    return None


def template_options(fs: FlagSet) -> dict:
    """The template tree's PoolOptions fields from the (file-filled) flags."""
    return {"template_device": fs["template-device"], "template_min_gpu": fs["template-min-gpu"]}


def template_options_error(opts: dict) -> str | None:
    from otedama_amd.pool.devicepath import valid_device

    if not valid_device(opts["template_device"]):
        return f"--template-device {opts['template_device']!r} must be empty (off), cpu or cuda:N"
    if opts["template_min_gpu"] < 0:
        return "--template-min-gpu must not be negative (0 = the measured default)"
    return None


def handshake_options(fs: FlagSet) -> dict:
    """The handshake batcher's PoolOptions fields from the (file-filled) flags."""
    return {"handshake_device": fs["handshake-device"], "handshake_batch_ms": fs["handshake-batch-ms"],
            "handshake_batch_max": fs["handshake-batch-max"], "handshake_min_gpu": fs["handshake-min-gpu"]}


def handshake_options_error(opts: dict) -> str | None:
    from otedama_amd.pool.devicepath import valid_device

    if not valid_device(opts["handshake_device"]):
        return f"--handshake-device {opts['handshake_device']!r} must be empty (off), cpu or cuda:N"
    if opts["handshake_batch_ms"] <= 0 or not 0 < opts["handshake_batch_max"] <= 21845:
        return "--handshake-batch-ms must be positive and --handshake-batch-max in 1..21845"
    if opts["handshake_min_gpu"] < 0:
        return "--handshake-min-gpu must not be negative (0 = the measured default)"
    return None


def seal_options(fs: FlagSet) -> dict:
    """The frame sealer's PoolOptions fields from the (file-filled) flags."""
    return {"seal_device": fs["seal-device"], "seal_min_gpu": fs["seal-min-gpu"]}


def seal_options_error(opts: dict) -> str | None:
    from otedama_amd.pool.devicepath import valid_device

    if not valid_device(opts["seal_device"]):
        return f"--seal-device {opts['seal_device']!r} must be empty (off), cpu or cuda:N"
    if opts["seal_min_gpu"] < 0:
        return "--seal-min-gpu must not be negative (0 = the measured default)"
    return None


def template_source(fs: FlagSet):
    """The pool's template source from the flags: a ``GbtFileSource`` over ``--template-file`` paying
    ``--payout-address`` (OP_RETURN without one), or None for the synthetic chain."""
    if not fs["template-file"]:
        return None
    from otedama_amd import btccrypto
    from otedama_amd.pool.server import PoolOptions
    from otedama_amd.pool.template import GbtFileSource

    script = btccrypto.address_script_pubkey(fs["payout-address"]) if fs["payout-address"] else b"\x6a"
    return GbtFileSource(fs["template-file"], script, fs.values.get("coinbase-message", PoolOptions.coinbase_message))


def pool_flags(stderr: TextIO) -> FlagSet:
    fs = FlagSet("pool", stderr)
    fs.string("algorithms", "sha256d", "Comma-separated algorithms to serve (sha256d, scrypt, x11).")
    fs.string("listen-sv2", "127.0.0.1:3336", "Stratum V2 listen address (port +1 per extra algorithm).")
    fs.string("listen-v1", "127.0.0.1:3333", "Stratum V1 listen address (port +1 per extra algorithm).")
    fs.string("payout-address", "", "Operator address paid by the coinbase (empty = OP_RETURN).")
    fs.float("difficulty", 1.0, "Initial share difficulty.")
    fs.bool("fixed-difficulty", False, "Pin every connection at --difficulty (vardiff off).")
    fs.float("share-seconds", 10.0, "Vardiff target seconds between shares per connection.")
    fs.float("retarget-seconds", 30.0, "Vardiff retarget window.")
    fs.float("block-interval", 600.0, "Seconds between synthetic network blocks.")
    fs.float("job-interval", 30.0, "Seconds between job refreshes (new ntime).")
    fs.string("journal", "", "SQLite share journal path (empty = in-memory).")
    fs.string("payout-scheme", "pplns", "Block payout accounting: pplns | prop.")
    fs.string("http-addr", "", "Address for /metrics /healthz /api/v1/{pool,workers,blocks} (empty disables).")
    fs.string("dialect", "reference", "SV2 wire dialect: reference | spec.")
    fs.bool("sv2-noise", False, "Encrypt SV2 connections with Noise NX (miners pin the printed authority key).")
    fs.string("noise-suite", "", "Noise suites accepted: empty = both, ellswift (current SV2) or legacy.")
    fs.string("noise-authority-key", "", "Hex secp256k1 secret signing the Noise certificate (empty = fresh per run).")
    fs.float("duration", 0.0, "Stop after this many seconds (0 = run until signalled).")
    fs.string("verify-device", "", "Validate submits in micro-batches: cpu or cuda:N (empty = off, one share at a time).")
    fs.float("verify-batch-ms", 2.0, "Micro-batch flush delay after the oldest pending submit, in milliseconds.")
    fs.int("verify-batch-max", 4096, "Micro-batch flush size.")
    fs.int("verify-min-gpu", 0, "Batches with fewer shares are hashed on the CPU (0 = the algorithm's measured default).")
    fs.string("job-device", "", "A job's SV2 standard-channel merkle roots in one call: cpu or cuda:N (empty = off).")
    fs.int("job-min-gpu", 0, "Fan-outs to fewer standard channels stay on the CPU (0 = the measured default).")
    fs.string("template-file", "", "JSON file holding a getblocktemplate result, re-read for every block (empty = synthetic).")
    fs.string("template-device", "", "A template's merkle trees in one call: cpu or cuda:N (empty = off, hashed in Python).")
    fs.int("template-min-gpu", 0, "Templates of fewer leaves stay on the CPU (0 = the measured default).")
    fs.string("handshake-device", "", "With --sv2-noise, the handshakes' secp256k1 arithmetic in batches: cpu or cuda:N (empty = off).")
    fs.float("handshake-batch-ms", 2.0, "Handshake batch flush delay after the oldest waiting handshake, in milliseconds.")
    fs.int("handshake-batch-max", 4096, "Handshake batch flush size.")
    fs.int("handshake-min-gpu", 0, "Batches of fewer handshakes are computed on the CPU (0 = the measured default).")
    fs.string("seal-device", "", "With --sv2-noise, a job's frames sealed in one batch: cpu or cuda:N (empty = off, sealed one by one).")
    fs.int("seal-min-gpu", 0, "Jobs of fewer frames are sealed on the CPU (0 = the measured default).")
    fs.string("config", "", "Path to the YAML config file (default: $OTEDAMA_CONFIG or ~/.config/otedama/config.yaml).")
    return fs


def cmd_pool(args: list[str], stdout: TextIO, stderr: TextIO) -> int:
    fs = pool_flags(stderr)
    rc = parse_subcommand(fs, args, stdout, stderr)
    if rc is not None:
        return rc
    apply_config_file(fs, stderr)
    algos = [a.strip() for a in fs["algorithms"].split(",") if a.strip()]
    for a in algos:
        if a not in ("sha256d", "scrypt", "x11"):
            stderr.write(f"pool: unsupported algorithm {a!r} (sha256d, scrypt, x11)\n")
            return EXIT_CONFIG
    if fs["payout-address"]:
        from otedama_amd.config import validate_bitcoin_address

        err = validate_bitcoin_address(fs["payout-address"])
        if err:
            stderr.write(f"pool: payout address invalid: {err}\n")
            return EXIT_CONFIG
    err = verify_options_error(verify_options(fs)) or job_options_error(job_options(fs)) \
        or template_options_error(template_options(fs)) or handshake_options_error(handshake_options(fs)) \
        or seal_options_error(seal_options(fs))
    if err:
        stderr.write(f"pool: {err}\n")
        return EXIT_CONFIG
    if fs["noise-suite"] not in ("", "ellswift", "legacy"):
        stderr.write("pool: --noise-suite must be ellswift or legacy (empty accepts both)\n")
        return EXIT_CONFIG
    if fs["noise-authority-key"]:
        from otedama_amd.btccrypto import N as CURVE_ORDER

        try:
            key = bytes.fromhex(fs["noise-authority-key"])
        except ValueError:
            key = b""
        if len(key) != 32 or not 0 < int.from_bytes(key, "big") < CURVE_ORDER:
            stderr.write("pool: --noise-authority-key must be 64 hex characters (a secp256k1 secret in [1, n))\n")
            return EXIT_CONFIG
    try:
        return asyncio.run(_serve(fs, algos, stdout))
    except OSError as exc:
        stderr.write(f"pool: {exc}\n")
        return EXIT_RUNTIME


async def _serve(fs, algos: list[str], stdout: TextIO) -> int:
    from otedama_amd.httpserver import HTTPServer
    from otedama_amd.metrics import Registry
    from otedama_amd.pool.server import PoolOptions, PoolServer

    reg = Registry()
    pools = []
    for k, algo in enumerate(algos):
        journal = fs["journal"]
        if journal and len(algos) > 1:
            journal = journal.replace(".db", f".{algo}.db") if journal.endswith(".db") else f"{journal}.{algo}"
        opts = PoolOptions(algorithm=algo, listen_sv2=_bump(fs["listen-sv2"], k), listen_v1=_bump(fs["listen-v1"], k),
                           payout_address=fs["payout-address"] or None, initial_difficulty=fs["difficulty"],
                           fixed_difficulty=fs["fixed-difficulty"],
                           target_share_seconds=fs["share-seconds"], retarget_seconds=fs["retarget-seconds"],
                           block_interval=fs["block-interval"], job_interval=fs["job-interval"],
                           journal_path=journal or ":memory:", payout_scheme=fs["payout-scheme"],
                           dialect=fs["dialect"], noise=fs["sv2-noise"], noise_suite=fs["noise-suite"],
                           coinbase_message=fs.values.get("coinbase-message", PoolOptions.coinbase_message),
                           noise_authority_secret=int(fs["noise-authority-key"] or "0", 16), **verify_options(fs), **job_options(fs),
                           **template_options(fs), **handshake_options(fs), **seal_options(fs))

        def log(level, msg):
            stdout.write(f"[{level}] {msg}\n")
            stdout.flush()

        p = PoolServer(opts, reg, log, template_source=template_source(fs))
        await p.start()
        pools.append(p)
    srv = None
    if fs["http-addr"]:
        srv = HTTPServer(fs["http-addr"], reg, api={"pool": lambda: [p.stats() for p in pools],
                                                    "stats": lambda: [p.stats() for p in pools],
                                                    "workers": lambda: [w for p in pools for w in p.workers()],
                                                    "blocks": lambda: [b for p in pools for b in p.blocks()]})
        srv.start()
        srv.set_ready(True)
        stdout.write(f"[info] http: listening on {srv.addr}\n")
    stop = asyncio.Event()
    loop = asyncio.get_running_loop()
    for sig in (signal.SIGINT, signal.SIGTERM):
        try:
            loop.add_signal_handler(sig, stop.set)
        except (NotImplementedError, RuntimeError):
            pass
    try:  # SIGUSR1: a new network block now, on every algorithm (operators and probes test stale-work handling)
        loop.add_signal_handler(signal.SIGUSR1, lambda: [p.new_block() for p in pools])
    except (NotImplementedError, RuntimeError, AttributeError):
        pass
    if fs["duration"] > 0:
        loop.call_later(fs["duration"], stop.set)
    await stop.wait()
    for p in pools:  # the exit line carries the timed validation log too (windowed quantiles for probes)
        stdout.write(json.dumps(dict(p.stats(), validate_log=p.validate_log())) + "\n")
        await p.stop()
    if srv:
        srv.stop()
    return EXIT_OK
