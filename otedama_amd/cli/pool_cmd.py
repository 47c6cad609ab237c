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
import functools
import json
import signal
from typing import TextIO

from otedama_amd.cli.flags import FlagSet
from otedama_amd.cli.main import EXIT_CONFIG, EXIT_OK, EXIT_RUNTIME, parse_subcommand
from otedama_amd.pool.devicepath import PATHS, valid_device


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
    default = type(ps)()
    pairs = [(flag, getattr(ps, field), getattr(default, field)) for flag, field in _FILE_FIELD.items()]
    for flag, value, unset in pairs + [("http-addr", cfg.http_addr, "")]:
        if flag in fs.set_flags or value == unset or value in ("", None):
            continue
        fs.values[flag] = value
    fs.values["coinbase-message"] = ps.coinbase_message


def _flag(field: str) -> str:
    return field.replace("_", "-")


# flag -> the pool_server field of the config file that fills it
_FILE_FIELD = {"algorithms": "algorithm", "listen-sv2": "listen_sv2", "listen-v1": "listen_v1",
               "difficulty": "initial_difficulty", "share-seconds": "target_share_seconds",
               "retarget-seconds": "vardiff_retarget_seconds", "journal": "journal_path",
               "template-file": "template_file",
               **{_flag(field): field for spec in PATHS.values() for field in spec.fields}}


def _options(spec, fs: FlagSet) -> dict:
    """The PoolOptions fields of one CPU-or-GPU path (pool/devicepath.py PATHS) from the (file-filled) flags."""
    return {field: fs[_flag(field)] for field in spec.fields}


def _options_error(spec, opts: dict) -> str | None:
    device, min_gpu = f"{spec.prefix}_device", f"{spec.prefix}_min_gpu"
    if not valid_device(opts[device]):
        return f"--{_flag(device)} {opts[device]!r} must be empty (off), cpu or cuda:N"
    if spec.batched:
        ms, most = f"{spec.prefix}_batch_ms", f"{spec.prefix}_batch_max"
        if opts[ms] <= 0 or not spec.batch_max_ok(opts[most]):
            return (f"--{_flag(ms)} must be positive and --{_flag(most)} in 1..{spec.batch_max_limit}"
                    if spec.batch_max_limit else f"--{_flag(ms)} and --{_flag(most)} must be positive")
    if opts[min_gpu] < 0:
        default = "the algorithm's measured default" if spec.per_algorithm else "the measured default"
        return f"--{_flag(min_gpu)} must not be negative (0 = {default})"
    return None


# verify_options(fs), verify_options_error(opts), and the same for job, template, handshake and seal
for _spec in PATHS.values():
    globals()[f"{_spec.prefix}_options"] = functools.partial(_options, _spec)
    globals()[f"{_spec.prefix}_options_error"] = functools.partial(_options_error, _spec)


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
    err = next(filter(None, (_options_error(spec, _options(spec, fs)) for spec in PATHS.values())), None)
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
                           noise_authority_secret=int(fs["noise-authority-key"] or "0", 16),
                           **{k: v for spec in PATHS.values() for k, v in _options(spec, fs).items()})

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
