"""The Python-visible surface of ``otedama_amd._native``, pinned: every name the module exports, each function's
signature line (pybind11 writes it as the first line of ``__doc__``: argument names, types and defaults), each
constant's value, and each class's constructor line and public attributes. The literal was recorded from the build
that preceded the bindings' split into ``bind_*`` functions; the module must equal it exactly, with nothing missing
and nothing extra. Runs without a GPU."""
from otedama_amd.ops.native import require_native

# fmt: off
SURFACE = {'AEAD_AES256GCM': ('const', 0),
 'AEAD_CHACHA20POLY1305': ('const', 1),
 'CpuMiner': ('class',
              '__init__(self: otedama_amd._native.CpuMiner, threads: typing.SupportsInt | typing.SupportsIndex, '
              "device_id: str = 'cpu-0', queue_cap: typing.SupportsInt | typing.SupportsIndex = 1024) -> None",
              ('device_id', 'poll', 'set_job', 'share_fd', 'start', 'stats', 'stop')),
 'GpuMiner': ('class',
              '__init__(self: otedama_amd._native.GpuMiner, device: typing.SupportsInt | typing.SupportsIndex, '
              'device_id: str, batch_nonces: typing.SupportsInt | typing.SupportsIndex = 4294967296, grid: '
              'typing.SupportsInt | typing.SupportsIndex = 2048, queue_cap: typing.SupportsInt | '
              'typing.SupportsIndex = 1024, sha_variants: typing.SupportsInt | typing.SupportsIndex = 128) -> None',
              ('device_id', 'poll', 'set_job', 'share_fd', 'start', 'stats', 'stop')),
 'MERKLE_TREE_MAX_LEAVES': ('const', 262144),
 'MERKLE_TREE_MAX_TREES': ('const', 65535),
 'Miner': ('class',
           'Initialize self.  See help(type(self)) for accurate signature.',
           ('device_id', 'poll', 'set_job', 'share_fd', 'start', 'stats', 'stop')),
 'POLY_MAX_MSG': ('const', 112),
 'POLY_ROW_BYTES': ('const', 160),
 'SCRYPT_COOP': ('const', 8),
 'SCRYPT_COOP2': ('const', 11),
 'SCRYPT_COOP_SPLIT': ('const', 12),
 'SCRYPT_LANE_W8': ('const', 9),
 'SCRYPT_PARAMS_SIZE': ('const', 112),
 'SEAL_HEAD_BYTES': ('const', 64),
 'SEAL_MAX_FRAMES': ('const', 16777215),
 'SEAL_MAX_PLAIN': ('const', 2048),
 'SECP_MAX_ROWS': ('const', 65536),
 'SECP_OUT_BYTES': ('const', 48),
 'SECP_ROW_BYTES': ('const', 128),
 'SHA256D_K_VALUES': ('const', (2, 3, 4, 6, 8, 12, 16)),
 'SHA256D_MAX_K': ('const', 16),
 'SHA256D_PARAMS_SIZE': ('const', 96),
 'SHA256D_V2_GROUP': ('const', 128),
 'SHA256D_V_GROUP': ('const', 64),
 'SHA256D_V_PARAMS_SIZE': ('const', 32),
 'SHARE_JOB_BLOCK_SIZE': ('const', 3200),
 'SHARE_RESULT_BYTES': ('const', 128),
 'X11_STAGES': ('const', 11),
 '_aead_seal_rows_host': ('def',
                          '_aead_seal_rows_host(frames: typing_extensions.Buffer, n: typing.SupportsInt | '
                          'typing.SupportsIndex) -> bytes'),
 '_clock_bounds': ('def',
                   '_clock_bounds(arg0: typing.SupportsFloat | typing.SupportsIndex, arg1: '
                   'collections.abc.Sequence[tuple[typing.SupportsFloat | typing.SupportsIndex, '
                   'typing.SupportsFloat | typing.SupportsIndex]]) -> list[float]'),
 '_cpu_scan_lanes': ('def',
                     '_cpu_scan_lanes(arg0: typing.SupportsInt | typing.SupportsIndex, arg1: bytes, arg2: bytes, '
                     'arg3: typing.SupportsInt | typing.SupportsIndex, arg4: typing.SupportsInt | '
                     'typing.SupportsIndex) -> list[int]'),
 '_launch_plan_rules': ('def',
                        '_launch_plan_rules(batch_nonces: typing.SupportsInt | typing.SupportsIndex = 0, '
                        'target_hi: typing.SupportsInt | typing.SupportsIndex = 0, capped: bool = True, '
                        'sha_variants: typing.SupportsInt | typing.SupportsIndex = 1, run: typing.SupportsInt | '
                        "typing.SupportsIndex = 1, reserve_cus: str = '', ncu: typing.SupportsInt | "
                        'typing.SupportsIndex = 256) -> dict'),
 '_launch_plan_walk': ('def',
                       '_launch_plan_walk(kind: str, batch: typing.SupportsInt | typing.SupportsIndex, cap: '
                       'typing.SupportsInt | typing.SupportsIndex, nvar: typing.SupportsInt | typing.SupportsIndex '
                       '= 1, lanes: typing.SupportsInt | typing.SupportsIndex = 0, start: typing.SupportsInt | '
                       'typing.SupportsIndex = 0, max_launches: typing.SupportsInt | typing.SupportsIndex = '
                       '1048576, variant_start: typing.SupportsInt | typing.SupportsIndex = 0, variant_stride: '
                       'typing.SupportsInt | typing.SupportsIndex = 1) -> tuple[list[tuple[int, int, int]], int]'),
 '_launch_poly1305_rows': ('def',
                           '_launch_poly1305_rows(rows: typing.SupportsInt | typing.SupportsIndex, n: '
                           'typing.SupportsInt | typing.SupportsIndex, tags: typing.SupportsInt | '
                           'typing.SupportsIndex, stream: typing.SupportsInt | typing.SupportsIndex = 0) -> None'),
 '_poly1305_rows_host': ('def', '_poly1305_rows_host(rows: typing_extensions.Buffer) -> bytes'),
 '_scrypt_romix_mode': ('def', '_scrypt_romix_mode() -> dict'),
 '_work_queue_flood': ('def',
                       '_work_queue_flood(cap: typing.SupportsInt | typing.SupportsIndex, n: typing.SupportsInt | '
                       'typing.SupportsIndex, hash_each: bool = True, batch: typing.SupportsInt | '
                       'typing.SupportsIndex = 1) -> dict'),
 'aead_open': ('def',
               'aead_open(kind: typing.SupportsInt | typing.SupportsIndex, key: bytes, nonce: bytes, sealed: '
               "bytes, aad: bytes = b'') -> object"),
 'aead_seal': ('def',
               'aead_seal(kind: typing.SupportsInt | typing.SupportsIndex, key: bytes, nonce: bytes, plain: bytes, '
               "aad: bytes = b'') -> bytes"),
 'aead_seal_many_cpu': ('def',
                        'aead_seal_many_cpu(frames: typing_extensions.Buffer, n: typing.SupportsInt | '
                        'typing.SupportsIndex) -> bytes'),
 'cpu_has_sha_ni': ('def', 'cpu_has_sha_ni() -> bool'),
 'cpu_scan_method': ('def', 'cpu_scan_method() -> str'),
 'cpu_scan_sha256d': ('def',
                      'cpu_scan_sha256d(header: bytes, target: bytes, start: typing.SupportsInt | '
                      'typing.SupportsIndex, count: typing.SupportsInt | typing.SupportsIndex) -> list[int]'),
 'ellswift_encode_native': ('def', 'ellswift_encode_native(x32: bytes, rand_bytes: bytes) -> object'),
 'gpu_arch_name': ('def', 'gpu_arch_name(arg0: typing.SupportsInt | typing.SupportsIndex) -> str'),
 'gpu_cu_count': ('def', 'gpu_cu_count(arg0: typing.SupportsInt | typing.SupportsIndex) -> int'),
 'gpu_device_count': ('def', 'gpu_device_count() -> int'),
 'hmac_sha256': ('def', 'hmac_sha256(arg0: bytes, arg1: bytes) -> bytes'),
 'launch_aead_seal': ('def',
                      'launch_aead_seal(frames: typing.SupportsInt | typing.SupportsIndex, in_bytes: '
                      'typing.SupportsInt | typing.SupportsIndex, n: typing.SupportsInt | typing.SupportsIndex, '
                      'out: typing.SupportsInt | typing.SupportsIndex, out_bytes: typing.SupportsInt | '
                      'typing.SupportsIndex, stream: typing.SupportsInt | typing.SupportsIndex = 0) -> None'),
 'launch_channel_roots': ('def',
                          'launch_channel_roots(job: typing.SupportsInt | typing.SupportsIndex, prefixes: '
                          'typing.SupportsInt | typing.SupportsIndex, n: typing.SupportsInt | '
                          'typing.SupportsIndex, roots: typing.SupportsInt | typing.SupportsIndex, stream: '
                          'typing.SupportsInt | typing.SupportsIndex = 0) -> None'),
 'launch_merkle_tree': ('def',
                        'launch_merkle_tree(leaves: typing.SupportsInt | typing.SupportsIndex, t: '
                        'typing.SupportsInt | typing.SupportsIndex, n: typing.SupportsInt | typing.SupportsIndex, '
                        'scratch: typing.SupportsInt | typing.SupportsIndex, out: typing.SupportsInt | '
                        'typing.SupportsIndex, stream: typing.SupportsInt | typing.SupportsIndex = 0) -> None'),
 'launch_scrypt': ('def',
                   'launch_scrypt(params: bytes, base: typing.SupportsInt | typing.SupportsIndex, count: '
                   'typing.SupportsInt | typing.SupportsIndex, xbuf: typing.SupportsInt | typing.SupportsIndex, '
                   'scratch: typing.SupportsInt | typing.SupportsIndex, gap: typing.SupportsInt | '
                   'typing.SupportsIndex, out: typing.SupportsInt | typing.SupportsIndex, cap: typing.SupportsInt '
                   '| typing.SupportsIndex, grid: typing.SupportsInt | typing.SupportsIndex, stream: '
                   'typing.SupportsInt | typing.SupportsIndex) -> None'),
 'launch_scrypt_digest': ('def',
                          'launch_scrypt_digest(headers: typing.SupportsInt | typing.SupportsIndex, n: '
                          'typing.SupportsInt | typing.SupportsIndex, xbuf: typing.SupportsInt | '
                          'typing.SupportsIndex, scratch: typing.SupportsInt | typing.SupportsIndex, gap: '
                          'typing.SupportsInt | typing.SupportsIndex, out: typing.SupportsInt | '
                          'typing.SupportsIndex, grid: typing.SupportsInt | typing.SupportsIndex, stream: '
                          'typing.SupportsInt | typing.SupportsIndex = 0) -> None'),
 'launch_secp256k1_mul': ('def',
                          'launch_secp256k1_mul(rows: typing.SupportsInt | typing.SupportsIndex, n: '
                          'typing.SupportsInt | typing.SupportsIndex, out: typing.SupportsInt | '
                          'typing.SupportsIndex, stream: typing.SupportsInt | typing.SupportsIndex = 0) -> None'),
 'launch_sha256d': ('def',
                    'launch_sha256d(params: bytes, base: typing.SupportsInt | typing.SupportsIndex, count: '
                    'typing.SupportsInt | typing.SupportsIndex, out: typing.SupportsInt | typing.SupportsIndex, '
                    'cap: typing.SupportsInt | typing.SupportsIndex, grid: typing.SupportsInt | '
                    'typing.SupportsIndex, stream: typing.SupportsInt | typing.SupportsIndex) -> None'),
 'launch_sha256d_digest': ('def',
                           'launch_sha256d_digest(headers: typing.SupportsInt | typing.SupportsIndex, n: '
                           'typing.SupportsInt | typing.SupportsIndex, out: typing.SupportsInt | '
                           'typing.SupportsIndex, stream: typing.SupportsInt | typing.SupportsIndex = 0) -> None'),
 'launch_sha256d_k': ('def',
                      'launch_sha256d_k(params: bytes, base: typing.SupportsInt | typing.SupportsIndex, count: '
                      'typing.SupportsInt | typing.SupportsIndex, out: typing.SupportsInt | typing.SupportsIndex, '
                      'cap: typing.SupportsInt | typing.SupportsIndex, grid: typing.SupportsInt | '
                      'typing.SupportsIndex, stream: typing.SupportsInt | typing.SupportsIndex) -> None'),
 'launch_sha256d_v': ('def',
                      'launch_sha256d_v(params: bytes, vars: typing.SupportsInt | typing.SupportsIndex, base: '
                      'typing.SupportsInt | typing.SupportsIndex, count: typing.SupportsInt | '
                      'typing.SupportsIndex, out: typing.SupportsInt | typing.SupportsIndex, cap: '
                      'typing.SupportsInt | typing.SupportsIndex, grid: typing.SupportsInt | typing.SupportsIndex, '
                      'stream: typing.SupportsInt | typing.SupportsIndex, occupancy8: bool = False, block: '
                      'typing.SupportsInt | typing.SupportsIndex = 256, chains: typing.SupportsInt | '
                      'typing.SupportsIndex = 1) -> None'),
 'launch_share_headers': ('def',
                          'launch_share_headers(job: typing.SupportsInt | typing.SupportsIndex, records: '
                          'typing.SupportsInt | typing.SupportsIndex, n: typing.SupportsInt | '
                          'typing.SupportsIndex, headers: typing.SupportsInt | typing.SupportsIndex, stream: '
                          'typing.SupportsInt | typing.SupportsIndex = 0) -> None'),
 'launch_share_pack': ('def',
                       'launch_share_pack(job: typing.SupportsInt | typing.SupportsIndex, records: '
                       'typing.SupportsInt | typing.SupportsIndex, headers: typing.SupportsInt | '
                       'typing.SupportsIndex, digests: typing.SupportsInt | typing.SupportsIndex, targets: '
                       'typing.SupportsInt | typing.SupportsIndex, n_targets: typing.SupportsInt | '
                       'typing.SupportsIndex, n: typing.SupportsInt | typing.SupportsIndex, results: '
                       'typing.SupportsInt | typing.SupportsIndex, stream: typing.SupportsInt | '
                       'typing.SupportsIndex = 0) -> None'),
 'launch_share_verdict': ('def',
                          'launch_share_verdict(job: typing.SupportsInt | typing.SupportsIndex, records: '
                          'typing.SupportsInt | typing.SupportsIndex, digests: typing.SupportsInt | '
                          'typing.SupportsIndex, targets: typing.SupportsInt | typing.SupportsIndex, n_targets: '
                          'typing.SupportsInt | typing.SupportsIndex, n: typing.SupportsInt | '
                          'typing.SupportsIndex, verdicts: typing.SupportsInt | typing.SupportsIndex, stream: '
                          'typing.SupportsInt | typing.SupportsIndex = 0) -> None'),
 'launch_x11': ('def',
                'launch_x11(params: bytes, base: typing.SupportsInt | typing.SupportsIndex, H: typing.SupportsInt '
                '| typing.SupportsIndex, stride: typing.SupportsInt | typing.SupportsIndex, n: typing.SupportsInt '
                '| typing.SupportsIndex, out: typing.SupportsInt | typing.SupportsIndex = 0, cap: '
                'typing.SupportsInt | typing.SupportsIndex = 0, stream: typing.SupportsInt | typing.SupportsIndex '
                '= 0) -> None'),
 'launch_x11_digest': ('def',
                       'launch_x11_digest(headers: typing.SupportsInt | typing.SupportsIndex, H: '
                       'typing.SupportsInt | typing.SupportsIndex, stride: typing.SupportsInt | '
                       'typing.SupportsIndex, n: typing.SupportsInt | typing.SupportsIndex, out: '
                       'typing.SupportsInt | typing.SupportsIndex, stream: typing.SupportsInt | '
                       'typing.SupportsIndex = 0) -> None'),
 'launch_x11_stage': ('def',
                      'launch_x11_stage(params: bytes, stage: typing.SupportsInt | typing.SupportsIndex, base: '
                      'typing.SupportsInt | typing.SupportsIndex, H: typing.SupportsInt | typing.SupportsIndex, '
                      'stride: typing.SupportsInt | typing.SupportsIndex, n: typing.SupportsInt | '
                      'typing.SupportsIndex, out: typing.SupportsInt | typing.SupportsIndex = 0, cap: '
                      'typing.SupportsInt | typing.SupportsIndex = 0, stream: typing.SupportsInt | '
                      'typing.SupportsIndex = 0) -> None'),
 'maps_range_writable': ('def',
                         'maps_range_writable(arg0: str, arg1: typing.SupportsInt | typing.SupportsIndex, arg2: '
                         'typing.SupportsInt | typing.SupportsIndex) -> bool'),
 'merkle_root': ('def', 'merkle_root(arg0: dict, arg1: typing.SupportsInt | typing.SupportsIndex) -> bytes'),
 'merkle_tree_cpu': ('def',
                     'merkle_tree_cpu(leaves: bytes, t: typing.SupportsInt | typing.SupportsIndex, n: '
                     'typing.SupportsInt | typing.SupportsIndex) -> bytes'),
 'scrypt_1024_1_1': ('def', 'scrypt_1024_1_1(arg0: bytes) -> bytes'),
 'scrypt_1024_1_1_batch': ('def', 'scrypt_1024_1_1_batch(arg0: collections.abc.Sequence[bytes]) -> list'),
 'scrypt_prepare': ('def', 'scrypt_prepare(arg0: bytes, arg1: bytes) -> bytes'),
 'scrypt_scratch_bytes': ('def',
                          'scrypt_scratch_bytes(arg0: typing.SupportsInt | typing.SupportsIndex, arg1: '
                          'typing.SupportsInt | typing.SupportsIndex) -> int'),
 'secp256k1_mul_cpu': ('def', 'secp256k1_mul_cpu(rows: typing_extensions.Buffer) -> bytes'),
 'sha256': ('def', 'sha256(arg0: bytes) -> bytes'),
 'sha256d': ('def', 'sha256d(arg0: bytes) -> bytes'),
 'sha256d_prepare': ('def', 'sha256d_prepare(arg0: bytes, arg1: bytes) -> bytes'),
 'sha256d_prepare_k': ('def', 'sha256d_prepare_k(headers: list, target: bytes) -> bytes'),
 'sha256d_prepare_v': ('def', 'sha256d_prepare_v(headers: list, target: bytes) -> tuple[bytes, bytes]'),
 'share_headers_cpu': ('def', 'share_headers_cpu(job_block: bytes, records: bytes) -> bytes'),
 'share_job_prepare': ('def',
                       'share_job_prepare(coinb1: bytes, coinb2: bytes, en_size: typing.SupportsInt | '
                       'typing.SupportsIndex, prev_hash: bytes, nbits: typing.SupportsInt | typing.SupportsIndex, '
                       'branches: collections.abc.Sequence[bytes]) -> bytes'),
 'share_results_cpu': ('def', 'share_results_cpu(job_block: bytes, records: bytes, targets: bytes) -> bytes'),
 'share_roots_cpu': ('def', 'share_roots_cpu(job_block: bytes, prefixes: bytes) -> bytes'),
 'sv2_scan': ('def',
              'sv2_scan(buf: typing_extensions.Buffer, max_frame: typing.SupportsInt | typing.SupportsIndex) -> '
              'tuple[list, int, int]'),
 'trace_mark': ('def', 'trace_mark(arg0: str) -> None'),
 'trace_pop': ('def', 'trace_pop() -> None'),
 'trace_push': ('def', 'trace_push(arg0: str) -> None'),
 'variant_header': ('def',
                    'variant_header(arg0: dict, arg1: typing.SupportsInt | typing.SupportsIndex) -> tuple[bytes, '
                    'int, int, int]'),
 'variant_space': ('def', 'variant_space(arg0: dict) -> int'),
 'x11': ('def', 'x11(msg: bytes) -> bytes'),
 'x11_luffa_sbox_selfcheck': ('def', 'x11_luffa_sbox_selfcheck() -> bool'),
 'x11_midstage_polls': ('def', 'x11_midstage_polls() -> bool'),
 'x11_prepare': ('def', 'x11_prepare(arg0: bytes, arg1: bytes) -> bytes'),
 'x11_stage': ('def', 'x11_stage(stage: typing.SupportsInt | typing.SupportsIndex, msg: bytes) -> bytes'),
 'x11_trace': ('def', 'x11_trace(msg: bytes) -> bytes')}
# fmt: on


def _surface(mod):
    out = {}
    for name in dir(mod):
        if name.startswith("__"):
            continue
        v = getattr(mod, name)
        if isinstance(v, type):
            out[name] = ("class", v.__init__.__doc__.splitlines()[0],
                         tuple(sorted(k for k in dir(v) if not k.startswith("_"))))
        elif callable(v):
            out[name] = ("def", v.__doc__.splitlines()[0])
        else:
            out[name] = ("const", v)
    return out


def test_native_surface_is_pinned():
    got = _surface(require_native())
    assert sorted(set(SURFACE) - set(got)) == [], "names missing from _native"
    assert sorted(set(got) - set(SURFACE)) == [], "names _native did not have"
    changed = {k: (SURFACE[k], got[k]) for k in SURFACE if got[k] != SURFACE[k]}
    assert changed == {}
    assert got == SURFACE
