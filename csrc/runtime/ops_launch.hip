// Launches for the Python ops layer (declared in otedama/search_launch.h): torch owns the buffers and the streams,
// so pointers and the stream arrive as integers, nothing here synchronises, and a HIP error is thrown as
// std::runtime_error. Host code only: the kernels and their launch_* functions are in csrc/kernels.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "otedama/hip_check.h"
#include "otedama/hitsink.h"
#include "otedama/job.h"
#include "otedama/search_launch.h"
#include "otedama/x11_launch.h"

namespace otedama {

namespace {

// Searches: hits go to the legacy device-memory slots after out[0]; no abort word.
HitSink ops_sink(uintptr_t out, uint32_t cap, uint32_t words) {
  HitSink s;
  s.out = reinterpret_cast<uint32_t*>(out);
  s.cap = cap;
  s.words = words;
  return s;
}

}  // namespace

void py_launch_sha256d(const Sha256dParams& p, uint32_t base, uint64_t count, uintptr_t out, uint32_t cap, int grid,
                       uintptr_t stream) {
  OTD_HIP(launch_sha256d_search(p, base, count, ops_sink(out, cap, 1), grid, reinterpret_cast<hipStream_t>(stream)));
}

void py_launch_sha256d_k(const Sha256dParamsK& p, uint32_t base, uint64_t count, uintptr_t out, uint32_t cap, int grid,
                         uintptr_t stream) {
  OTD_HIP(launch_sha256d_search_k(p, base, count, ops_sink(out, cap, 2), grid, reinterpret_cast<hipStream_t>(stream)));
}

void py_launch_sha256d_v(const Sha256dParamsV& p, uintptr_t vars, uint32_t base, uint64_t count, uintptr_t out,
                         uint32_t cap, int grid, uintptr_t stream, int block, int chains) {
  OTD_HIP(launch_sha256d_search_v(p, reinterpret_cast<const Sha256dVariant*>(vars), base, count,
                                  ops_sink(out, cap, 2), grid, reinterpret_cast<hipStream_t>(stream), block, chains));
}

void py_launch_scrypt(const ScryptParams& p, uint32_t base, uint32_t count, uintptr_t xbuf, uintptr_t scratch, int gap,
                      uintptr_t out, uint32_t cap, int grid, uintptr_t stream) {
  OTD_HIP(launch_scrypt_search(p, base, count, reinterpret_cast<void*>(xbuf), reinterpret_cast<void*>(scratch), gap,
                               ops_sink(out, cap, 1), grid, reinterpret_cast<hipStream_t>(stream)));
}

void py_launch_x11_stage(const X11Params& p, int stage, uint32_t base, uintptr_t H, uint32_t stride, uint32_t n,
                         uintptr_t out, uint32_t cap, uintptr_t stream) {
  const HitSink s = ops_sink(out, cap, 1);
  OTD_HIP(x11_launch_stage(stage, p, base, reinterpret_cast<uint64_t*>(H), stride, n, out ? &s : nullptr,
                           reinterpret_cast<hipStream_t>(stream)));
}

void py_launch_x11(const X11Params& p, uint32_t base, uintptr_t H, uint32_t stride, uint32_t n, uintptr_t out,
                   uint32_t cap, uintptr_t stream) {
  const HitSink s = ops_sink(out, cap, 1);
  OTD_HIP(x11_launch_chain(p, base, reinterpret_cast<uint64_t*>(H), stride, n, out ? &s : nullptr,
                           reinterpret_cast<hipStream_t>(stream)));
}

void py_launch_sha256d_digest(uintptr_t headers, uint32_t n, uintptr_t out, uintptr_t stream) {
  hip_check(launch_sha256d_digest(reinterpret_cast<const uint8_t*>(headers), n, reinterpret_cast<uint8_t*>(out),
                                  reinterpret_cast<hipStream_t>(stream)),
            "launch_sha256d_digest");
}

void py_launch_scrypt_digest(uintptr_t headers, uint32_t n, uintptr_t xbuf, uintptr_t scratch, int gap, uintptr_t out,
                             int grid, uintptr_t stream) {
  hip_check(launch_scrypt_digest(reinterpret_cast<const uint8_t*>(headers), n, reinterpret_cast<void*>(xbuf),
                                 reinterpret_cast<void*>(scratch), gap, reinterpret_cast<uint8_t*>(out), grid,
                                 reinterpret_cast<hipStream_t>(stream)),
            "launch_scrypt_digest");
}

void py_launch_x11_digest(uintptr_t headers, uintptr_t H, uint32_t stride, uint32_t n, uintptr_t out,
                          uintptr_t stream) {
  hip_check(launch_x11_digest(reinterpret_cast<const uint8_t*>(headers), reinterpret_cast<uint64_t*>(H), stride, n,
                              reinterpret_cast<uint8_t*>(out), reinterpret_cast<hipStream_t>(stream)),
            "launch_x11_digest");
}

void py_launch_share_headers(uintptr_t job, uintptr_t records, uint32_t n, uintptr_t headers, uintptr_t stream) {
  hip_check(launch_share_headers(reinterpret_cast<const void*>(job), reinterpret_cast<const uint8_t*>(records), n,
                                 reinterpret_cast<uint8_t*>(headers), reinterpret_cast<hipStream_t>(stream)),
            "launch_share_headers");
}

void py_launch_share_verdict(uintptr_t job, uintptr_t records, uintptr_t digests, uintptr_t targets,
                             uint32_t n_targets, uint32_t n, uintptr_t verdicts, uintptr_t stream) {
  hip_check(launch_share_verdict(reinterpret_cast<const void*>(job), reinterpret_cast<const uint8_t*>(records),
                                 reinterpret_cast<const uint8_t*>(digests), reinterpret_cast<const uint8_t*>(targets),
                                 n_targets, n, reinterpret_cast<uint8_t*>(verdicts),
                                 reinterpret_cast<hipStream_t>(stream)),
            "launch_share_verdict");
}

void py_launch_share_pack(uintptr_t job, uintptr_t records, uintptr_t headers, uintptr_t digests, uintptr_t targets,
                          uint32_t n_targets, uint32_t n, uintptr_t results, uintptr_t stream) {
  hip_check(launch_share_pack(reinterpret_cast<const void*>(job), reinterpret_cast<const uint8_t*>(records),
                              reinterpret_cast<const uint8_t*>(headers), reinterpret_cast<const uint8_t*>(digests),
                              reinterpret_cast<const uint8_t*>(targets), n_targets, n,
                              reinterpret_cast<uint8_t*>(results), reinterpret_cast<hipStream_t>(stream)),
            "launch_share_pack");
}

void py_launch_channel_roots(uintptr_t job, uintptr_t prefixes, uint32_t n, uintptr_t roots, uintptr_t stream) {
  hip_check(launch_channel_roots(reinterpret_cast<const void*>(job), reinterpret_cast<const uint8_t*>(prefixes), n,
                                 reinterpret_cast<uint8_t*>(roots), reinterpret_cast<hipStream_t>(stream)),
            "launch_channel_roots");
}

void py_launch_merkle_tree(uintptr_t leaves, uint32_t t, uint32_t n, uintptr_t scratch, uintptr_t out,
                           uintptr_t stream) {
  hip_check(launch_merkle_tree(reinterpret_cast<const uint8_t*>(leaves), t, n, reinterpret_cast<uint8_t*>(scratch),
                               reinterpret_cast<uint8_t*>(out), reinterpret_cast<hipStream_t>(stream)),
            "launch_merkle_tree");
}

void py_launch_secp256k1_mul(uintptr_t rows, uint32_t n, uintptr_t out, uintptr_t stream) {
  hip_check(launch_secp256k1_mul(reinterpret_cast<const uint8_t*>(rows), n, reinterpret_cast<uint8_t*>(out),
                                 reinterpret_cast<hipStream_t>(stream)),
            "launch_secp256k1_mul");
}

void py_launch_aead_seal(uintptr_t in, uint64_t in_bytes, uint32_t n, uintptr_t out, uint64_t out_bytes,
                         uintptr_t stream) {
  hip_check(launch_aead_seal(reinterpret_cast<const uint8_t*>(in), in_bytes, n, reinterpret_cast<uint8_t*>(out),
                             out_bytes, reinterpret_cast<hipStream_t>(stream)),
            "launch_aead_seal");
}

void py_launch_poly1305_rows(uintptr_t rows, uint32_t n, uintptr_t tags, uintptr_t stream) {
  hip_check(launch_poly1305_rows(reinterpret_cast<const uint8_t*>(rows), n, reinterpret_cast<uint8_t*>(tags),
                                 reinterpret_cast<hipStream_t>(stream)),
            "launch_poly1305_rows");
}

}  // namespace otedama
