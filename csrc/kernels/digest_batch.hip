// digest_batch — "hash these headers" on gfx950: n unrelated 80-byte headers in, n 32-byte digests out, for
// SHA-256d, scrypt and X11. The search kernels take one prepared header and a nonce range and keep only the word
// their filter compares; these ops return every bit of every digest, in the byte order PowAlgorithm.hash returns
// (the raw little-endian hash, not display order).
//
// Layout for all three: header i at headers + 80 * i, digest i at out + 32 * i, both arrays 16-byte aligned (80 and
// 32 are multiples of 16, so every header is five 16-byte loads and every digest two 16-byte stores). One header per
// lane, blocks of 256, a guard for the tail.
//
//   SHA-256d  otd_sha256d_digest below: all 64 + 64 + 64 rounds, no midstate (the headers share nothing) and no
//             early exit; the same v_bitop3 / v_alignbit round functions as the search kernels (cdna_bitops.h).
//   scrypt    otd_scrypt_pbkdf_in_hdr / _out_hdr below: per-lane job blocks around the search's PBKDF2 device
//             functions (scrypt_pbkdf_dev.h), with the search's own ROMix launch (scrypt_search.hip) between them.
//             They live here and not next to the search kernels because any kernel added to that file changed the
//             register allocation of otd_scrypt_pbkdf_out.
//   X11       launch_x11_digest below: k_blake512_hdr (x11_stages_a.hip) as stage 0, the search's stages 1..10 in
//             trace mode (ECHO writes the planes), then otd_x11_gather_digest packs words 0..3 of each item.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cdna_bitops.h"
#include "scrypt_pbkdf_dev.h"
#include "otedama/hip_check.h"
#include "otedama/job.h"
#include "otedama/search_launch.h"
#include "otedama/x11.h"
#include "otedama/x11_launch.h"

namespace {
using namespace otedama_dev;
using namespace otedama_dev::scryptk;
}  // namespace

extern "C" __global__ __launch_bounds__(256) void otd_sha256d_digest(const uint4* __restrict__ headers, uint32_t n,
                                                                     uint4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[20];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const uint4 v = headers[uint64_t(i) * 5u + q];
    w[4 * q] = __builtin_bswap32(v.x); w[4 * q + 1] = __builtin_bswap32(v.y);
    w[4 * q + 2] = __builtin_bswap32(v.z); w[4 * q + 3] = __builtin_bswap32(v.w);
  }
  // hash 1: header bytes 0..63, then bytes 64..79 with the padding of an 80-byte message
  uint32_t st[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) st[k] = kSha256IVd[k];
  sha256_compress(st, w);
  {
    const uint32_t blk[16] = {w[16], w[17], w[18], w[19], 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 640u};
    sha256_compress(st, blk);
  }
  // hash 2: the 32-byte digest of hash 1 as one padded block
  uint32_t d[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = kSha256IVd[k];
  {
    const uint32_t blk[16] = {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7],
                              0x80000000u, 0, 0, 0, 0, 0, 0, 256u};
    sha256_compress(d, blk);
  }
  // the digest's bytes are the state words big-endian
  out[2 * uint64_t(i)] = make_uint4(__builtin_bswap32(d[0]), __builtin_bswap32(d[1]), __builtin_bswap32(d[2]),
                                    __builtin_bswap32(d[3]));
  out[2 * uint64_t(i) + 1] = make_uint4(__builtin_bswap32(d[4]), __builtin_bswap32(d[5]), __builtin_bswap32(d[6]),
                                        __builtin_bswap32(d[7]));
}

// Digest ops (otedama::launch_scrypt_digest): the same three stages over `count` unrelated headers, header i at
// headers[5 * i] (80 bytes, 16-byte aligned), one header per lane. Each lane forms its own job block and runs the
// search's PBKDF2 device functions on it; the ROMix launch between the two is the search's.
extern "C" __global__ __launch_bounds__(256) void otd_scrypt_pbkdf_in_hdr(const uint4* __restrict__ headers,
                                                                          uint32_t count, uint4* __restrict__ xbuf) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  otedama::ScryptParams p;
  const uint32_t nonce = scrypt_job_from_header(headers + uint64_t(i) * 5u, p);
  uint32_t X[32];
  scrypt_pbkdf_in(p, nonce, X);
  store_entry(xbuf + (uint64_t(i) << 3), X);
}

// digests[2 * i], digests[2 * i + 1] = the 32 bytes hashlib.scrypt returns for header i.
extern "C" __global__ __launch_bounds__(256) void otd_scrypt_pbkdf_out_hdr(const uint4* __restrict__ headers,
                                                                           uint32_t count,
                                                                           const uint4* __restrict__ xbuf,
                                                                           uint4* __restrict__ digests) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  otedama::ScryptParams p;
  const uint32_t nonce = scrypt_job_from_header(headers + uint64_t(i) * 5u, p);
  uint32_t X[32];
  load_entry(xbuf + (uint64_t(i) << 3), X);
  uint32_t d[8];
  (void)scrypt_pbkdf_out<true>(p, nonce, X, d);
  digests[2 * uint64_t(i)] = make_uint4(bswap(d[0]), bswap(d[1]), bswap(d[2]), bswap(d[3]));
  digests[2 * uint64_t(i) + 1] = make_uint4(bswap(d[4]), bswap(d[5]), bswap(d[6]), bswap(d[7]));
}

// The X11 digest is the first 32 bytes of the ECHO output: words 0..3 of item i, from the planes (word w of item i at
// H[w * stride + i], little-endian) to out[2 * i], out[2 * i + 1].
extern "C" __global__ __launch_bounds__(256) void otd_x11_gather_digest(const uint64_t* __restrict__ H, uint32_t stride,
                                                                        uint32_t n, uint4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t h[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) h[w] = H[size_t(w) * stride + i];
  out[2 * uint64_t(i)] = make_uint4(uint32_t(h[0]), uint32_t(h[0] >> 32), uint32_t(h[1]), uint32_t(h[1] >> 32));
  out[2 * uint64_t(i) + 1] = make_uint4(uint32_t(h[2]), uint32_t(h[2] >> 32), uint32_t(h[3]), uint32_t(h[3] >> 32));
}

namespace otedama {

hipError_t launch_sha256d_digest(const uint8_t* headers, uint32_t n, uint8_t* out, hipStream_t s) {
  if (n == 0 || !headers || !out || !aligned16(headers, out)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(otd_sha256d_digest, dim3((n + 255u) / 256u), dim3(256), 0, s,
                     reinterpret_cast<const uint4*>(headers), n, reinterpret_cast<uint4*>(out));
  return hipGetLastError();
}

// `n` unrelated 80-byte headers (16-byte aligned, densely packed) -> n 32-byte digests (16-byte aligned), the bytes
// hashlib.scrypt(h, salt=h, n=1024, r=1, p=1) returns. One header per lane slot: n <= grid * 256, xbuf holds
// grid * 256 * 128 bytes. The ROMix runs with a sink that has no abort word, as the ops searches do.
hipError_t launch_scrypt_digest(const uint8_t* headers, uint32_t n, void* xbuf, void* scratch, int gap, uint8_t* out,
                                int grid, hipStream_t stream) {
  if (n == 0 || grid <= 0 || uint64_t(n) > uint64_t(grid) * 256u || !headers || !xbuf || !scratch || !out)
    return hipErrorInvalidValue;
  if (!scrypt_gap_valid(gap) || !aligned16(headers, out)) return hipErrorInvalidValue;
  const uint4* H = reinterpret_cast<const uint4*>(headers);
  uint4* X = static_cast<uint4*>(xbuf);
  const int eg = int((n + 255) / 256);
  hipLaunchKernelGGL(otd_scrypt_pbkdf_in_hdr, dim3(eg), dim3(256), 0, stream, H, n, X);
  if (launch_scrypt_romix(n, X, static_cast<uint4*>(scratch), gap, HitSink{}, grid, stream) != hipSuccess)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(otd_scrypt_pbkdf_out_hdr, dim3(eg), dim3(256), 0, stream, H, n, static_cast<const uint4*>(X),
                     reinterpret_cast<uint4*>(out));
  return hipGetLastError();
}

// H: 8 * stride u64 of scratch (the stage planes), n <= stride.
hipError_t launch_x11_digest(const uint8_t* headers, uint64_t* H, uint32_t stride, uint32_t n, uint8_t* out,
                             hipStream_t s) {
  if (n == 0 || n > stride || !headers || !H || !out || !aligned16(headers, out)) return hipErrorInvalidValue;
  hipError_t e = x11_launch_blake_hdr(headers, H, stride, n, s);
  const X11Params none{};  // stages 1..10 read nothing of the job without a sink
  for (int st = 1; e == hipSuccess && st < kX11StageCount; ++st) e = x11_launch_stage(st, none, 0u, H, stride, n, nullptr, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(otd_x11_gather_digest, dim3((n + 255u) / 256u), dim3(256), 0, s,
                     static_cast<const uint64_t*>(H), stride, n, reinterpret_cast<uint4*>(out));
  return hipGetLastError();
}

}  // namespace otedama
