// Device functions of the scrypt PBKDF2 layers (stages 1 and 3 of scrypt(1024, 1, 1)) and the 128-byte state
// entries they exchange with ROMix through xbuf: shared by the search kernels (scrypt_search.hip) and the digest op
// (digest_batch.hip), so a digest is computed by the code the search runs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cdna_bitops.h"
#include "otedama/job.h"

namespace otedama_dev {
namespace scryptk {

__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

__device__ __forceinline__ void store_entry(uint4* __restrict__ dst, const uint32_t X[32]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) dst[q] = make_uint4(X[4 * q], X[4 * q + 1], X[4 * q + 2], X[4 * q + 3]);
}
__device__ __forceinline__ void load_entry(const uint4* __restrict__ src, uint32_t T[32]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const uint4 v = src[q];
    T[4 * q] = v.x; T[4 * q + 1] = v.y; T[4 * q + 2] = v.z; T[4 * q + 3] = v.w;
  }
}

// HMAC-SHA256 pad states for key K' (8 words).
__device__ __forceinline__ void hmac_states(const uint32_t key[8], uint32_t istate[8], uint32_t ostate[8]) {
  uint32_t blk[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) blk[i] = key[i] ^ 0x36363636u;
#pragma unroll
  for (int i = 8; i < 16; ++i) blk[i] = 0x36363636u;
#pragma unroll
  for (int i = 0; i < 8; ++i) istate[i] = kSha256IVd[i];
  sha256_compress(istate, blk);
#pragma unroll
  for (int i = 0; i < 8; ++i) blk[i] = key[i] ^ 0x5c5c5c5cu;
#pragma unroll
  for (int i = 8; i < 16; ++i) blk[i] = 0x5c5c5c5cu;
#pragma unroll
  for (int i = 0; i < 8; ++i) ostate[i] = kSha256IVd[i];
  sha256_compress(ostate, blk);
}

// Outer HMAC step: H(opad-state || digest) with fixed padding (768-bit message).
__device__ __forceinline__ void hmac_outer(const uint32_t ostate[8], const uint32_t digest[8], uint32_t out[8]) {
  uint32_t blk[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) blk[i] = digest[i];
  blk[8] = 0x80000000u;
#pragma unroll
  for (int i = 9; i < 15; ++i) blk[i] = 0u;
  blk[15] = 768u;
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = ostate[i];
  sha256_compress(out, blk);
}

// Stage 1: PBKDF2 #1 for `nonce` -> X[32] (LE words of the 128-byte B).
__device__ __forceinline__ void scrypt_pbkdf_in(const otedama::ScryptParams& p, uint32_t nonce, uint32_t X[32]) {
  // K' = SHA-256(header80) (key longer than the block size).
  uint32_t hdrbe[20];
#pragma unroll
  for (int i = 0; i < 19; ++i) hdrbe[i] = bswap(p.hdr[i]);
  hdrbe[19] = bswap(nonce);
  uint32_t key[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = p.hmid[i];
  {
    uint32_t blk[16] = {hdrbe[16], hdrbe[17], hdrbe[18], hdrbe[19], 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 640u};
    sha256_compress(key, blk);
  }
  uint32_t istate[8], ostate[8];
  hmac_states(key, istate, ostate);
  // salt = header80, 4 blocks of 32 bytes.
  uint32_t ist2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ist2[i] = istate[i];
  sha256_compress(ist2, hdrbe);  // header bytes 0..63
#pragma unroll
  for (int blkno = 1; blkno <= 4; ++blkno) {
    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = ist2[i];
    uint32_t blk[16] = {hdrbe[16], hdrbe[17], hdrbe[18], hdrbe[19], uint32_t(blkno), 0x80000000u,
                        0, 0, 0, 0, 0, 0, 0, 0, 0, (64u + 84u) * 8u};
    sha256_compress(st, blk);
    uint32_t t[8];
    hmac_outer(ostate, st, t);
#pragma unroll
    for (int i = 0; i < 8; ++i) X[8 * (blkno - 1) + i] = bswap(t[i]);
  }
}

// Stage 3: PBKDF2 #2 over X (salt = X || INT(1)); returns final state word 7. kFull (the digest op): `full` also
// receives the whole final state, the digest as big-endian words. The search instantiates the default, in which the
// other seven words of the last compression are dead code.
template <bool kFull = false>
__device__ __forceinline__ uint32_t scrypt_pbkdf_out(const otedama::ScryptParams& p, uint32_t nonce,
                                                     const uint32_t X[32], uint32_t* full = nullptr) {
  uint32_t key[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = p.hmid[i];
  {
    uint32_t blk[16] = {bswap(p.hdr[16]), bswap(p.hdr[17]), bswap(p.hdr[18]), bswap(nonce), 0x80000000u,
                        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 640u};
    sha256_compress(key, blk);
  }
  uint32_t istate[8], ostate[8];
  hmac_states(key, istate, ostate);
  uint32_t st[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] = istate[i];
  uint32_t blk[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) blk[i] = bswap(X[i]);
  sha256_compress(st, blk);
#pragma unroll
  for (int i = 0; i < 16; ++i) blk[i] = bswap(X[16 + i]);
  sha256_compress(st, blk);
  uint32_t tail[16] = {1u, 0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, (64u + 132u) * 8u};
  sha256_compress(st, tail);
  uint32_t out[8];
  hmac_outer(ostate, st, out);
  if constexpr (kFull) {
#pragma unroll
    for (int i = 0; i < 8; ++i) full[i] = out[i];
  }
  return out[7];
}

// Digest ops: the job block of one unrelated header, formed per lane from its 80 bytes (five 16-byte loads; the
// search kernels receive the same block as a kernarg from scrypt_prepare). Returns the header's own nonce word.
__device__ __forceinline__ uint32_t scrypt_job_from_header(const uint4* __restrict__ hdr, otedama::ScryptParams& p) {
  uint32_t w[20];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const uint4 v = hdr[q];
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int i = 0; i < 19; ++i) p.hdr[i] = w[i];
  uint32_t blk[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) blk[i] = bswap(w[i]);
#pragma unroll
  for (int i = 0; i < 8; ++i) p.hmid[i] = kSha256IVd[i];
  sha256_compress(p.hmid, blk);
  p.target_hi = 0u;
  return w[19];
}

}  // namespace scryptk
}  // namespace otedama_dev
