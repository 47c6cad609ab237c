// The SHA-256 helpers of the merkle folds (share_verify.hip, channel_roots.hip, merkle_tree.hip): the padding block
// of a 64-byte message as constants, the hash of a digest, and an unsigned min. Shared text, identical gfx950 code:
// each of the three files compiles to the kernels it had with a copy of its own (docs/KERNELS.md, "Template tree").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cdna_bitops.h"

namespace otedama_dev {

// The second block of every 64-byte message (left | right) is the padding block {0x80000000, 0 x 14, 512}: its
// schedule and K + W are compile-time constants, so only the round function remains.
struct PadKW {
  uint32_t kw[64];
};
__device__ constexpr uint32_t c_ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
__device__ constexpr PadKW pad64_kw() {
  uint32_t w[64] = {};
  w[0] = 0x80000000u;
  w[15] = 512u;
  for (int t = 16; t < 64; ++t) {
    const uint32_t a = w[t - 15], b = w[t - 2];
    w[t] = (c_ror(b, 17) ^ c_ror(b, 19) ^ (b >> 10)) + w[t - 7] + (c_ror(a, 7) ^ c_ror(a, 18) ^ (a >> 3)) + w[t - 16];
  }
  PadKW r = {};
  for (int t = 0; t < 64; ++t) r.kw[t] = sha256_k(t) + w[t];
  return r;
}

__device__ __forceinline__ void sha256_compress_pad64(uint32_t st[8]) {
  constexpr PadKW kPad64 = pad64_kw();
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    const uint32_t t1 = h + bS1(e) + ch(e, f, g) + kPad64.kw[t];
    const uint32_t t2 = bS0(a) + maj(a, b, c);
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// SHA-256 of the 32-byte digest whose big-endian words are in[8]: one padded block.
__device__ __forceinline__ void sha256_of_digest(const uint32_t in[8], uint32_t out[8]) {
  const uint32_t blk[16] = {in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], 0x80000000u, 0, 0, 0, 0, 0, 0, 256u};
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = kSha256IVd[k];
  sha256_compress(out, blk);
}

__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

}  // namespace otedama_dev
