// aead_seal — "n frames with n keys in, every frame's tag and ciphertext out" on gfx950: the ChaCha20-Poly1305 seals
// of a job's Noise frames (buffers, heads and limits: otedama/aead.h; the arithmetic: otedama/chacha_poly.h).
//
//   otd_aead_seal      one frame per lane, blocks of 256, tail guard. A head comes in as four 16-byte loads. The lane
//                      then walks its frame 64 bytes a step: one ChaCha20 block in registers, up to four 16-byte
//                      loads of plaintext, xor, four 16-byte stores of ciphertext, four Poly1305 blocks. Lanes of a
//                      wave with shorter frames sit out the later steps (the loop bound is the lane's own, public,
//                      length). The tag is stored last, in front of the ciphertext. Lanes read and write at a stride
//                      of 64 bytes or more: nothing is coalesced, and at a few hundred bytes a frame nothing needs
//                      to be. No LDS.
//   otd_poly1305_rows  a test entry: one row of (one-time key, length, message) per lane through the same Poly1305,
//                      so a test can reach the final reduction's h >= p case, which no AEAD input does.
//
// A head is trusted for nothing: a lane whose offsets or length break otedama/aead.h's rules, or whose plaintext or
// region would leave the two buffers, writes nothing. The host checks the same rules before it enqueues.
//
// No branch and no address depends on a key, the keystream or the plaintext; rotates are v_alignbit_b32
// (cdna_bitops.h), Poly1305's products v_mad_u64_u32.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cdna_bitops.h"
#include "otedama/aead.h"
#include "otedama/chacha_poly.h"
#include "otedama/hip_check.h"
#include "otedama/search_launch.h"

namespace {

struct DevBits {
  static __device__ __forceinline__ uint32_t rol(uint32_t x, uint32_t n) { return otedama_dev::rol(x, n); }
};

using otedama::chachapoly::chacha20_block;
using otedama::chachapoly::keep_bytes;
using otedama::chachapoly::Poly1305;

}  // namespace

extern "C" __global__ __launch_bounds__(256) void otd_aead_seal(const uint4* __restrict__ in, uint32_t n,
                                                                uint64_t in_bytes, uint4* __restrict__ out,
                                                                uint64_t out_bytes) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint4* head = in + 4u * uint64_t(i);
  const uint4 q0 = head[0], q1 = head[1], q2 = head[2], q3 = head[3];
  const uint32_t key[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
  const uint32_t n1 = q2.x, n2 = q2.y, len = q2.z, in_off = q2.w, out_off = q3.x;
  const uint32_t padded = (len + 15u) & ~15u;
  if (len > otedama::kSealMaxPlain || ((in_off | out_off) & 15u) != 0 || uint64_t(in_off) + padded > in_bytes ||
      uint64_t(out_off) + 16u + padded > out_bytes)
    return;
  const uint4* src = in + in_off / 16u;
  uint4* region = out + out_off / 16u;
  uint4* dst = region + 1;

  uint32_t ks[16];
  chacha20_block<DevBits>(key, 0, 0, n1, n2, ks);
  Poly1305 p;
  p.init(ks);
  const uint32_t blocks = padded / 16u;
  for (uint32_t b = 0; b < blocks; b += 4) {
    chacha20_block<DevBits>(key, b / 4u + 1u, 0, n1, n2, ks);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      if (b + j < blocks) {
        const uint4 v = src[b + j];
        uint32_t w[4] = {v.x ^ ks[4 * j], v.y ^ ks[4 * j + 1], v.z ^ ks[4 * j + 2], v.w ^ ks[4 * j + 3]};
        const uint32_t left = len - 16u * (b + j);  // at least 1
        if (left < 16u) keep_bytes(w, left);
        dst[b + j] = make_uint4(w[0], w[1], w[2], w[3]);
        p.block(w[0], w[1], w[2], w[3], 1);
      }
    }
  }
  p.block(0, 0, len, 0, 1);  // u64 0 (no associated data) | u64 len
  uint32_t tag[4];
  p.finish(tag);
  region[0] = make_uint4(tag[0], tag[1], tag[2], tag[3]);
}

extern "C" __global__ __launch_bounds__(256) void otd_poly1305_rows(const uint4* __restrict__ rows, uint32_t n,
                                                                    uint4* __restrict__ tags) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint4* row = rows + (otedama::kPolyRowBytes / 16u) * uint64_t(i);
  const uint4 q0 = row[0], q1 = row[1];
  const uint32_t len = row[2].x;
  if (len > otedama::kPolyMaxMsg) {
    tags[i] = make_uint4(0, 0, 0, 0);
    return;
  }
  const uint32_t key[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
  Poly1305 p;
  p.init(key);
  const uint32_t full = len / 16u;
  for (uint32_t b = 0; b < full; ++b) {
    const uint4 v = row[3 + b];
    p.block(v.x, v.y, v.z, v.w, 1);
  }
  if (len % 16u) {
    const uint4 v = row[3 + full];  // full <= 6 here: inside the row
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    p.last(w, len % 16u);
  }
  uint32_t tag[4];
  p.finish(tag);
  tags[i] = make_uint4(tag[0], tag[1], tag[2], tag[3]);
}

namespace otedama {

hipError_t launch_aead_seal(const uint8_t* in, uint64_t in_bytes, uint32_t n, uint8_t* out, uint64_t out_bytes,
                            hipStream_t s) {
  if (n == 0 || n > kSealMaxFrames || !in || !out || !aligned16(in, out)) return hipErrorInvalidValue;
  if (in_bytes < uint64_t(n) * kSealHeadBytes || (in_bytes >> 32) || (out_bytes >> 32) || ((in_bytes | out_bytes) & 15u))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(otd_aead_seal, dim3((n + 255u) / 256u), dim3(256), 0, s, reinterpret_cast<const uint4*>(in), n,
                     in_bytes, reinterpret_cast<uint4*>(out), out_bytes);
  return hipGetLastError();
}

hipError_t launch_poly1305_rows(const uint8_t* rows, uint32_t n, uint8_t* tags, hipStream_t s) {
  if (n == 0 || n > kSealMaxFrames || !rows || !tags || !aligned16(rows, tags)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(otd_poly1305_rows, dim3((n + 255u) / 256u), dim3(256), 0, s,
                     reinterpret_cast<const uint4*>(rows), n, reinterpret_cast<uint4*>(tags));
  return hipGetLastError();
}

}  // namespace otedama
