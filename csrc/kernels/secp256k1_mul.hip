// secp256k1_mul — "n scalars and n points in, the x of every product out" on gfx950: the curve arithmetic of a batch of
// Noise NX responder handshakes (rows, limits and status rules: otedama/secp256k1.h).
//
//   otd_secp256k1_mul  one row per lane, blocks of 256, tail guard. A row comes in as six 16-byte loads (scalar and
//                      point) and the dword that holds kind, the 31 bytes of padding are not read; its result leaves
//                      as three 16-byte stores.
//
// Field elements are eight 32-bit limbs, little-endian, always fully reduced. A product is 64 multiply-adds
// 32 x 32 + 32 + 32 -> 64 (v_mad_u64_u32; the sum cannot overflow), row by row into sixteen limbs; the high eight are
// folded in with 2^256 = 2^32 + 977 (mod p): one multiply-add by 977 and the neighbouring limb per limb, the few bits
// that come out of the top folded once more. Inversion and square root are fixed addition chains (255 squarings, 15 or
// 13 products). mul and sqr are real calls, not inlined, with their operands and result in registers: the ladder's
// body (18 of them an iteration) and the chains stay small enough for the instruction cache.
//
// The curve layer (otedama/secp256k1_curve.h) is the CPU twin's: Jacobian coordinates, a = 0, a fixed 256 doublings
// and mixed additions, the scalar shifted through its registers, selects (v_cndmask) for the bit and for the point at
// infinity. No branch and no address depends on a scalar.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "otedama/hip_check.h"
#include "otedama/search_launch.h"
#include "otedama/secp256k1_curve.h"

namespace {

struct Fe32 {
  struct fe {
    uint32_t v[8];
  };

  // r + c·(2^32 + 977) mod 2^256 for c < 2^34: returns the carry out of the top limb
  static __device__ __forceinline__ uint32_t fold(fe& r, uint64_t c) {
    const uint64_t lo = c * 977u;
    uint64_t t = uint64_t(r.v[0]) + uint32_t(lo);
    r.v[0] = uint32_t(t);
    t = (t >> 32) + r.v[1] + (lo >> 32) + uint32_t(c);
    r.v[1] = uint32_t(t);
    t = (t >> 32) + r.v[2] + (c >> 32);
    r.v[2] = uint32_t(t);
#pragma unroll
    for (int i = 3; i < 8; ++i) {
      t = (t >> 32) + r.v[i];
      r.v[i] = uint32_t(t);
    }
    return uint32_t(t >> 32);
  }

  // r - p when r >= p or `over` (the value is r + 2^256)
  static __device__ __forceinline__ void reduce_once(fe& r, uint32_t over) {
    fe s = r;
    const uint32_t carry = fold(s, 1);
    const bool take = (over | carry) != 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = take ? s.v[i] : r.v[i];
  }

  static __device__ __noinline__ fe mul(fe a, fe b) {
    uint32_t r[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      uint32_t c = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint64_t t = uint64_t(a.v[i]) * b.v[j] + r[i + j] + c;
        r[i + j] = uint32_t(t);
        c = uint32_t(t >> 32);
      }
      r[i + 8] = c;
    }
    fe o;
    uint64_t t = 0;
    uint32_t below = 0;  // the high limb one place down: its 2^32 share of the fold
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      t = (t >> 32) + uint64_t(r[8 + j]) * 977u + r[j] + below;
      o.v[j] = uint32_t(t);
      below = r[8 + j];
    }
    uint32_t c = fold(o, (t >> 32) + below);  // below 2^33
    fold(o, c);                               // a second carry leaves a value below 2^67: it cannot carry again
    reduce_once(o, 0);
    return o;
  }
  static __device__ __forceinline__ fe sqr(fe a) { return mul(a, a); }

  static __device__ __forceinline__ fe add(fe a, fe b) {
    fe s;
    uint64_t t = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      t = (t >> 32) + a.v[i] + b.v[i];
      s.v[i] = uint32_t(t);
    }
    reduce_once(s, uint32_t(t >> 32));
    return s;
  }

  static __device__ __forceinline__ fe sub(fe a, fe b) {
    fe d, e;
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint64_t t = uint64_t(a.v[i]) - b.v[i] - borrow;
      d.v[i] = uint32_t(t);
      borrow = uint32_t(t >> 63);
    }
    // a < b: add p back, which is subtracting 2^32 + 977 mod 2^256
    uint32_t bw = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint64_t t = uint64_t(d.v[i]) - (i == 0 ? 977u : i == 1 ? 1u : 0u) - bw;
      e.v[i] = uint32_t(t);
      bw = uint32_t(t >> 63);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) d.v[i] = borrow ? e.v[i] : d.v[i];
    return d;
  }

  static __device__ __forceinline__ fe select(bool c, fe a, fe b) {
    fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
  }
  static __device__ __forceinline__ bool is_zero(fe a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) o |= a.v[i];
    return o == 0;
  }
  static __device__ __forceinline__ bool odd(fe a) { return (a.v[0] & 1u) != 0; }
  static __device__ __forceinline__ fe small(uint32_t v) {
    fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = i == 0 ? v : 0u;
    return r;
  }
  static __device__ __forceinline__ fe from_words(const uint32_t w[8]) {
    fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = w[i];
    reduce_once(r, 0);
    return r;
  }
  static __device__ __forceinline__ void to_words(fe a, uint32_t w[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = a.v[i];
  }
};

// the big-endian 256-bit value in two 16-byte loads as little-endian words
__device__ __forceinline__ void be_words(const uint4 hi, const uint4 lo, uint32_t w[8]) {
  w[7] = __builtin_bswap32(hi.x);
  w[6] = __builtin_bswap32(hi.y);
  w[5] = __builtin_bswap32(hi.z);
  w[4] = __builtin_bswap32(hi.w);
  w[3] = __builtin_bswap32(lo.x);
  w[2] = __builtin_bswap32(lo.y);
  w[1] = __builtin_bswap32(lo.z);
  w[0] = __builtin_bswap32(lo.w);
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void otd_secp256k1_mul(const uint4* __restrict__ rows, uint32_t n,
                                                                    uint4* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint4* in = rows + 8u * uint64_t(i);
  const uint4 q0 = in[0], q1 = in[1], q2 = in[2], q3 = in[3], q4 = in[4], q5 = in[5], q6 = in[6];
  uint32_t k[8], pa[8], pb[8], x[8], parity;
  be_words(q0, q1, k);
  be_words(q2, q3, pa);
  be_words(q4, q5, pb);
  const uint32_t status = otedama::secp::Curve<Fe32>::row(k, pa, pb, q6.x & 0xFFu, x, parity);
  uint4* o = out + 3u * uint64_t(i);
  o[0] = make_uint4(__builtin_bswap32(x[7]), __builtin_bswap32(x[6]), __builtin_bswap32(x[5]), __builtin_bswap32(x[4]));
  o[1] = make_uint4(__builtin_bswap32(x[3]), __builtin_bswap32(x[2]), __builtin_bswap32(x[1]), __builtin_bswap32(x[0]));
  o[2] = make_uint4(status | (parity << 8), 0u, 0u, 0u);
}

namespace otedama {

hipError_t launch_secp256k1_mul(const uint8_t* rows, uint32_t n, uint8_t* out, hipStream_t s) {
  if (n == 0 || n > kSecpMaxRows || !rows || !out || !aligned16(rows, out)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(otd_secp256k1_mul, dim3((n + 255u) / 256u), dim3(256), 0, s,
                     reinterpret_cast<const uint4*>(rows), n, reinterpret_cast<uint4*>(out));
  return hipGetLastError();
}

}  // namespace otedama
