// secp256k1 scalar multiplication in batches (csrc/kernels/secp256k1_mul.hip, csrc/cpu/secp256k1.cpp): the rows both
// read and write, the limits both keep, and the status rules both follow. It is what a Noise NX responder needs from
// the curve: e·G, e·X and s·X of every accepted connection (otedama_amd/stratum/noise.py).
//
// Input row, 128 bytes:  scalar[32] big-endian | point[64] | kind u8 | 31 bytes (zero; not read)
//   kind 0  the base point G; point is not read
//   kind 1  point[0..31] is an x-only key, lifted to the even y (noise.dh)
//   kind 2  point[0..63] is an ElligatorSwift encoding u | t, decoded as stratum/ellswift.py decode() does (u and t
//           reduced mod p, 0 replaced by 1, t doubled when u^3 + t^2 + 7 = 0), then lifted (ellswift.ecdh_x)
// Output row, 48 bytes:  x[32] big-endian affine x of scalar·point | status u8 | y_parity u8 | 14 zero bytes
//   status 0  ok
//   status 1  the scalar is 0 or at or above the group order n
//   status 2  a kind 1 x at or above p, or not on the curve
//   status 3  unknown kind (it wins over the other two: nothing else of such a row is looked at)
// A row with nonzero status has x and y_parity zero.
#pragma once
#include <cstddef>
#include <cstdint>

namespace otedama {

constexpr uint32_t kSecpRowBytes = 128;
constexpr uint32_t kSecpOutBytes = 48;
constexpr uint32_t kSecpMaxRows = 65536;

constexpr uint32_t kSecpKindG = 0, kSecpKindXOnly = 1, kSecpKindEllSwift = 2;
constexpr uint32_t kSecpOk = 0, kSecpBadScalar = 1, kSecpBadPoint = 2, kSecpBadKind = 3;

// The rows in plain C++ (4 x 64-bit limbs). Throws std::invalid_argument for n == 0 or n above kSecpMaxRows.
void secp256k1_mul_cpu(const uint8_t* rows, uint32_t n, uint8_t* out);

// stratum/ellswift.py encode(x, rand) with rand(33) served from `rnd`, 33 bytes a try: 1 and the 64 bytes in out, 0
// when the stream ran out before a try succeeded, -1 when x is not the x coordinate of a curve point.
int ellswift_encode_cpu(const uint8_t x[32], const uint8_t* rnd, size_t rnd_len, uint8_t out[64]);

}  // namespace otedama
