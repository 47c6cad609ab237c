// ChaCha20-Poly1305 sealing (RFC 8439, empty associated data) in plain C++, written once for the host and for gfx950:
// the arithmetic of the batched frame seal (csrc/kernels/aead_seal.hip; buffers and limits: otedama/aead.h). The
// OpenSSL twin (csrc/cpu/aead.cpp, aead_seal_many_cpu) is a different implementation on purpose.
//
// B provides rol(x, n), a 32-bit rotate left: the kernel passes the cdna_bitops.h helper, the host PlainBits.
//
// Keys, keystream and plaintext are secrets: no branch and no memory index is made from them, the final h >= p
// subtraction of Poly1305 is a select. Lengths and counters are public; loops and masks depend on them.
//
// Poly1305 keeps h and r in five 26-bit limbs: a block is 25 multiply-adds 32 x 32 + 64 -> 64 (v_mad_u64_u32; the
// sums stay below 2^62), then one carry pass. h is only partly reduced between blocks, below 2^130 + a few bits.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define OTD_CP_FN __host__ __device__ inline
#else
#define OTD_CP_FN inline
#endif

namespace otedama {
namespace chachapoly {

struct PlainBits {
  static OTD_CP_FN uint32_t rol(uint32_t x, uint32_t n) { return (x << n) | (x >> (32u - n)); }
};

template <class B>
OTD_CP_FN void quarter_round(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
  a += b; d = B::rol(d ^ a, 16);
  c += d; b = B::rol(b ^ c, 12);
  a += b; d = B::rol(d ^ a, 8);
  c += d; b = B::rol(b ^ c, 7);
}

// One 64-byte block of the ChaCha20 keystream as sixteen little-endian words: key (eight words), the 32-bit block
// counter and the 96-bit nonce n0 | n1 | n2.
template <class B>
OTD_CP_FN void chacha20_block(const uint32_t key[8], uint32_t block, uint32_t n0, uint32_t n1, uint32_t n2,
                              uint32_t out[16]) {
  uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                     key[4],      key[5],      key[6],      key[7],      block,  n0,     n1,     n2};
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = in[i];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    quarter_round<B>(x[0], x[4], x[8], x[12]);
    quarter_round<B>(x[1], x[5], x[9], x[13]);
    quarter_round<B>(x[2], x[6], x[10], x[14]);
    quarter_round<B>(x[3], x[7], x[11], x[15]);
    quarter_round<B>(x[0], x[5], x[10], x[15]);
    quarter_round<B>(x[1], x[6], x[11], x[12]);
    quarter_round<B>(x[2], x[7], x[8], x[13]);
    quarter_round<B>(x[3], x[4], x[9], x[14]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = x[i] + in[i];
}

// Zero the bytes from `keep` (1..15) on of a 16-byte block held as four little-endian words.
OTD_CP_FN void keep_bytes(uint32_t w[4], uint32_t keep) {
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t have = keep > 4 * i ? keep - 4 * i : 0;  // bytes of this word that stay
    w[i] = have >= 4 ? w[i] : have == 0 ? 0u : (w[i] & ((1u << (8 * have)) - 1u));
  }
}

struct Poly1305 {
  uint32_t r0, r1, r2, r3, r4;
  uint32_t s1, s2, s3, s4;  // 5 r_i
  uint32_t h0, h1, h2, h3, h4;
  uint32_t pad[4];

  // k: the one-time key r | s as eight little-endian words. r is clamped here.
  OTD_CP_FN void init(const uint32_t k[8]) {
    r0 = k[0] & 0x3ffffffu;
    r1 = ((k[0] >> 26) | (k[1] << 6)) & 0x3ffff03u;
    r2 = ((k[1] >> 20) | (k[2] << 12)) & 0x3ffc0ffu;
    r3 = ((k[2] >> 14) | (k[3] << 18)) & 0x3f03fffu;
    r4 = (k[3] >> 8) & 0x00fffffu;
    s1 = r1 * 5u; s2 = r2 * 5u; s3 = r3 * 5u; s4 = r4 * 5u;
    h0 = h1 = h2 = h3 = h4 = 0;
    pad[0] = k[4]; pad[1] = k[5]; pad[2] = k[6]; pad[3] = k[7];
  }

  // h = (h + t + top * 2^128) * r, partly reduced. top is 1 for a full 16-byte block.
  OTD_CP_FN void block(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t top) {
    h0 += t0 & 0x3ffffffu;
    h1 += ((t0 >> 26) | (t1 << 6)) & 0x3ffffffu;
    h2 += ((t1 >> 20) | (t2 << 12)) & 0x3ffffffu;
    h3 += ((t2 >> 14) | (t3 << 18)) & 0x3ffffffu;
    h4 += (t3 >> 8) | (top << 24);
    uint64_t d0 = uint64_t(h0) * r0 + uint64_t(h1) * s4 + uint64_t(h2) * s3 + uint64_t(h3) * s2 + uint64_t(h4) * s1;
    uint64_t d1 = uint64_t(h0) * r1 + uint64_t(h1) * r0 + uint64_t(h2) * s4 + uint64_t(h3) * s3 + uint64_t(h4) * s2;
    uint64_t d2 = uint64_t(h0) * r2 + uint64_t(h1) * r1 + uint64_t(h2) * r0 + uint64_t(h3) * s4 + uint64_t(h4) * s3;
    uint64_t d3 = uint64_t(h0) * r3 + uint64_t(h1) * r2 + uint64_t(h2) * r1 + uint64_t(h3) * r0 + uint64_t(h4) * s4;
    uint64_t d4 = uint64_t(h0) * r4 + uint64_t(h1) * r3 + uint64_t(h2) * r2 + uint64_t(h3) * r1 + uint64_t(h4) * r0;
    uint32_t c = uint32_t(d0 >> 26); h0 = uint32_t(d0) & 0x3ffffffu;
    d1 += c; c = uint32_t(d1 >> 26); h1 = uint32_t(d1) & 0x3ffffffu;
    d2 += c; c = uint32_t(d2 >> 26); h2 = uint32_t(d2) & 0x3ffffffu;
    d3 += c; c = uint32_t(d3 >> 26); h3 = uint32_t(d3) & 0x3ffffffu;
    d4 += c; c = uint32_t(d4 >> 26); h4 = uint32_t(d4) & 0x3ffffffu;
    h0 += c * 5u; c = h0 >> 26; h0 &= 0x3ffffffu;
    h1 += c;
  }

  // The message's last block when it is short: w holds its `len` bytes (1..15), the rest of w is not looked at. A
  // 0x01 byte follows the message, then zeros, and no 2^128.
  OTD_CP_FN void last(const uint32_t w[4], uint32_t len) {
    uint32_t t[4] = {w[0], w[1], w[2], w[3]};
    keep_bytes(t, len);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
      if (len / 4 == i) t[i] |= 1u << (8 * (len % 4));
    block(t[0], t[1], t[2], t[3], 0);
  }

  // tag = ((h mod 2^130 - 5) + s) mod 2^128 as four little-endian words
  OTD_CP_FN void finish(uint32_t tag[4]) {
    uint32_t c;
    c = h1 >> 26; h1 &= 0x3ffffffu;
    h2 += c; c = h2 >> 26; h2 &= 0x3ffffffu;
    h3 += c; c = h3 >> 26; h3 &= 0x3ffffffu;
    h4 += c; c = h4 >> 26; h4 &= 0x3ffffffu;
    h0 += c * 5u; c = h0 >> 26; h0 &= 0x3ffffffu;
    h1 += c; c = h1 >> 26; h1 &= 0x3ffffffu;
    h2 += c; c = h2 >> 26; h2 &= 0x3ffffffu;
    h3 += c; c = h3 >> 26; h3 &= 0x3ffffffu;
    h4 += c;  // h < 2^130 now: a carry out of h4 would have left h1..h4 near zero after the fold above
    // g = h + 5 - 2^130: not negative exactly when h >= p
    uint32_t g0 = h0 + 5u; c = g0 >> 26; g0 &= 0x3ffffffu;
    uint32_t g1 = h1 + c; c = g1 >> 26; g1 &= 0x3ffffffu;
    uint32_t g2 = h2 + c; c = g2 >> 26; g2 &= 0x3ffffffu;
    uint32_t g3 = h3 + c; c = g3 >> 26; g3 &= 0x3ffffffu;
    const uint32_t g4 = h4 + c - (1u << 26);
    const uint32_t take = (g4 >> 31) - 1u;  // all ones when h >= p
    h0 = (h0 & ~take) | (g0 & take);
    h1 = (h1 & ~take) | (g1 & take);
    h2 = (h2 & ~take) | (g2 & take);
    h3 = (h3 & ~take) | (g3 & take);
    h4 = (h4 & ~take) | (g4 & take);
    const uint32_t w0 = h0 | (h1 << 26);
    const uint32_t w1 = (h1 >> 6) | (h2 << 20);
    const uint32_t w2 = (h2 >> 12) | (h3 << 14);
    const uint32_t w3 = (h3 >> 18) | (h4 << 8);
    uint64_t f = uint64_t(w0) + pad[0];
    tag[0] = uint32_t(f);
    f = uint64_t(w1) + pad[1] + (f >> 32);
    tag[1] = uint32_t(f);
    f = uint64_t(w2) + pad[2] + (f >> 32);
    tag[2] = uint32_t(f);
    f = uint64_t(w3) + pad[3] + (f >> 32);
    tag[3] = uint32_t(f);
  }
};

// Poly1305 of a whole message held as little-endian words (word i = bytes 4i..4i+3; words past the message are
// not read beyond its last block).
OTD_CP_FN void poly1305_words(const uint32_t key[8], const uint32_t* msg, uint32_t len, uint32_t tag[4]) {
  Poly1305 p;
  p.init(key);
  uint32_t at = 0;
  for (; at + 16 <= len; at += 16) p.block(msg[at / 4], msg[at / 4 + 1], msg[at / 4 + 2], msg[at / 4 + 3], 1);
  if (at < len) p.last(msg + at / 4, len - at);
  p.finish(tag);
}

// One frame on byte pointers: the Poly key from block counter 0, the data keystream from block counter 1 on, the
// nonce four zero bytes and counter64 little-endian; the MAC over the ciphertext zero-padded to 16 bytes, then
// u64 0 | u64 len. out_ct takes len bytes, out_tag 16.
template <class B>
OTD_CP_FN void seal(const uint8_t key[32], uint64_t counter64, const uint8_t* plain, uint32_t len, uint8_t* out_ct,
                    uint8_t out_tag[16]) {
  uint32_t k[8], ks[16], tag[4];
  memcpy(k, key, 32);
  const uint32_t n1 = uint32_t(counter64), n2 = uint32_t(counter64 >> 32);
  chacha20_block<B>(k, 0, 0, n1, n2, ks);
  Poly1305 p;
  p.init(ks);
  for (uint32_t at = 0; at < len; at += 16) {
    if (at % 64 == 0) chacha20_block<B>(k, at / 64 + 1, 0, n1, n2, ks);
    const uint32_t have = len - at < 16 ? len - at : 16;
    uint32_t w[4] = {0, 0, 0, 0};
    memcpy(w, plain + at, have);
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] ^= ks[(at % 64) / 4 + i];
    if (have < 16) keep_bytes(w, have);
    memcpy(out_ct + at, w, have);
    p.block(w[0], w[1], w[2], w[3], 1);
  }
  p.block(0, 0, len, 0, 1);
  p.finish(tag);
  memcpy(out_tag, tag, 16);
  for (int i = 0; i < 16; ++i) ks[i] = 0;
  for (int i = 0; i < 8; ++i) k[i] = 0;
}

}  // namespace chachapoly
}  // namespace otedama
