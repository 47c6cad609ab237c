// AEAD (AES-256-GCM, ChaCha20-Poly1305) for wallet storage and the Noise transport.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

namespace otedama {

enum class AeadKind { kAes256Gcm = 0, kChaCha20Poly1305 = 1 };
constexpr int kAeadTagBytes = 16;

// Returns ciphertext || 16-byte tag. key: 32 bytes, nonce: 12 bytes.
std::string aead_seal(AeadKind kind, const std::string& key, const std::string& nonce, const std::string& plain,
                      const std::string& aad);
// Returns false on authentication failure (wrong key or tampered data).
bool aead_open(AeadKind kind, const std::string& key, const std::string& nonce, const std::string& sealed,
               const std::string& aad, std::string* plain);

// Batched frame sealing: n ChaCha20-Poly1305 seals with n keys, empty associated data and the Noise transport's nonce
// (four zero bytes, then the 64-bit counter little-endian), as one buffer in and one buffer out. The gfx950 kernel
// otd_aead_seal (csrc/kernels/aead_seal.hip), aead_seal_many_cpu (OpenSSL) and aead_seal_rows_host (the kernel's
// arithmetic, otedama/chacha_poly.h, compiled for the host) read and write the same bytes.
//
// Input: n heads of 64 bytes, then the data region.
//   head   key[32] | counter u64 | len u32 | in_off u32 | out_off u32 | 12 zero bytes      (little-endian)
//   in_off   byte offset of the plaintext from the start of the input, a multiple of 16; the plaintext is
//            zero-padded to a multiple of 16 bytes and lies inside the input
//   out_off  byte offset of the frame's region in the output, a multiple of 16
// Output: per frame a region of 16 + roundup16(len) bytes at out_off: the tag, then the ciphertext, then zeros up to
// the next multiple of 16. Nothing outside the regions is written.
// Limits: len <= kSealMaxPlain, 1 <= n <= kSealMaxFrames, both buffers below 4 GiB.
constexpr uint32_t kSealHeadBytes = 64;
constexpr uint32_t kSealMaxPlain = 2048;
constexpr uint32_t kSealMaxFrames = (1u << 24) - 1;

// Checks every head against the limits and the two buffer sizes; returns the end of the furthest output region.
// Throws std::invalid_argument for a head that breaks a rule above (out_bytes 0: the output size is not checked).
size_t aead_seal_check(const uint8_t* in, size_t in_bytes, uint32_t n, size_t out_bytes);
// The regions into out (the caller zeroes it; out_bytes at least aead_seal_check's result). One EVP context for all
// n frames.
void aead_seal_many_cpu(const uint8_t* in, size_t in_bytes, uint32_t n, uint8_t* out, size_t out_bytes);
void aead_seal_rows_host(const uint8_t* in, size_t in_bytes, uint32_t n, uint8_t* out, size_t out_bytes);

// Poly1305 rows, a test entry (otd_poly1305_rows; the pool does not use it): n rows of kPolyRowBytes,
//   one-time key r | s [32] | len u32 | 12 zero bytes | message[kPolyMaxMsg], zero after len
// -> n 16-byte tags. A row with len above kPolyMaxMsg gets a zero tag.
constexpr uint32_t kPolyRowBytes = 160;
constexpr uint32_t kPolyMaxMsg = 112;
void poly1305_rows_host(const uint8_t* rows, uint32_t n, uint8_t* tags);

}  // namespace otedama
