// Host AEAD primitives for the control plane, on OpenSSL EVP (libcrypto 3).
//
//  * AES-256-GCM: wallet.dat seed encryption (internal/lightning/seedstore.go:80-164 uses
//    Go's crypto/cipher GCM with a 12-byte nonce and 16-byte tag appended to the ciphertext;
//    we emit the same ciphertext||tag layout so files are interchangeable).
//  * ChaCha20-Poly1305 (IETF, 96-bit nonce): the Noise NX transport cipher
//    (stratum/noise.go:211-249).
// Neither is on the mining hot path, so plain EVP calls are enough.
//  * Batched frame sealing (otedama/aead.h): the pool's job fan-out seals n frames with n keys in one call,
//    aead_seal_many_cpu on one reused EVP context; aead_seal_rows_host and poly1305_rows_host run the gfx950
//    kernel's own arithmetic (otedama/chacha_poly.h) on the host, for tests on machines without a GPU.
#include "otedama/aead.h"

#include <openssl/evp.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "otedama/chacha_poly.h"

namespace otedama {
namespace {

struct CtxFree {
  void operator()(EVP_CIPHER_CTX* c) const { EVP_CIPHER_CTX_free(c); }
};
using Ctx = std::unique_ptr<EVP_CIPHER_CTX, CtxFree>;

const EVP_CIPHER* cipher_for(AeadKind k) {
  return k == AeadKind::kAes256Gcm ? EVP_aes_256_gcm() : EVP_chacha20_poly1305();
}

void check(int ok, const char* what) {
  if (ok != 1) throw std::runtime_error(std::string("aead: ") + what + " failed");
}

}  // namespace

std::string aead_seal(AeadKind kind, const std::string& key, const std::string& nonce, const std::string& plain,
                      const std::string& aad) {
  if (key.size() != 32) throw std::invalid_argument("aead: key must be 32 bytes");
  if (nonce.size() != 12) throw std::invalid_argument("aead: nonce must be 12 bytes");
  Ctx ctx(EVP_CIPHER_CTX_new());
  if (!ctx) throw std::bad_alloc();
  const auto* k = reinterpret_cast<const unsigned char*>(key.data());
  const auto* n = reinterpret_cast<const unsigned char*>(nonce.data());
  check(EVP_EncryptInit_ex(ctx.get(), cipher_for(kind), nullptr, nullptr, nullptr), "init");
  check(EVP_CIPHER_CTX_ctrl(ctx.get(), EVP_CTRL_AEAD_SET_IVLEN, 12, nullptr), "ivlen");
  check(EVP_EncryptInit_ex(ctx.get(), nullptr, nullptr, k, n), "key");
  int len = 0;
  if (!aad.empty())
    check(EVP_EncryptUpdate(ctx.get(), nullptr, &len, reinterpret_cast<const unsigned char*>(aad.data()),
                            static_cast<int>(aad.size())),
          "aad");
  std::string out(plain.size() + kAeadTagBytes, '\0');
  auto* o = reinterpret_cast<unsigned char*>(&out[0]);
  int total = 0;
  if (!plain.empty()) {
    check(EVP_EncryptUpdate(ctx.get(), o, &len, reinterpret_cast<const unsigned char*>(plain.data()),
                            static_cast<int>(plain.size())),
          "update");
    total = len;
  }
  check(EVP_EncryptFinal_ex(ctx.get(), o + total, &len), "final");
  total += len;
  check(EVP_CIPHER_CTX_ctrl(ctx.get(), EVP_CTRL_AEAD_GET_TAG, kAeadTagBytes, o + total), "tag");
  out.resize(total + kAeadTagBytes);
  return out;
}

bool aead_open(AeadKind kind, const std::string& key, const std::string& nonce, const std::string& sealed,
               const std::string& aad, std::string* plain) {
  if (key.size() != 32) throw std::invalid_argument("aead: key must be 32 bytes");
  if (nonce.size() != 12) throw std::invalid_argument("aead: nonce must be 12 bytes");
  if (sealed.size() < kAeadTagBytes) return false;
  Ctx ctx(EVP_CIPHER_CTX_new());
  if (!ctx) throw std::bad_alloc();
  const size_t clen = sealed.size() - kAeadTagBytes;
  check(EVP_DecryptInit_ex(ctx.get(), cipher_for(kind), nullptr, nullptr, nullptr), "init");
  check(EVP_CIPHER_CTX_ctrl(ctx.get(), EVP_CTRL_AEAD_SET_IVLEN, 12, nullptr), "ivlen");
  check(EVP_DecryptInit_ex(ctx.get(), nullptr, nullptr, reinterpret_cast<const unsigned char*>(key.data()),
                           reinterpret_cast<const unsigned char*>(nonce.data())),
        "key");
  int len = 0;
  if (!aad.empty())
    check(EVP_DecryptUpdate(ctx.get(), nullptr, &len, reinterpret_cast<const unsigned char*>(aad.data()),
                            static_cast<int>(aad.size())),
          "aad");
  std::string out(clen, '\0');
  auto* o = reinterpret_cast<unsigned char*>(&out[0]);
  int total = 0;
  if (clen) {
    check(EVP_DecryptUpdate(ctx.get(), o, &len, reinterpret_cast<const unsigned char*>(sealed.data()),
                            static_cast<int>(clen)),
          "update");
    total = len;
  }
  std::string tag = sealed.substr(clen);
  check(EVP_CIPHER_CTX_ctrl(ctx.get(), EVP_CTRL_AEAD_SET_TAG, kAeadTagBytes, &tag[0]), "settag");
  if (EVP_DecryptFinal_ex(ctx.get(), o + total, &len) != 1) {
    // authentication failure: wipe whatever was decrypted
    for (auto& c : out) c = 0;
    return false;
  }
  out.resize(total + len);
  *plain = std::move(out);
  return true;
}

// ---------------------------------------------------------------- batched frame sealing (buffers: otedama/aead.h)
namespace {

struct SealHead {
  const uint8_t* key;
  uint64_t counter;
  uint32_t len, in_off, out_off;
};

SealHead seal_head(const uint8_t* in, uint32_t i) {
  const uint8_t* h = in + size_t(i) * kSealHeadBytes;
  SealHead s;
  s.key = h;
  std::memcpy(&s.counter, h + 32, 8);
  std::memcpy(&s.len, h + 40, 4);
  std::memcpy(&s.in_off, h + 44, 4);
  std::memcpy(&s.out_off, h + 48, 4);
  return s;
}

uint32_t up16(uint32_t v) { return (v + 15u) & ~15u; }

}  // namespace

size_t aead_seal_check(const uint8_t* in, size_t in_bytes, uint32_t n, size_t out_bytes) {
  if (n == 0 || n > kSealMaxFrames) throw std::invalid_argument("aead seal: need 1..2^24-1 frames");
  if (!in || in_bytes < size_t(n) * kSealHeadBytes || (in_bytes & 15u) || (uint64_t(in_bytes) >> 32) ||
      (uint64_t(out_bytes) >> 32))
    throw std::invalid_argument("aead seal: the input is n 64-byte heads and a data region, a multiple of 16 "
                                "bytes, below 4 GiB");
  size_t end = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const SealHead h = seal_head(in, i);
    if (h.len > kSealMaxPlain) throw std::invalid_argument("aead seal: a frame is at most 2048 bytes");
    if (h.counter == UINT64_MAX) throw std::invalid_argument("aead seal: counter 2^64-1 is not a nonce");
    if ((h.in_off | h.out_off) & 15u) throw std::invalid_argument("aead seal: offsets are multiples of 16");
    if (h.in_off < uint64_t(n) * kSealHeadBytes || uint64_t(h.in_off) + up16(h.len) > in_bytes)
      throw std::invalid_argument("aead seal: a plaintext lies outside the data region");
    const uint64_t region_end = uint64_t(h.out_off) + 16u + up16(h.len);
    if ((region_end >> 32) || (out_bytes && region_end > out_bytes))
      throw std::invalid_argument("aead seal: a region lies outside the output");
    if (region_end > end) end = size_t(region_end);
  }
  return end;
}

void aead_seal_many_cpu(const uint8_t* in, size_t in_bytes, uint32_t n, uint8_t* out, size_t out_bytes) {
  aead_seal_check(in, in_bytes, n, out_bytes ? out_bytes : 1);
  Ctx ctx(EVP_CIPHER_CTX_new());
  if (!ctx) throw std::bad_alloc();
  check(EVP_EncryptInit_ex(ctx.get(), EVP_chacha20_poly1305(), nullptr, nullptr, nullptr), "init");
  check(EVP_CIPHER_CTX_ctrl(ctx.get(), EVP_CTRL_AEAD_SET_IVLEN, 12, nullptr), "ivlen");
  for (uint32_t i = 0; i < n; ++i) {
    const SealHead h = seal_head(in, i);
    unsigned char nonce[12] = {0, 0, 0, 0};
    std::memcpy(nonce + 4, &h.counter, 8);
    check(EVP_EncryptInit_ex(ctx.get(), nullptr, nullptr, h.key, nonce), "key");
    unsigned char* region = out + h.out_off;
    int len = 0, total = 0;
    if (h.len) {
      check(EVP_EncryptUpdate(ctx.get(), region + 16, &len, in + h.in_off, int(h.len)), "update");
      total = len;
    }
    check(EVP_EncryptFinal_ex(ctx.get(), region + 16 + total, &len), "final");
    check(EVP_CIPHER_CTX_ctrl(ctx.get(), EVP_CTRL_AEAD_GET_TAG, kAeadTagBytes, region), "tag");
    std::memset(region + 16 + h.len, 0, up16(h.len) - h.len);
  }
}

void aead_seal_rows_host(const uint8_t* in, size_t in_bytes, uint32_t n, uint8_t* out, size_t out_bytes) {
  aead_seal_check(in, in_bytes, n, out_bytes ? out_bytes : 1);
  for (uint32_t i = 0; i < n; ++i) {
    const SealHead h = seal_head(in, i);
    uint8_t* region = out + h.out_off;
    chachapoly::seal<chachapoly::PlainBits>(h.key, h.counter, in + h.in_off, h.len, region + 16, region);
    std::memset(region + 16 + h.len, 0, up16(h.len) - h.len);
  }
}

void poly1305_rows_host(const uint8_t* rows, uint32_t n, uint8_t* tags) {
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t* row = rows + size_t(i) * kPolyRowBytes;
    uint32_t key[8], len, msg[kPolyMaxMsg / 4], tag[4] = {0, 0, 0, 0};
    std::memcpy(key, row, 32);
    std::memcpy(&len, row + 32, 4);
    std::memcpy(msg, row + 48, kPolyMaxMsg);
    if (len <= kPolyMaxMsg) chachapoly::poly1305_words(key, msg, len, tag);
    std::memcpy(tags + size_t(i) * 16, tag, 16);
  }
}

}  // namespace otedama
