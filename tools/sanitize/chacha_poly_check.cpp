// Stand-alone host check of the frame seal's arithmetic (csrc/include/otedama/chacha_poly.h, what the gfx950 kernel
// otd_aead_seal runs) for ASan + UBSan builds (tools/sanitize/run.sh): aead_seal_rows_host and the OpenSSL twin
// aead_seal_many_cpu on exactly sized heap buffers against one EVP seal a frame, over the lengths, batch sizes,
// counters, keys and plaintexts of tests/seal_cases.py; poly1305_rows_host against the big-integer tags of that file's
// table and against OpenSSL's Poly1305 on random rows; and the heads that break the rules.
#include <openssl/evp.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "otedama/aead.h"
#include "otedama/chacha_poly.h"
using namespace otedama;

namespace {

uint64_t rng_state = 0xC4AC4A20901DULL;
uint64_t rng() {  // xorshift64
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
void random_bytes(uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) p[i] = uint8_t(rng() >> 32);
}

int failures = 0;
void expect(bool ok, const char* what, size_t i) {
  if (!ok) {
    std::fprintf(stderr, "FAIL %s (case %zu)\n", what, i);
    ++failures;
  }
}

struct Frame {
  uint8_t key[32];
  uint64_t counter;
  std::vector<uint8_t> plain;
};

const uint64_t kCounters[] = {0, 1, 0xFFFFFFFFull, 0x100000000ull, 1ull << 63, 0xFFFFFFFFFFFFFFFEull};

Frame make_frame(size_t i, uint32_t len) {
  Frame f;
  f.plain.resize(len);
  random_bytes(f.key, 32);
  random_bytes(f.plain.data(), len);
  if (i % 7 == 5) std::memset(f.key, 0, 32);
  if (i % 7 == 6) std::memset(f.key, 0xFF, 32);
  if (i % 5 == 3) std::memset(f.plain.data(), 0, len);
  if (i % 5 == 4) std::memset(f.plain.data(), 0xFF, len);
  f.counter = kCounters[i % 6];
  return f;
}

uint32_t up16(uint32_t v) { return (v + 15u) & ~15u; }

// the input buffer of otedama/aead.h, sized exactly
std::vector<uint8_t> pack(const std::vector<Frame>& frames, size_t* out_bytes) {
  size_t in_off = frames.size() * kSealHeadBytes, out_off = 0, total = in_off;
  for (const Frame& f : frames) total += up16(uint32_t(f.plain.size()));
  std::vector<uint8_t> buf(total, 0);
  for (size_t i = 0; i < frames.size(); ++i) {
    const Frame& f = frames[i];
    uint8_t* h = buf.data() + i * kSealHeadBytes;
    const uint32_t len = uint32_t(f.plain.size()), src = uint32_t(in_off), dst = uint32_t(out_off);
    std::memcpy(h, f.key, 32);
    std::memcpy(h + 32, &f.counter, 8);
    std::memcpy(h + 40, &len, 4);
    std::memcpy(h + 44, &src, 4);
    std::memcpy(h + 48, &dst, 4);
    if (len) std::memcpy(buf.data() + in_off, f.plain.data(), len);
    in_off += up16(len);
    out_off += 16 + up16(len);
  }
  *out_bytes = out_off;
  return buf;
}

// one EVP seal with a fresh context: tag, ciphertext, zero padding, as a region
std::vector<uint8_t> reference(const Frame& f) {
  const std::string key(reinterpret_cast<const char*>(f.key), 32);
  std::string nonce(12, '\0');
  std::memcpy(&nonce[4], &f.counter, 8);
  const std::string plain(reinterpret_cast<const char*>(f.plain.data()), f.plain.size());
  const std::string sealed = aead_seal(AeadKind::kChaCha20Poly1305, key, nonce, plain, "");
  std::vector<uint8_t> region(16 + up16(uint32_t(plain.size())), 0);
  std::memcpy(region.data(), sealed.data() + plain.size(), 16);
  std::memcpy(region.data() + 16, sealed.data(), plain.size());
  return region;
}

void check_batch(const std::vector<Frame>& frames, const char* what) {
  size_t out_bytes = 0;
  const std::vector<uint8_t> in = pack(frames, &out_bytes);
  expect(aead_seal_check(in.data(), in.size(), uint32_t(frames.size()), 0) == out_bytes, what, 0);
  std::vector<uint8_t> host(out_bytes, 0), twin(out_bytes, 0), want;
  aead_seal_rows_host(in.data(), in.size(), uint32_t(frames.size()), host.data(), host.size());
  aead_seal_many_cpu(in.data(), in.size(), uint32_t(frames.size()), twin.data(), twin.size());
  for (const Frame& f : frames) {
    const std::vector<uint8_t> r = reference(f);
    want.insert(want.end(), r.begin(), r.end());
  }
  expect(want.size() == out_bytes && host == want, what, 1);
  expect(twin == want, what, 2);
  // the header's seal on byte pointers, into buffers of exactly len and 16 bytes
  for (size_t i = 0; i < frames.size(); i += 17) {
    const Frame& f = frames[i];
    std::vector<uint8_t> ct(f.plain.size()), tag(16);
    chachapoly::seal<chachapoly::PlainBits>(f.key, f.counter, f.plain.data(), uint32_t(f.plain.size()), ct.data(),
                                            tag.data());
    const std::vector<uint8_t> r = reference(f);
    expect(std::memcmp(tag.data(), r.data(), 16) == 0 &&
               (ct.empty() || std::memcmp(ct.data(), r.data() + 16, ct.size()) == 0),
           what, 100 + i);
  }
}

bool throws(const std::vector<uint8_t>& in, uint32_t n, size_t out_bytes) {
  std::vector<uint8_t> out(out_bytes, 0);
  int thrown = 0;
  try {
    aead_seal_rows_host(in.data(), in.size(), n, out.data(), out.size());
  } catch (const std::invalid_argument&) {
    ++thrown;
  }
  try {
    aead_seal_many_cpu(in.data(), in.size(), n, out.data(), out.size());
  } catch (const std::invalid_argument&) {
    ++thrown;
  }
  return thrown == 2;
}

std::vector<uint8_t> hex(const char* s) {
  std::vector<uint8_t> out;
  for (; s[0] && s[1]; s += 2) {
    unsigned v = 0;
    std::sscanf(s, "%2x", &v);
    out.push_back(uint8_t(v));
  }
  return out;
}

std::vector<uint8_t> poly_row(const uint8_t key[32], const std::vector<uint8_t>& msg) {
  std::vector<uint8_t> row(kPolyRowBytes, 0);
  const uint32_t len = uint32_t(msg.size());
  std::memcpy(row.data(), key, 32);
  std::memcpy(row.data() + 32, &len, 4);
  if (len) std::memcpy(row.data() + 48, msg.data(), len);
  return row;
}

void check_poly() {
  uint8_t r1[32] = {1}, rmax[32];
  const std::vector<uint8_t> rm = hex("ffffff0ffcffff0ffcffff0ffcffff0f");
  std::memcpy(rmax, rm.data(), 16);
  std::memset(rmax + 16, 0xFF, 16);
  struct Case {
    const uint8_t* key;
    std::vector<uint8_t> msg, tag;
  };
  auto ff = [](size_t n, int at = -1, uint8_t v = 0) {
    std::vector<uint8_t> m(n, 0xFF);
    if (at >= 0) m[size_t(at)] = v;
    return m;
  };
  const Case table[] = {
      {r1, ff(32), hex("03000000000000000000000000000000")},          // h = p + 3
      {r1, ff(32, 16, 0xFC), hex("00000000000000000000000000000000")},  // h = p
      {r1, ff(32, 16, 0xFB), hex("faffffffffffffffffffffffffffffff")},  // h = p - 1
      {r1, ff(32, 16, 0xFD), hex("01000000000000000000000000000000")},  // h = p + 1
      {rmax, ff(64), hex("900fe32bc15fa8d7bca8efe4c7e37eb1")},
      {rmax, ff(17), hex("7cfe7ff768f81f2763f8bf565df85f86")},
  };
  size_t i = 0;
  for (const Case& c : table) {
    const std::vector<uint8_t> row = poly_row(c.key, c.msg);
    std::vector<uint8_t> tag(16);
    poly1305_rows_host(row.data(), 1, tag.data());
    expect(tag == c.tag, "poly1305 table", i++);
  }
  // random rows of 0..112 bytes against OpenSSL's Poly1305, in one batch
  EVP_MAC* mac = EVP_MAC_fetch(nullptr, "POLY1305", nullptr);
  if (!mac) throw std::runtime_error("no POLY1305 in libcrypto");
  const size_t n = 400;
  std::vector<uint8_t> rows, want(n * 16), got(n * 16);
  for (size_t k = 0; k < n; ++k) {
    uint8_t key[32];
    random_bytes(key, 32);
    std::vector<uint8_t> msg(k < 113 ? k : rng() % 113);
    random_bytes(msg.data(), msg.size());
    const std::vector<uint8_t> row = poly_row(key, msg);
    rows.insert(rows.end(), row.begin(), row.end());
    EVP_MAC_CTX* mc = EVP_MAC_CTX_new(mac);
    size_t outl = 0;
    const uint8_t none = 0;
    if (!mc || EVP_MAC_init(mc, key, 32, nullptr) != 1 ||
        EVP_MAC_update(mc, msg.empty() ? &none : msg.data(), msg.size()) != 1 ||
        EVP_MAC_final(mc, want.data() + 16 * k, &outl, 16) != 1 || outl != 16)
      throw std::runtime_error("EVP_MAC POLY1305 failed");
    EVP_MAC_CTX_free(mc);
  }
  EVP_MAC_free(mac);
  poly1305_rows_host(rows.data(), uint32_t(n), got.data());
  for (size_t k = 0; k < n; ++k) expect(std::memcmp(&got[16 * k], &want[16 * k], 16) == 0, "poly1305 random", k);
  // a length over the row's limit: a zero tag, nothing read past the row
  uint8_t key[32];
  random_bytes(key, 32);
  std::vector<uint8_t> row = poly_row(key, std::vector<uint8_t>(kPolyMaxMsg, 7)), tag(16, 9);
  const uint32_t over = kPolyMaxMsg + 1;
  std::memcpy(row.data() + 32, &over, 4);
  poly1305_rows_host(row.data(), 1, tag.data());
  expect(tag == std::vector<uint8_t>(16, 0), "poly1305 over the limit", 0);
}

}  // namespace

int main() {
  // every length 0..130 and the block and limit edges, forwards and backwards, in one batch
  std::vector<uint32_t> lengths;
  for (uint32_t l = 0; l <= 130; ++l) lengths.push_back(l);
  for (uint32_t l : {191u, 192u, 193u, 255u, 256u, 257u, 1023u, 1024u, 2047u, 2048u}) lengths.push_back(l);
  std::vector<Frame> frames;
  for (size_t i = 0; i < lengths.size(); ++i) frames.push_back(make_frame(i, lengths[i]));
  for (size_t i = lengths.size(); i-- > 0;) frames.push_back(make_frame(frames.size(), lengths[i]));
  check_batch(frames, "lengths");
  for (size_t n : {1u, 63u, 64u, 65u, 257u}) {
    std::vector<Frame> batch;
    for (size_t i = 0; i < n; ++i) batch.push_back(make_frame(i + n, 55));
    check_batch(batch, "sizes");
  }
  check_poly();

  // heads that break the rules: both entries refuse them and write nothing
  std::vector<Frame> two = {make_frame(0, 55), make_frame(1, 20)};
  size_t out_bytes = 0;
  const std::vector<uint8_t> good = pack(two, &out_bytes);
  expect(!throws(good, 2, out_bytes), "a good batch", 0);
  expect(throws(good, 0, out_bytes) && throws(good, 3, out_bytes) && throws(good, 2, out_bytes - 16), "limits", 0);
  const struct {
    size_t at;
    uint32_t value;
  } broken[] = {{40, kSealMaxPlain + 1}, {44, 136}, {44, uint32_t(good.size())}, {44, 64}, {48, 8},
                {48, uint32_t(out_bytes)}, {64 + 48, 0xFFFFFFF0u}};
  size_t k = 0;
  for (const auto& b : broken) {
    std::vector<uint8_t> in = good;
    std::memcpy(in.data() + b.at, &b.value, 4);
    expect(throws(in, 2, out_bytes), "a broken head", k++);
  }
  std::vector<uint8_t> last = good;
  std::memset(last.data() + 32, 0xFF, 8);  // counter 2^64 - 1
  expect(throws(last, 2, out_bytes), "the counter that is no nonce", 0);

  if (failures) {
    std::fprintf(stderr, "chacha_poly_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("chacha_poly_check: %zu frames of the length batch, 5 size batches, 406 Poly1305 rows, 11 refused "
              "inputs: clean\n", frames.size());
  return 0;
}
