// Stand-alone host check of the batched secp256k1 multiplication's CPU twin (csrc/cpu/secp256k1.cpp) for ASan + UBSan
// builds (tools/sanitize/run.sh): secp256k1_mul_cpu on exactly sized heap buffers against OpenSSL's EC_POINT_mul on
// NID_secp256k1, over the special scalars of tests/secp_cases.py on G and on x-only keys, 2,000 seeded random rows,
// batches of one row and of 65536, the bad rows and the limit violations. OpenSSL is only the oracle here: the twin
// does not use it.
#include <openssl/bn.h>
#include <openssl/ec.h>
#include <openssl/obj_mac.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "otedama/secp256k1.h"
using namespace otedama;

namespace {

EC_GROUP* group;
BN_CTX* ctx;
BIGNUM* order;

uint64_t rng_state = 0x5EC9256F00DULL;
uint64_t rng() {  // xorshift64
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
void random_bytes(uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) p[i] = uint8_t(rng() >> 32);
}

struct Row {
  uint8_t b[kSecpRowBytes];
};

Row make_row(const BIGNUM* k, uint8_t kind, const uint8_t* point, size_t point_len) {
  Row r;
  std::memset(r.b, 0, sizeof r.b);
  BN_bn2binpad(k, r.b, 32);
  if (point_len) std::memcpy(r.b + 32, point, point_len);
  r.b[96] = kind;
  return r;
}

// what OpenSSL says the output row is (kinds 0 and 1 only)
void reference(const Row& r, uint8_t out[kSecpOutBytes]) {
  std::memset(out, 0, kSecpOutBytes);
  const uint8_t kind = r.b[96];
  if (kind > 2) {
    out[32] = kSecpBadKind;
    return;
  }
  BIGNUM* k = BN_bin2bn(r.b, 32, nullptr);
  if (BN_is_zero(k) || BN_cmp(k, order) >= 0) {
    out[32] = kSecpBadScalar;
    BN_free(k);
    return;
  }
  EC_POINT* res = EC_POINT_new(group);
  int ok = 1;
  if (kind == 0) {
    ok = EC_POINT_mul(group, res, k, nullptr, nullptr, ctx);
  } else {
    BIGNUM* x = BN_bin2bn(r.b + 32, 32, nullptr);
    EC_POINT* pt = EC_POINT_new(group);
    if (!EC_POINT_set_compressed_coordinates(group, pt, x, 0, ctx)) {  // the even y; fails for x >= p or off the curve
      out[32] = kSecpBadPoint;
      ok = 0;
    } else {
      ok = EC_POINT_mul(group, res, nullptr, pt, k, ctx);
    }
    EC_POINT_free(pt);
    BN_free(x);
  }
  if (ok) {
    BIGNUM *x = BN_new(), *y = BN_new();
    EC_POINT_get_affine_coordinates(group, res, x, y, ctx);
    BN_bn2binpad(x, out, 32);
    out[33] = uint8_t(BN_is_odd(y));
    BN_free(x);
    BN_free(y);
  }
  EC_POINT_free(res);
  BN_free(k);
}

// exactly sized heap buffers in and out; returns the rows that differ from the reference
int run(const std::vector<Row>& rows, const std::vector<std::vector<uint8_t>>& want) {
  std::vector<uint8_t> in(rows.size() * kSecpRowBytes), out(rows.size() * kSecpOutBytes, 0xEE);
  for (size_t i = 0; i < rows.size(); ++i) std::memcpy(&in[i * kSecpRowBytes], rows[i].b, kSecpRowBytes);
  secp256k1_mul_cpu(in.data(), uint32_t(rows.size()), out.data());
  int bad = 0;
  for (size_t i = 0; i < rows.size(); ++i)
    bad += std::memcmp(&out[i * kSecpOutBytes], want[i % want.size()].data(), kSecpOutBytes) != 0;
  return bad;
}

int check(const std::vector<Row>& rows) {
  std::vector<std::vector<uint8_t>> want(rows.size(), std::vector<uint8_t>(kSecpOutBytes));
  for (size_t i = 0; i < rows.size(); ++i) reference(rows[i], want[i].data());
  return run(rows, want);
}

}  // namespace

int main() {
  group = EC_GROUP_new_by_curve_name(NID_secp256k1);
  ctx = BN_CTX_new();
  order = BN_new();
  EC_GROUP_get_order(group, order, ctx);
  int fails = 0, cases = 0;

  // the special scalars: 1, 2, 3, n - 1, n - 2, (n - 1) / 2, (n + 1) / 2, 2^255, 2^128 - 1, 56 bits
  std::vector<BIGNUM*> scalars;
  auto add_word = [&](unsigned long w) { BIGNUM* b = BN_new(); BN_set_word(b, w); scalars.push_back(b); };
  add_word(1); add_word(2); add_word(3);
  for (unsigned long d : {1ul, 2ul}) { BIGNUM* b = BN_dup(order); BN_sub_word(b, d); scalars.push_back(b); }
  { BIGNUM* b = BN_dup(order); BN_sub_word(b, 1); BN_rshift1(b, b); scalars.push_back(b); }
  { BIGNUM* b = BN_dup(order); BN_add_word(b, 1); BN_rshift1(b, b); scalars.push_back(b); }
  { BIGNUM* b = BN_new(); BN_set_bit(b, 255); scalars.push_back(b); }
  { BIGNUM* b = BN_new(); BN_set_bit(b, 128); BN_sub_word(b, 1); scalars.push_back(b); }
  { BIGNUM* b = BN_new(); BN_set_word(b, 0x00C0FFEE12345677ul); scalars.push_back(b); }

  // x-only keys: x = 1 and the x of eight multiples of G
  std::vector<std::vector<uint8_t>> xs;
  { std::vector<uint8_t> one(32, 0); one[31] = 1; xs.push_back(one); }
  for (int i = 0; i < 8; ++i) {
    uint8_t kb[32], ob[kSecpOutBytes];
    random_bytes(kb, 32);
    kb[0] &= 0x7F;
    BIGNUM* k = BN_bin2bn(kb, 32, nullptr);
    reference(make_row(k, 0, nullptr, 0), ob);
    xs.emplace_back(ob, ob + 32);
    BN_free(k);
  }

  std::vector<Row> rows;
  for (BIGNUM* k : scalars) {
    rows.push_back(make_row(k, 0, nullptr, 0));
    for (const auto& x : xs) rows.push_back(make_row(k, 1, x.data(), 32));
  }
  fails += check(rows);
  cases += int(rows.size());

  // 2,000 random rows: kind 0, kind 1 on a known key, kind 1 on a random x (about half are off the curve)
  std::vector<Row> rnd;
  for (int i = 0; i < 2000; ++i) {
    uint8_t kb[32], xb[32];
    random_bytes(kb, 32);
    if (i % 5) kb[0] &= 0x7F;  // the others may land at or above n
    BIGNUM* k = BN_bin2bn(kb, 32, nullptr);
    if (i % 3 == 0) {
      rnd.push_back(make_row(k, 0, nullptr, 0));
    } else if (i % 3 == 1) {
      rnd.push_back(make_row(k, 1, xs[size_t(i) % xs.size()].data(), 32));
    } else {
      random_bytes(xb, 32);
      rnd.push_back(make_row(k, 1, xb, 32));
    }
    BN_free(k);
  }
  fails += check(rnd);
  cases += int(rnd.size());

  // the bad rows: scalar 0, n, 2^256 - 1; x = p, x = 5; kind 9
  {
    std::vector<Row> bad;
    BIGNUM* zero = BN_new();
    BIGNUM* seven = BN_new();
    BN_set_word(seven, 7);
    uint8_t ff[32], p[32], five[32] = {0};
    std::memset(ff, 0xFF, 32);
    std::memset(p, 0xFF, 32);
    p[27] = 0xFE; p[28] = 0xFF; p[29] = 0xFF; p[30] = 0xFC; p[31] = 0x2F;
    five[31] = 5;
    bad.push_back(make_row(zero, 0, nullptr, 0));
    bad.push_back(make_row(order, 1, xs[1].data(), 32));
    Row all = make_row(seven, 1, xs[1].data(), 32);
    std::memcpy(all.b, ff, 32);
    bad.push_back(all);
    bad.push_back(make_row(seven, 1, p, 32));
    bad.push_back(make_row(seven, 1, five, 32));
    bad.push_back(make_row(seven, 9, xs[1].data(), 32));
    std::vector<std::vector<uint8_t>> want(bad.size(), std::vector<uint8_t>(kSecpOutBytes, 0));
    const uint8_t status[6] = {1, 1, 1, 2, 2, 3};
    for (size_t i = 0; i < bad.size(); ++i) {
      uint8_t ref[kSecpOutBytes];
      reference(bad[i], ref);
      want[i][32] = status[i];
      fails += std::memcmp(ref, want[i].data(), kSecpOutBytes) != 0;  // the reference agrees on what is bad
    }
    fails += run(bad, want);
    cases += int(bad.size());
    BN_free(zero);
    BN_free(seven);
  }

  // n = 1 and n = 65536
  fails += check(std::vector<Row>(rows.begin() + 4, rows.begin() + 5));
  {
    std::vector<Row> tile(rnd.begin(), rnd.begin() + 64), big(kSecpMaxRows);
    std::vector<std::vector<uint8_t>> want(64, std::vector<uint8_t>(kSecpOutBytes));
    for (size_t i = 0; i < 64; ++i) reference(tile[i], want[i].data());
    for (size_t i = 0; i < big.size(); ++i) big[i] = tile[i % 64];
    fails += run(big, want);
    cases += 1 + int(big.size());
  }

  int limits = 0;
  for (uint32_t n : {0u, kSecpMaxRows + 1}) {
    uint8_t in[kSecpRowBytes] = {0}, out[kSecpOutBytes];
    try {
      secp256k1_mul_cpu(in, n, out);
    } catch (const std::invalid_argument&) {
      ++limits;
    }
  }
  fails += limits != 2;
  for (BIGNUM* b : scalars) BN_free(b);
  BN_free(order);
  BN_CTX_free(ctx);
  EC_GROUP_free(group);
  std::printf("secp256k1_check: %d rows, %d limit violations refused, %d failures\n", cases, limits, fails);
  return fails != 0;
}
