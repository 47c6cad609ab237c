// The batched secp256k1 multiplication in plain C++ (rows and rules: otedama/secp256k1.h; the curve layer shared with
// the gfx950 kernel: otedama/secp256k1_curve.h) and the ElligatorSwift encoder of stratum/ellswift.py.
//
// Field elements are 4 x 64-bit limbs, little-endian, always fully reduced. A product is 16 multiply-adds into
// unsigned __int128; its high half is folded in with 2^256 = 2^32 + 977 (mod p).
#include "otedama/secp256k1.h"

#include <cstring>
#include <stdexcept>

#include "otedama/secp256k1_curve.h"

namespace otedama {
namespace {

using u128 = unsigned __int128;

struct Fe64 {
  struct fe {
    uint64_t v[4];
  };
  static constexpr uint64_t kFold = 0x1000003D1ull;  // 2^256 mod p

  // r + c·2^256 (mod 2^256), c < 2^64: returns the carry out of the top limb
  static uint64_t fold(fe& r, uint64_t c) {
    u128 t = u128(c) * kFold;
    for (int i = 0; i < 4; ++i) {
      t += r.v[i];
      r.v[i] = uint64_t(t);
      t >>= 64;
    }
    return uint64_t(t);
  }

  // r - p when r >= p or `over` (the value is r + 2^256)
  static void reduce_once(fe& r, uint64_t over) {
    fe s = r;
    const uint64_t carry = fold(s, 1);
    const uint64_t m = uint64_t(0) - uint64_t((over | carry) != 0);
    for (int i = 0; i < 4; ++i) r.v[i] = (s.v[i] & m) | (r.v[i] & ~m);
  }

  static fe mul(fe a, fe b) {
    uint64_t r[8] = {};
    for (int i = 0; i < 4; ++i) {
      uint64_t c = 0;
      for (int j = 0; j < 4; ++j) {
        const u128 t = u128(a.v[i]) * b.v[j] + r[i + j] + c;
        r[i + j] = uint64_t(t);
        c = uint64_t(t >> 64);
      }
      r[i + 4] = c;
    }
    fe o;
    u128 t = 0;
    for (int j = 0; j < 4; ++j) {
      t += u128(r[4 + j]) * kFold + r[j];
      o.v[j] = uint64_t(t);
      t >>= 64;
    }
    uint64_t c = fold(o, uint64_t(t));  // t < 2^34
    c = fold(o, c);                     // a second carry leaves a value below 2^68: it cannot carry again
    reduce_once(o, 0);
    return o;
  }
  static fe sqr(fe a) { return mul(a, a); }

  static fe add(fe a, fe b) {
    fe s;
    u128 t = 0;
    for (int i = 0; i < 4; ++i) {
      t += u128(a.v[i]) + b.v[i];
      s.v[i] = uint64_t(t);
      t >>= 64;
    }
    reduce_once(s, uint64_t(t));
    return s;
  }

  static fe sub(fe a, fe b) {
    fe d;
    uint64_t borrow = 0;
    for (int i = 0; i < 4; ++i) {
      const u128 t = u128(a.v[i]) - b.v[i] - borrow;
      d.v[i] = uint64_t(t);
      borrow = uint64_t(t >> 64) & 1u;
    }
    // a < b: add p back, which is subtracting 2^32 + 977 mod 2^256
    fe e;
    uint64_t bw = 0;
    for (int i = 0; i < 4; ++i) {
      const u128 t = u128(d.v[i]) - (i == 0 ? kFold : 0) - bw;
      e.v[i] = uint64_t(t);
      bw = uint64_t(t >> 64) & 1u;
    }
    const uint64_t m = uint64_t(0) - borrow;
    for (int i = 0; i < 4; ++i) d.v[i] = (e.v[i] & m) | (d.v[i] & ~m);
    return d;
  }

  static fe select(bool c, fe a, fe b) {
    const uint64_t m = uint64_t(0) - uint64_t(c);
    fe r;
    for (int i = 0; i < 4; ++i) r.v[i] = (a.v[i] & m) | (b.v[i] & ~m);
    return r;
  }
  static bool is_zero(fe a) { return (a.v[0] | a.v[1] | a.v[2] | a.v[3]) == 0; }
  static bool odd(fe a) { return (a.v[0] & 1u) != 0; }
  static fe small(uint32_t v) { return fe{{v, 0, 0, 0}}; }
  static fe from_words(const uint32_t w[8]) {
    fe r;
    for (int i = 0; i < 4; ++i) r.v[i] = uint64_t(w[2 * i]) | (uint64_t(w[2 * i + 1]) << 32);
    reduce_once(r, 0);
    return r;
  }
  static void to_words(fe a, uint32_t w[8]) {
    for (int i = 0; i < 4; ++i) {
      w[2 * i] = uint32_t(a.v[i]);
      w[2 * i + 1] = uint32_t(a.v[i] >> 32);
    }
  }
};

using C = secp::Curve<Fe64>;
using fe = Fe64::fe;

void load_be(const uint8_t* b, uint32_t w[8]) {
  for (int i = 0; i < 8; ++i) {
    const uint8_t* p = b + 4 * (7 - i);
    w[i] = (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3];
  }
}

void store_be(const uint32_t w[8], uint8_t* b) {
  for (int i = 0; i < 8; ++i) {
    uint8_t* p = b + 4 * (7 - i);
    p[0] = uint8_t(w[i] >> 24);
    p[1] = uint8_t(w[i] >> 16);
    p[2] = uint8_t(w[i] >> 8);
    p[3] = uint8_t(w[i]);
  }
}

fe neg(fe a) { return Fe64::sub(Fe64::small(0), a); }

// stratum/ellswift.py xswiftec_inv: false where it returns None
bool xswiftec_inv(fe x, fe u, unsigned which, fe& t) {
  const uint32_t cw[8] = OTD_SECP_C, hw[8] = OTD_SECP_HALF;
  const fe c = C::constant(cw), half = C::constant(hw);
  const fe g = C::curve_rhs(u);  // u^3 + 7
  fe v, s;
  if ((which & 2) == 0) {
    if (C::is_x(Fe64::sub(neg(x), u))) return false;
    v = x;
    const fe den = Fe64::add(Fe64::add(Fe64::sqr(u), Fe64::mul(u, v)), Fe64::sqr(v));
    if (Fe64::is_zero(den)) return false;
    s = Fe64::mul(neg(g), C::inv(den));
  } else {
    s = Fe64::sub(x, u);
    if (Fe64::is_zero(s)) return false;
    const fe g4 = Fe64::add(Fe64::add(g, g), Fe64::add(g, g));
    const fe su2 = Fe64::mul(s, Fe64::sqr(u));
    const fe inner = Fe64::add(g4, Fe64::add(Fe64::add(su2, su2), su2));
    fe r;
    if (!C::sqrt(Fe64::mul(neg(s), inner), r)) return false;
    if ((which & 1) && Fe64::is_zero(r)) return false;
    v = Fe64::mul(Fe64::sub(Fe64::mul(r, C::inv(s)), u), half);
  }
  fe w;
  if (!C::sqrt(s, w) || Fe64::is_zero(w)) return false;
  const unsigned k = which & 5;
  const fe one = Fe64::small(1);
  const fe cc = (k == 0 || k == 4) ? Fe64::sub(one, c) : Fe64::add(one, c);
  const fe body = Fe64::mul(w, Fe64::add(Fe64::mul(Fe64::mul(u, cc), half), v));
  t = (k == 0 || k == 5) ? neg(body) : body;
  return true;
}

}  // namespace

void secp256k1_mul_cpu(const uint8_t* rows, uint32_t n, uint8_t* out) {
  if (n == 0 || n > kSecpMaxRows) throw std::invalid_argument("secp256k1_mul_cpu: n must be in 1..65536");
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t* in = rows + size_t(i) * kSecpRowBytes;
    uint8_t* o = out + size_t(i) * kSecpOutBytes;
    uint32_t k[8], pa[8], pb[8], x[8], parity = 0;
    load_be(in, k);
    load_be(in + 32, pa);
    load_be(in + 64, pb);
    const uint32_t status = C::row(k, pa, pb, in[96], x, parity);
    std::memset(o, 0, kSecpOutBytes);
    store_be(x, o);
    o[32] = uint8_t(status);
    o[33] = uint8_t(parity);
    // the scalar's copy leaves the stack with the call
    volatile uint32_t* wipe = k;
    for (int j = 0; j < 8; ++j) wipe[j] = 0;
  }
}

int ellswift_encode_cpu(const uint8_t x32[32], const uint8_t* rnd, size_t rnd_len, uint8_t out[64]) {
  const uint32_t pw[8] = OTD_SECP_P;
  uint32_t xw[8];
  load_be(x32, xw);
  if (secp::words_ge(xw, pw)) return -1;
  const fe x = Fe64::from_words(xw);
  if (!C::is_x(x)) return -1;
  for (size_t at = 0; at + 33 <= rnd_len; at += 33) {
    uint32_t uw[8], tw[8];
    load_be(rnd + at, uw);
    const fe u = Fe64::from_words(uw);  // reduced mod p
    if (Fe64::is_zero(u)) continue;
    fe t;
    if (!xswiftec_inv(x, u, rnd[at + 32] & 7u, t) || Fe64::is_zero(t)) continue;
    Fe64::to_words(u, uw);
    Fe64::to_words(t, tw);
    store_be(uw, out);
    store_be(tw, out + 32);
    return 1;
  }
  return 0;
}

}  // namespace otedama
