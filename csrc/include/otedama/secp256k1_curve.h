// The curve layer of the batched secp256k1 multiplication, written once over a field type F and used with 8 x 32-bit
// limbs on gfx950 (csrc/kernels/secp256k1_mul.hip) and 4 x 64-bit limbs on the host (csrc/cpu/secp256k1.cpp).
//
// F provides: fe (a field element, always fully reduced), mul, sqr, add, sub, select(c, a, b) = c ? a : b without a
// branch, is_zero, odd, from_words (eight little-endian 32-bit words of a value below 2^256, reduced mod p),
// to_words, and small(v).
//
// Control flow of mul() does not depend on the scalar: a fixed 256 doublings and 256 mixed additions, the scalar
// shifted out of its registers one bit an iteration (no memory index is made from it), every choice a select, the
// point at infinity in the accumulator a flag. What a row's public part decides (its kind, the ElligatorSwift
// cases) is branched on.
#pragma once
#include <cstdint>

#include "otedama/secp256k1.h"

#if defined(__HIPCC__)
#define OTD_SECP_FN __host__ __device__ inline
#define OTD_SECP_ROLLED _Pragma("unroll 1")
#else
#define OTD_SECP_FN inline
#define OTD_SECP_ROLLED
#endif

namespace otedama {
namespace secp {

// little-endian 32-bit words
#define OTD_SECP_N {0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}
#define OTD_SECP_P {0xFFFFFC2Fu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}
#define OTD_SECP_GX {0x16F81798u, 0x59F2815Bu, 0x2DCE28D9u, 0x029BFCDBu, 0xCE870B07u, 0x55A06295u, 0xF9DCBBACu, 0x79BE667Eu}
#define OTD_SECP_GY {0xFB10D4B8u, 0x9C47D08Fu, 0xA6855419u, 0xFD17B448u, 0x0E1108A8u, 0x5DA4FBFCu, 0x26A3C465u, 0x483ADA77u}
// sqrt(-3), the root a^((p+1)/4) gives (BIP324's c), and 1/2
#define OTD_SECP_C {0x1CD5F852u, 0x7D8D27AEu, 0xDA14ECD4u, 0xC61F6D15u, 0xA797962Cu, 0x233770C2u, 0x3507F1DFu, 0x0A2D2BA9u}
#define OTD_SECP_HALF {0x7FFFFE18u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x7FFFFFFFu}

// a >= b for 256-bit values in little-endian words
OTD_SECP_FN bool words_ge(const uint32_t a[8], const uint32_t b[8]) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = uint64_t(a[i]) - b[i] - borrow;
    borrow = uint32_t(d >> 63);
  }
  return borrow == 0;
}

OTD_SECP_FN bool words_zero(const uint32_t a[8]) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= a[i];
  return o == 0;
}

template <class F>
struct Curve {
  using fe = typename F::fe;

  struct Jac {
    fe x, y, z;
  };

  static OTD_SECP_FN fe constant(const uint32_t (&w)[8]) { return F::from_words(w); }

  static OTD_SECP_FN fe sqrn(fe a, int n) {
    OTD_SECP_ROLLED
    for (int i = 0; i < n; ++i) a = F::sqr(a);
    return a;
  }

  // a^(p - 2) (root == false) or a^((p + 1) / 4) (root == true): one addition chain over the run of 223 ones both
  // exponents begin with.
  static OTD_SECP_FN fe pow_chain(fe a, bool root) {
    const fe x2 = F::mul(F::sqr(a), a);
    const fe x3 = F::mul(F::sqr(x2), a);
    const fe x6 = F::mul(sqrn(x3, 3), x3);
    const fe x9 = F::mul(sqrn(x6, 3), x3);
    const fe x11 = F::mul(sqrn(x9, 2), x2);
    const fe x22 = F::mul(sqrn(x11, 11), x11);
    const fe x44 = F::mul(sqrn(x22, 22), x22);
    const fe x88 = F::mul(sqrn(x44, 44), x44);
    const fe x176 = F::mul(sqrn(x88, 88), x88);
    const fe x220 = F::mul(sqrn(x176, 44), x44);
    const fe x223 = F::mul(sqrn(x220, 3), x3);
    fe t = F::mul(sqrn(x223, 23), x22);
    if (root) {
      t = F::mul(sqrn(t, 6), x2);
      return sqrn(t, 2);
    }
    t = F::mul(sqrn(t, 5), a);
    t = F::mul(sqrn(t, 3), x2);
    return F::mul(sqrn(t, 2), a);
  }

  static OTD_SECP_FN fe inv(fe a) { return pow_chain(a, false); }  // inv(0) = 0

  // r = a^((p + 1) / 4); true when r^2 == a
  static OTD_SECP_FN bool sqrt(fe a, fe& r) {
    r = pow_chain(a, true);
    return F::is_zero(F::sub(F::sqr(r), a));
  }

  static OTD_SECP_FN fe curve_rhs(fe x) { return F::add(F::mul(F::sqr(x), x), F::small(7)); }

  static OTD_SECP_FN bool is_x(fe x) {
    fe r;
    return sqrt(curve_rhs(x), r);
  }

  // the even y of x, false when x is not on the curve
  static OTD_SECP_FN bool lift_even(fe x, fe& y) {
    fe r;
    const bool on = sqrt(curve_rhs(x), r);
    y = F::select(F::odd(r), F::sub(F::small(0), r), r);
    return on;
  }

  // stratum/ellswift.py xswiftec
  static OTD_SECP_FN fe xswiftec(fe u, fe t) {
    const uint32_t cw[8] = OTD_SECP_C, hw[8] = OTD_SECP_HALF;
    const fe half = constant(hw);
    if (F::is_zero(u)) u = F::small(1);
    if (F::is_zero(t)) t = F::small(1);
    const fe g = curve_rhs(u);  // u^3 + 7
    if (F::is_zero(F::add(g, F::sqr(t)))) t = F::add(t, t);
    const fe X = F::mul(F::sub(g, F::sqr(t)), inv(F::add(t, t)));
    const fe Y = F::mul(F::add(X, t), inv(F::mul(constant(cw), u)));
    const fe y2 = F::sqr(Y);
    const fe y4 = F::add(y2, y2);
    const fe x1 = F::add(u, F::add(y4, y4));
    if (is_x(x1)) return x1;
    const fe xy = F::mul(X, inv(Y));
    const fe x2 = F::mul(F::sub(F::sub(F::small(0), xy), u), half);
    if (is_x(x2)) return x2;
    return F::mul(F::sub(xy, u), half);
  }

  static OTD_SECP_FN Jac jselect(bool c, const Jac& a, const Jac& b) {
    Jac r;
    r.x = F::select(c, a.x, b.x);
    r.y = F::select(c, a.y, b.y);
    r.z = F::select(c, a.z, b.z);
    return r;
  }

  // 2·p, a = 0 (4 squarings, 3 products); z = 0 stays z = 0
  static OTD_SECP_FN Jac jdouble(const Jac& p) {
    const fe ysq = F::sqr(p.y);
    fe s = F::mul(p.x, ysq);
    s = F::add(s, s);
    s = F::add(s, s);
    const fe xx = F::sqr(p.x);
    const fe m = F::add(F::add(xx, xx), xx);
    Jac r;
    r.x = F::sub(F::sub(F::sqr(m), s), s);
    fe y4 = F::sqr(ysq);
    y4 = F::add(y4, y4);
    y4 = F::add(y4, y4);
    y4 = F::add(y4, y4);
    r.y = F::sub(F::mul(m, F::sub(s, r.x)), y4);
    const fe yz = F::mul(p.y, p.z);
    r.z = F::add(yz, yz);
    return r;
  }

  // p + (x2, y2, 1) for p != ±(x2, y2) and p not at infinity (3 squarings, 8 products); for those three inputs the
  // result is a meaningless point the caller does not select
  static OTD_SECP_FN Jac jadd_affine(const Jac& p, fe x2, fe y2) {
    const fe z1z1 = F::sqr(p.z);
    const fe u2 = F::mul(x2, z1z1);
    const fe s2 = F::mul(F::mul(y2, p.z), z1z1);
    const fe h = F::sub(u2, p.x);
    const fe r = F::sub(s2, p.y);
    const fe hh = F::sqr(h);
    const fe hhh = F::mul(h, hh);
    const fe v = F::mul(p.x, hh);
    Jac o;
    o.x = F::sub(F::sub(F::sub(F::sqr(r), hhh), v), v);
    o.y = F::sub(F::mul(r, F::sub(v, o.x)), F::mul(p.y, hhh));
    o.z = F::mul(p.z, h);
    return o;
  }

  // k·(px, py) for 0 < k < n: affine x and y. For such a k the accumulator never equals ±(px, py) where an addition
  // is selected (that needs 2m = ±1 mod n for a proper prefix m of k, so k = n or n + 2), so jadd_affine's three
  // excluded inputs only occur in additions that are dropped: before the first set bit, and with k = n - 1 at its
  // last, clear bit.
  static OTD_SECP_FN void mul(const uint32_t k[8], fe px, fe py, fe& rx, fe& ry) {
    uint32_t kk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) kk[i] = k[i];
    Jac base, acc;
    base.x = px;
    base.y = py;
    base.z = F::small(1);
    acc.x = F::small(0);
    acc.y = F::small(1);
    acc.z = F::small(0);
    bool inf = true;
    OTD_SECP_ROLLED
    for (int i = 0; i < 256; ++i) {
      const bool bit = (kk[7] >> 31) != 0;
#pragma unroll
      for (int j = 7; j > 0; --j) kk[j] = (kk[j] << 1) | (kk[j - 1] >> 31);
      kk[0] <<= 1;
      const Jac d = jdouble(acc);
      const Jac s = jselect(inf, base, jadd_affine(d, px, py));
      acc = jselect(bit, s, d);
      inf = inf & !bit;
    }
    const fe zi = inv(acc.z);
    const fe zi2 = F::sqr(zi);
    rx = F::mul(acc.x, zi2);
    ry = F::mul(acc.y, F::mul(zi2, zi));
  }

  // One row. k, pa, pb: the scalar and the two halves of point as little-endian 32-bit words of their big-endian
  // values. x: the result the same way, zero unless the status returned is kSecpOk.
  static OTD_SECP_FN uint32_t row(const uint32_t k[8], const uint32_t pa[8], const uint32_t pb[8], uint32_t kind,
                                  uint32_t x[8], uint32_t& parity) {
    const uint32_t nw[8] = OTD_SECP_N, pw[8] = OTD_SECP_P, gx[8] = OTD_SECP_GX, gy[8] = OTD_SECP_GY;
    uint32_t status = kSecpOk;
    fe px = constant(gx), py = constant(gy);
    if (kind > kSecpKindEllSwift) {
      status = kSecpBadKind;
    } else if (words_zero(k) || words_ge(k, nw)) {
      status = kSecpBadScalar;
    } else if (kind == kSecpKindXOnly) {
      fe y;
      const fe xx = F::from_words(pa);
      if (words_ge(pa, pw) || !lift_even(xx, y)) {
        status = kSecpBadPoint;
      } else {
        px = xx;
        py = y;
      }
    } else if (kind == kSecpKindEllSwift) {
      px = xswiftec(F::from_words(pa), F::from_words(pb));
      lift_even(px, py);  // every encoding decodes to a point
    }
    // a refused row runs the same ladder, over 1·G, and drops the result
    uint32_t kk[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) kk[i] = status == kSecpOk ? k[i] : (i == 0 ? 1u : 0u);
    if (status != kSecpOk) {
      px = constant(gx);
      py = constant(gy);
    }
    fe rx, ry;
    mul(kk, px, py, rx, ry);
    uint32_t xw[8];
    F::to_words(rx, xw);
    const uint32_t keep = status == kSecpOk ? 0xFFFFFFFFu : 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = xw[i] & keep;
    parity = (F::odd(ry) ? 1u : 0u) & keep;
    return status;
  }
};

}  // namespace secp
}  // namespace otedama
