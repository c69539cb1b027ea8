// GLV scalar splits on G1 (phi(x, y) = (BETA x, y) = LAMBDA P in the prime-order
// subgroup): k = k1 + k2 LAMBDA with 128-bit halves, for the EC-FFT's twiddle
// table (ecfft.hip) and the batch scalar multiplication (batch_mul.hip).
#pragma once
#include "curve.hpp"

namespace ecg {

template <class C>
constexpr bool has_glv() {
  return C::EXT == 1 && C::Gen::GLV != 0;
}

// GLV split of a canonical scalar k < r (BLS12-381 G1): k = k2 * LAMBDA + k1,
// 0 <= k1 < LAMBDA < 2^128, k2 < r / LAMBDA < 2^128 (bit-serial division by
// the fixed 128-bit LAMBDA; runs once per twiddle when the table is built).
template <class C>
ECG_DEV void glv_split(const uint32_t* k, uint32_t* k1, uint32_t* k2) {
  uint32_t lam[5];
#pragma unroll
  for (int i = 0; i < 4; i++) lam[i] = (i & 1) ? (uint32_t)(C::Gen::LAMBDA[i >> 1] >> 32) : (uint32_t)C::Gen::LAMBDA[i >> 1];
  lam[4] = 0;
  uint32_t rem[5] = {0, 0, 0, 0, 0};
  uint32_t q[4] = {0, 0, 0, 0};
  for (int b = 255; b >= 0; b--) {
#pragma unroll
    for (int i = 4; i > 0; i--) rem[i] = (rem[i] << 1) | (rem[i - 1] >> 31);
    rem[0] = (rem[0] << 1) | ((k[b >> 5] >> (b & 31)) & 1);
    bool ge = true;  // rem >= lam ?
#pragma unroll
    for (int i = 4; i >= 0; i--) {
      if (rem[i] != lam[i]) {
        ge = rem[i] > lam[i];
        break;
      }
    }
    if (ge) {
      uint32_t br = 0;
#pragma unroll
      for (int i = 0; i < 5; i++) {
        const uint64_t d = (uint64_t)rem[i] - lam[i] - br;
        rem[i] = (uint32_t)d;
        br = (uint32_t)(d >> 63);
      }
      if (b < 128) q[b >> 5] |= 1u << (b & 31);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    k1[i] = rem[i];
    k2[i] = q[i];
  }
}

// 32-bit words of a u64 constant array
template <int N>
ECG_DEV void words_of(const uint64_t (&v)[N], uint32_t* w) {
#pragma unroll
  for (int i = 0; i < N; i++) {
    w[2 * i] = (uint32_t)v[i];
    w[2 * i + 1] = (uint32_t)(v[i] >> 32);
  }
}

// c = floor((k g + 2^319) / 2^320) for k < 2^256 (8 words) and g < 2^256 (8
// words): the rounded k * (b / r) of the lattice split, c < 2^128
ECG_DEV void glv_round(const uint32_t* k, const uint32_t* g, uint32_t* c) {
  uint32_t pr[16];
#pragma unroll
  for (int i = 0; i < 16; i++) pr[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t t = (uint64_t)k[i] * g[j] + pr[i + j] + carry;
      pr[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
    pr[i + 8] = (uint32_t)carry;
  }
  uint64_t t = (uint64_t)pr[9] + 0x80000000u;  // + 2^319
  pr[9] = (uint32_t)t;
#pragma unroll
  for (int i = 10; i < 14; i++) {
    t = (uint64_t)pr[i] + (t >> 32);
    c[i - 10] = (uint32_t)t;
  }
}

// low 128 bits of x * y (4 words each)
ECG_DEV void mul_lo128(const uint32_t* x, const uint32_t* y, uint32_t* z) {
  uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; i + j < 4; j++) {
      const uint64_t t = (uint64_t)x[i] * y[j] + r[i + j] + carry;
      r[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) z[i] = r[i];
}

ECG_DEV void sub128(uint32_t* x, const uint32_t* y) {  // x -= y mod 2^128
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint64_t d = (uint64_t)x[i] - y[i] - br;
    x[i] = (uint32_t)d;
    br = (d >> 63) & 1;
  }
}

// |v| with the sign in bit 127 (|v| < 2^126: GLV_LATTICE bound)
ECG_DEV void sign_magnitude128(uint32_t* v) {
  if (!(v[3] >> 31)) return;
  const uint32_t z[4] = {0, 0, 0, 0};
  uint32_t m[4] = {z[0], z[1], z[2], z[3]};
  sub128(m, v);
#pragma unroll
  for (int i = 0; i < 4; i++) v[i] = m[i];
  v[3] |= 0x80000000u;
}

// GLV lattice split of k < r (BN254 G1, GLV = 2; constants and bounds in
// tools/gen_params.py): k = k1 + k2 LAMBDA mod r, each half as a 127-bit
// magnitude with its sign in bit 127.  Once per twiddle, when the table is
// built.
template <class C>
ECG_DEV void glv_lattice_split(const uint32_t* k, uint32_t* k1, uint32_t* k2) {
  using G = typename C::Gen;
  uint32_t g1[8], g2[8], a1[4], a2[4], nb1[4], b2[4], c1[4], c2[4], t[4];
  words_of(G::G1, g1);
  words_of(G::G2, g2);
  words_of(G::A1, a1);
  words_of(G::A2, a2);
  words_of(G::NB1, nb1);
  words_of(G::B2, b2);
  glv_round(k, g1, c1);
  glv_round(k, g2, c2);
#pragma unroll
  for (int i = 0; i < 4; i++) k1[i] = k[i];
  mul_lo128(c1, a1, t);
  sub128(k1, t);
  mul_lo128(c2, a2, t);
  sub128(k1, t);
  mul_lo128(c1, nb1, k2);
  mul_lo128(c2, b2, t);
  sub128(k2, t);
  sign_magnitude128(k1);
  sign_magnitude128(k2);
}

// the sign bit of a lattice half (GLV = 2), cleared from k; false otherwise
template <class C>
ECG_DEV bool glv_take_sign(uint32_t* k) {
  if constexpr (C::Gen::GLV == 2) {
    const bool neg = k[3] >> 31;
    k[3] &= 0x7fffffffu;
    return neg;
  } else {
    return false;
  }
}

}  // namespace ecg
