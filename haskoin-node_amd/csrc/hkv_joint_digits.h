// hkv_joint_digits.h — joint radix-8 digits of k1 + k2 lambda over Z[lambda]
// (lambda^2 + lambda + 1 = 0), for the chain launch of the table-and-chain
// shape (hkv_kernels.hip 2a). Pure C++ (no HIP include): the kernels and
// tests/joint_digits.cpp compile this same text, the latter on the CPU under
// ASan and UBSan against rows of the Python model (tests/joint_digits.py).
//
// The chain computes (k1 + k2 lambda) Q'. Z[lambda] has six units,
// (-1)^s lambda^e, and a unit acts on a point for free:
// (x, y) -> (beta^e x, (-1)^s y). The pair (k1, k2) is recoded jointly in
// base 8: the digit of a class of Z[lambda] / 8 is its representative of
// least norm a^2 - a b + b^2 (components at most 5 in absolute value). The 63
// non-zero digits fall into 11 orbits under the units, 10 of six and
// {4, 4 lambda, 4 lambda^2}, so one window is three doublings and one
// addition from an 11-entry table: 129 doublings and 44 additions where the
// Booth chain runs 124 and 66. Ties on the boundary of the hexagon break per
// orbit: each orbit's digits are its representative's unit multiples, so the
// digit set is closed under the units (4 = -4 mod 8: that orbit keeps the
// three unnegated digits).
//
// Table entries, as a + b lambda, in build order (each is its predecessor
// plus a unit, so the table build stays a walk of mixed additions of unit
// images of Q'):
//   (1,0) (2,0) (3,0) (4,0) (4,1) (3,1) (2,1) (3,2) (4,2) (4,3) (5,3)
// 44 digits cover |k1|, |k2| < 2^129: each step leaves |k'| <= (|k| + 5) / 8,
// so after 43 steps both components lie in {-1, 0, 1}, and every such pair is
// itself a digit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HKV_JD_FN __host__ __device__ inline
#define HKV_JD_UNROLL _Pragma("unroll")
#else
#define HKV_JD_FN inline
#define HKV_JD_UNROLL
#endif

namespace hkv {

constexpr int JD_WINDOWS = 44;  // digits per scalar pair
constexpr int JD_WORDS = 11;    // 7-bit codes, four to a word: window w at bit 7 (w % 4) of word w / 4
constexpr int JD_ENTRIES = 11;  // table entries (orbits)
// a digit's code: bits 0..3 the table entry (JD_ZERO: the zero digit), bits
// 4..5 e, bit 6 s: the digit is (-1)^s lambda^e times the entry
constexpr uint32_t JD_ZERO = 15u, JD_ENTRY_MASK = 15u, JD_CODE_MASK = 127u;
constexpr int JD_E_SHIFT = 4, JD_S_SHIFT = 6;

// entry j + 1 = entry j + (-1)^s lambda^e Q', j = 0..9: e at bits 2j, 2j + 1
// of JD_STEP_E, s at bit j of JD_STEP_S
constexpr uint32_t JD_STEP_E = (1u << 6) | (2u << 12) | (1u << 16);
constexpr uint32_t JD_STEP_S = (1u << 4) | (1u << 5) | (1u << 6);

// the class (k1 mod 8) * 8 + (k2 mod 8): code | (d1 + 8) << 7 | (d2 + 8) << 11
HKV_JD_FN uint32_t jd_class(uint32_t c) {
  static constexpr uint16_t T[64] = {
      0x440f, 0x4c10, 0x5411, 0x5c12, 0x6413, 0x2c52, 0x3451, 0x3c50, 0x4480, 0x4ce0, 0x54e6, 0x5ce7, 0x64e9,
      0x2cd4, 0x34d5, 0x3cd6, 0x4501, 0x4d06, 0x5561, 0x5d65, 0x6568, 0x6d6a, 0x3558, 0x3d57, 0x4582, 0x4d85,
      0x5587, 0x5de2, 0x65e4, 0x29ca, 0x35da, 0x3dd9, 0x4603, 0x4e04, 0x5608, 0x5e09, 0x2223, 0x2a49, 0x3248,
      0x3a44, 0x42c2, 0x4a99, 0x529a, 0x5e8a, 0x22a4, 0x2aa2, 0x32c7, 0x3ac5, 0x4341, 0x4b17, 0x5318, 0x1b2a,
      0x2328, 0x2b25, 0x3321, 0x3b46, 0x43c0, 0x4b96, 0x5395, 0x5b94, 0x23a9, 0x2ba7, 0x33a6, 0x3ba0};
  return T[c & 63u];
}

// bits [pos, pos + 3) of a 160-bit value (pos <= 129)
HKV_JD_FN uint32_t jd_bits3(const uint32_t k[5], int pos) {
  const int w = pos >> 5, s = pos & 31;
  uint32_t v = k[w] >> s;
  if (s > 29 && w < 4) v |= k[w + 1] << (32 - s);
  return v & 7u;
}

// The 44 digits of k1 + k2 lambda, packed into out[0..11). k1, k2: signed, in
// two's complement over five words, |k| < 2^129. Window w sees bits 3w..3w+2
// of each half plus a carry c in {0, 1}: with t = bits + c and d the digit of
// the class of (t1, t2), (k - d) / 8 is the higher bits plus (t - d) / 8.
HKV_JD_FN void joint_recode(const uint32_t k1[5], const uint32_t k2[5], uint32_t out[JD_WORDS]) {
  int c1 = 0, c2 = 0;
  HKV_JD_UNROLL
  for (int q = 0; q < JD_WORDS; ++q) {
    uint32_t word = 0;
    HKV_JD_UNROLL
    for (int j = 0; j < 4; ++j) {
      const int pos = 3 * (4 * q + j);
      const int t1 = (int)jd_bits3(k1, pos) + c1, t2 = (int)jd_bits3(k2, pos) + c2;
      const uint32_t row = jd_class((((uint32_t)t1 & 7u) << 3) | ((uint32_t)t2 & 7u));
      const int d1 = (int)((row >> 7) & 15u) - 8, d2 = (int)((row >> 11) & 15u) - 8;
      c1 = (t1 - d1) / 8;  // exact: 0 or 8 over 8
      c2 = (t2 - d2) / 8;
      word |= (row & JD_CODE_MASK) << (7 * j);
    }
    out[q] = word;
  }
}

// two's complement of a five-word magnitude under neg
HKV_JD_FN void jd_signed(uint32_t k[5], bool neg) {
  const uint32_t m = neg ? 0xFFFFFFFFu : 0u;
  uint32_t c = neg ? 1u : 0u;
  HKV_JD_UNROLL
  for (int q = 0; q < 5; ++q) {
    const uint32_t v = (k[q] ^ m) + c;
    c = (c != 0u && v == 0u) ? 1u : 0u;
    k[q] = v;
  }
}

}  // namespace hkv
