// hkv_kernels.hip — batch secp256k1 ECDSA verify kernels for gfx950.
//
// Pipeline per batch (no MFMA: 256-bit integer work). Every launch shape is
// y-free: the key's y is never on the critical path (section 2b).
//   1. hkv_prologue_kernel + hkv_inv_kernel + hkv_glv_kernel (full-grid
//      batches) — record parse (compact sig + SEC1 pubkey incl. hybrid keys,
//      w = x^3 + 7 instead of the sqrt), high-S policy, m = msg mod n, s^-1
//      (batched), u1 = m/s, u2 = r/s, GLV split of u2, Booth digits. Writes a
//      SoA intermediate.
//   2. hkv_ecmult_kernel<true, STDPRO> (mid-size batches) — per-lane table
//      of 1..2^(QW-1) * Q' (8 entries at the default radix 16) on an isomorphic curve of E_w (one
//      common Z, so all Q additions are mixed), then a shared doubling chain
//      of 132 bits with radix-16 Booth digits for k1*Q' and k2*(lambda Q')
//      (only the paired-form instance, ILP = true, remains; above the
//      mid-size range the same two phases run as two launches, 2a:
//      hkv_qtable_kernel then hkv_chain_kernel, over per-signature tables,
//      with the plain forms, and on joint radix-8 digits over Z[lambda]:
//      an 11-entry table, 44 windows of 3 doublings and one addition,
//      hkv_joint_digits.h); it leaves
//      B' = u2*Q' to
//   2b. hkv_finish_kernel, hkv_rare_kernel, hkv_yverdict_kernel — u1*G from
//      per-window tables, y0 = num/den from "x(u1 G + u2 Q) == r", and the
//      verdict "y_c^2 == w with the key's parity" (rare lanes: exact sqrt path).
//   2c. hkv_pair_split_kernel<STD> — small batches (a block) in one launch:
//      per workgroup 32 signatures on 4 waves (k1 chains, k2 chains, two lanes
//      per signature; the signature wave: parse, u1*G; the key's sqrt), the
//      halves joined exactly (R = A + B, Jacobian x compare); STD = standard
//      inputs (verifyStdInput's parse and hashes inside the same launch).
//   3. hkv_gtable_kernel    — once per context: the fixed-base tables.
//   4. hkv_gen_*            — synthetic valid batches (keyless construction,
//      SURVEY.md §8(c)) for the benchmark and the tests.
//
// Reference semantics restated: libsecp256k1 secp256k1_ec_pubkey_parse,
// secp256k1_ecdsa_signature_parse_compact, secp256k1_ecdsa_signature_normalize,
// secp256k1_ecdsa_verify, and haskoin-core verifyHashSig (normalize first)
// [dep; pinned /root/reference/stack.yaml:8-10; SURVEY.md §8(a) a1, a3-a6].
#include "hkv_group.h"
#include "hkv_hash.h"
#include "hkv_layout.h"
#include "hkv_joint_digits.h"
#include "hkv_internal.h"
#include "hkv_sighash_dev.h"
#include "hkv_tail_plan.h"

namespace hkv {

// ---------------------------------------------------------------------------
// record access
// ---------------------------------------------------------------------------
// little-endian 32-bit word at byte offset `off` of the record (off compile-time)
HKV_DEV uint32_t rec_word_at(const uint32_t* w, int off) {
  const int k = off >> 2, s = off & 3;
  if (s == 0) return w[k];
  return __builtin_amdgcn_alignbyte(w[k + 1], w[k], s);
}
// 32 big-endian bytes at byte offset `off` -> 8 limbs (limb 0 least significant)
HKV_DEV void rec_be256(uint32_t out[8], const uint32_t* w, int off) {
#pragma unroll
  for (int j = 0; j < 8; ++j) out[7 - j] = __builtin_bswap32(rec_word_at(w, off + 4 * j));
}

// p - n: r + n < p  <=>  r < p - n
__constant__ static const uint32_t PMN[8] = {0x2FC9BAEEu, 0x402DA172u, 0x50B75FC4u, 0x45512319u, 1u, 0, 0, 0};

// ---------------------------------------------------------------------------
// the intermediates (hkv_layout.h): a view of im or aux, the one place that
// forms [word row * n_pad + signature]. The signature index is the lane's
// 32-bit one, widened here at the use. One-word access keeps the caller's
// index type I for the two sites that form theirs in 64 bits: the inverse
// kernel's i - stride and the rare list's base + rank.
// The hand-offs that move several fields of one lane together (B', A, the
// join inputs) stay loops over get / put at their sites: written as shared
// functions over these methods they compiled to other code in the chain,
// mid-size, finish, pair, block and tail kernels (profiles/r12_im_layout/).
// Where the view is held matters to the compiler too. A named view in the
// body of hkv_ecmult_kernel or hkv_chain_kernel, or as finish_lane's
// parameter, changed those kernels' loops, and so did any form of the
// verdict kernel but the one below: the two kernels index im themselves at
// their five sites, finish_lane builds its view at each use from its own
// im, n_pad, and the verdict kernel calls ld8 / st8 on its im. All other
// code holds a view and passes it on.
// ---------------------------------------------------------------------------
template <class W>  // uint32_t, or const uint32_t for a read-only view
struct SoA {
  W* p;
  uint32_t n_pad;
  // (the row is never negative; saying so keeps the product's sign known)
  template <class I>
  HKV_DEV size_t at(Field f, int k, I i) const { return (size_t)(uint32_t)(f.off + k) * n_pad + i; }
  // word k of field f
  template <class I>
  HKV_DEV uint32_t get(Field f, int k, I i) const { return p[at(f, k, i)]; }
  template <class I>
  HKV_DEV void put(Field f, int k, I i, uint32_t v) const { p[at(f, k, i)] = v; }
  template <class I>
  HKV_DEV uint32_t get(Field f, I i) const { return get(f, 0, i); }
  template <class I>
  HKV_DEV void put(Field f, I i, uint32_t v) const { put(f, 0, i, v); }
  // an eight-limb value
  // (the eight-limb move on a bare pointer: get8 / put8, and the verdict kernel directly)
  static HKV_DEV void ld8(const uint32_t* __restrict__ q, uint32_t n_pad, int w, uint32_t i, uint32_t* v) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = q[(size_t)(w + k) * n_pad + i];
  }
  static HKV_DEV void st8(uint32_t* __restrict__ q, uint32_t n_pad, int w, uint32_t i, const uint32_t* v) {
#pragma unroll
    for (int k = 0; k < 8; ++k) q[(size_t)(w + k) * n_pad + i] = v[k];
  }
  HKV_DEV void get8(Field f, uint32_t i, uint32_t* v) const { ld8(p, n_pad, f.off, i, v); }
  HKV_DEV void put8(Field f, uint32_t i, const uint32_t* v) const { st8(p, n_pad, f.off, i, v); }
  HKV_DEV void get8(Field f, uint32_t i, fe& a) const { get8(f, i, a.v); }
  HKV_DEV void get8(Field f, uint32_t i, sc& a) const { get8(f, i, a.v); }
  HKV_DEV void put8(Field f, uint32_t i, const fe& a) const { put8(f, i, a.v); }
  HKV_DEV void put8(Field f, uint32_t i, const sc& a) const { put8(f, i, a.v); }
  HKV_DEV operator SoA<const uint32_t>() const { return {p, n_pad}; }
};
using SoAView = SoA<uint32_t>;
using SoACView = SoA<const uint32_t>;

// ---------------------------------------------------------------------------
// 1. prologue
// ---------------------------------------------------------------------------
#ifndef HKV_PROLOGUE_WAVES
#define HKV_PROLOGUE_WAVES 4  // min waves per SIMD the prologue's register allocation targets
#endif

// secp256k1_ec_pubkey_parse of the record's key (words 24..40: pklen,
// SEC1 bytes): 02/03 + x (x < p, x^3 + 7 a square, y of the prefix's
// parity), 04/06/07 + x, y (x, y < p, on the curve, 06/07 parity). Returns
// the affine point in x, y (normalised). Call from wave-uniform control flow
// (the sqrt is a wave-uniform branch).
HKV_DEV bool pubkey_parse_rec(const uint32_t* w, fe& x, fe& y) {
  const uint32_t pklen = w[24] & 0xFFu;
  const uint32_t prefix = (w[24] >> 8) & 0xFFu;
  const bool comp = (pklen == 33u) && (prefix == 2u || prefix == 3u);
  const bool unc = (pklen == 65u) && (prefix == 4u || prefix == 6u || prefix == 7u);
  fe rhs, t;
  rec_be256(x.v, w, 98);
  rec_be256(y.v, w, 130);
  bool pk_ok = (comp || unc) && u256_lt_p(x.v);
  if (unc) pk_ok = pk_ok && u256_lt_p(y.v);
  fe_sqr(t, x);
  fe_mul(t, t, x);
  fe seven;
  fe_set_u32(seven, 7);
  fe_add(rhs, t, seven);
  if (__any(comp)) {
    fe yc, y2;
    fe_sqrt_cand(yc, rhs);
    fe_sqr(y2, yc);
    const bool is_sq = fe_equal(y2, rhs);
    fe_normalize(yc);
    fe ny;
    fe_neg(ny, yc);
    fe_normalize(ny);
    const bool flip = (yc.v[0] & 1u) != (prefix & 1u);
    if (comp) {
      pk_ok = pk_ok && is_sq;
      y = flip ? ny : yc;
    }
  }
  if (unc) {
    fe y2;
    fe_sqr(y2, y);
    pk_ok = pk_ok && fe_equal(y2, rhs);
    if (prefix != 4u) pk_ok = pk_ok && ((y.v[0] & 1u) == (prefix & 1u));  // hybrid parity
  }
  return pk_ok;
}
// The y-free form of the parse: the same accept rules except the
// one that needs the square root — x^3 + 7 of a compressed key is not shown
// to be a square here; the finish kernels' y_c^2 == w test rejects a
// non-square (no y_c exists), and their rare paths test it explicitly.
// Outputs x, w = x^3 + 7 (normalised) and FLAG_YODD / FLAG_COMP.
// (The head repeats pubkey_parse_rec's on purpose: shared through a helper it
// compiled to other code — hkv_prologue_kernel 80 -> 82 VGPRs, 6 -> 5 waves.)
HKV_DEV bool pubkey_parse_rec_w(const uint32_t* w, fe& x, fe& rhs, uint32_t& pflags) {
  const uint32_t pklen = w[24] & 0xFFu;
  const uint32_t prefix = (w[24] >> 8) & 0xFFu;
  const bool comp = (pklen == 33u) && (prefix == 2u || prefix == 3u);
  const bool unc = (pklen == 65u) && (prefix == 4u || prefix == 6u || prefix == 7u);
  fe y, t;
  rec_be256(x.v, w, 98);
  rec_be256(y.v, w, 130);
  bool pk_ok = (comp || unc) && u256_lt_p(x.v);
  if (unc) pk_ok = pk_ok && u256_lt_p(y.v);
  fe_sqr(t, x);
  fe_mul(t, t, x);
  fe seven;
  fe_set_u32(seven, 7);
  fe_add(rhs, t, seven);
  fe_normalize(rhs);
  if (unc) {
    fe y2;
    fe_sqr(y2, y);
    pk_ok = pk_ok && fe_equal(y2, rhs);
    if (prefix != 4u) pk_ok = pk_ok && ((y.v[0] & 1u) == (prefix & 1u));  // hybrid parity
  }
  const bool yodd = comp ? (prefix & 1u) != 0 : (y.v[0] & 1u) != 0;
  pflags = (yodd ? FLAG_YODD : 0u) | (comp ? FLAG_COMP : 0u);
  return pk_ok;
}

__global__ void __launch_bounds__(WG, HKV_PROLOGUE_WAVES) hkv_prologue_kernel(const uint32_t* __restrict__ recs, uint32_t n,
                                                          uint32_t n_pad, uint32_t mode,
                                                          uint32_t* __restrict__ im) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n_pad) return;
  uint32_t w[REC_WORDS];
  if (i < n) {
    const uint2* src = reinterpret_cast<const uint2*>(recs + (size_t)i * REC_WORDS);
#pragma unroll
    for (int k = 0; k < REC_WORDS / 2; ++k) {
      uint2 v = src[k];
      w[2 * k] = v.x;
      w[2 * k + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < REC_WORDS; ++k) w[k] = 0;
  }

  // --- signature: compact parse (overflow -> fail), normalize / high-S policy
  sc r, s, m;
  rec_be256(r.v, w, 32);
  rec_be256(s.v, w, 64);
  rec_be256(m.v, w, 0);
  bool ok = (i < n) && u256_lt(r.v, SC_N) && u256_lt(s.v, SC_N);
  const bool high = sc_is_high(s);
  if (mode == HKV_MODE_HASKOIN) {
    sc ns;
    sc_neg(ns, s);
    if (high) s = ns;  // secp256k1_ecdsa_signature_normalize
  } else {
    ok = ok && !high;  // secp256k1_ecdsa_verify rejects high-S
  }
  ok = ok && !u256_is_zero(r.v) && !u256_is_zero(s.v);
  sc_cond_sub_n(m.v);  // m = msg32 mod n (msg32 < 2^256 < 2n)

  // --- pubkey: secp256k1_ec_pubkey_parse (y-free: y stays implicit, w = x^3 + 7 goes to IM_W)
  fe x, wv;
  uint32_t pflags = 0;
  ok = pubkey_parse_rec_w(w, x, wv, pflags) && ok;

  const uint32_t flags = (ok ? FLAG_VALID : 0u) | pflags;
  const SoAView iv = {im, n_pad};
  iv.put(IM_FLAGS, i, flags);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    iv.put(IM_QX, k, i, x.v[k]);
    iv.put(IM_W, k, i, wv.v[k]);
    iv.put(IM_R, k, i, r.v[k]);
    iv.put(IM_S, k, i, s.v[k]);
    iv.put(IM_M, k, i, m.v[k]);
  }
}

// Key-only check (the keys of a CHECKMULTISIG script: haskoin-core decodes
// every key with importPubKey, so one key off the curve fails the input
// whatever its signatures do): bit i = record i's key parses. Bits leave as
// one 64-bit ballot word per wave (i's wave covers 64 consecutive records).
// recs holds records [rbase, ...): record i is read at recs[i - rbase] (the
// multisig tail's key-check window; rbase a multiple of 64).
HKV_DEV void key_check_lane(const uint32_t* __restrict__ recs, uint32_t i, uint32_t n, uint32_t* __restrict__ bits,
                            uint32_t rbase = 0) {
  uint32_t w[REC_WORDS];
#pragma unroll
  for (int k = 0; k < REC_WORDS; ++k) w[k] = 0;
  if (i < n) {
#pragma unroll
    for (int k = 24; k < 42; ++k) w[k] = recs[(size_t)(i - rbase) * REC_WORDS + k];
  }
  fe x, y;
  const bool ok = pubkey_parse_rec(w, x, y) && i < n;
  const uint64_t ball = __ballot(ok);
  const uint32_t wbase = i & ~63u;
  if ((threadIdx.x & 63) == 0 && wbase < n) {  // (a wave wholly past n writes nothing)
    bits[wbase / 32] = (uint32_t)ball;
    bits[wbase / 32 + 1] = (uint32_t)(ball >> 32);
  }
}

// ---------------------------------------------------------------------------
// 1b. scalar kernel: s^-1 by Montgomery's batch trick over BATCH_INV
//     signatures per thread (strided for coalescing), then u1 = m/s,
//     u2 = r/s and the GLV split of u2.
// ---------------------------------------------------------------------------
template <int L>
HKV_DEV void shr_bits(uint32_t* a, int b) {
#pragma unroll
  for (int q = 0; q < L - 1; ++q) a[q] = (a[q] >> b) | (a[q + 1] << (32 - b));
  a[L - 1] >>= b;
}
// Radix-2^QW / radix-2^20 Booth recoding (LSB first, MSB-first consumption in
// the ecmult kernel): d = ((v + 1) >> 1) - ((v >> W) << W), v = bits
// [pos-1, pos+W-1]; sum_w d_w 2^(QW w) reproduces the scalar (< 2^129).
HKV_DEV void write_qdigits(SoAView iv, uint32_t i, uint32_t* S1, uint32_t* S2) {
  constexpr uint32_t QM = (1u << QW) - 1u;
  uint32_t p1 = 0, p2 = 0;
#pragma unroll 1
  for (int w = 0; w < NWIN; ++w) {
    const uint32_t v1 = p1 | ((S1[0] & QM) << 1), v2 = p2 | ((S2[0] & QM) << 1);
    p1 = (S1[0] >> (QW - 1)) & 1u;
    p2 = (S2[0] >> (QW - 1)) & 1u;
    shr_bits<5>(S1, QW);
    shr_bits<5>(S2, QW);
    const int d1 = (int)((v1 + 1u) >> 1) - (int)((v1 >> QW) << QW);
    const int d2 = (int)((v2 + 1u) >> 1) - (int)((v2 >> QW) << QW);
    iv.put(IM_DIG, w, i, (uint32_t)(d1 + QBIAS) | ((uint32_t)(d2 + QBIAS) << QDIG_BITS));
  }
}
HKV_DEV void write_gdigits(SoAView iv, uint32_t i, uint32_t* SL, uint32_t* SH) {
  uint32_t pl = 0, ph = 0;
#pragma unroll 1
  for (int j = 0; j < GWIN; ++j) {
    constexpr uint32_t M = (1u << GTAB_W) - 1u;
    const uint32_t vl = pl | ((SL[0] & M) << 1), vh = ph | ((SH[0] & M) << 1);
    pl = (SL[0] >> (GTAB_W - 1)) & 1u;
    ph = (SH[0] >> (GTAB_W - 1)) & 1u;
    shr_bits<4>(SL, GTAB_W);
    shr_bits<4>(SH, GTAB_W);
    const int dl = (int)((vl + 1u) >> 1) - (int)((vl >> GTAB_W) << GTAB_W);
    const int dh = (int)((vh + 1u) >> 1) - (int)((vh >> GTAB_W) << GTAB_W);
    iv.put(IM_GDIG, 2 * j, i, (uint32_t)(dl < 0 ? -dl : dl) | (dl < 0 ? GD_NEG : 0u));
    iv.put(IM_GDIG, 2 * j + 1, i, (uint32_t)(dh < 0 ? -dh : dh) | (dh < 0 ? GD_NEG : 0u));
  }
}

// (at one wave per SIMD the loop is load-latency bound: each iteration's
// operands are loaded one iteration ahead)
__global__ void __launch_bounds__(WG) hkv_inv_kernel(uint32_t n_pad, uint32_t stride, uint32_t* __restrict__ im) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= stride) return;
  const SoAView iv = {im, n_pad};
  // forward: prefix products c_k = s_0 * ... * s_k (invalid lanes use s = 1)
  sc c;
  sc_set_u32(c, 1);
  int kn = 0;  // number of signatures of this lane
  {
    sc sv;
    uint32_t fl = 0;
    iv.get8(IM_S, t, sv);  // t < stride <= n_pad
    fl = iv.get(IM_FLAGS, t);
#pragma unroll 1
    for (int k = 0; k < BATCH_INV; ++k) {
      const uint32_t i = t + (uint32_t)k * stride;
      if (i >= n_pad) break;
      kn = k + 1;
      const uint32_t inext = i + stride;
      sc sn;
      uint32_t fn = 0;
      if (k + 1 < BATCH_INV && inext < n_pad) {
        iv.get8(IM_S, inext, sn);
        fn = iv.get(IM_FLAGS, inext);
      }
      if (!(fl & FLAG_VALID)) sc_set_u32(sv, 1);
      sc_mul(c, c, sv);
      iv.put8(IM_C, i, c);
      sv = sn;
      fl = fn;
    }
  }
  sc inv;
  sc_inv(inv, c);
  // backward: s_k^-1 = inv * c_{k-1} (stored over c_k); inv *= s_k
  if (kn == 0) return;
  {
    int k = kn - 1;
    uint32_t i = t + (uint32_t)k * stride;
    sc prev, sv;
    uint32_t fl = iv.get(IM_FLAGS, i);
    iv.get8(IM_S, i, sv);
    if (k > 0) iv.get8(IM_C, i - stride, prev);
#pragma unroll 1
    for (; k >= 0; --k) {
      i = t + (uint32_t)k * stride;
      sc pn, sn;
      uint32_t fn = 0;
      if (k > 0) {  // the next (lower) signature's operands
        fn = iv.get(IM_FLAGS, (size_t)i - stride);  // (formed in 64 bits, as it always was)
        iv.get8(IM_S, i - stride, sn);
        if (k > 1) iv.get8(IM_C, i - 2 * stride, pn);
      }
      if (k == 0) sc_set_u32(prev, 1);
      sc sinv;
      sc_mul(sinv, inv, prev);
      iv.put8(IM_C, i, sinv);
      if (!(fl & FLAG_VALID)) sc_set_u32(sv, 1);
      sc_mul(inv, inv, sv);
      prev = pn;
      sv = sn;
      fl = fn;
    }
  }
}

// 1c. per signature: u1 = m/s, u2 = r/s, GLV split of u2, Booth digits.
HKV_DEV void glv_lane(SoAView iv, uint32_t i, uint32_t flags, const sc& sinv) {
  sc m, r, u1, u2;
  iv.get8(IM_M, i, m);
  iv.get8(IM_R, i, r);
  sc_mul(u1, m, sinv);
  sc_mul(u2, r, sinv);
  uint32_t k1[5], k2[5];
  bool n1, n2;
  const bool glv_ok = glv_split(u2, k1, n1, k2, n2);
  uint32_t f = flags | (n1 ? FLAG_NEG1 : 0u) | (n2 ? FLAG_NEG2 : 0u) | (glv_ok ? 0u : FLAG_GLV_OVF);
  if (!glv_ok) f &= ~FLAG_VALID;  // unreachable for a correct basis; fail closed
  iv.put(IM_FLAGS, i, f);
  const bool use = (f & FLAG_VALID) != 0;
  uint32_t S1[5], S2[5], SL[4], SH[4];
#pragma unroll
  for (int q = 0; q < 5; ++q) { S1[q] = use ? k1[q] : 0u; S2[q] = use ? k2[q] : 0u; }
#pragma unroll
  for (int q = 0; q < 4; ++q) { SL[q] = use ? u1.v[q] : 0u; SH[q] = use ? u1.v[4 + q] : 0u; }
  write_qdigits(iv, i, S1, S2);
  write_gdigits(iv, i, SL, SH);
}
__global__ void __launch_bounds__(WG) hkv_glv_kernel(uint32_t n_pad, uint32_t* __restrict__ im) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n_pad) return;
  const SoAView iv = {im, n_pad};
  const uint32_t flags = iv.get(IM_FLAGS, i);
  sc sinv;
  iv.get8(IM_C, i, sinv);
  glv_lane(iv, i, flags, sinv);
}

// 1c'. large standard-input batches (hkv_api.cpp enqueue_std_chunk): the
//      prologue ran before the hash half had written the messages, so the
//      finish kernel (LATE) first redoes the G digits of its lane from the
//      final record: m = msg mod n, u1 = m s^-1 (IM_C still holds s^-1: the
//      ecmult kernel writes B' over the Q digits only). A record the hash half
//      zeroed (a failed HASH160 / script check) makes the lane invalid.
//      Returns the lane's flags.
HKV_DEV uint32_t late_u1_lane(const uint32_t* __restrict__ recs, uint32_t i, SoAView iv, uint32_t f) {
  const uint32_t* w = recs + (size_t)i * REC_WORDS;
  if ((w[24] & 0xFFu) == 0u) f &= ~FLAG_VALID;
  const bool use = (f & FLAG_VALID) != 0;
  sc m, sinv, u1;
#pragma unroll
  for (int j = 0; j < 8; ++j) m.v[7 - j] = __builtin_bswap32(w[j]);
  sc_cond_sub_n(m.v);
  iv.get8(IM_C, i, sinv);
  sc_mul(u1, m, sinv);
  uint32_t SL[4], SH[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { SL[q] = use ? u1.v[q] : 0u; SH[q] = use ? u1.v[4 + q] : 0u; }
  write_gdigits(iv, i, SL, SH);
  return f;
}

// ---------------------------------------------------------------------------
// 1d. small batches (a block) and the standard-input lane prologue (1e): no
//     separate prologue launch. One lane runs a signature's scalar work,
//     per-lane s^-1 included, in two halves: the small-batch kernels' signature
//     wave (2c, 2d: wave 2) runs the u2 half before the barrier that releases
//     the chain waves and the u1 half after it.
// ---------------------------------------------------------------------------
// The u2 half of a signature: compact-range checks, the mode's high-S policy,
// s^-1, u2 = r/s, the GLV split of u2, the Q digits, r -> im. ok is the
// caller's validity so far (updated); sinv is s^-1 (of 1 when !ok) for the u1
// half (sig_lane_g).
HKV_DEV void sig_lane_q(sc r, sc s, uint32_t mode, SoAView iv, uint32_t i, bool& ok, bool& glv_ok, bool& n1, bool& n2,
                        sc& sinv) {
  ok = ok && u256_lt(r.v, SC_N) && u256_lt(s.v, SC_N);
  const bool high = sc_is_high(s);
  if (mode == HKV_MODE_HASKOIN) {
    sc ns;
    sc_neg(ns, s);
    if (high) s = ns;  // secp256k1_ecdsa_signature_normalize
  } else {
    ok = ok && !high;  // secp256k1_ecdsa_verify rejects high-S
  }
  ok = ok && !u256_is_zero(r.v) && !u256_is_zero(s.v);
  if (!ok) sc_set_u32(s, 1);
  sc u2;
  sc_inv(sinv, s);
  sc_mul(u2, r, sinv);
  uint32_t k1[5], k2[5];
  glv_ok = glv_split(u2, k1, n1, k2, n2);
  const bool use = ok && glv_ok;
  uint32_t S1[5], S2[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) { S1[q] = use ? k1[q] : 0u; S2[q] = use ? k2[q] : 0u; }
  write_qdigits(iv, i, S1, S2);
#pragma unroll
  for (int k = 0; k < 8; ++k) iv.put(IM_R, k, i, r.v[k]);
}
// The u1 half: m = msg32 mod n, u1 = m / s, the G digits (zero unless use).
HKV_DEV void sig_lane_g(sc m, const sc& sinv, bool use, SoAView iv, uint32_t i) {
  sc_cond_sub_n(m.v);  // m = msg32 mod n
  sc u1;
  sc_mul(u1, m, sinv);
  uint32_t SL[4], SH[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { SL[q] = use ? u1.v[q] : 0u; SH[q] = use ? u1.v[4 + q] : 0u; }
  write_gdigits(iv, i, SL, SH);
}
// flags as the full-grid kernels leave them (hkv_glv_kernel)
HKV_DEV uint32_t split_flags(bool ok, uint32_t pk_ok, bool glv_ok, bool n1, bool n2) {
  uint32_t f = (ok && (pk_ok & 1u)) ? FLAG_VALID : 0u;
  f |= pk_ok & (FLAG_YODD | FLAG_COMP);
  f |= (n1 ? FLAG_NEG1 : 0u) | (n2 ? FLAG_NEG2 : 0u) | (glv_ok ? 0u : FLAG_GLV_OVF);
  if (!glv_ok) f &= ~FLAG_VALID;
  return f;
}

struct StdArgs {
  const uint8_t* txs;
  uint32_t n_tx;
  const uint32_t* txt;
  const uint8_t* scripts;
  uint32_t scripts_len;
  const hkv_input_job* jobs;
  int32_t forkid;
  // the multisig scan the block kernel runs on its square-root wave
  // (hkv_ms_scan_kernel's operands; null: the host launches the scan)
  uint32_t* ms_desc;
  uint64_t* ms_off;
  unsigned long long* ms_ctr;
  // the tx offsets when the kernel builds the index rows of its inputs' txs
  // itself (the block kernel, txc_fill: no index launch); null: txt holds them
  const uint32_t* tx_off;
};
// the standard-input lane prologue (1e) run at the head of the mid-size
// ecmult kernel's lane (defined below, after the std parse helpers)
HKV_DEV void std_lane_prologue(uint32_t i, uint32_t n, SoAView iv, const StdArgs& sa);

// ---------------------------------------------------------------------------
// 2. ecmult + x compare
// ---------------------------------------------------------------------------
// Per-lane Q table, entry-major then lane: entry e of lane L is 96 contiguous
// bytes (quads x0 x1 | y0 y1 | bx0 bx1) at quad offset (e * n_lanes + L) * 6,
// so a lookup reads 64 contiguous bytes per lane (half a 128-B line) whatever
// entry the neighbouring lanes pick.
HKV_DEV uint4* qtab_ptr(uint32_t* qs, uint32_t n_lanes, uint32_t lane, int entry, int c) {
  return reinterpret_cast<uint4*>(qs) + ((size_t)entry * n_lanes + lane) * QTAB_QUADS_PER_ENTRY + c;
}
HKV_DEV void qtab_store(uint32_t* __restrict__ qs, uint32_t n_lanes, uint32_t lane, int entry, int c, const fe& a) {
  uint4* p = qtab_ptr(qs, n_lanes, lane, entry, c);
  p[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
  p[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}
HKV_DEV void qtab_load(const uint32_t* __restrict__ qs, uint32_t n_lanes, uint32_t lane, int entry, int c, fe& a) {
  const uint4* p = qtab_ptr(const_cast<uint32_t*>(qs), n_lanes, lane, entry, c);
  const uint4 v0 = p[0], v1 = p[1];
  a.v[0] = v0.x; a.v[1] = v0.y; a.v[2] = v0.z; a.v[3] = v0.w;
  a.v[4] = v1.x; a.v[5] = v1.y; a.v[6] = v1.z; a.v[7] = v1.w;
}

template <bool ILP>
HKV_DEV void ec_double(gej& acc) {
  if constexpr (ILP) gej_double_ilp(acc, acc);
  else gej_double<true>(acc, acc);  // 3 or 4 waves per SIMD: the fast scans (hkv_field.h FC)
}
template <bool ILP>
HKV_DEV void ec_accumulate(gej& acc, bool& inf, const fe& az, const fe& tx, const fe& ty, bool take) {
  if constexpr (ILP) gej_accumulate_ilp(acc, inf, az, tx, ty, take);
  else gej_accumulate<true>(acc, inf, az, tx, ty, take);
}

template <bool ILP = false>
HKV_DEV void gsum_lane(SoACView iv, const uint32_t* __restrict__ gtab, uint32_t i, bool valid, gej& A, bool& ainf);
HKV_DEV void gej_add_var(gej& acc, bool& inf, const gej& b, bool binf);
HKV_DEV bool x_matches_r(const fe& Xin, const fe& Z, const uint32_t r[8]);

// the lane's key as Q' = (x w, w^2) on E_w (w = x^3 + 7)
HKV_DEV void lane_q(ge& q, SoACView iv, uint32_t i, bool valid) {
  fe x, w;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    x.v[k] = iv.get(IM_QX, k, i);
    w.v[k] = iv.get(IM_W, k, i);
  }
  fe_mul(q.x, x, w);
  fe_sqr(q.y, w);
  if (!valid) ge_set_g(q);  // dummy point; all digits are zero for this lane
}

// The lane's Q table: j*Q', j = 1..QTAB_ENTRIES, affine on the isomorphic
// curve of scale Zg, with beta*x beside every entry.
// Pass 1 streams raw entries to the lane's scratch (z-ratios H_j parked in
// the beta*x slot of entry j-1); pass 2 walks back rescaling every entry
// to the common Z (rho_j = prod_{k>j} H_k) and writes beta*x.
HKV_DEV void qtable_build(const ge& q, uint32_t* __restrict__ qs, uint32_t n_lanes, uint32_t lane, fe& Zg) {
  gej p2, pj;
  gej_set_ge(p2, q);
  gej_double(p2, p2);  // 2Q (Jacobian, scale Z2)
  fe z2, qx, qy;       // Q' = phi_Z2(Q) = (x Z2^2, y Z2^3)
  fe_sqr(z2, p2.z);
  fe_mul(qx, q.x, z2);
  fe_mul(z2, z2, p2.z);
  fe_mul(qy, q.y, z2);
  qtab_store(qs, n_lanes, lane, 0, 0, qx);
  qtab_store(qs, n_lanes, lane, 0, 2, qy);
  qtab_store(qs, n_lanes, lane, 1, 0, p2.x);
  qtab_store(qs, n_lanes, lane, 1, 2, p2.y);
  pj.x = p2.x;
  pj.y = p2.y;
  fe_set_u32(pj.z, 1);
#pragma unroll 1
  for (int j = 2; j < QTAB_ENTRIES; ++j) {  // P_{j+1} = P_j + Q' (mixed, never degenerate)
    bool hz, rz;
    fe h;
    gej_add_ge_core(pj, pj, pj.z, qx, qy, hz, rz, &h);
    qtab_store(qs, n_lanes, lane, j, 0, pj.x);
    qtab_store(qs, n_lanes, lane, j, 2, pj.y);
    qtab_store(qs, n_lanes, lane, (j - 1), 4, h);
  }
  fe_mul(Zg, p2.z, pj.z);  // total scale: phi_Z2 then phi_Zc, Zc = pj.z
  fe beta;
#pragma unroll
  for (int k = 0; k < 8; ++k) beta.v[k] = FE_BETA[k];
  {
    fe bx;
    fe_mul(bx, pj.x, beta);
    qtab_store(qs, n_lanes, lane, QTAB_ENTRIES - 1, 4, bx);
  }
  fe rho;
  fe_set_u32(rho, 1);
#pragma unroll 1
  for (int j = QTAB_ENTRIES - 2; j >= 0; --j) {
    fe x, y, t;
    if (j >= 1) {
      qtab_load(qs, n_lanes, lane, j, 4, t);  // H_{j+1}
      fe_mul(rho, rho, t);
    }
    qtab_load(qs, n_lanes, lane, j, 0, x);
    qtab_load(qs, n_lanes, lane, j, 2, y);
    fe_sqr(t, rho);
    fe_mul(x, x, t);
    fe_mul(t, t, rho);
    fe_mul(y, y, t);
    qtab_store(qs, n_lanes, lane, j, 0, x);
    qtab_store(qs, n_lanes, lane, j, 2, y);
    fe_mul(x, x, beta);
    qtab_store(qs, n_lanes, lane, j, 4, x);
  }
}

// The joint form of the table launch (hkv_joint_digits.h, hkv_layout.h JQ_*):
// the 11 entries (a + b lambda) Q' of the joint digits' orbits, x | y only, in
// the Booth table's 48 quads per signature. Entry j is entry j - 1 plus a unit
// image (beta^e x, +-y) of Q'. Q' and 2Q start on one Z, so the walk is nine
// co-Z additions with update (hkv_group.h gej_zaddu): Qc = (Xq, Yq), Q' on the
// running point's Z, stays in registers, each step leaves both on the new Z,
// and no Z is carried. A step with e != 0 (three of the nine) turns Xq into
// the image's x in place and takes it back from the updated image, Xq =
// beta^-e W1, with beta^-1 = beta^2: a beta product before and after. (The
// other way, Xq H^2 beside the image, holds Xq and H^2 across the addition
// and spilled at 128 VGPRs, where this one takes 120 and no scratch.) Pass 2
// rescales entries 9..1 to the last one's Z, where Qc already stands: it is
// entry 0. The running product of pass 2 ends as rho = H_2 ... H_10, and
// Zg = Z2 rho. In product scans: 7 + 4, 9 x 6 + 3 x 2 the walk, 45 pass 2. The
// nine z-ratios H_2..H_10 wait between the passes where nothing else lives:
// four in LDS (idle in this launch: 32 KiB per workgroup, four workgroups per
// CU), two in the lane's 4 spare quads, one in its Zg slot (written after the
// build) and two in entry 10's slot, whose raw x, y stay in registers until
// pass 2 has read them. A sum of two of these small multiples of Q' vanishes
// only for a key of small order on a twist, whose verdict is reject whatever
// the table holds.
typedef uint32_t JqLds[4][8][WG];
HKV_DEV uint4* jq_ptr(uint32_t* qs, uint32_t n_lanes, uint32_t lane, int entry, int c) {
  return reinterpret_cast<uint4*>(qs) + ((size_t)entry * n_lanes + lane) * JQ_QUADS_PER_ENTRY + c;
}
HKV_DEV void quads_store(uint4* p, const fe& a) {
  p[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
  p[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}
HKV_DEV void quads_load(const uint4* p, fe& a) {
  const uint4 v0 = p[0], v1 = p[1];
  a.v[0] = v0.x; a.v[1] = v0.y; a.v[2] = v0.z; a.v[3] = v0.w;
  a.v[4] = v1.x; a.v[5] = v1.y; a.v[6] = v1.z; a.v[7] = v1.w;
}
HKV_DEV void jq_load(const uint32_t* __restrict__ qs, uint32_t n_lanes, uint32_t lane, int entry, int c, fe& a) {
  quads_load(jq_ptr(const_cast<uint32_t*>(qs), n_lanes, lane, entry, c), a);
}
struct JqPark {
  JqLds* lds;
  uint4 *spare, *zslot, *last;  // 4 quads, 2 quads, entry 10's 4 quads
  // slot h = j - 2 of H_j (h is uniform)
  HKV_DEV uint4* quads(int h) const { return h < 6 ? spare + 2 * (h - 4) : h == 6 ? zslot : last + 2 * (h - 7); }
  HKV_DEV void store(int h, const fe& a) const {
    if (h < 4) {
#pragma unroll
      for (int k = 0; k < 8; ++k) (*lds)[h][k][threadIdx.x] = a.v[k];
    } else {
      quads_store(quads(h), a);
    }
  }
  HKV_DEV void load(int h, fe& a) const {
    if (h < 4) {
#pragma unroll
      for (int k = 0; k < 8; ++k) a.v[k] = (*lds)[h][k][threadIdx.x];
    } else {
      quads_load(quads(h), a);
    }
  }
};
// a := beta^e a, e = 1, 2
template <bool FC>
HKV_DEV void fe_mul_beta_pow(fe& a, uint32_t e) {
  fe beta, b;
#pragma unroll
  for (int k = 0; k < 8; ++k) beta.v[k] = FE_BETA[k];
  fe_mul<FC>(b, a, beta);
  if (e == 2u) {  // beta^2 x = -(x + beta x)
    fe_add(b, a, b);
    fe_neg(b, b);
  }
  a = b;
}
// zslot: the lane's Zg slot (the caller writes Zg there after the build)
// FC: the products' fast scans (hkv_field.h). -DHKV_QTABLE_FC=0 / 1 is the A/B.
#ifndef HKV_QTABLE_FC
#define HKV_QTABLE_FC 0
#endif
template <bool FC = (HKV_QTABLE_FC != 0)>
HKV_DEV void qtable_build_joint(const ge& q, uint32_t* __restrict__ qs, uint32_t n_lanes, uint32_t lane, uint4* zslot,
                                JqLds* lds, fe& Zg) {
  static_assert(JD_ENTRIES == JQ_ENTRIES, "one entry per orbit");
  const JqPark park = {lds, reinterpret_cast<uint4*>(qs) + (size_t)JQ_ENTRIES * JQ_QUADS_PER_ENTRY * n_lanes +
                                (size_t)lane * JQ_SPARE_QUADS,
                       zslot, jq_ptr(qs, n_lanes, lane, JQ_ENTRIES - 1, 0)};
  gej p2;
  gej_set_ge(p2, q);
  gej_double<FC>(p2, p2);  // 2Q (Jacobian, scale Z2)
  fe xq, yq;               // Qc: Q' on the running point's Z
  {
    fe z2;  // Q' = phi_Z2(Q) = (x Z2^2, y Z2^3)
    fe_sqr<FC>(z2, p2.z);
    fe_mul<FC>(xq, q.x, z2);
    fe_mul<FC>(z2, z2, p2.z);
    fe_mul<FC>(yq, q.y, z2);
  }
  quads_store(jq_ptr(qs, n_lanes, lane, 1, 0), p2.x);
  quads_store(jq_ptr(qs, n_lanes, lane, 1, 2), p2.y);
#pragma unroll 1
  for (int j = 2; j < JQ_ENTRIES; ++j) {
    // entry j = entry j - 1 + (-1)^s lambda^e Q' (uniform in j); p2.x, p2.y: the running point
    const uint32_t e = (JD_STEP_E >> (2 * (j - 1))) & 3u;
    const bool neg = ((JD_STEP_S >> (j - 1)) & 1u) != 0;
    fe h;
    if (e != 0u) fe_mul_beta_pow<FC>(xq, e);  // the image's x
    fe_cneg(yq, yq, neg);
    gej_zaddu<FC>(p2.x, p2.y, xq, yq, p2.x, p2.y, h);
    fe_cneg(yq, yq, neg);                    // Yq = +-A1
    if (e != 0u) fe_mul_beta_pow<FC>(xq, 3u - e);  // Xq = beta^-e W1
    if (j < JQ_ENTRIES - 1) {  // (the last entry's x, y wait in p2)
      quads_store(jq_ptr(qs, n_lanes, lane, j, 0), p2.x);
      quads_store(jq_ptr(qs, n_lanes, lane, j, 2), p2.y);
    }
    park.store(j - 2, h);
  }
  // Qc stands at the last Z: entry 0 at the final scale
  quads_store(jq_ptr(qs, n_lanes, lane, 0, 0), xq);
  quads_store(jq_ptr(qs, n_lanes, lane, 0, 2), yq);
  fe rho;  // rho_j = prod_{k > j} H_k
  park.load(JQ_ENTRIES - 3, rho);
#pragma unroll 1
  for (int j = JQ_ENTRIES - 2;; --j) {
    fe x, y, t;
    jq_load(qs, n_lanes, lane, j, 0, x);
    jq_load(qs, n_lanes, lane, j, 2, y);
    fe_sqr<FC>(t, rho);
    fe_mul<FC>(x, x, t);
    fe_mul<FC>(t, t, rho);
    fe_mul<FC>(y, y, t);
    quads_store(jq_ptr(qs, n_lanes, lane, j, 0), x);
    quads_store(jq_ptr(qs, n_lanes, lane, j, 2), y);
    if (j == 1) break;
    park.load(j - 2, t);  // H_j
    fe_mul<FC>(rho, rho, t);
  }
  fe_mul<FC>(Zg, p2.z, rho);  // total scale: phi_Z2 then phi_Zc, Zc = H_2 ... H_10
  quads_store(park.last, p2.x);
  quads_store(park.last + 2, p2.y);
}

// The shared doubling chain of k1 * Q' + k2 * lambda(Q'), 33 radix-16 windows
// from the top, over the lane's table: acc, inf = the sum B' on the table's
// curve. Window w's digit word is loaded one window ahead, hiding its
// latency. signs: the lane's GLV signs (bit 0: k1, bit 1: k2), read once per
// term from the caller's LDS slot.
template <bool ILP>
HKV_DEV void q_chain(gej& acc, bool& inf, SoACView iv, uint32_t i, bool valid, const uint32_t* __restrict__ qs,
                     uint32_t n_lanes, uint32_t lane, const uint32_t& signs) {
  inf = true;
  fe_set_zero(acc.x);
  fe_set_zero(acc.y);
  fe_set_zero(acc.z);
  uint32_t dw = valid ? iv.get(IM_DIG, NWIN - 1, i) : DIG_ZERO;
  int win = NWIN - 1;
  bool dbl = false;       // the first window starts from infinity: no doublings
  int x1 = 0, x2 = 0;     // the merged top window's second terms (pair_chain)
  int nterm = 2;          // Q terms of the current window
  {
    // the top two windows as one digit in [0, 16] per half, taken as
    // min(m, 8) + (m - 8)+ (pair_chain): two additions where every wave
    // ran the second window's 4 doublings (5 % of the halves reach 2^127)
    const uint32_t dw2 = valid ? iv.get(IM_DIG, NWIN - 2, i) : DIG_ZERO;
    const int t1 = (((int)(dw & QDIG_MASK) - QBIAS) << QW) + (int)(dw2 & QDIG_MASK) - QBIAS;
    const int t2 = (((int)((dw >> QDIG_BITS) & QDIG_MASK) - QBIAS) << QW) + (int)((dw2 >> QDIG_BITS) & QDIG_MASK) - QBIAS;
    if (!__any(t1 < 0 || t1 > 2 * QBIAS || t2 < 0 || t2 > 2 * QBIAS)) {
      const int e1 = t1 < QBIAS ? t1 : QBIAS, e2 = t2 < QBIAS ? t2 : QBIAS;
      x1 = t1 - e1;
      x2 = t2 - e2;
      dw = (uint32_t)(e1 + QBIAS) | ((uint32_t)(e2 + QBIAS) << QDIG_BITS);
      win = NWIN - 2;
      nterm = 4;
    }
  }
#pragma unroll 1
  for (; win >= 0; --win) {
    const int d1 = (int)(dw & QDIG_MASK) - QBIAS, d2 = (int)((dw >> QDIG_BITS) & QDIG_MASK) - QBIAS;
    const uint32_t dw_next = (win > 0 && valid) ? iv.get(IM_DIG, win - 1, i) : DIG_ZERO;
    if (dbl) {
#pragma unroll 1
      for (int d = 0; d < QW; ++d) {
        if (!inf) ec_double<ILP>(acc);
      }
    }
    dbl = true;
    // Q terms: slot 0 = k1 * Q', slot 1 = k2 * lambda(Q') (terms 2, 3: the
    // merged top window's second terms, run only when a lane of the wave has one)
#pragma unroll 1
    for (int t = 0; t < nterm; ++t) {
      const int slot = t & 1;
      const int dg = t < 2 ? (slot == 0 ? d1 : d2) : (slot == 0 ? x1 : x2);
      const bool take = dg != 0;
      if (t >= 2 && !__any(take)) continue;
      const int mg = dg < 0 ? -dg : dg;
      const int ie = mg ? mg - 1 : 0;
      const bool neg = (dg < 0) != (((signs >> slot) & 1u) != 0);
      fe tx, ty;
      qtab_load(qs, n_lanes, lane, ie, (slot == 0 ? 0 : 4), tx);
      qtab_load(qs, n_lanes, lane, ie, 2, ty);
      fe_cneg(ty, ty, neg);
      const bool was_inf = inf;
      ec_accumulate<ILP>(acc, inf, acc.z, tx, ty, take);
      // only the first nonzero digit of a lane starts from infinity: skip
      // the 24 selects in every window where no lane of the wave does
      if (__any(take && was_inf)) gej_accumulate_from_inf(acc, inf, tx, ty, take && was_inf);
    }
    nterm = 2;
    dw = dw_next;
  }
}

// The chain on joint radix-8 digits (hkv_joint_digits.h), 2a's chain launch.
// The preamble: the lane's signed k1, k2 rebuilt exactly from its Booth digit
// words (word(w): window w's, low to high; sum_w d_w 16^w with a running
// carry) and its GLV signs, then recoded into the lane's column of jd.
template <class DigitWord>
HKV_DEV void joint_digits_lane(uint32_t (*jd)[WG], uint32_t signs, DigitWord word) {
  constexpr uint32_t QM = (1u << QW) - 1u;
  uint32_t k1[5] = {0, 0, 0, 0, 0}, k2[5] = {0, 0, 0, 0, 0};
  int c1 = 0, c2 = 0;
#pragma unroll
  for (int w = 0; w < NWIN; ++w) {
    const uint32_t dw = word(w);
    const int t1 = (int)(dw & QDIG_MASK) - QBIAS + c1, t2 = (int)((dw >> QDIG_BITS) & QDIG_MASK) - QBIAS + c2;
    const uint32_t n1 = (uint32_t)t1 & QM, n2 = (uint32_t)t2 & QM;
    c1 = (t1 - (int)n1) >> QW;
    c2 = (t2 - (int)n2) >> QW;
    const int q = (QW * w) >> 5, sh = (QW * w) & 31;  // (the magnitudes are below 2^129: word 4 at most)
    k1[q] |= n1 << sh;
    k2[q] |= n2 << sh;
    if (sh + QW > 32 && q < 4) {
      k1[q + 1] |= n1 >> (32 - sh);
      k2[q + 1] |= n2 >> (32 - sh);
    }
  }
  jd_signed(k1, (signs & 1u) != 0);
  jd_signed(k2, (signs & 2u) != 0);
  uint32_t out[JD_WORDS];
  joint_recode(k1, k2, out);
#pragma unroll
  for (int q = 0; q < JD_WORDS; ++q) jd[q][threadIdx.x] = out[q];
}
// The window loop: from the highest window in which a lane of the wave has a
// non-zero digit, three doublings and one addition of the digit's entry under
// its unit: beta x by one product where a lane of the wave needs it (beta^2 x
// = -(x + beta x) under the lane mask), y negated by s.
HKV_DEV void q_chain_joint(gej& acc, bool& inf, const uint32_t (*jd)[WG], const uint32_t* __restrict__ qs,
                           uint32_t n_lanes, uint32_t lane) {
  inf = true;
  fe_set_zero(acc.x);
  fe_set_zero(acc.y);
  fe_set_zero(acc.z);
  int win = JD_WINDOWS - 1;
#pragma unroll 1
  while (win > 0 && !__any(((jd[win >> 2][threadIdx.x] >> (7 * (win & 3))) & JD_ENTRY_MASK) != JD_ZERO)) --win;
  bool dbl = false;  // the first window starts from infinity: no doublings
#pragma unroll 1
  for (; win >= 0; --win) {
    const uint32_t code = (jd[win >> 2][threadIdx.x] >> (7 * (win & 3))) & JD_CODE_MASK;
    const uint32_t ent = code & JD_ENTRY_MASK;
    const bool take = ent != JD_ZERO;
    if (dbl) {
#pragma unroll 1
      for (int d = 0; d < 3; ++d) {
        if (!inf) ec_double<false>(acc);
      }
    }
    dbl = true;
    const int ie = take ? (int)ent : 0;
    const uint32_t e = (code >> JD_E_SHIFT) & 3u;
    const bool e2 = take && e == 2u;
    fe tx, ty;
    jq_load(qs, n_lanes, lane, ie, 0, tx);
    const bool e1 = take && e == 1u;
    if (__any(e1 || e2)) {  // beta x by a product (the table keeps x | y); beta^2 x = -(x + beta x)
      fe beta, bx;
#pragma unroll
      for (int k = 0; k < 8; ++k) beta.v[k] = FE_BETA[k];
      fe_mul<true>(bx, tx, beta);
      fe_cmov(tx, bx, e1);
      fe_add(bx, tx, bx);
      fe_cmov(tx, bx, e2);
      fe_cneg(tx, tx, e2);
    }
    jq_load(qs, n_lanes, lane, ie, 2, ty);
    fe_cneg(ty, ty, (code >> JD_S_SHIFT) != 0u);
    const bool was_inf = inf;
    ec_accumulate<false>(acc, inf, acc.z, tx, ty, take);
    if (__any(take && was_inf)) gej_accumulate_from_inf(acc, inf, tx, ty, take && was_inf);
  }
}

// Optional clock probe (hkv_profile_clock): shader-clock and constant-rate
// counters into clk[slot], clk[slot + 1] around block 0's work (slot 0 at its
// start, 2 at its end), so bench.py prices the roofline at the clock the
// launch actually ran at.
HKV_DEV void clock_probe(unsigned long long* __restrict__ clk, int slot) {
  if (clk != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
    clk[slot] = clock64();
    clk[slot + 1] = wall_clock64();
  }
}

// ILP: the paired-product group forms; full-grid launches of mid-size
// batches (at most 2 waves per SIMD: 32k-131k signatures) take the <true>
// instance, which is allocated for 2 waves per SIMD (no spill). Larger
// batches run the table and chain launches (2a below) with the plain forms:
// their 4 waves per SIMD already fill the issue slots.
// STDPRO (mid-size standard-input batches): each lane first runs the
// standard-input lane prologue (1e: std_parse, s^-1, GLV, digits into im)
// for its input, so the latency-bound prologue phase runs inside this launch's
// occupancy instead of as a launch of its own before it.
// (ILP stays a parameter for the instances' names in traces and tools; the
// plain-form instance went with 2a, so the allocation is the 2-wave one)
template <bool ILP, bool STDPRO = false>
__global__ void __launch_bounds__(WG, 2) hkv_ecmult_kernel(uint32_t* __restrict__ im, uint32_t n, uint32_t n_pad,
                                                           uint32_t* __restrict__ qs,
                                                           unsigned long long* __restrict__ clk, StdArgs sa) {
  static_assert(ILP, "only the paired-form (mid-size) instance is built: larger batches run 2a");
  const uint32_t n_lanes = gridDim.x * WG;
  const uint32_t lane = blockIdx.x * WG + threadIdx.x;
  // per-lane LDS slots for state the chain does not touch (the table scale
  // Zg, used only after the last window) and the GLV signs the accumulate
  // reads once per term: at 4 waves per SIMD (128 VGPRs) these were spilled
  // to scratch; LDS is idle in this kernel (9 KiB per workgroup)
  __shared__ uint32_t park[9][WG];
  // optional clock probe (hkv_profile_clock): shader-clock and constant-rate
  // counters around block 0's work, so bench.py prices the roofline at the
  // clock the launch actually ran at
  clock_probe(clk, 0);

  for (uint32_t base = blockIdx.x * WG; base < n_pad; base += gridDim.x * WG) {
    const uint32_t i = base + threadIdx.x;
    if constexpr (STDPRO) std_lane_prologue(i, n, SoAView{im, n_pad}, sa);  // (read back below by the same lane)
    // (im indexed here, not through a view held by this body: see the view's header)
    const uint32_t flags = im[(size_t)IM_FLAGS.off * n_pad + i];
    const bool valid = (i < n) && (flags & FLAG_VALID);
    ge q;
    lane_q(q, SoACView{im, n_pad}, i, valid);
    const bool neg1 = (flags & FLAG_NEG1) != 0, neg2 = (flags & FLAG_NEG2) != 0;

    fe Zg;
    qtable_build(q, qs, n_lanes, lane, Zg);
#pragma unroll
    for (int k = 0; k < 8; ++k) park[k][threadIdx.x] = Zg.v[k];
    park[8][threadIdx.x] = (neg1 ? 1u : 0u) | (neg2 ? 2u : 0u);

    gej acc;
    bool inf;
    q_chain<ILP>(acc, inf, SoACView{im, n_pad}, i, valid, qs, n_lanes, lane, park[8][threadIdx.x]);

    // hand B' = (X, Y, Z acc * Zg) on E_w to the finish kernel
    fe zt;
#pragma unroll
    for (int k = 0; k < 8; ++k) Zg.v[k] = park[k][threadIdx.x];
    fe_mul(zt, acc.z, Zg);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      im[(size_t)(IM_BX.off + k) * n_pad + i] = acc.x.v[k];
      im[(size_t)(IM_BY.off + k) * n_pad + i] = acc.y.v[k];
      im[(size_t)(IM_BZ.off + k) * n_pad + i] = zt.v[k];
    }
    im[(size_t)IM_FLAGS.off * n_pad + i] = flags | (inf ? FLAG_BINF : 0u);
  }
  clock_probe(clk, 2);
}

// ---------------------------------------------------------------------------
// 2a. Batches above half the resident grid (the 1M headline, large
//     standard-input batches): the table build and the window chain as two
//     launches, one signature per lane at 4 waves per SIMD, over chunks of cn
//     signatures (i0 .. i0 + cn, cn a multiple of WG). Signature s of the
//     chunk owns table slot s of qs and the Zg slot behind the chunk's tables
//     (hkv_layout.h HKV_REC_CHUNK). The chain launch is bound by VALU issue,
//     and the table launch, which moves 1.9 KB per signature in its joint
//     form (within a quarter of its memory time: DESIGN 4.2, round 16), still
//     issues VALU at about 85 % of the chain's rate. A 1M
//     chunk is four times the resident grid, so a workgroup slot that frees
//     early takes the next workgroup. The earlier form, one kernel whose
//     resident lanes each looped over four signatures, ran the same
//     instruction count 4.6 % longer at a lower average occupancy, and so do
//     these launches in chunks of one resident grid one after another (DESIGN
//     4.2, round 10): keep the chunk well above the resident grid. A chunk
//     may run in parts (hkv_layout.h HKV_REC_PART), two at a time on two
//     streams, each in a slot of its own inside the chunk's scratch: the
//     kernels take the slot's base as qs and the part as (i0, cn).
//     With HKV_JOINT_DIGITS (hkv_layout.h, the default) the table launch
//     builds the 11 entries (a + b lambda) Q' of hkv_joint_digits.h and the
//     chain launch recodes its lane's Booth digits into joint radix-8 digits
//     in LDS: 44 windows of three doublings and one addition (q_chain_joint)
//     where the Booth chain (q_chain) runs 33 of four and two.
// ---------------------------------------------------------------------------
HKV_DEV uint4* zg_ptr(uint32_t* qs, uint32_t cn, uint32_t s) {
  return reinterpret_cast<uint4*>(qs) + (size_t)cn * QTAB_QUADS + (size_t)s * QTAB_ZG_QUADS;
}

__global__ void __launch_bounds__(WG, HKV_ECMULT_WAVES) hkv_qtable_kernel(const uint32_t* __restrict__ im, uint32_t n,
                                                                       uint32_t n_pad, uint32_t i0, uint32_t cn,
                                                                       uint32_t* __restrict__ qs) {
  const uint32_t s = blockIdx.x * WG + threadIdx.x;  // < cn: the grid is cn / WG blocks
  const uint32_t i = i0 + s;
  const SoACView iv = {im, n_pad};
  const uint32_t flags = iv.get(IM_FLAGS, i);
  const bool valid = (i < n) && (flags & FLAG_VALID);
  ge q;
  lane_q(q, iv, i, valid);
  fe Zg;
  uint4* z = zg_ptr(qs, cn, s);
  if constexpr (JOINT_DIGITS) {
    __shared__ JqLds park;
    qtable_build_joint(q, qs, cn, s, z, &park, Zg);
  } else {
    qtable_build(q, qs, cn, s, Zg);
  }
  z[0] = make_uint4(Zg.v[0], Zg.v[1], Zg.v[2], Zg.v[3]);
  z[1] = make_uint4(Zg.v[4], Zg.v[5], Zg.v[6], Zg.v[7]);
}

__global__ void __launch_bounds__(WG, HKV_ECMULT_WAVES) hkv_chain_kernel(uint32_t* __restrict__ im, uint32_t n,
                                                                      uint32_t n_pad, uint32_t i0, uint32_t cn,
                                                                      const uint32_t* __restrict__ qs,
                                                                      unsigned long long* __restrict__ clk) {
  // the lane's GLV signs, read once per term (q_chain): held in a register
  // they were spilled to scratch at 128 VGPRs; LDS is idle in this kernel.
  // The joint form keeps the lane's 44 digit codes there instead (11 KiB per
  // workgroup): each lane reads only its own column, so no barrier.
  __shared__ uint32_t lds[JOINT_DIGITS ? JD_WORDS : 1][WG];
  // optional clock probe (hkv_profile_clock), as in hkv_ecmult_kernel
  clock_probe(clk, 0);
  const uint32_t s = blockIdx.x * WG + threadIdx.x;  // < cn: the grid is cn / WG blocks
  const uint32_t i = i0 + s;
  // (im indexed here, not through a view held by this body: see the view's header)
  const uint32_t flags = im[(size_t)IM_FLAGS.off * n_pad + i];
  const bool valid = (i < n) && (flags & FLAG_VALID);
  const uint32_t sg = ((flags & FLAG_NEG1) ? 1u : 0u) | ((flags & FLAG_NEG2) ? 2u : 0u);
  gej acc;
  bool inf;
  if constexpr (JOINT_DIGITS) {
    joint_digits_lane(lds, sg, [&](int w) {
      return valid ? im[(size_t)(IM_DIG.off + w) * n_pad + i] : DIG_ZERO;
    });
    q_chain_joint(acc, inf, lds, qs, cn, s);
  } else {
    lds[0][threadIdx.x] = sg;
    q_chain<false>(acc, inf, SoACView{im, n_pad}, i, valid, qs, cn, s, lds[0][threadIdx.x]);
  }

  // hand B' = (X, Y, Z acc * Zg) on E_w to the finish kernel
  fe Zg, zt;
  {
    const uint4* z = zg_ptr(const_cast<uint32_t*>(qs), cn, s);
    const uint4 v0 = z[0], v1 = z[1];
    Zg.v[0] = v0.x; Zg.v[1] = v0.y; Zg.v[2] = v0.z; Zg.v[3] = v0.w;
    Zg.v[4] = v1.x; Zg.v[5] = v1.y; Zg.v[6] = v1.z; Zg.v[7] = v1.w;
  }
  fe_mul(zt, acc.z, Zg);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    im[(size_t)(IM_BX.off + k) * n_pad + i] = acc.x.v[k];
    im[(size_t)(IM_BY.off + k) * n_pad + i] = acc.y.v[k];
    im[(size_t)(IM_BZ.off + k) * n_pad + i] = zt.v[k];
  }
  im[(size_t)IM_FLAGS.off * n_pad + i] = flags | (inf ? FLAG_BINF : 0u);
  clock_probe(clk, 2);
}

// ---------------------------------------------------------------------------
// 2c. Pair-lane split kernel (small batches: a block). A workgroup takes
//     PAIR_SIGS = 32 signatures on 4 waves, one per SIMD of its CU:
//       wave 0: k1 * Q' chains, two lanes per signature (pair form,
//               hkv_group.h pair_double / pair_accumulate), then the join;
//       wave 1: k2 * lambda(Q') chains, two lanes per signature;
//       wave 2: the u2 half of the signature (s^-1, u2, GLV, Q digits;
//               lanes 0-31), then the u1 half and A = u1 G from the
//               per-window tables;
//       wave 3: the key's y0 = sqrt(w) of its parity (lanes 0-31).
//     Barrier P publishes the Q digits, A (wave 2) and y0 (wave 3) reach the
//     join through aux, half 1's sum through LDS (barrier A); barrier B ends
//     the group. Every chain wave runs alone on its SIMD, where it is
//     issue-bound: the pair forms put each step's independent products on two
//     lanes of one instruction stream.
//     STD (hkv_verify_std_inputs*): the signatures are standard inputs, not
//     records. Every wave runs the cheap half of verifyStdInput for its
//     inputs (std_parse: template, strict DER, the key bytes), so the chains
//     start without waiting for any hash; wave 2 runs the other half (the
//     HASH160 / SHA-256 script checks and the sighash, std_hash) after
//     barrier P, beside the chains — u1 = m / s is the only thing that needs
//     the message — and writes the input's verify record.
// ---------------------------------------------------------------------------
constexpr int PAIR_TPB = 256;  // (PAIR_SIGS: hkv_layout.h)
// phase-stamp slots (clk[4 + slot]; include/hkv.h hkv_profile_phases)
enum : int { STAMP_START = 0, STAMP_TABLE0, STAMP_P, STAMP_CHAIN0, STAMP_A, STAMP_JOIN, STAMP_SIG, STAMP_GSUM,
             STAMP_SQRT, STAMP_TABLE1, STAMP_CHAIN1, STAMP_COUNT };
// compress the even bits of a 64-bit lane mask into 32 bits (signature c = lanes 2c, 2c + 1)
HKV_DEV uint32_t even_bits(uint64_t x) {
  x &= 0x5555555555555555ull;
  x = (x | (x >> 1)) & 0x3333333333333333ull;
  x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
  x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
  x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
  return (uint32_t)x;
}
// the record words 24..41 (pklen, SEC1 bytes) of a parsed standard input's
// key, as hkv_std_input_kernel writes them (zero when the parse failed)
HKV_DEV void std_key_words(uint32_t kw[REC_WORDS], const StdIn& x) {
#pragma unroll
  for (int k = 0; k < 24; ++k) kw[k] = 0;
#pragma unroll
  for (int w = 0; w < 18; ++w) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int q = 4 * w + b;  // byte 96 + q of the record
      uint32_t byte = 0;
      if (q == 0) byte = x.pub_len;
      else if ((uint32_t)(q - 1) < x.pub_len && q - 1 < 65) byte = x.pub[q - 1];
      v |= byte << (8 * b);
    }
    kw[24 + w] = x.ok ? v : 0u;
  }
}
// the standard-input operands (hkv_verify_std_inputs*)

// Pair-form pieces shared by the small-batch kernels (2c, 2d). Each chain
// lane keeps its own coordinate of every table entry in LDS: ql is one chain
// wave's [QTAB_ENTRIES][8][64] table (x, or beta * x when half = 1, on the
// even lane; y on the odd lane).
typedef uint32_t QLane[QTAB_ENTRIES][8][64];

// j * q, j = 1..QTAB_ENTRIES, on the isomorphic curve of scale Zg, in pair
// form: Q = x | y is affine on its own curve (the a = 0 formulas never use
// b). Forward: 2Q, Q' = phi_Z2(Q), P_{j+1} = P_j + Q' (pair additions; each
// lane keeps its raw coordinate in its LDS table slot, the pair's even lane
// the z-ratio H_{j+1} in hl); backward: rho_j = prod_{k>j} H_k, entry j =
// (x rho^2, y rho^3) (beta * x on the half-1 even lanes) rescaled in place —
// four product levels per entry (rho H, rho^2, [x beta | rho^3],
// [. rho^2 | y rho^3]) instead of six one-lane products, and no global
// scratch round trip on the dependent loads. Returns Zg on both lanes.
typedef uint32_t HLane[QTAB_ENTRIES - 1][8][32];
HKV_DEV void pair_table(const fe& Q, int half, uint32_t odd, QLane& ql, HLane& hl, uint32_t ln, fe& Zg) {
  const uint32_t pc = (ln >> 1) & 31u;  // the pair's H slot
  auto put = [&](int j, const fe& v) {
#pragma unroll
    for (int k = 0; k < 8; ++k) ql[j][k][ln] = v.v[k];
  };
  fe P = Q, Z, O1, O2, zz, zs, R, Qp;
  fe_set_u32(Z, 1);
  pair_double(P, Z, odd);     // 2Q = X2 | Y2, Z2 on the odd lane
  fe_bc1(zz, Z);              // Z2             | Z2
  fe_sqr(zs, zz);             // Z2^2
  fe_sel(O1, Q, zz, odd);     // x              | Z2
  fe_mul(R, O1, zs);          // x Z2^2         | Z2^3
  fe_mul(O2, Q, R);           //                | y Z2^3
  fe_sel(Qp, R, O2, odd);     // Q' = phi_Z2(Q): x Z2^2 | y Z2^3
  put(0, Qp);
  put(1, P);
  fe_set_u32(Z, 1);           // P_2 = (X2, Y2, 1) on the curve of scale Z2
#pragma unroll 1
  for (int j = 2; j < QTAB_ENTRIES; ++j) {
    fe H;
    pair_add_affine(P, Z, Qp, odd, H);
    put(j, P);
    if (!odd) {
#pragma unroll
      for (int k = 0; k < 8; ++k) hl[j - 1][k][pc] = H.v[k];  // H_{j+1}
    }
  }
  fe zc;
  fe_bc1(zc, Z);
  fe_mul(Zg, zz, zc);         // total scale: phi_Z2 then phi_Zc
  fe beta, one;
#pragma unroll
  for (int k = 0; k < 8; ++k) beta.v[k] = FE_BETA[k];
  fe_set_u32(one, 1);
  fe bsel;                    // the even lane's x factor: beta (half 1) or 1
  fe_sel(bsel, half ? beta : one, one, odd);
  {
    fe bx;
    fe_mul(bx, P, bsel);      // beta x | y (x 1)
    put(QTAB_ENTRIES - 1, bx);
  }
  fe rho;
  fe_set_u32(rho, 1);
#pragma unroll 1
  for (int j = QTAB_ENTRIES - 2; j >= 0; --j) {
    fe c, t, h;
    if (j >= 1) {
#pragma unroll
      for (int k = 0; k < 8; ++k) h.v[k] = hl[j][k][pc];  // H_{j+1}
      fe_mul(rho, rho, h);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) c.v[k] = ql[j][k][ln];    // x | y of entry j
    fe_sqr(t, rho);                            // rho^2
    fe_sel(O1, c, t, odd);                     // x              | rho^2
    fe_sel(O2, bsel, rho, odd);                // beta or 1      | rho
    fe_mul(R, O1, O2);                         // beta x         | rho^3
    fe_sel(O1, R, c, odd);                     // beta x         | y
    fe_sel(O2, t, R, odd);                     // rho^2          | rho^3
    fe_mul(R, O1, O2);                         // beta x rho^2   | y rho^3
    put(j, R);
  }
}

// The windows w_hi..w_lo (radix 16, top first) of one chain in pair form,
// from infinity: P = X | Y, Z on the odd lane. half 0 takes k1's digits,
// half 1 k2's; negh: the GLV half is negative.
HKV_DEV void pair_chain(fe& P, fe& Z, bool& inf, const QLane& ql, SoACView iv, uint32_t i, bool valid, bool negh,
                        int half, uint32_t odd, uint32_t ln, int w_hi, int w_lo) {
  inf = true;
  fe_set_zero(P);
  fe_set_zero(Z);
  // the half's digit and the odd lane's negation as VGPR arithmetic (a shift
  // count, a mask), so no lane-mask SGPR pair is live through the windows:
  // two such pairs were lane-spilled and reloaded (4 v_readlane) in every
  // window
  const uint32_t dshift = half ? QDIG_BITS : 0u;
  const uint32_t negm = negh ? odd : 0u;  // the GLV half's sign on the odd (y) lane
  auto digit = [&](uint32_t w) { return (int)((w >> dshift) & QDIG_MASK) - QBIAS; };
  uint32_t dw = valid ? iv.get(IM_DIG, w_hi, i) : DIG_ZERO;
  bool dbl = false;  // the first window starts from infinity: no doublings
  if (w_hi == NWIN - 1 && w_hi > w_lo) {
    // The top two windows as one digit m = 2^QW d_top + d_next. The GLV
    // halves are < 2^128 in practice (the bound the device split asserts is
    // 2^129), so d_top is bit 127 and m is the unsigned value of bits
    // 124..127 plus bit 123, in [0, 16]: taken as min(m, 8) + (m - 8)+ from
    // the 8-entry table, one addition at most, where a top digit of 1 on any
    // pair of the wave made every pair run the next window's 4 doublings (5 %
    // of the halves reach 2^127: 80 % of the block kernel's groups). A wave
    // with any m outside [0, 16] runs the windows one by one.
    const uint32_t dw2 = valid ? iv.get(IM_DIG, w_hi - 1, i) : DIG_ZERO;
    const int m = (digit(dw) << QW) + digit(dw2);
    if (!__any(m < 0 || m > 2 * QBIAS)) {
      const int e1 = m < QBIAS ? m : QBIAS, e2 = m - e1;
      fe T;
#pragma unroll
      for (int k = 0; k < 8; ++k) T.v[k] = ql[e1 ? e1 - 1 : 0][k][ln];
      fe_cneg_mask(T, T, negm);
      pair_accumulate_from_inf(P, Z, inf, T, e1 != 0);
      if (__any(e2 != 0)) {
#pragma unroll
        for (int k = 0; k < 8; ++k) T.v[k] = ql[e2 ? e2 - 1 : 0][k][ln];
        fe_cneg_mask(T, T, negm);
        pair_accumulate(P, Z, inf, T, e2 != 0, odd);  // T[8] + T[8] (m = 16): its exact doubling
      }
      w_hi -= 2;
      dbl = true;
      dw = (w_hi >= w_lo && valid) ? iv.get(IM_DIG, w_hi, i) : DIG_ZERO;
    }
  }
#pragma unroll 1
  for (int win = w_hi; win >= w_lo; --win) {
    const int dg = digit(dw);
    const int mg = dg < 0 ? -dg : dg;
    const int ie = mg ? mg - 1 : 0;
    const uint32_t dw_next = (win > w_lo && valid) ? iv.get(IM_DIG, win - 1, i) : DIG_ZERO;
    if (dbl) {
#pragma unroll 1
      for (int d = 0; d < QW; ++d) {
        if (!inf) pair_double(P, Z, odd);
      }
    }
    dbl = true;
    const bool take = dg != 0;
    fe T;
#pragma unroll
    for (int k = 0; k < 8; ++k) T.v[k] = ql[ie][k][ln];
    fe_cneg_mask(T, T, ((uint32_t)(dg >> 31) & odd) ^ negm);  // y -> -y on the odd lane: (dg < 0) != negh
    const bool was_inf = inf;
    pair_accumulate(P, Z, inf, T, take, odd);
    if (__any(take && was_inf)) pair_accumulate_from_inf(P, Z, inf, T, take && was_inf);
    dw = dw_next;
  }
}

// a pair-form chain's sum (X | Y, Z on the odd lane) to LDS: word-major
// [25][sigs] (X, Y, Z, inf), signature slot c
HKV_DEV void pair_publish(uint32_t* __restrict__ xch, int sigs, uint32_t c, const fe& P, const fe& Z, bool inf,
                          uint32_t odd) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (!odd) xch[k * sigs + c] = P.v[k];
    else {
      xch[(8 + k) * sigs + c] = P.v[k];
      xch[(16 + k) * sigs + c] = Z.v[k];
    }
  }
  if (odd) xch[24 * sigs + c] = inf ? 1u : 0u;
}
HKV_DEV void xch_read(const uint32_t* __restrict__ xch, int sigs, uint32_t c, gej& b, bool& binf) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    b.x.v[k] = xch[k * sigs + c];
    b.y.v[k] = xch[(8 + k) * sigs + c];
    b.z.v[k] = xch[(16 + k) * sigs + c];
  }
  binf = xch[24 * sigs + c] != 0;
}

// ---- the roles both small-batch kernels share ----
// An input's tx bytes and prevout script as the block kernel's LDS copy
// (TxCache below): t[off] is byte off of the batch's tx buffer, s[k] byte k
// of the script; null members read HBM.
struct TxView {
  const uint8_t* t;
  const uint8_t* s;
};
// the key words of signature i (record words 24..41; STD: parsed from its
// input, which x receives)
template <bool STD>
HKV_DEV void key_words_of(uint32_t i, uint32_t n, const uint32_t* __restrict__ recs, const StdArgs& sa,
                          uint32_t kw[REC_WORDS], StdIn& x, TxView v = {nullptr, nullptr}, bool key_only = false) {
  if constexpr (STD) {
    std_parse(x, sa.txs, sa.n_tx, sa.txt, sa.scripts, sa.scripts_len, sa.jobs, i, n, sa.forkid, v.t, v.s, key_only);
    std_key_words(kw, x);
  } else {
#pragma unroll
    for (int k = 0; k < REC_WORDS; ++k) kw[k] = (k >= 24 && i < n) ? recs[(size_t)i * REC_WORDS + k] : 0u;
  }
}
// Q' = (x w, w^2) on E_w of signature i's key (G, a dummy, for a key that
// does not parse: the lane's digits are zero)
template <bool STD>
HKV_DEV void key_point(uint32_t i, uint32_t n, const uint32_t* __restrict__ recs, const StdArgs& sa, ge& q,
                       TxView v = {nullptr, nullptr}) {
  uint32_t kw[REC_WORDS];
  StdIn xs = {};
  key_words_of<STD>(i, n, recs, sa, kw, xs, v, true);
  fe w;
  uint32_t pflags;
  const bool pk = pubkey_parse_rec_w(kw, q.x, w, pflags) && i < n;
  fe xw, ww;
  fe_mul(xw, q.x, w);
  fe_sqr(ww, w);
  q.x = xw;
  q.y = ww;
  if (!pk) ge_set_g(q);
}
// The signature wave, first half (lanes with on): range and high-S policy,
// s^-1, u2, the GLV split and Booth digits, r and the flags into im.
template <bool STD>
HKV_DEV void sig_wave_parse(uint32_t i, bool on, uint32_t n, uint32_t mode, SoAView iv,
                            const uint32_t* __restrict__ recs, const StdArgs& sa, StdIn& x, sc& m, sc& sinv,
                            bool& use, uint32_t& flags, TxView v = {nullptr, nullptr}) {
  flags = 0;
  use = false;
  if (!on) return;
  bool ok = i < n, glv_ok, n1, n2;
  uint32_t kw[REC_WORDS];
  key_words_of<STD>(i, n, recs, sa, kw, x, v);
  sc r, s;
  if constexpr (STD) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { r.v[k] = x.r[k]; s.v[k] = x.s[k]; }
    ok = ok && x.ok;
  } else {
    uint32_t w[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) w[k] = i < n ? recs[(size_t)i * REC_WORDS + k] : 0u;
    rec_be256(r.v, w, 32);
    rec_be256(s.v, w, 64);
    rec_be256(m.v, w, 0);
  }
  sig_lane_q(r, s, mode, iv, i, ok, glv_ok, n1, n2, sinv);
  use = ok && glv_ok;
  fe kx, kwv;
  uint32_t pflags = 0;
  const bool pk = pubkey_parse_rec_w(kw, kx, kwv, pflags) && i < n;
  flags = split_flags(ok, (pk ? 1u : 0u) | pflags, glv_ok, n1, n2);
  iv.put(IM_FLAGS, i, flags);
}
// 1e. Mid-size standard-input batches (at most 2 waves per SIMD; the
//     overlapped path of hkv_api.cpp enqueue_std_chunk): std_parse
//     (verifyStdInput's parse half), the prologue, s^-1 and the GLV split in
//     one lane per input (sig_lane_q / sig_lane_g: a per-lane variable-time
//     safegcd instead of the batch trick) at the head of the mid-size ecmult
//     kernel (STDPRO). Nothing here writes the input's record: the hash half
//     (hkv_std_input_kernel, on a second stream from the start) writes it
//     whole, and the finish kernel (LATE) redoes u1 from it after the join; s^-1
//     stays in IM_C for that.
HKV_DEV void std_lane_prologue(uint32_t i, uint32_t n, SoAView iv, const StdArgs& sa) {
  bool glv_ok, n1, n2;
  uint32_t kw[REC_WORDS];
  StdIn x = {};
  key_words_of<true>(i, n, nullptr, sa, kw, x);
  sc r, s, m, sinv;
#pragma unroll
  for (int k = 0; k < 8; ++k) { r.v[k] = x.r[k]; s.v[k] = x.s[k]; m.v[k] = 0; }
  bool ok = i < n && x.ok;
  sig_lane_q(r, s, HKV_MODE_HASKOIN, iv, i, ok, glv_ok, n1, n2, sinv);
  sig_lane_g(m, sinv, ok && glv_ok, iv, i);
  fe kx, kwv;
  uint32_t pflags = 0;
  const bool pk = pubkey_parse_rec_w(kw, kx, kwv, pflags) && i < n;
  iv.put(IM_FLAGS, i, split_flags(ok, (pk ? 1u : 0u) | pflags, glv_ok, n1, n2));
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    iv.put(IM_QX, k, i, kx.v[k]);
    iv.put(IM_W, k, i, kwv.v[k]);
    iv.put(IM_C, k, i, sinv.v[k]);
  }
}

// The signature wave, second half (whole wave: the STD hashes are
// block-synchronous): STD — the script checks, the sighash and the input's
// verify record; then u1 = m / s and A = u1 G into aux.
// SPREAD: the signature inputs are lanes 0..SPREAD-1 and the wave's other
// lanes compute the three BIP143 per-tx hashes side by side (SPREAD = 16);
// 0: each input's lane computes them in turn; -1: another wave has put them
// in r32 + 8 (the block kernel's wave 0, blk_tx_hashes).
template <bool STD, int SPREAD = 0>
HKV_DEV void sig_wave_gsum(uint32_t i, bool on, uint32_t n, SoAView iv, const uint32_t* __restrict__ gtab, SoAView av,
                           uint32_t* __restrict__ recs, const StdArgs& sa, uint32_t* shabuf, StdIn& x, sc m,
                           const sc& sinv, bool use, uint32_t flags) {
  uint32_t stdok = 0;
  if constexpr (STD) {
    uint32_t* r32 = recs + (size_t)(on && i < n ? i : 0) * REC_WORDS;
    if (!on) x.ok = false;
    uint32_t d[8];
    // (r32 is scratch until the record is written: words 0-7 for a BIP143
    // SINGLE hashOutputs, 8-31 for the tx's BIP143 hashes, which the fused
    // launch computes per input instead of an index-kernel pass)
    if constexpr (SPREAD > 0)  // every input that may sign with the BIP143 form
      bip143_tx_hashes_spread(sa.txs, x.row, x.ok && (x.segwit || sa.forkid >= 0), r32 + 8, shabuf, SPREAD, x.T);
    const bool live = std_hash(x, sa.txs, sa.forkid, r32, shabuf, d, r32 + 8, SPREAD != 0);
    if (on) {
      if (i < n) std_write_record(r32, x, live, d);  // the input's verify record (hkv_std_input_kernel's)
      uint32_t w[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) w[k] = !x.ok ? 0u : (live ? d[k] : (k == 0 ? 1u : 0u));
      rec_be256(m.v, w, 0);
      stdok = x.ok ? AUXF_STDOK : 0u;
    }
  }
  if (!on) return;
  sig_lane_g(m, sinv, use, iv, i);
  gej A;
  bool ainf;
  gsum_lane(iv, gtab, i, (flags & FLAG_VALID) != 0, A, ainf);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    av.put(AUX_AX, k, i, A.x.v[k]);
    av.put(AUX_AY, k, i, A.y.v[k]);
    av.put(AUX_AZ, k, i, A.z.v[k]);
  }
  av.put(AUX_FLAGS, i, (ainf ? AUXF_AINF : 0u) | stdok);
}
// The key's y0 = sqrt(w) with the key's y parity, and whether w is a square
template <bool STD>
HKV_DEV void sqrt_lane(uint32_t i, uint32_t n, const uint32_t* __restrict__ recs, const StdArgs& sa, SoAView av,
                       TxView v = {nullptr, nullptr}) {
  uint32_t kw[REC_WORDS];
  StdIn xs = {};
  key_words_of<STD>(i, n, recs, sa, kw, xs, v, true);
  fe x, w, y0, y2, ny;
  uint32_t pflags = 0;
  (void)pubkey_parse_rec_w(kw, x, w, pflags);
  fe_sqrt_cand(y0, w);
  fe_sqr(y2, y0);
  const bool is_sq = fe_equal(y2, w);
  fe_normalize(y0);
  fe_neg(ny, y0);
  fe_normalize(ny);
  if ((y0.v[0] & 1u) != ((pflags & FLAG_YODD) ? 1u : 0u)) y0 = ny;
#pragma unroll
  for (int k = 0; k < 8; ++k) av.put(AUX_Y0, k, i, y0.v[k]);
  av.put(AUX_SQ, i, is_sq ? AUXF_SQ : 0u);
}
// A, y0, the join flags and r of signature i (aux / im)
HKV_DEV void join_inputs(SoACView iv, SoACView av, uint32_t i, gej& A, fe& y0, uint32_t r[8], uint32_t& af,
                         bool& is_sq) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    A.x.v[k] = av.get(AUX_AX, k, i);
    A.y.v[k] = av.get(AUX_AY, k, i);
    A.z.v[k] = av.get(AUX_AZ, k, i);
    y0.v[k] = av.get(AUX_Y0, k, i);
    r[k] = iv.get(IM_R, k, i);
  }
  af = av.get(AUX_FLAGS, i);
  is_sq = av.get(AUX_SQ, i) != 0;
}

// One group of PAIR_SIGS signatures (records base .. base + 31) on the
// workgroup's four waves: the body of hkv_pair_split_kernel, shared with the
// multisig tail kernel (which passes slot-relative im / aux and shifted
// record / verdict pointers, so its scratch is sized by the grid, not the batch).
template <bool STD>
HKV_DEV void pair_group(uint32_t base, uint32_t* __restrict__ im, uint32_t n, uint32_t n_pad,
                        const uint32_t* __restrict__ gtab, uint32_t* __restrict__ bits, uint32_t n_words,
                        uint32_t* __restrict__ aux, uint32_t* __restrict__ recs, uint32_t mode,
                        unsigned long long* __restrict__ clk, const StdArgs& sa, QLane* qlds, HLane* hlds,
                        uint32_t* xch, uint32_t* shabuf) {
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t ln = threadIdx.x & 63;
  const uint32_t odd = (ln & 1u) ? 0xFFFFFFFFu : 0u;
  const bool stamp = clk != nullptr && blockIdx.x == 0 && ln == 0;
  auto mark = [&](int slot) {
    if (stamp) clk[4 + slot] = wall_clock64();
  };
  // (im and aux stay raw pointers in this signature on purpose: the multisig
  // tail hands over slot-relative ones, and the views are built from those)
  const SoAView iv = {im, n_pad}, av = {aux, n_pad};
  if (wv == 2) {
    // ---- the signature: u2 half (lanes 0-31), then the u1 half and A = u1 G ----
    const uint32_t i = base + ln;
    const bool on = ln < PAIR_SIGS;
    uint32_t flags;
    bool use;
    sc sinv, m;
    StdIn x = {};
    sig_wave_parse<STD>(i, on, n, mode, iv, recs, sa, x, m, sinv, use, flags);
    __threadfence_block();
    mark(STAMP_SIG);
    __syncthreads();  // barrier P
    sig_wave_gsum<STD>(i, on, n, iv, gtab, av, recs, sa, shabuf, x, m, sinv, use, flags);
    __threadfence_block();
    mark(STAMP_GSUM);
    __syncthreads();  // barrier A
    __syncthreads();  // barrier B
    return;
  }
  if (wv == 3) {
    // ---- the key's y0 = sqrt(w) with the key's y parity (lanes 0-31) ----
    __syncthreads();  // barrier P (nothing to wait for: the key bytes are input)
    if (ln < PAIR_SIGS) sqrt_lane<STD>(base + ln, n, recs, sa, av);
    __threadfence_block();
    mark(STAMP_SQRT);
    __syncthreads();  // barrier A
    __syncthreads();  // barrier B
    return;
  }

  // ---- chain waves: half = wv (0: k1 * Q', 1: k2 * lambda(Q')) ----
  const int half = wv;
  const uint32_t c = ln >> 1;                    // signature of the pair
  const uint32_t i = base + c;
  ge q;
  key_point<STD>(i, n, recs, sa, q);
  // ---- table: j*Q', j = 1..QTAB_ENTRIES, on the isomorphic curve of scale Zg ----
  fe Zg, Qxy;
  fe_sel(Qxy, q.x, q.y, odd);
  pair_table(Qxy, half, odd, qlds[half], hlds[half], ln, Zg);
  mark(half ? STAMP_TABLE1 : STAMP_TABLE0);
  __syncthreads();  // barrier P: the signature wave's digits, r and flags are in im
  if (half == 0) mark(STAMP_P);
  const uint32_t flags = iv.get(IM_FLAGS, i);
  const bool valid = (i < n) && (flags & FLAG_VALID);
  const bool negh = (flags & (half ? FLAG_NEG2 : FLAG_NEG1)) != 0;

  // ---- the chain: 33 radix-16 windows, pair form ----
  fe P, Z;
  bool inf;
  pair_chain(P, Z, inf, qlds[half], iv, i, valid, negh, half, odd, ln, NWIN - 1, 0);

  mark(half ? STAMP_CHAIN1 : STAMP_CHAIN0);
  // ---- join: half 1's sum to half 0 through LDS ----
  if (half == 1) pair_publish(xch, PAIR_SIGS, c, P, Z, inf, odd);
  fe Y, Zx;
  fe_xch(Y, P);   // even lane: Y of the pair
  fe_xch(Zx, Z);  // even lane: Z of the pair
  __syncthreads();  // barrier A: half 1's sum, A and y0 are published
  if (half == 0) mark(STAMP_A);
  bool accept = false;
  if (half == 0) {  // both lanes compute; the even lane's result is the verdict
    gej acc, b;
    acc.x = P;
    acc.y = Y;
    acc.z = Zx;
    bool binf;
    xch_read(xch, PAIR_SIGS, c, b, binf);
    gej_add_var(acc, inf, b, binf);  // B' = u2 Q' on E_w (iso scale Zg)
    gej A;
    fe y0;
    uint32_t r[8], af;
    bool is_sq;
    join_inputs(iv, av, i, A, y0, r, af, is_sq);
    // B = phi^-1(B') = (X, Y, Z Zg y0) on E, R = A + B exactly, x compare
    gej bb;
    bb.x = acc.x;
    bb.y = acc.y;
    fe zt;
    fe_mul(zt, acc.z, Zg);
    fe_mul(bb.z, zt, y0);
    bool rinf = (af & AUXF_AINF) != 0;
    gej_add_var(A, rinf, bb, inf);
    accept = valid && is_sq && !rinf && x_matches_r(A.x, A.z, r) && (!STD || (af & AUXF_STDOK));
  }
  const uint64_t ball = __ballot(accept && !odd);
  if (half == 0) mark(STAMP_JOIN);
  if (half == 0 && ln == 0) {
    const uint32_t wi = base / 32;
    if (wi < n_words) bits[wi] = even_bits(ball);
  }
  __syncthreads();  // barrier B: the next group's writers of xch / aux wait for the readers
}

template <bool STD>
__global__ void __launch_bounds__(PAIR_TPB, 2) hkv_pair_split_kernel(uint32_t* __restrict__ im, uint32_t n,
                                                                     uint32_t n_pad,
                                                                     const uint32_t* __restrict__ gtab,
                                                                     uint32_t* __restrict__ bits, uint32_t n_words,
                                                                     uint32_t* __restrict__ aux,
                                                                     uint32_t* __restrict__ recs,
                                                                     uint32_t mode,
                                                                     unsigned long long* __restrict__ clk,
                                                                     StdArgs sa) {
  // per chain wave: QTAB_ENTRIES entries x 8 words x 64 lanes (each lane keeps
  // its own coordinate of every entry: x or beta*x on the even lane, y on the odd)
  __shared__ QLane qlds[2];
  __shared__ HLane hlds[2];
  __shared__ uint32_t xch[25 * PAIR_SIGS];
  __shared__ uint32_t shabuf[STD ? 16 * WG : 1];  // std_hash's per-lane SHA-256 blocks ([word][thread])
  // optional phase stamps of workgroup 0 (hkv_profile_phases): constant-rate
  // clock at the phase boundaries of each wave, slot STAMP_*
  if (clk != nullptr && blockIdx.x == 0 && threadIdx.x == 0) clk[4 + STAMP_START] = wall_clock64();
  for (uint32_t base = blockIdx.x * PAIR_SIGS; base < n_pad; base += gridDim.x * PAIR_SIGS)
    pair_group<STD>(base, im, n, n_pad, gtab, bits, n_words, aux, recs, mode, clk, sa, qlds, hlds, xch, shabuf);
}

// ---------------------------------------------------------------------------
// 2d. Block kernel (a block: at most BLK_SIGS signatures per CU). In the
//     pair kernel one signature's chain is the latency: 128 doublings and 33
//     additions of one pair of lanes, started only once the signature is
//     parsed (the digits). Here each chain's radix-16 windows are cut in
//     three segments, each run against the table of its own base point:
//       wave 0: windows 0..K1-1 against the table of Q' (lanes 0-31 k1,
//               lanes 32-63 k2); then S_lo = their sum and T = A + S_lo on E;
//       wave 1: Q1 = 2^(4 K1) Q' and Q2 = 2^(4 K2) Q' by doublings from t = 0
//               (four lanes per signature, quad_double; Q1 is handed to wave
//               3 on the way), then the table of Q2 and windows K2..NWIN-1;
//               then S_hi, R = U + S_hi on E, the x compare, the verdicts;
//       wave 3: the key's y0 = sqrt(w) (lanes 0-15), then the table of Q1 and
//               windows K1..K2-1; then S_mid and U = T + S_mid on E;
//       wave 2: the signature (lanes 0-15), then u1 * G (STD: the hashes,
//               then the multisig scan of the group's inputs).
//     The doublings on wave 1's path stay 128 (the floor for a 128-bit
//     scalar), but only NWIN - K2 of the additions and none of the waits for
//     the signature lie on it; waves 0 and 3 work beside it.
//     16 signatures per workgroup of 4 waves (one per SIMD): a 4,000-input
//     block fills 250 CUs. The hand-offs are LDS flags (release / acquire at
//     workgroup scope) instead of workgroup barriers, so no wave waits at a
//     barrier for a phase it does not need.
// ---------------------------------------------------------------------------
// (17, 27) since the chain waves parse keys without the DER signature (wave
// 1's doublings start 6 us earlier; profiles/r04r_blk_k/summary.txt): was (18, 28)
#ifndef HKV_BLK_K1
#define HKV_BLK_K1 17
#endif
#ifndef HKV_CHAIN_PRIO  // the block kernel's chain waves' issue priority (s_setprio; 0: off)
#define HKV_CHAIN_PRIO 3
#endif
#ifndef HKV_BLK_K2
#define HKV_BLK_K2 27
#endif
#ifndef HKV_BLK_K1_HASHED  // the lo / mid split of a group with BIP143 per-tx hashes on wave 0 (0: BLK_K1)
#define HKV_BLK_K1_HASHED 16
#endif
constexpr int BLK_K1 = HKV_BLK_K1, BLK_K2 = HKV_BLK_K2;
static_assert(HKV_BLK_K1_HASHED == 0 || (HKV_BLK_K1_HASHED >= 2 && HKV_BLK_K1_HASHED < HKV_BLK_K2), "three segments");
static_assert(BLK_K1 >= 2 && BLK_K1 < BLK_K2 && BLK_K2 <= NWIN - 1, "three non-empty segments");
constexpr int BLK_TPB = 256;  // (BLK_SIGS: hkv_layout.h)

// The workgroup's 16 input txs and prevout scripts in LDS (STD): every wave's
// parse of an input (template, pushes, DER, the key) and the signature
// wave's sighash generator read a tx byte by byte through chains of dependent
// loads, which a lone wave pays at HBM latency; all 256 threads copy the
// group's txs (up to TXC_WORDS dwords each, from the dword holding the tx's
// first byte) and scripts once, behind one barrier. A tx or script that does
// not fit is read from HBM as before.
constexpr uint32_t TXC_WORDS = 512;   // 2 KB per input
constexpr uint32_t SPKC_WORDS = 24;   // 96 B per prevout script
struct TxCache {
  uint32_t tx[BLK_SIGS][TXC_WORDS];
  uint32_t spk[BLK_SIGS][SPKC_WORDS];
  long long tx_d[BLK_SIGS];   // (first copied dword's address) - txs; -1 << 62: not copied
  uint32_t spk_b[BLK_SIGS];   // the script's first byte within spk[c]; ~0u: not copied
};
template <bool STD> struct TxCacheOf { using type = TxCache; };
template <> struct TxCacheOf<false> { using type = uint32_t; };
constexpr long long TXC_NONE = -(1ll << 62);

// input c's view (after the barrier that follows txc_fill)
HKV_DEV TxView txc_view(const TxCache& tc, uint32_t c) {
  TxView v;
  const long long d = tc.tx_d[c];
  const uint32_t b = tc.spk_b[c];
  // v.t lies outside the LDS object (only v.t + off, off in the tx, lands in
  // it), so it is formed on the 64-bit flat address as an integer: pointer
  // arithmetic would let the compiler move the subtraction into the 32-bit
  // LDS address space, where it wraps
  const uintptr_t g = reinterpret_cast<uintptr_t>(static_cast<const void*>(&tc.tx[c][0]));
  v.t = d != TXC_NONE ? reinterpret_cast<const uint8_t*>(g - (uintptr_t)d) : nullptr;
  v.s = b != ~0u ? reinterpret_cast<const uint8_t*>(&tc.spk[c][0]) + b : nullptr;
  return v;
}
HKV_DEV void txc_fill(TxCache& tc, const StdArgs& sa, uint32_t base, uint32_t n) {
  const uint32_t c = threadIdx.x >> 4, k = threadIdx.x & 15u;  // 16 threads per input
  const uint32_t jx = base + c;
  uint32_t st = 0, len = 0, so = 0, sl = 0, t = ~0u;
  bool sok = false;
  if (jx < n) {
    const hkv_input_job jb = sa.jobs[jx];
    if (jb.tx < sa.n_tx) {
      if (sa.tx_off != nullptr) {  // the whole wire form; its row is built below
        t = jb.tx;
        st = sa.tx_off[t];
        const uint32_t e = sa.tx_off[t + 1];
        len = e >= st ? e - st : 0u;
      } else {
        const uint32_t* row = sa.txt + (size_t)jb.tx * TXT_WORDS;
        if (row[TXT_FLAGS] & TXF_OK) {
          st = row[TXT_START];
          len = row[TXT_LOCK] + 4u - st;
        }
      }
    }
    sok = jb.script_off <= sa.scripts_len && sa.scripts_len - jb.script_off >= jb.script_len && jb.script_len != 0;
    so = jb.script_off;
    sl = jb.script_len;
  }
  // aligned dwords covering the bytes (each holds at least one byte of the
  // range, so none crosses into a page the range does not touch)
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(sa.txs) + st, pa = p0 & ~(uintptr_t)3;
  const uint32_t nw = (uint32_t)((p0 + len - pa + 3) >> 2);
  const bool tfit = len != 0 && nw <= TXC_WORDS;
  if (tfit) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(pa);
    for (uint32_t j = k; j < nw; j += 16u) tc.tx[c][j] = src[j];
  }
  const uintptr_t q0 = reinterpret_cast<uintptr_t>(sa.scripts) + so, qa = q0 & ~(uintptr_t)3;
  const uint32_t nws = (uint32_t)((q0 + sl - qa + 3) >> 2);
  const bool sfit = sok && nws <= SPKC_WORDS;
  if (sfit) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(qa);
    for (uint32_t j = k; j < nws; j += 16u) tc.spk[c][j] = src[j];
  }
  if (k == 0) {
    tc.tx_d[c] = tfit ? (long long)(pa - reinterpret_cast<uintptr_t>(sa.txs)) : TXC_NONE;
    tc.spk_b[c] = sfit ? (uint32_t)(q0 - qa) : ~0u;
  }
  if (sa.tx_off != nullptr) {
    // the index row of each input's tx (hkv_tx_index_kernel's bounds-checked
    // parse, from the copy when the tx fits), into txt for this group's
    // readers (after the caller's barrier), the multisig scan and the tail
    // kernel; inputs of one tx write the same row
    __syncthreads();
    if (k == 0 && t != ~0u) {
      const TxView v = txc_view(tc, c);
      uint32_t row[8];
      tx_index_row(v.t != nullptr ? v.t : sa.txs, sa.tx_off, t, row);
      uint32_t* w = const_cast<uint32_t*>(sa.txt) + (size_t)t * TXT_WORDS;
#pragma unroll
      for (int q = 0; q < 8; ++q) w[q] = row[q];
    }
  }
}
template <bool STD, class C>
HKV_DEV TxView blk_view(const C& tc, uint32_t c) {
  if constexpr (STD) return txc_view(tc, c);
  else return TxView{nullptr, nullptr};
}
// The three BIP143 per-tx hashes of the group's inputs on one wave (lane
// w 16 + c: hash w of input c's tx, bip143_tx_hashes_spread) into each
// input's record scratch (words 8..31, read by its sighash and overwritten
// by its record). Every input whose tx carries a witness section, or every
// input on a fork-id network, gets them; the sighash uses them only for the
// BIP143 form, which needs a witness tx (or FORKID).
// input i's tx needs the BIP143 per-tx hashes (row: its index row)
HKV_DEV bool blk_needs_tx_hashes(const StdArgs& sa, uint32_t i, uint32_t n, const uint32_t*& row) {
  row = sa.txt;
  if (i >= n) return false;
  const hkv_input_job jb = sa.jobs[i];
  if (jb.tx >= sa.n_tx) return false;
  row = sa.txt + (size_t)jb.tx * TXT_WORDS;
  const uint32_t f = row[TXT_FLAGS];
  return (f & TXF_OK) && ((f & TXF_WITNESS) || sa.forkid >= 0);
}
HKV_DEV void blk_tx_hashes(const StdArgs& sa, const TxCache& tc, uint32_t base, uint32_t n, uint32_t* recs,
                           uint32_t* shabuf) {
  const uint32_t c = (threadIdx.x & 63u) & (BLK_SIGS - 1), i = base + c;
  const uint32_t* row;
  const bool need = blk_needs_tx_hashes(sa, i, n, row);
  bip143_tx_hashes_spread(sa.txs, row, need, recs + (size_t)(i < n ? i : 0u) * REC_WORDS + 8, shabuf, BLK_SIGS,
                          txc_view(tc, c).t);
}
enum : int { BF_SIG = 0, BF_A = 1, BF_Y = 2, BF_T = 3, BF_Q = 4, BF_U = 5, BF_H = 6, BF_COUNT = 7 };
constexpr int STAMP_CHAIN_MID = STAMP_COUNT;  // the twelfth phase slot (hkv_profile_phases reads 12)
// publish: every prior write of the wave (LDS and global) before the flag
HKV_DEV void blk_post(uint32_t* f, uint32_t seq) {
  __threadfence_block();
  __hip_atomic_store(f, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
HKV_DEV void blk_wait(uint32_t* f, uint32_t seq) {
  while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != seq) __builtin_amdgcn_s_sleep(1);
}
// lanes of one wave exchanged data through LDS: the writes before the reads
HKV_DEV void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// A chain wave's two halves (lanes 0-31 k1, 32-63 k2) summed on the k1
// lanes in pair form: S = P (X | Y), Z on both lanes, on the wave's curve
HKV_DEV void halves_sum(uint32_t* xk, uint32_t c, int half, uint32_t odd, fe& P, const fe& Z, bool& inf, fe& Zs) {
  if (half == 1) pair_publish(xk, BLK_SIGS, c, P, Z, inf, odd);
  fe_bc1(Zs, Z);
  wave_lds_sync();
  if (half == 0) {
    gej b;
    bool binf;
    xch_read(xk, BLK_SIGS, c, b, binf);
    fe Pb;
    fe_sel(Pb, b.x, b.y, odd);
    pair_add_var(P, Zs, inf, Pb, b.z, binf, odd);
  }
}
// acc (pair form, on E) += phi^-1 of a segment's sum S (pair form): S is
// Jacobian on E_w at the isomorphic scale zs (its table's Zg times its base
// point's Z), so on E its Z is Zs zs y0
HKV_DEV void add_segment(fe& Pacc, fe& Zacc, bool& ainf, const fe& P, const fe& Zs, bool sinf, const fe& zs,
                         const fe& y0, uint32_t odd) {
  fe zt, zb;
  fe_mul(zt, Zs, zs);
  fe_mul(zb, zt, y0);
  pair_add_var(Pacc, Zacc, ainf, P, zb, sinf, odd);
}
// a pair-form point from / to an LDS exchange slot (X, Y, Z, inf word-major)
HKV_DEV void pair_from_xch(const uint32_t* xk, uint32_t c, uint32_t odd, fe& P, fe& Z, bool& inf) {
  gej b;
  xch_read(xk, BLK_SIGS, c, b, inf);
  fe_sel(P, b.x, b.y, odd);
  Z = b.z;
}
HKV_DEV void pair_to_xch(uint32_t* xk, uint32_t c, uint32_t odd, const fe& P, const fe& Z, bool inf) {
  pair_publish(xk, BLK_SIGS, c, P, Z, inf, odd);  // Z is on both lanes: the odd lane's copy is stored
}

template <bool STD>
__global__ void __launch_bounds__(BLK_TPB, 1) hkv_block_kernel(uint32_t* __restrict__ im, uint32_t n, uint32_t n_pad,
                                                               const uint32_t* __restrict__ gtab,
                                                               uint32_t* __restrict__ qs,
                                                               uint32_t* __restrict__ bits, uint32_t n_words,
                                                               uint32_t* __restrict__ aux,
                                                               uint32_t* __restrict__ recs, uint32_t mode,
                                                               unsigned long long* __restrict__ clk, StdArgs sa) {
  __shared__ QLane qlds[3];                     // the Q' (wave 0), Q2 (wave 1) and Q1 (wave 3) tables
  __shared__ HLane hlds[3];                     // their z-ratios while they are built
  __shared__ uint32_t xch[5][25 * BLK_SIGS];    // k2 -> k1 of waves 0, 1, 3; T (0 -> 3); U (3 -> 1)
  __shared__ uint32_t qpub[3][8][BLK_SIGS];     // Q1 = (X, Y, Z), wave 1 -> wave 3
  __shared__ uint32_t shabuf[STD ? 16 * WG : 1];
  __shared__ uint32_t bflag[BF_COUNT];
  __shared__ typename TxCacheOf<STD>::type tcache;  // STD: the group's txs and scripts
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t ln = threadIdx.x & 63;
  const uint32_t odd = (ln & 1u) ? 0xFFFFFFFFu : 0u;
  const bool stamp = clk != nullptr && blockIdx.x == 0 && ln == 0;
  auto mark = [&](int slot) {
    if (stamp) clk[4 + slot] = wall_clock64();
  };
  const SoAView iv = {im, n_pad}, av = {aux, n_pad};
  if (threadIdx.x < BF_COUNT) bflag[threadIdx.x] = 0;
  if (clk != nullptr && threadIdx.x == 0 && blockIdx.x < 4096) clk[16 + 2 * blockIdx.x] = wall_clock64();
  __syncthreads();
  if (wv == 0) mark(STAMP_START);

  uint32_t seq = 0;
  for (uint32_t base = blockIdx.x * BLK_SIGS; base < n_pad; base += gridDim.x * BLK_SIGS) {
    ++seq;
    if constexpr (STD) {
      txc_fill(tcache, sa, base, n);
      __syncthreads();
    }
    if (wv == 2) {
      const uint32_t i = base + ln;
      const bool on = ln < BLK_SIGS;
      uint32_t flags;
      bool use;
      sc sinv, m;
      StdIn x = {};
      sig_wave_parse<STD>(i, on, n, mode, iv, recs, sa, x, m, sinv, use, flags,
                          blk_view<STD>(tcache, ln & (BLK_SIGS - 1)));
      blk_post(&bflag[BF_SIG], seq);
      mark(STAMP_SIG);
      if constexpr (STD) blk_wait(&bflag[BF_H], seq);  // the BIP143 per-tx hashes (wave 0)
      sig_wave_gsum<STD, (STD ? -1 : BLK_SIGS)>(i, on, n, iv, gtab, av, recs, sa, shabuf, x, m, sinv, use, flags);
      blk_post(&bflag[BF_A], seq);
      mark(STAMP_GSUM);
      // STD: the multisig scan of the group's inputs (off every critical path)
      if constexpr (STD) {
        if (sa.ms_desc != nullptr)
          ms_scan_lane(sa.txs, sa.n_tx, sa.txt, sa.scripts, sa.scripts_len, sa.jobs, i, on && i < n, sa.forkid,
                       sa.ms_desc, sa.ms_off, sa.ms_ctr, shabuf);
      }
      __syncthreads();  // the group's LDS is read before the next group's writes
      continue;
    }
    // ---- chain waves 0, 1, 3: lanes 0-31 k1, 32-63 k2 (two lanes per chain) ----
#if HKV_CHAIN_PRIO
    // the chain waves ahead of the signature wave wherever the CU arbitrates
    // between waves (same box, three runs: configs[0] 246.7 -> 244.5 /
    // 244.6 us, configs[2] 248.7 -> 246.6 / 247.3 us, profiles/r04r_prio/)
    __builtin_amdgcn_s_setprio(HKV_CHAIN_PRIO);
#endif
    // the lo / mid split: a group whose wave 0 runs BIP143 per-tx hashes
    // before its chain (a witness input, or a fork-id network) gives the mid
    // segment one window of the lo segment (HKV_BLK_K1_HASHED)
    int k1 = BLK_K1;
#if HKV_BLK_K1_HASHED
    if constexpr (STD) {
      const uint32_t* row_;
      if (__any(blk_needs_tx_hashes(sa, base + (ln & (BLK_SIGS - 1)), n, row_))) k1 = HKV_BLK_K1_HASHED;
    }
#endif
    const int half = (int)(ln >> 5);
    const uint32_t c = (ln & 31u) >> 1;
    const uint32_t i = base + c;
    const int slot = wv == 3 ? 2 : wv;            // table / exchange slot of the wave
    fe Zg, zb, P, Z;                              // table scale, base point's Z
    if (wv == 0) {
      ge q;
      key_point<STD>(i, n, recs, sa, q, blk_view<STD>(tcache, c));
      fe_sel(P, q.x, q.y, odd);
      fe_set_u32(zb, 1);
      pair_table(P, half, odd, qlds[0], hlds[0], ln, Zg);
      mark(STAMP_TABLE0);
      // STD: the BIP143 per-tx hashes for the signature wave, in the time
      // this wave waits for the digits (the s^-1 the signature wave computes)
      if constexpr (STD) {
        blk_tx_hashes(sa, tcache, base, n, recs, shabuf);
        blk_post(&bflag[BF_H], seq);
      }
    } else if (wv == 1) {
      // Q1, Q2 on four lanes per signature (lanes 4c'..4c'+3: X | Y | Z | .)
      const uint32_t cq = ln >> 2, qd = ln & 3u;
      const uint32_t m0 = qd == 0 ? ~0u : 0u, m1 = qd == 1 ? ~0u : 0u, m2 = qd == 2 ? ~0u : 0u;
      ge q;
      key_point<STD>(base + cq, n, recs, sa, q, blk_view<STD>(tcache, cq));
      fe V;
      fe_set_u32(V, 1);
      fe_sel(V, V, q.y, m1);
      fe_sel(V, V, q.x, m0);  // x | y | 1 | 1
#pragma unroll 1
      for (int d = 0; d < QW * k1; ++d) quad_double(V, m0, m1, m2);
      if (qd < 3) {
#pragma unroll
        for (int k = 0; k < 8; ++k) qpub[qd][k][cq] = V.v[k];
      }
      blk_post(&bflag[BF_Q], seq);
#pragma unroll 1
      for (int d = QW * k1; d < QW * BLK_K2; ++d) quad_double(V, m0, m1, m2);
      // to the chains' pair layout: X2 | Y2 with Z2 on both lanes; (X2, Y2) is
      // an affine point of the isomorphic curve of scale Z2
      const int src_p = (int)(4 * c + (odd ? 1u : 0u)), src_z = (int)(4 * c + 2);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        P.v[k] = (uint32_t)__shfl((int)V.v[k], src_p);
        zb.v[k] = (uint32_t)__shfl((int)V.v[k], src_z);
      }
      pair_table(P, half, odd, qlds[1], hlds[1], ln, Zg);
      mark(STAMP_TABLE1);
    } else {
      if (ln < BLK_SIGS) sqrt_lane<STD>(base + ln, n, recs, sa, av, blk_view<STD>(tcache, ln));
      blk_post(&bflag[BF_Y], seq);
      mark(STAMP_SQRT);
      blk_wait(&bflag[BF_Q], seq);  // Q1 from wave 1
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        P.v[k] = qpub[odd ? 1 : 0][k][c];
        zb.v[k] = qpub[2][k][c];
      }
      pair_table(P, half, odd, qlds[2], hlds[2], ln, Zg);
    }
    blk_wait(&bflag[BF_SIG], seq);  // the digits, r and flags are in im
    if (wv == 0) mark(STAMP_P);
    const uint32_t flags = iv.get(IM_FLAGS, i);
    const bool valid = (i < n) && (flags & FLAG_VALID);
    const bool negh = (flags & (half ? FLAG_NEG2 : FLAG_NEG1)) != 0;
    const int w_hi = wv == 0 ? k1 - 1 : (wv == 1 ? NWIN - 1 : BLK_K2 - 1);
    const int w_lo = wv == 0 ? 0 : (wv == 1 ? BLK_K2 : k1);
    fe zs;  // the segment's isomorphic scale (formed before the chain: off the join's path)
    fe_mul(zs, Zg, zb);
    bool inf;
    pair_chain(P, Z, inf, qlds[slot], iv, i, valid, negh, half, odd, ln, w_hi, w_lo);
    mark(wv == 0 ? STAMP_CHAIN0 : (wv == 1 ? STAMP_CHAIN1 : STAMP_CHAIN_MID));
    fe Zs;
    halves_sum(xch[slot], c, half, odd, P, Z, inf, Zs);  // S = P | Zs on E_w at scale Zg * zb
    if (wv == 0) {
      // ---- T = A + phi^-1(S_lo) on E (A = u1 G, y0 the key's y) ----
      blk_wait(&bflag[BF_A], seq);
      blk_wait(&bflag[BF_Y], seq);
      mark(STAMP_A);
      if (half == 0) {
        gej A;
        fe y0, PA;
        uint32_t r[8], af;
        bool is_sq;
        join_inputs(iv, av, i, A, y0, r, af, is_sq);
        bool tinf = (af & AUXF_AINF) != 0;
        fe_sel(PA, A.x, A.y, odd);
        add_segment(PA, A.z, tinf, P, Zs, inf, zs, y0, odd);
        pair_to_xch(xch[3], c, odd, PA, A.z, tinf);
      }
      blk_post(&bflag[BF_T], seq);
    } else if (wv == 3) {
      // ---- U = T + phi^-1(S_mid) on E ----
      // (S_mid's Z on E is formed before T arrives: y0 was published by this
      // wave before its chain)
      fe zbs;
      if (half == 0) {
        fe y0, zt;
#pragma unroll
        for (int k = 0; k < 8; ++k) y0.v[k] = av.get(AUX_Y0, k, i);
        fe_mul(zt, Zs, zs);
        fe_mul(zbs, zt, y0);
      }
      blk_wait(&bflag[BF_T], seq);
      if (half == 0) {
        fe PT, ZT;
        bool tinf;
        pair_from_xch(xch[3], c, odd, PT, ZT, tinf);
        pair_add_var(PT, ZT, tinf, P, zbs, inf, odd);
        pair_to_xch(xch[4], c, odd, PT, ZT, tinf);
      }
      blk_post(&bflag[BF_U], seq);
    } else {
      // ---- R = U + phi^-1(S_hi) on E, the x compare, the verdicts ----
      // (the join inputs and S_hi's scale on E are formed before U arrives:
      // A and y0 were published long before this chain ended)
      blk_wait(&bflag[BF_A], seq);
      blk_wait(&bflag[BF_Y], seq);
      bool accept = false;
      gej A;
      fe y0, zb;
      uint32_t r[8], af;
      bool is_sq;
      if (half == 0) {
        join_inputs(iv, av, i, A, y0, r, af, is_sq);
        fe zt;
        fe_mul(zt, Zs, zs);
        fe_mul(zb, zt, y0);
      }
      blk_wait(&bflag[BF_U], seq);
      if (half == 0) {
        fe PR, ZR;
        bool rinf;
        pair_from_xch(xch[4], c, odd, PR, ZR, rinf);
        pair_add_var(PR, ZR, rinf, P, zb, inf, odd);
        // the even lane holds X
        accept = valid && is_sq && !rinf && x_matches_r(PR, ZR, r) && (!STD || (af & AUXF_STDOK));
      }
      const uint64_t ball = __ballot(accept && !odd);
      mark(STAMP_JOIN);
      if (ln == 0) {
        const uint32_t wi = base / 32;
        if (wi < n_words) reinterpret_cast<uint16_t*>(bits)[base / BLK_SIGS] = (uint16_t)(even_bits(ball) & 0xFFFFu);
      }
    }
    __syncthreads();  // the group's LDS (tables, exchanges, flags' data) is read before the next group's writes
  }
  if (clk != nullptr && threadIdx.x == 0 && blockIdx.x < 4096) clk[16 + 2 * blockIdx.x + 1] = wall_clock64();
}

// ---------------------------------------------------------------------------
// 2b. y-free finish (full-grid batches). The ecmult kernel leaves
//   B' = u2 * Q' = (X, Y, Z) on E_w : y^2 = x^3 + 7 w^3, Q' = (x w, w^2) =
//   phi(Q) for the isomorphism phi(x, y) = (y0^2 x, y0^3 y), y0 = the key's y,
//   so B = u2 * Q = (X / (Z^2 w), Y y0 / (Z^3 w^2)) is linear in y0. With
//   A = u1 * G = (XA, YA, ZA), the affine sum's x is K1 - K2 y0, and
//   "x(A + B) == r" solves to y0 = num / den with
//     num = Y^2 ZA^6 + YA^2 Z^6 w^3 - H^2 (r T + XA Z^2 w + X ZA^2),
//     den = 2 Y YA Z^3 w ZA^3,  H = X ZA^2 - XA Z^2 w,  T = Z^2 w ZA^2
//   (r + n: num - H^2 n T). The signature verifies against the key iff
//   y_c = num / den is a square root of w with the key's parity — the check
//   also rejects a compressed key whose x^3 + 7 is not a square (no root
//   exists), which the y-free parse leaves open. The rare lanes where the
//   formula does not apply (A or B infinity, A = +-B: H = 0) take an exact
//   slow path with the square root. hkv_finish_kernel computes the u1 * G sum
//   (per-window tables: no doublings) and num, num_{r+n}, den;
//   hkv_yverdict_kernel inverts den by Montgomery's trick over BATCH_INV
//   signatures per lane and writes the verdict bitmap.
// ---------------------------------------------------------------------------
// acc (+inf) += b (+binf), both Jacobian on one curve, exact in every case
HKV_DEV void gej_add_var(gej& acc, bool& inf, const gej& b, bool binf) {
  gej a2;
  fe z2, z3;
  fe_sqr(z2, b.z);
  fe_mul(z3, z2, b.z);
  fe_mul(a2.x, acc.x, z2);
  fe_mul(a2.y, acc.y, z3);
  fe_mul(a2.z, acc.z, b.z);
  bool ainf = inf;
  gej_accumulate(a2, ainf, acc.z, b.x, b.y, !binf && !inf);
  const bool take_b = inf && !binf, keep_a = binf;
  gej_cmov(a2, b, take_b);
  gej_cmov(a2, acc, keep_a);
  acc = a2;
  inf = keep_a ? inf : (take_b ? false : ainf);
}

// x(R) == r (mod p) for Jacobian (X, ., Z): r Z^2 == X, or (r + n) Z^2 == X when r < p - n
HKV_DEV bool x_matches_r(const fe& Xin, const fe& Z, const uint32_t r[8]) {
  fe zz, X = Xin, t, rf;
  fe_sqr(zz, Z);
  fe_normalize(X);
#pragma unroll
  for (int k = 0; k < 8; ++k) rf.v[k] = r[k];
  fe_mul(t, rf, zz);
  fe_normalize(t);
  bool eq = fe_eq_norm(t, X);
  const bool small_r = u256_lt(r, PMN);
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) rf.v[k] = addc(r[k], SC_N[k], c);
  fe_mul(t, rf, zz);
  fe_normalize(t);
  return eq || (small_r && fe_eq_norm(t, X));
}

// (VERDICT_BATCH, the verdict kernel's signatures per lane: hkv_layout.h)
// den^-1: Bernstein-Yang safegcd mod p (hkv_safegcd.h); it replaced the
// Fermat chain (255S + 15M): verdict kernel 160 -> 135 us at 1M
#ifndef HKV_FINISH_WAVES
#define HKV_FINISH_WAVES 3  // waves per SIMD the finish kernel's register allocation targets: 3 (168 VGPRs,
                            // 180 B/lane spilled) is 0.8% faster than 2 (208 VGPRs), 4 (179 VGPRs spilled)
                            // 1-2% slower (profiles/r02_variants_finish_waves.log, r02_variants_yfree.log)
#endif
HKV_DEV void gtab_entry(const uint32_t* __restrict__ gtab, int t, uint32_t gd, fe& tx, fe& ty) {
  const uint32_t mag = gd & GD_MAG;
  const uint4* e = reinterpret_cast<const uint4*>(gtab) + ((size_t)t * GTAB_ENTRIES + (mag ? mag - 1 : 0)) * 4;
  const uint4 a0 = e[0], a1 = e[1], a2 = e[2], a3 = e[3];
  tx.v[0] = a0.x; tx.v[1] = a0.y; tx.v[2] = a0.z; tx.v[3] = a0.w;
  tx.v[4] = a1.x; tx.v[5] = a1.y; tx.v[6] = a1.z; tx.v[7] = a1.w;
  ty.v[0] = a2.x; ty.v[1] = a2.y; ty.v[2] = a2.z; ty.v[3] = a2.w;
  ty.v[4] = a3.x; ty.v[5] = a3.y; ty.v[6] = a3.z; ty.v[7] = a3.w;
}

// A = u1 * G of signature i: one affine addition per window, from the
// per-window tables (no doublings); ILP: the paired-product addition (mid-size
// launches, at most 2 waves per SIMD)
template <bool ILP>
HKV_DEV void gsum_lane(SoACView iv, const uint32_t* __restrict__ gtab, uint32_t i, bool valid, gej& A, bool& ainf) {
  // ---- A = u1 * G: one affine addition per window, table t = 2j + h holds
  // multiples of 2^(GTAB_W j + 128 h) G; the next entry is loaded before
  // the current addition
  // (window 0 starts the sum: A = its entry, affine, without an addition)
  uint32_t gd = valid ? iv.get(IM_GDIG, i) : 0u;
  fe tx, ty;
  gtab_entry(gtab, 0, gd, tx, ty);
  fe_cneg(A.y, ty, (gd & GD_NEG) != 0);
  A.x = tx;
  fe_set_u32(A.z, 1);
  ainf = (gd & GD_MAG) == 0;
  gd = valid ? iv.get(IM_GDIG, 1, i) : 0u;
  gtab_entry(gtab, 1, gd, tx, ty);
#pragma unroll 1
  for (int t = 1; t < 2 * GWIN; ++t) {
    const uint32_t gdn = (t + 1 < 2 * GWIN && valid) ? iv.get(IM_GDIG, t + 1, i) : 0u;
    fe nx, nyy;
    if (t + 1 < 2 * GWIN) gtab_entry(gtab, t + 1, gdn, nx, nyy);
    const bool take = (gd & GD_MAG) != 0;
    fe_cneg(ty, ty, (gd & GD_NEG) != 0);
    const bool was_inf = ainf;
    ec_accumulate<ILP>(A, ainf, A.z, tx, ty, take);
    if (__any(take && was_inf)) gej_accumulate_from_inf(A, ainf, tx, ty, take && was_inf);
    gd = gdn;
    tx = nx;
    ty = nyy;
  }
}

// one signature's finish (hkv_finish_kernel): whole waves call it (the
// rare-lane compaction ballots)
// ILP (mid-size launches, at most 2 waves per SIMD): the paired-product
// forms, independent products interleaved two at a time
// LATE (large standard-input batches): the lane's G digits and validity come
// from its final record first (late_u1_lane; its own digit words, read back
// below by the same lane)
// (im, n_pad and a view built at each use: see the view's header)
template <bool ILP, bool LATE>
HKV_DEV void finish_lane(uint32_t* __restrict__ im, uint32_t n, uint32_t n_pad, const uint32_t* __restrict__ gtab,
                         uint32_t* __restrict__ rare_ctr, uint32_t i0, uint32_t cn, uint32_t i, uint32_t flags,
                         const uint32_t* __restrict__ recs) {
  if constexpr (LATE) {
    if (i < n) flags = late_u1_lane(recs, i, SoAView{im, n_pad}, flags);
  }
  const bool valid = (i < n) && (flags & FLAG_VALID);

  gej A;
  bool ainf;
  gsum_lane<ILP>(SoAView{im, n_pad}, gtab, i, valid, A, ainf);

  // ---- B' from the ecmult kernel, w, r (not hoisted above the loop: it
  // would hold 56 more VGPRs through every addition)
  asm volatile("" ::: "memory");
  gej B;
  fe w;
  uint32_t r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    B.x.v[k] = SoAView{im, n_pad}.get(IM_BX, k, i);
    B.y.v[k] = SoAView{im, n_pad}.get(IM_BY, k, i);
    B.z.v[k] = SoAView{im, n_pad}.get(IM_BZ, k, i);
    w.v[k] = SoAView{im, n_pad}.get(IM_W, k, i);
    r[k] = SoAView{im, n_pad}.get(IM_R, k, i);
  }
  const bool binf = (flags & FLAG_BINF) != 0;

  // ---- num, num_{r+n}, den (formula above), ordered for short live ranges:
  // a = Y ZA^3, b = YA Z^3 give Y^2 ZA^6 = a^2, YA^2 Z^6 = b^2, den = 2 a b w
  fe ZA2, ZA3, Z2, Z3, U1, H, T, S1, HH, t, num, numn, den;
  fe rf, nf;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    rf.v[k] = r[k];
    nf.v[k] = SC_N[k];
  }
  bool hz;
  if constexpr (ILP) {
    fe a, b, t2, t3;
    fe_sqr2(ZA2, A.z, Z2, B.z);
    fe_mul2(ZA3, ZA2, A.z, Z3, Z2, B.z);
    fe_mul2(Z2, Z2, w, U1, B.x, ZA2);      // Z^2 w, X ZA^2
    fe_mul2(t, A.x, Z2, T, Z2, ZA2);       // XA Z^2 w, Z^2 w ZA^2
    fe_sub(H, U1, t);
    hz = fe_is_zero(H);
    fe_add(S1, t, U1);
    fe_sqrmul(HH, H, t, rf, T);
    fe_add(S1, S1, t);                     // r T + XA Z^2 w + X ZA^2
    fe_mul2(a, B.y, ZA3, b, A.y, Z3);
    fe_sqrmul(num, a, den, a, b);          // Y^2 ZA^6, a b
    fe_sqrmul(t, w, den, den, w);          // w^2, a b w
    fe_add(den, den, den);                 // 2 Y YA Z^3 w ZA^3
    fe_sqrmul(b, b, t, t, w);              // YA^2 Z^6, w^3
    fe_mul2(t, t, b, t2, HH, S1);
    fe_add(num, num, t);
    fe_sub(num, num, t2);
    fe_mul(t3, T, nf);
    fe_mul(t3, HH, t3);
    fe_sub(numn, num, t3);                 // the r + n candidate
  } else {
    fe_sqr(ZA2, A.z);
    fe_mul(ZA3, ZA2, A.z);
    fe_sqr(Z2, B.z);
    fe_mul(Z3, Z2, B.z);
    fe_mul(Z2, Z2, w);            // Z^2 w
    fe_mul(U1, B.x, ZA2);         // X ZA^2
    fe_mul(t, A.x, Z2);           // XA Z^2 w
    fe_sub(H, U1, t);
    hz = fe_is_zero(H);
    fe_add(S1, t, U1);
    fe_mul(T, Z2, ZA2);           // Z^2 w ZA^2
    fe_mul(t, rf, T);
    fe_add(S1, S1, t);            // r T + XA Z^2 w + X ZA^2
    fe_sqr(HH, H);
    fe a, b;
    fe_mul(a, B.y, ZA3);
    fe_mul(b, A.y, Z3);
    fe_mul(den, a, b);
    fe_mul(den, den, w);
    fe_add(den, den, den);        // 2 Y YA Z^3 w ZA^3
    fe_sqr(num, a);               // Y^2 ZA^6
    fe_sqr(t, w);
    fe_mul(t, t, w);              // w^3
    fe_sqr(b, b);                 // YA^2 Z^6
    fe_mul(t, t, b);
    fe_add(num, num, t);
    fe_mul(t, HH, S1);
    fe_sub(num, num, t);
    fe_mul(t, T, nf);
    fe_mul(t, HH, t);
    fe_sub(numn, num, t);         // the r + n candidate
  }

  uint32_t fo = flags;
  if (!valid) fo |= FLAG_DECIDED;
  // the formula needs A, B finite and A != +-B; those lanes (adversarial
  // only: u1 = 0, or u1 G = +-u2 Q) keep B' and park A for hkv_rare_kernel
  const bool rare = valid && (ainf || binf || hz);
  // compact the rare lanes' indices (one atomic per wave) so the slow path
  // runs in dense waves: in an adversarial batch ~1-2% of the lanes are rare,
  // which would put one in most waves
  const uint64_t rmask = __ballot(rare);
  if (rmask) {
    uint32_t base = 0;
    const int lead = __builtin_ctzll(rmask);
    if ((int)(threadIdx.x & 63) == lead) base = atomicAdd(rare_ctr, (uint32_t)__popcll(rmask));
    base = __shfl(base, lead);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(rmask >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)rmask, 0u));
    // (the window's rare lanes are listed in its own [i0, i0 + cn) of the row,
    // under its own counter: at most cn of them; the clamp keeps a stale count
    // from a failed earlier call inside the window)
    if (rare && base + rank < cn) SoAView{im, n_pad}.put(IM_RARE_LIST, (size_t)i0 + base + rank, i);
  }
  if (rare) {
    fo |= FLAG_RARE | (ainf ? FLAG_AINF : 0u);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      SoAView{im, n_pad}.put(IM_AX, k, i, A.x.v[k]);
      SoAView{im, n_pad}.put(IM_AY, k, i, A.y.v[k]);
      SoAView{im, n_pad}.put(IM_AZ, k, i, A.z.v[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      SoAView{im, n_pad}.put(IM_NUM, k, i, num.v[k]);
      SoAView{im, n_pad}.put(IM_NUMN, k, i, numn.v[k]);
      SoAView{im, n_pad}.put(IM_DEN, k, i, den.v[k]);
    }
  }
  SoAView{im, n_pad}.put(IM_FLAGS, i, fo);
}

template <bool ILP, bool LATE>
__global__ void __launch_bounds__(WG, ILP ? 2 : HKV_FINISH_WAVES) hkv_finish_kernel(uint32_t* __restrict__ im, uint32_t n,
                                                                                 uint32_t n_pad, uint32_t i0,
                                                                                 uint32_t cn,
                                                                                 const uint32_t* __restrict__ gtab,
                                                                                 uint32_t* __restrict__ rare_ctr,
                                                                                 const uint32_t* __restrict__ recs) {
  // the window [i0, i0 + cn) of the batch (whole waves: cn is a multiple of WG)
  const uint32_t s = blockIdx.x * WG + threadIdx.x;
  if (s >= cn) return;
  const uint32_t i = i0 + s;
  finish_lane<ILP, LATE>(im, n, n_pad, gtab, rare_ctr, i0, cn, i, SoAView{im, n_pad}.get(IM_FLAGS, i), recs);
}

// the exact slow path for the finish kernel's rare lanes: y0 = sqrt(w) of
// the key's parity (no root: the key does not parse), B on E = (X, Y, Z y0)
// (phi^-1 of B'), R = A + B with every degenerate case, the x compare.
// Lane k takes the k-th compacted rare index of the window [i0, i0 + cn)
// (listed from i0 of the row, counted by the window's own word); lanes past
// the count return.
__global__ void __launch_bounds__(WG) hkv_rare_kernel(uint32_t* __restrict__ im, uint32_t n_pad, uint32_t i0,
                                                      uint32_t cn, const uint32_t* __restrict__ rare_ctr) {
  const uint32_t k = blockIdx.x * WG + threadIdx.x;
  if (k >= min(*rare_ctr, cn)) return;
  const SoAView iv = {im, n_pad};
  const uint32_t i = iv.get(IM_RARE_LIST, (size_t)i0 + k);
  const uint32_t flags = iv.get(IM_FLAGS, i);
  const bool rare = true;
  gej A, B;
  fe w;
  uint32_t r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    A.x.v[k] = iv.get(IM_AX, k, i);
    A.y.v[k] = iv.get(IM_AY, k, i);
    A.z.v[k] = iv.get(IM_AZ, k, i);
    B.x.v[k] = iv.get(IM_BX, k, i);
    B.y.v[k] = iv.get(IM_BY, k, i);
    B.z.v[k] = iv.get(IM_BZ, k, i);
    w.v[k] = iv.get(IM_W, k, i);
    r[k] = iv.get(IM_R, k, i);
  }
  fe y0, y2, ny;
  fe_sqrt_cand(y0, w);
  fe_sqr(y2, y0);
  const bool is_sq = fe_equal(y2, w);
  fe_normalize(y0);
  fe_neg(ny, y0);
  fe_normalize(ny);
  if ((y0.v[0] & 1u) != ((flags & FLAG_YODD) ? 1u : 0u)) y0 = ny;
  gej b = B;
  fe_mul(b.z, B.z, y0);
  bool rinf = (flags & FLAG_AINF) != 0;
  gej_add_var(A, rinf, b, (flags & FLAG_BINF) != 0);
  const bool acc_ok = is_sq && !rinf && x_matches_r(A.x, A.z, r);
  if (rare) iv.put(IM_FLAGS, i, flags | FLAG_DECIDED | (acc_ok ? FLAG_ACCEPT : 0u));
}

// verdicts: den^-1 by Montgomery's trick over VERDICT_BATCH signatures per lane
// over the window [i0, i0 + cn) of the batch (signature i = i0 + t + k * stride;
// i0, cn and stride are multiples of WG, so a wave's 64 lanes hold 64
// consecutive signatures and their verdicts leave as one ballot word, and no
// verdict word belongs to two windows)
__global__ void __launch_bounds__(WG) hkv_yverdict_kernel(uint32_t* __restrict__ im, uint32_t n_pad, uint32_t i0,
                                                          uint32_t cn, uint32_t stride, uint32_t* __restrict__ bits,
                                                          uint32_t n_words, uint32_t* __restrict__ rare_ctr) {
  // (im through ld8 / st8 and indexed here: see the view's header)
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t == 0) *rare_ctr = 0;  // re-arm the window's count for the next batch (the rare kernel has read it)
  // (the steps s = t + k * stride are window-relative, below VERDICT_BATCH * stride <= 2^32, and compared with
  // cn before i0 is added: a window at the end of the largest batch does not wrap)
  const uint32_t first = i0 + t;
  // one wave per SIMD at 1M: the loops are load-latency bound, so each
  // iteration's operands are loaded one iteration ahead
  fe c;
  fe_set_u32(c, 1);
  int kn = 0;
  {
    fe d;
    SoACView::ld8(im, n_pad, IM_DEN.off, first, d.v);  // t < stride <= cn
    uint32_t fl = im[(size_t)IM_FLAGS.off * n_pad + first];
#pragma unroll 1
    for (int k = 0; k < VERDICT_BATCH; ++k) {
      const uint32_t s = t + (uint32_t)k * stride;
      if (s >= cn) break;
      const uint32_t i = i0 + s;
      kn = k + 1;
      const uint32_t inext = i + stride;
      fe dn;
      uint32_t fn = 0;
      if (k + 1 < VERDICT_BATCH && s + stride < cn) {
        SoACView::ld8(im, n_pad, IM_DEN.off, inext, dn.v);
        fn = im[(size_t)IM_FLAGS.off * n_pad + inext];
      }
      if (fl & FLAG_DECIDED) fe_set_u32(d, 1);
      fe_mul(c, c, d);
      SoAView::st8(im, n_pad, IM_C.off, i, c.v);
      d = dn;
      fl = fn;
    }
  }
  fe inv;
  fe_normalize(c);  // safegcd wants 0 < c < p
  sgcd::inv_mod_p(inv.v, c.v);
  struct Ops {
    uint32_t f;
    fe prev, d, num, w;
    uint32_t r[8];
  };
  auto load_ops = [&](Ops& o, int k) {
    const uint32_t i = first + (uint32_t)k * stride;
    o.f = im[(size_t)IM_FLAGS.off * n_pad + i];
    if (k > 0) SoACView::ld8(im, n_pad, IM_C.off, i - stride, o.prev.v);
    SoACView::ld8(im, n_pad, IM_DEN.off, i, o.d.v);
    SoACView::ld8(im, n_pad, IM_NUM.off, i, o.num.v);
    SoACView::ld8(im, n_pad, IM_W.off, i, o.w.v);
    SoACView::ld8(im, n_pad, IM_R.off, i, o.r);
  };
  Ops cur;
  if (kn > 0) load_ops(cur, kn - 1);
#pragma unroll 1
  for (int k = kn - 1; k >= 0; --k) {
    const uint32_t i = first + (uint32_t)k * stride;  // < i0 + cn; kn is wave-uniform (cn, stride multiples of 64)
    Ops nxt;
    if (k > 0) load_ops(nxt, k - 1);
    const uint32_t f = cur.f;
    const bool decided = (f & FLAG_DECIDED) != 0;
    fe dinv;
    if (k == 0) fe_set_u32(cur.prev, 1);
    fe_mul(dinv, inv, cur.prev);
    if (decided) fe_set_u32(cur.d, 1);
    fe_mul(inv, inv, cur.d);
    bool accept = (f & FLAG_ACCEPT) != 0;
    if (!decided) {
      fe yc, y2;
      const uint32_t want = (f & FLAG_YODD) ? 1u : 0u;
      fe_mul(yc, cur.num, dinv);
      fe_normalize(yc);
      fe_sqr(y2, yc);
      bool ok = fe_equal(y2, cur.w) && (yc.v[0] & 1u) == want;
      const bool small_r = u256_lt(cur.r, PMN);
      if (__any(!ok && small_r)) {
        fe numn;
        SoACView::ld8(im, n_pad, IM_NUMN.off, i, numn.v);
        fe_mul(yc, numn, dinv);
        fe_normalize(yc);
        fe_sqr(y2, yc);
        ok = ok || (small_r && fe_equal(y2, cur.w) && (yc.v[0] & 1u) == want);
      }
      accept = ok;
    }
    cur = nxt;
    const uint64_t ball = __ballot(accept);
    if ((threadIdx.x & 63) == 0) {
      const uint32_t wi = i / 32;
      if (wi < n_words) bits[wi] = (uint32_t)ball;
      if (wi + 1 < n_words) bits[wi + 1] = (uint32_t)(ball >> 32);
    }
  }
}
// ---------------------------------------------------------------------------
// shared helpers for table init / generators: simple MSB-first double-and-add
// with complete additions (slow, used off the timed path only).
// ---------------------------------------------------------------------------
HKV_DEV void gej_add_affine_complete(gej& acc, bool& inf, const ge& b, bool take) {
  const bool was_inf = inf;
  gej_accumulate(acc, inf, acc.z, b.x, b.y, take);
  gej_accumulate_from_inf(acc, inf, b.x, b.y, take && was_inf);
}
// r = a*G + b*P (either scalar may be zero), affine output; returns false if infinity
HKV_DEV bool ecmult_simple(ge& out, const sc& a, const sc& b, const ge& p) {
  ge g;
  ge_set_g(g);
  gej acc;
  bool inf = true;
  fe_set_zero(acc.x);
  fe_set_zero(acc.y);
  fe_set_zero(acc.z);
  for (int bit = 255; bit >= 0; --bit) {
    if (__any(!inf)) {
      gej d;
      gej_double(d, acc);
      gej_cmov(acc, d, !inf);
    }
    const bool ba = (a.v[bit >> 5] >> (bit & 31)) & 1u;
    const bool bb = (b.v[bit >> 5] >> (bit & 31)) & 1u;
    gej_add_affine_complete(acc, inf, g, ba);
    gej_add_affine_complete(acc, inf, p, bb);
  }
  if (inf) return false;
  fe zi, zi2, zi3;
  fe_inv(zi, acc.z);
  fe_sqr(zi2, zi);
  fe_mul(zi3, zi2, zi);
  fe_mul(out.x, acc.x, zi2);
  fe_mul(out.y, acc.y, zi3);
  fe_normalize(out.x);
  fe_normalize(out.y);
  return true;
}

// 3. fixed-base tables: entry j (1..2^(GTAB_W-1)) of table t = 2 w + h is
//    j * 2^(GTAB_W w + 128 h) G (mod n): tables 0 and 1 are j * G and
//    j * 2^128 G; the y-free finish kernel uses all GTAB_TABLES.
__global__ void __launch_bounds__(WG) hkv_gtable_kernel(uint32_t* __restrict__ gtab) {
  const int tid = blockIdx.x * WG + threadIdx.x;
  if (tid >= GTAB_TABLES * GTAB_ENTRIES) return;
  const int t = tid / GTAB_ENTRIES, j = tid % GTAB_ENTRIES + 1;
  sc a, zero;
#pragma unroll
  for (int k = 0; k < 8; ++k) { a.v[k] = 0; zero.v[k] = 0; }
  // scalar j * 2^(GTAB_W (t / 2) + 128 (t % 2)) mod n: 2^off (off < 256, < n) times j
  {
    const int off = GTAB_W * (t / 2) + 128 * (t % 2);
    sc p2, jj;
#pragma unroll
    for (int k = 0; k < 8; ++k) { p2.v[k] = 0; jj.v[k] = 0; }
    p2.v[off >> 5] = 1u << (off & 31);
    jj.v[0] = (uint32_t)j;
    sc_mul(a, jj, p2);
  }
  ge g, out;
  ge_set_g(g);
  ecmult_simple(out, a, zero, g);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    gtab[tid * 16 + k] = out.x.v[k];
    gtab[tid * 16 + 8 + k] = out.y.v[k];
  }
}

// ---------------------------------------------------------------------------
// 4. synthetic batch generator (keyless construction)
// ---------------------------------------------------------------------------
HKV_DEV uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
HKV_DEV void rand_scalar(sc& r, uint64_t& st) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t v = splitmix64(st);
    r.v[2 * k] = (uint32_t)v;
    r.v[2 * k + 1] = (uint32_t)(v >> 32);
  }
  sc_cond_sub_n(r.v);
  if (u256_is_zero(r.v)) r.v[0] = 1;
}

__global__ void __launch_bounds__(WG) hkv_gen_pool_kernel(uint64_t seed, uint32_t npool,
                                                          uint32_t* __restrict__ pool) {
  const uint32_t j = blockIdx.x * WG + threadIdx.x;
  if (j >= npool) return;
  uint64_t st = seed * 0x2545F4914F6CDD1Dull + j * 0x9E3779B97F4A7C15ull + 0x5851F42D4C957F2Dull;
  sc d, zero;
  rand_scalar(d, st);
#pragma unroll
  for (int k = 0; k < 8; ++k) zero.v[k] = 0;
  ge g, q;
  ge_set_g(g);
  ecmult_simple(q, d, zero, g);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    pool[(size_t)j * 16 + k] = q.x.v[k];
    pool[(size_t)j * 16 + 8 + k] = q.y.v[k];
  }
}

HKV_DEV void put_be256(uint8_t* dst, const uint32_t v[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t x = v[7 - j];
    dst[4 * j + 0] = (uint8_t)(x >> 24);
    dst[4 * j + 1] = (uint8_t)(x >> 16);
    dst[4 * j + 2] = (uint8_t)(x >> 8);
    dst[4 * j + 3] = (uint8_t)x;
  }
}

// Valid (msg32, r, s, Q) without a secret key: R = aG + bQ, r = R.x mod n,
// s = r/b, msg = a*s; low-S by s -> n-s (verifies with -R, same x).
// Record i of the launch is record index0 + i of the batch (seed): its random
// stream depends on the batch index only, so a rank that generates records
// [lo, hi) with index0 = lo writes exactly that slice of the one global batch
// (bench.py's configs[4] leg; oracle/hkv_oracle.c hkvo_gen_batch restates it).
// invalid_permille of the records are then mutated into one of five classes
// that reject in both modes (GEN_CLS_*); labels (optional, ballot words, bit i
// = record index0 + i verifies) are the construction labels.
enum : uint32_t { GEN_CLS_MSG = 0, GEN_CLS_R = 1, GEN_CLS_S = 2, GEN_CLS_KEY = 3, GEN_CLS_NEGKEY = 4, GEN_NCLS = 5 };
__global__ void __launch_bounds__(WG) hkv_gen_records_kernel(uint64_t seed, uint64_t index0, uint32_t n,
                                                             const uint32_t* __restrict__ pool,
                                                             uint32_t npool, uint32_t unc_permille,
                                                             uint32_t invalid_permille,
                                                             uint8_t* __restrict__ recs,
                                                             uint32_t* __restrict__ labels) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  bool label = false;
  if (i < n) {
    const uint64_t g = index0 + i;
    uint64_t st = seed * 0xD1B54A32D192ED03ull + g * 0x9E3779B97F4A7C15ull + 0x8CB92BA72F3D8DD7ull;
    sc a, b;
    rand_scalar(a, st);
    rand_scalar(b, st);
    const uint64_t pick = splitmix64(st);
    const uint32_t j = (uint32_t)(pick % npool);
    const bool unc = ((pick >> 40) % 1000u) < unc_permille;
    ge q, R;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      q.x.v[k] = pool[(size_t)j * 16 + k];
      q.y.v[k] = pool[(size_t)j * 16 + 8 + k];
    }
    ecmult_simple(R, a, b, q);
    sc r, s, bi, m;
#pragma unroll
    for (int k = 0; k < 8; ++k) r.v[k] = R.x.v[k];
    sc_cond_sub_n(r.v);
    sc_inv(bi, b);
    sc_mul(s, r, bi);
    sc_mul(m, a, s);                 // msg = a*s BEFORE the low-S flip:
    if (sc_is_high(s)) sc_neg(s, s);  // (m, r, -s) verifies with -R (same x)
    // the mutation draw comes after every draw of the valid record, so a
    // batch with invalid_permille = 0 is the plain generator's batch
    uint64_t mut = 0;
    bool bad = false;
    uint32_t cls = 0, bit = 0;
    if (invalid_permille) {
      mut = splitmix64(st);
      bad = (mut % 1000u) < invalid_permille;
      cls = (uint32_t)((mut >> 16) % GEN_NCLS);
      bit = (uint32_t)(mut >> 32) & 255u;
      if (bad && cls == GEN_CLS_KEY && npool > 1) {  // another key of the pool
        const uint32_t j2 = (j + 1u + (uint32_t)((mut >> 40) % (npool - 1u))) % npool;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          q.x.v[k] = pool[(size_t)j2 * 16 + k];
          q.y.v[k] = pool[(size_t)j2 * 16 + 8 + k];
        }
      }
      if (bad && cls == GEN_CLS_KEY && npool <= 1) cls = GEN_CLS_MSG;
      if (bad && cls == GEN_CLS_NEGKEY) {  // -Q: y -> p - y (compressed keys: the other prefix)
        fe ny;
        fe_neg(ny, q.y);
        fe_normalize(ny);
        q.y = ny;
      }
    }
    label = !bad;
    uint8_t* o = recs + (size_t)i * REC_SIZE;
    put_be256(o, m.v);
    put_be256(o + 32, r.v);
    put_be256(o + 64, s.v);
    o[96] = unc ? 65 : 33;
    if (unc) {
      o[97] = 4;
      put_be256(o + 98, q.x.v);
      put_be256(o + 130, q.y.v);
    } else {
      o[97] = (uint8_t)(2u | (q.y.v[0] & 1u));
      put_be256(o + 98, q.x.v);
      for (int k = 130; k < 162; ++k) o[k] = 0;
    }
    for (int k = 162; k < REC_SIZE; ++k) o[k] = 0;
    // a bit of msg32, r or s (big-endian byte bit / 8, bit bit % 8): msg and
    // r then fail x(R) == r, r or s may overflow n; an s flip cannot land on
    // n - s, so high-S normalisation (HASKOIN) does not rescue it either
    if (bad && cls <= GEN_CLS_S) o[32u * cls + (bit >> 3)] ^= (uint8_t)(1u << (bit & 7u));
  }
  if (labels != nullptr) {
    const uint64_t ball = __ballot(label);
    if ((threadIdx.x & 63) == 0 && i < n) {  // ceil(n / 64) * 2 words
      const uint32_t wi = i / 32;
      labels[wi] = (uint32_t)ball;
      labels[wi + 1] = (uint32_t)(ball >> 32);
    }
  }
}

// Block-mix generator hooks (bench.py configs[2], tests): random keys with
// their compressed pubkey and HASH160, and ECDSA signatures of given msg32s.
__global__ void __launch_bounds__(WG) hkv_gen_keys_kernel(uint64_t seed, uint32_t n, uint8_t* __restrict__ priv,
                                                          uint8_t* __restrict__ pub, uint8_t* __restrict__ h160) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  uint64_t st = seed * 0x9FB21C651E98DF25ull + (uint64_t)i * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull;
  sc d, zero;
  rand_scalar(d, st);
#pragma unroll
  for (int k = 0; k < 8; ++k) zero.v[k] = 0;
  ge g, q;
  ge_set_g(g);
  ecmult_simple(q, d, zero, g);
  put_be256(priv + (size_t)i * 32, d.v);
  uint8_t* pk = pub + (size_t)i * 33;
  pk[0] = (uint8_t)(2u | (q.y.v[0] & 1u));
  put_be256(pk + 1, q.x.v);
  // HASH160 = RIPEMD160(SHA256(pk)): one SHA-256 block of 33 bytes
  uint32_t w[16], h[8], rip[5];
  w[0] = ((uint32_t)pk[0] << 24) | (q.x.v[7] >> 8);
#pragma unroll
  for (int k = 1; k < 8; ++k) w[k] = (q.x.v[8 - k] << 24) | (q.x.v[7 - k] >> 8);
  w[8] = (q.x.v[0] << 24) | 0x800000u;
#pragma unroll
  for (int k = 9; k < 15; ++k) w[k] = 0;
  w[15] = 33 * 8;
  sha256_init(h);
  sha256_compress(h, w);
  ripemd160_of_digest(rip, h);
  uint8_t* o = h160 + (size_t)i * 20;
#pragma unroll
  for (int k = 0; k < 20; ++k) o[k] = (uint8_t)(rip[k >> 2] >> (8 * (k & 3)));
}

__global__ void __launch_bounds__(WG) hkv_gen_sign_kernel(uint64_t seed, uint32_t n, const uint8_t* __restrict__ priv,
                                                          const uint32_t* __restrict__ key_idx,
                                                          const uint8_t* __restrict__ msg, uint32_t msg_stride,
                                                          uint8_t* __restrict__ sig) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  uint64_t st = seed * 0xC2B2AE3D27D4EB4Full + (uint64_t)i * 0x9E3779B97F4A7C15ull + 0x165667B19E3779F9ull;
  const uint32_t kidx = key_idx ? key_idx[i] : i;
  sc d, m, k, zero, r, s, t, ki;
  const uint8_t* dp = priv + (size_t)kidx * 32;
  const uint8_t* mp = msg + (size_t)i * msg_stride;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    d.v[7 - q] = ((uint32_t)dp[4 * q] << 24) | ((uint32_t)dp[4 * q + 1] << 16) | ((uint32_t)dp[4 * q + 2] << 8) |
                 dp[4 * q + 3];
    m.v[7 - q] = ((uint32_t)mp[4 * q] << 24) | ((uint32_t)mp[4 * q + 1] << 16) | ((uint32_t)mp[4 * q + 2] << 8) |
                 mp[4 * q + 3];
    zero.v[q] = 0;
  }
  sc_cond_sub_n(m.v);
  rand_scalar(k, st);
  ge g, R;
  ge_set_g(g);
  ecmult_simple(R, k, zero, g);
#pragma unroll
  for (int q = 0; q < 8; ++q) r.v[q] = R.x.v[q];
  sc_cond_sub_n(r.v);
  sc_mul(t, r, d);
  sc_add(t, t, m);
  sc_inv(ki, k);
  sc_mul(s, ki, t);
  if (sc_is_high(s)) sc_neg(s, s);
  put_be256(sig + (size_t)i * 64, r.v);
  put_be256(sig + (size_t)i * 64 + 32, s.v);
}

// ---------------------------------------------------------------------------
// debug / known-answer kernel for the tests (field, scalar, GLV ops)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(WG) hkv_debug_kernel(uint32_t op, uint32_t n, const uint32_t* __restrict__ a,
                                                       const uint32_t* __restrict__ b,
                                                       uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  fe x, y, z;
  sc u, v, wres;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    x.v[k] = a[i * 8 + k];
    y.v[k] = b[i * 8 + k];
    u.v[k] = x.v[k];
    v.v[k] = y.v[k];
  }
  uint32_t res[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) res[k] = 0;
  // the third operands: row (i + 1) mod n
  const uint32_t inext = (i + 1 == n) ? 0u : i + 1;
  auto load_next = [&](fe& r, const uint32_t* __restrict__ src) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r.v[k] = src[inext * 8 + k];
  };
  auto raw_norm = [&](fe& r) {  // raw | normalised
#pragma unroll
    for (int k = 0; k < 8; ++k) res[k] = r.v[k];
    fe_normalize(r);
#pragma unroll
    for (int k = 0; k < 8; ++k) res[8 + k] = r.v[k];
  };
  auto norm_raw = [&](fe& r) {  // normalised | raw (ops 1..4)
#pragma unroll
    for (int k = 0; k < 8; ++k) res[8 + k] = r.v[k];
    fe_normalize(r);
#pragma unroll
    for (int k = 0; k < 8; ++k) res[k] = r.v[k];
  };
  auto norm_pair = [&](fe& r1, fe& r2) {
    fe_normalize(r1);
    fe_normalize(r2);
#pragma unroll
    for (int k = 0; k < 8; ++k) { res[k] = r1.v[k]; res[8 + k] = r2.v[k]; }
  };
  switch (op) {
    case HKV_DBG_FE_MUL: fe_mul<true>(z, x, y); norm_raw(z); break;
    case HKV_DBG_FE_SQR: fe_sqr<true>(z, x); norm_raw(z); break;
    case HKV_DBG_FE_ADD: fe_add(z, x, y); norm_raw(z); break;
    case HKV_DBG_FE_SUB: fe_sub(z, x, y); norm_raw(z); break;
    case HKV_DBG_FE_INV: fe_inv(z, x); fe_normalize(z); for (int k = 0; k < 8; ++k) res[k] = z.v[k]; break;
    case HKV_DBG_FE_SQRT: fe_sqrt_cand(z, x); fe_normalize(z); for (int k = 0; k < 8; ++k) res[k] = z.v[k]; break;
    case HKV_DBG_SC_MUL: sc_mul(wres, u, v); for (int k = 0; k < 8; ++k) res[k] = wres.v[k]; break;
    case HKV_DBG_SC_INV: sc_inv(wres, u); for (int k = 0; k < 8; ++k) res[k] = wres.v[k]; break;
    case HKV_DBG_GLV: {
      uint32_t k1[5], k2[5];
      bool n1, n2;
      const bool okk = glv_split(u, k1, n1, k2, n2);
      for (int k = 0; k < 5; ++k) { res[k] = k1[k]; res[5 + k] = k2[k]; }
      res[10] = (n1 ? 1u : 0u) | (n2 ? 2u : 0u) | (okk ? 0u : 4u);
      break;
    }
    case HKV_DBG_ECMULT_G: {  // x-only affine of u*G (+ y)
      ge g, o;
      sc zero;
      for (int k = 0; k < 8; ++k) zero.v[k] = 0;
      ge_set_g(g);
      const bool okk = ecmult_simple(o, u, zero, g);
      for (int k = 0; k < 8; ++k) { res[k] = o.x.v[k]; res[8 + k] = o.y.v[k]; }
      if (!okk) res[15] ^= 0xFFFFFFFFu;
      break;
    }
    case HKV_DBG_MUL512: mul512(res, x.v, y.v); break;
    case HKV_DBG_SQR512: sqr512(res, x.v); break;
    case HKV_DBG_FE_CNEG: fe_cneg(z, x, (y.v[0] & 1u) != 0); raw_norm(z); break;
    case HKV_DBG_FE_CNEG_MASK: fe_cneg_mask(z, x, 0u - (y.v[0] & 1u)); raw_norm(z); break;
    case HKV_DBG_FE_NEG: fe_neg(z, x); raw_norm(z); break;
    case HKV_DBG_FE_HALF: fe_half(z, x); raw_norm(z); break;
    case HKV_DBG_FE_SHL: {
      const uint32_t s = y.v[0];
      if (s == 1u) fe_shl(z, x, 1);
      else fe_shl(z, x, (int)s);
      raw_norm(z);
      break;
    }
    case HKV_DBG_FE_SHL_VAR: fe_shl_var(z, x, y.v[0]); raw_norm(z); break;
    case HKV_DBG_FE_MUL_SMALL: fe_mul_small(z, x, y.v[0]); raw_norm(z); break;
    case HKV_DBG_FE_MUL_SMALL2: {
      fe xn, z2;
      load_next(xn, a);
      fe_mul_small2(z, x, y.v[0], z2, xn, y.v[1]);
      norm_pair(z, z2);
      break;
    }
    case HKV_DBG_FE_LIN2: {
      const uint32_t kk = b[inext * 8];
      fe_lin2(z, x, kk & 0xFFu, y, (kk >> 8) & 0xFFu);
      raw_norm(z);
      break;
    }
    case HKV_DBG_FE_MUL_ADD: {
      fe xn;
      load_next(xn, a);
      fe_mul_add<true>(z, x, y, xn);
      raw_norm(z);
      break;
    }
    case HKV_DBG_FE_MUL2: {
      fe xn, yn, z2;
      load_next(xn, a);
      load_next(yn, b);
      fe_mul2(z, x, y, z2, xn, yn);
      norm_pair(z, z2);
      break;
    }
    case HKV_DBG_FE_SQR2: {
      fe z2;
      fe_sqr2(z, x, z2, y);
      norm_pair(z, z2);
      break;
    }
    case HKV_DBG_FE_SQRMUL: {
      fe xn, z2;
      load_next(xn, a);
      fe_sqrmul(z, x, z2, y, xn);
      norm_pair(z, z2);
      break;
    }
    case HKV_DBG_FE_MUL_REF: fe_mul_ref(z, x, y); raw_norm(z); break;
    case HKV_DBG_FE_SQR_REF: fe_sqr_ref(z, x); raw_norm(z); break;
    case HKV_DBG_FE_NORMALIZE: z = x; fe_normalize(z); for (int k = 0; k < 8; ++k) res[k] = z.v[k]; break;
    case HKV_DBG_FE_IS_ZERO: res[0] = fe_is_zero(x) ? 1u : 0u; break;
    case HKV_DBG_FE_EQUAL: res[0] = fe_equal(x, y) ? 1u : 0u; break;
    case HKV_DBG_U256_LT_P: res[0] = u256_lt_p(x.v) ? 1u : 0u; break;
    case HKV_DBG_SC_ADD: sc_add(wres, u, v); for (int k = 0; k < 8; ++k) res[k] = wres.v[k]; break;
    case HKV_DBG_SC_SUB: sc_sub(wres, u, v); for (int k = 0; k < 8; ++k) res[k] = wres.v[k]; break;
    case HKV_DBG_SC_NEG: sc_neg(wres, u); for (int k = 0; k < 8; ++k) res[k] = wres.v[k]; break;
    case HKV_DBG_SC_SQR: sc_sqr(wres, u); for (int k = 0; k < 8; ++k) res[k] = wres.v[k]; break;
    case HKV_DBG_SC_IS_HIGH: res[0] = sc_is_high(u) ? 1u : 0u; break;
    case HKV_DBG_INV_MOD_P: sgcd::inv_mod_p(res, x.v); break;
    case HKV_DBG_FE_MUL_SUM:
    case HKV_DBG_FE_MUL_SUM_RA:
    case HKV_DBG_FE_MUL_SUM_RB:
    case HKV_DBG_FE_MUL_SUM_RD: {
      fe xn, yn;
      load_next(xn, a);
      load_next(yn, b);
      if (op == HKV_DBG_FE_MUL_SUM_RA) { fe_mul_sum<true>(x, x, y, xn, yn); z = x; }
      else if (op == HKV_DBG_FE_MUL_SUM_RB) { fe_mul_sum<true>(y, x, y, xn, yn); z = y; }
      else if (op == HKV_DBG_FE_MUL_SUM_RD) { fe_mul_sum<true>(yn, x, y, xn, yn); z = yn; }
      else fe_mul_sum<true>(z, x, y, xn, yn);
      raw_norm(z);
      break;
    }
    case HKV_DBG_FE_SQRMUL_SUM:
    case HKV_DBG_FE_SQRMUL_SUM_RA:
    case HKV_DBG_FE_SQRMUL_SUM_RD: {
      fe xn;
      load_next(xn, a);
      if (op == HKV_DBG_FE_SQRMUL_SUM_RA) { fe_sqrmul_sum<true>(x, x, y, xn); z = x; }
      else if (op == HKV_DBG_FE_SQRMUL_SUM_RD) { fe_sqrmul_sum<true>(xn, x, y, xn); z = xn; }
      else fe_sqrmul_sum<true>(z, x, y, xn);
      raw_norm(z);
      break;
    }
    case HKV_DBG_FE_NEG_COMPL: fe_neg_compl(z, x); raw_norm(z); break;
    case HKV_DBG_FC_MUL:
    case HKV_DBG_FC_SQR:
    case HKV_DBG_FC_MUL_ADD:
    case HKV_DBG_FC_MUL_SUM:
    case HKV_DBG_FC_SQRMUL_SUM:
    case HKV_DBG_FC_MUL_MASK: {
      fe xn, yn;
      load_next(xn, a);
      load_next(yn, b);
      uint64_t T = 0, rare;
      if (op == HKV_DBG_FC_SQR) rare = sqr256_red_ps_fc(z.v, T, x.v, x.v);
      else if (op == HKV_DBG_FC_MUL_ADD) rare = mul256_red_add_ps_fc(z.v, T, x.v, y.v, xn.v);
      else if (op == HKV_DBG_FC_MUL_SUM) rare = mul256_red_sum_ps_fc(z.v, T, x.v, y.v, xn.v, yn.v);
      else if (op == HKV_DBG_FC_SQRMUL_SUM) rare = sqrmul256_red_sum_ps_fc(z.v, T, x.v, y.v, xn.v);
      else rare = mul256_red_ps_fc(z.v, T, x.v, y.v);
      if (op == HKV_DBG_FC_MUL_MASK) {
        res[0] = (uint32_t)rare;
        res[1] = (uint32_t)(rare >> 32);
        break;
      }
      for (int k = 0; k < 8; ++k) res[k] = z.v[k];
      res[8] = (uint32_t)T;
      res[9] = (uint32_t)(T >> 32);
      res[10] = (uint32_t)(rare >> (threadIdx.x & 63u)) & 1u;
      break;
    }
    case HKV_DBG_JOINT_RECODE: {
      __shared__ uint32_t jd[JD_WORDS][WG];
      uint32_t S1[5], S2[5], dig[NWIN];
      for (int k = 0; k < 5; ++k) { S1[k] = x.v[k]; S2[k] = y.v[k]; }
      uint32_t p1 = 0, p2 = 0;  // (write_qdigits' digits, kept in registers)
#pragma unroll
      for (int w = 0; w < NWIN; ++w) {
        constexpr uint32_t QM = (1u << QW) - 1u;
        const uint32_t v1 = p1 | ((S1[0] & QM) << 1), v2 = p2 | ((S2[0] & QM) << 1);
        p1 = (S1[0] >> (QW - 1)) & 1u;
        p2 = (S2[0] >> (QW - 1)) & 1u;
        shr_bits<5>(S1, QW);
        shr_bits<5>(S2, QW);
        const int d1 = (int)((v1 + 1u) >> 1) - (int)((v1 >> QW) << QW);
        const int d2 = (int)((v2 + 1u) >> 1) - (int)((v2 >> QW) << QW);
        dig[w] = (uint32_t)(d1 + QBIAS) | ((uint32_t)(d2 + QBIAS) << QDIG_BITS);
      }
      joint_digits_lane(jd, (x.v[5] & 1u) | ((y.v[5] & 1u) << 1), [&](int w) { return dig[w]; });
      for (int k = 0; k < JD_WORDS; ++k) res[k] = jd[k][threadIdx.x];
      break;
    }
    case HKV_DBG_JOINT_TABLE: {
      __shared__ JqLds park;
      uint32_t tab[(QTAB_QUADS + QTAB_ZG_QUADS) * 4];  // the lane's table and Zg slot: n_lanes = 1, lane 0
      ge g, q;
      sc zero;
      for (int k = 0; k < 8; ++k) zero.v[k] = 0;
      ge_set_g(g);
      if (y.v[1] != 0u) {  // a is the key's x: Q' as the table launch forms it (lane_q)
        fe w;
        fe_sqr(w, x);
        fe_mul(w, w, x);
        fe_set_u32(z, 7);
        fe_add(w, w, z);
        fe_mul(q.x, x, w);
        fe_sqr(q.y, w);
      } else if (!ecmult_simple(q, u, zero, g)) {
        q = g;
      }
      fe Zg, zi, zi2, t;
      qtable_build_joint(q, tab, 1u, 0u, reinterpret_cast<uint4*>(tab) + QTAB_QUADS, &park, Zg);
      if ((y.v[0] & 15u) == 15u) {
        fe_normalize(Zg);
        for (int k = 0; k < 8; ++k) res[k] = Zg.v[k];
        break;
      }
      const int j = (int)(y.v[0] & 15u) < JD_ENTRIES ? (int)(y.v[0] & 15u) : 0;
      jq_load(tab, 1u, 0u, j, 0, x);
      jq_load(tab, 1u, 0u, j, 2, z);
      fe_inv(zi, Zg);
      fe_sqr(zi2, zi);
      fe_mul(x, x, zi2);
      fe_mul(t, zi2, zi);
      fe_mul(z, z, t);
      norm_pair(x, z);
      break;
    }
    default: break;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) out[i * 16 + k] = res[k];
}

// The group ops of the known-answer hook (hkv_internal.h): lane i takes rows
// 2i and 2i + 1 of a (k1 | z1) and b (k2 | w), builds P1 = k1 G, P2 = k2 G with
// ecmult_simple, lifts P1 to (x z1^2, y z1^3, z1), applies the op and returns
// the affine result in out row 2i, the infinity flag in out row 2i + 1.
__global__ void __launch_bounds__(WG) hkv_debug_group_kernel(uint32_t op, uint32_t lanes,
                                                             const uint32_t* __restrict__ a,
                                                             const uint32_t* __restrict__ b,
                                                             uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= lanes) return;
  sc k1, k2, zero;
  fe z1, w;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    k1.v[k] = a[(2 * i) * 8 + k];
    z1.v[k] = a[(2 * i + 1) * 8 + k];
    k2.v[k] = b[(2 * i) * 8 + k];
    w.v[k] = b[(2 * i + 1) * 8 + k];
    zero.v[k] = 0;
  }
  const uint32_t sel = w.v[0];
  const bool take = (sel & 1u) != 0;
  ge g, p1, p2, o;
  ge_set_g(g);
  fe_set_zero(o.x);
  fe_set_zero(o.y);
  bool oinf = false;
  uint32_t flag = 0;
  if (op == HKV_DBG_X_MATCHES_R) {
    fe X, zz, xin;
#pragma unroll
    for (int k = 0; k < 8; ++k) xin.v[k] = k1.v[k];
    fe_sqr(zz, z1);
    fe_mul(X, xin, zz);
    o.x.v[0] = x_matches_r(X, z1, k2.v) ? 1u : 0u;
  } else if (op == HKV_DBG_ECMULT) {
    sc kp;
#pragma unroll
    for (int k = 0; k < 8; ++k) kp.v[k] = z1.v[k];
    p1 = g;
    const bool pok = ecmult_simple(p2, kp, zero, g);  // P (never infinity: the tests pass kp != 0)
    if (!pok) p2 = g;
    oinf = !ecmult_simple(p1, k1, k2, p2);
    if (!oinf) o = p1;
  } else {
    p1 = g;
    p2 = g;
    ge t;
    const bool ok1 = ecmult_simple(t, k1, zero, g);
    if (ok1) p1 = t;
    const bool ok2 = ecmult_simple(t, k2, zero, g);
    if (ok2) p2 = t;
    gej acc;
    fe zz, zzz;
    fe_sqr(zz, z1);
    fe_mul(zzz, zz, z1);
    fe_mul(acc.x, p1.x, zz);
    fe_mul(acc.y, p1.y, zzz);
    acc.z = z1;
    bool inf = !ok1 || (sel & 2u) != 0;
    switch (op) {
      case HKV_DBG_GEJ_DOUBLE: gej_double<true>(acc, acc); break;
      case HKV_DBG_GEJ_DOUBLE_ILP: gej_double_ilp(acc, acc); break;
      case HKV_DBG_GEJ_ACCUMULATE: gej_accumulate<true>(acc, inf, acc.z, p2.x, p2.y, take); break;
      case HKV_DBG_GEJ_ACCUMULATE_ILP: gej_accumulate_ilp(acc, inf, acc.z, p2.x, p2.y, take); break;
      case HKV_DBG_GEJ_ADD_AFFINE_COMPLETE: gej_add_affine_complete(acc, inf, p2, take); break;
      case HKV_DBG_GEJ_ADD_VAR: {
        gej bj;
        fe_sqr(zz, w);
        fe_mul(zzz, zz, w);
        fe_mul(bj.x, p2.x, zz);
        fe_mul(bj.y, p2.y, zzz);
        bj.z = w;
        gej_add_var(acc, inf, bj, !ok2 || (sel & 4u) != 0);
        break;
      }
      default: break;
    }
    oinf = inf;
    if (!inf) {
      fe zi, zi2, zi3;
      fe_inv(zi, acc.z);
      fe_sqr(zi2, zi);
      fe_mul(zi3, zi2, zi);
      fe_mul(o.x, acc.x, zi2);
      fe_mul(o.y, acc.y, zi3);
      fe_normalize(o.x);
      fe_normalize(o.y);
    }
  }
  flag = oinf ? 1u : 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    out[(2 * i) * 16 + k] = oinf ? 0u : o.x.v[k];
    out[(2 * i) * 16 + 8 + k] = oinf ? 0u : o.y.v[k];
  }
  out[(2 * i + 1) * 16] = flag;
#pragma unroll
  for (int k = 1; k < 16; ++k) out[(2 * i + 1) * 16 + k] = 0;
}

}  // namespace hkv

namespace hkv {

// ---------------------------------------------------------------------------
// 2e. The multisig tail (hkv_verify_std_inputs*: bare / P2SH / P2WSH /
//     P2SH-P2WSH CHECKMULTISIG inputs). The scan (hkv_ms_scan_kernel, or the
//     block kernel's signature wave) leaves every multisig input's desc words,
//     its record ranges and the batch total (candidates | key checks << 32)
//     on the device. This one launch follows it on the stream, so the host
//     never reads the total: with no multisig input every workgroup returns
//     at once; otherwise, in four phases,
//       1. (fused paths, whose index pass hashed nothing) the BIP143 per-tx
//          hashes of the batch's txs into their index rows;
//       2. per input, its key-check records and, per signature, its sighash
//          and candidate records (hkv_sighash_dev.h ms_emit_lane);
//       3. the key checks (secp256k1_ec_pubkey_parse) and the candidate
//          verifies — the pair-form group of the small-batch kernel
//          (pair_group), one group of 32 candidates per workgroup at a time,
//          on slot-relative scratch sized by the grid;
//       4. per input, haskoin's countMulSig over its candidate verdicts
//          (ms_resolve_lane), ORed into the batch's verdict words.
//     The phases run as one ordered work queue, not as grid barriers: the
//     launch's items (phase 1's hash chunks, then phase 2's record chunks,
//     then phase 3's key-check chunks and candidate groups, then phase 4's
//     walk chunks) are claimed in that order by a device counter, and a
//     workgroup starts an item only once every item of the phase before has
//     completed (one running count of completed items: since no item starts
//     before the phase before it has completed, "count >= the phase's first
//     item index" says exactly that). A workgroup waits only when no earlier
//     item is left to claim, i.e. for items other workgroups are running — so
//     progress never depends on a workgroup that is not resident, and the
//     launch needs no co-residency (a cooperative launch, which guarantees
//     it, cost ~23 us per call on the block path: profiles/r05a/coop_ab.txt).
//     The wait is bounded anyway (~seconds, far above one item): a workgroup
//     that gives up leaves the verdicts it owns at 0 (reject, never a false
//     accept) and reports HKV_STATUS_TAIL_FAULT through the device's sticky
//     latch and the call's status word. Each call counts in its own queue
//     slot and scan sum (the parity of its tail epoch) and its tail zeroes
//     the other pair for the next call, so nothing a faulted launch leaves
//     behind reaches a later one. (The tail inside the block kernel instead —
//     groups claimed from the queue, the tail's items after them — saved this
//     launch but cost ~15 us per block: profiles/r05e/fused_tail_ab.txt.)
//
//     Records in rounds: the candidate and key-check records live in two
//     fixed windows (win_cand / win_keys records, host-sized to a budget,
//     hkv_api.cpp MS_WIN_*), not in buffers sized by the 16-of-16 bound, so
//     phases 2 and 3 run once per round r over records
//     [r * win, (r + 1) * win) of the scan's allocation: the emit writes
//     only the records in the round's windows (hashing only the signatures
//     with one there), the verifies read them and write their verdict bits
//     at the global index. Phase 4 reads every round's bits. A round has
//     items only for the records it holds (none for an empty window; the
//     last group's valid slots end at the round's end): the queue's
//     arithmetic is hkv_tail_plan.h, walked item by item on the CPU against
//     a model of these buffers by tests/tail_plan.cpp.
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
enum : uint32_t { TQ_CLAIM = 0, TQ_DONE = 1, TQ_SLOT = 8 };  // slot words: claim, done (completed items)
// wait (thread 0) until `done` reaches `want`; false on a timeout (fault reported).
// The test hook (force_fault) gives up at every phase transition without
// looking at the count: a launch with any multisig input has items of at
// least three phases, so some workgroup claims an item whose phase it has not
// seen complete and the fault is raised whatever the scheduling
HKV_DEV bool tail_wait(const MsTail& a, unsigned int* done, uint32_t want) {
  uint32_t spins = 0;
  while (a.force_fault || __hip_atomic_load(done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < want) {
    if (a.force_fault || spins++ >= (1u << 24)) {
      atomicOr(a.fault, 1u);
      if (a.status) atomicOr(a.status, (uint32_t)HKV_STATUS_TAIL_FAULT);
      return false;
    }
    __builtin_amdgcn_s_sleep(8);
  }
  return true;
}
// an item's writes published, then its count: every wave waits for its own
// stores (a barrier does not), then one agent-scope release (the XCD's L2
// write-back) with the count
HKV_DEV void publish_count(unsigned int* ctr) {
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(PAIR_TPB, 1) hkv_ms_tail_kernel(MsTail a) {
  __shared__ QLane qlds[2];
  __shared__ HLane hlds[2];
  __shared__ uint32_t xch[25 * PAIR_SIGS];
  __shared__ uint32_t buf[16 * PAIR_TPB];  // sha256_stream blocks ([word][thread])
  __shared__ TailItem item_s;  // the claimed item (thread 0's tail_item)
  __shared__ uint32_t go_s;
  // this launch's queue slot and scan sum (zeroed by the launch before this
  // one on the device's ordered stream of calls); workgroup 0 zeroes the
  // other slot and sum, the next launch's
  unsigned int* q = a.bar + (a.epoch & 1u) * TQ_SLOT;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    unsigned int* nx = a.bar + ((a.epoch + 1u) & 1u) * TQ_SLOT;
#pragma unroll
    for (int k = 0; k < (int)TQ_SLOT; ++k) __hip_atomic_store(&nx[k], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.total_next, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the scan's sum: final (the scan ran before this launch on the stream)
  const unsigned long long total = __hip_atomic_load(a.total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t n_cand = (uint32_t)total, n_keys = (uint32_t)(total >> 32);
  if (n_keys == 0) return;  // no multisig input (every input has >= 1 key): uniform over the grid
  const uint32_t T = PAIR_TPB;
  // the queue's items, rounds and ranges: hkv_tail_plan.h, and nothing here
  // (windows: multiples of 64, >= 64)
  const uint32_t n1 = (a.hash_txs != TX_HASHES_NONE) ? (3 * a.n_tx + T - 1) / T : 0;  // hash chunks
  const TailPlan plan = tail_plan(a.n, n1, n_cand, n_keys, a.win_cand, a.win_keys, T, PAIR_SIGS);
  const uint32_t slots = gridDim.x * PAIR_SIGS, sbase = blockIdx.x * PAIR_SIGS;
  const StdArgs none{};
  uint32_t seen = 0;  // the first item index of the latest phase known complete before it (this workgroup's view)
  for (;;) {
    if (threadIdx.x == 0) {
      const uint32_t it = atomicAdd(&q[TQ_CLAIM], 1u);
      uint32_t ok = it < plan.e4 ? 1u : 0u;
      // x.start, the first item of this item's phase: every item before it
      // must have completed (items are claimed in phase order, so only
      // running items can be outstanding)
      if (ok) {
        const TailItem x = tail_item(plan, it);
        if (x.start > seen) {
          ok = tail_wait(a, &q[TQ_DONE], x.start) ? 1u : 0u;
          if (ok) seen = x.start;
        }
        item_s = x;
      }
      go_s = ok;
    }
    __syncthreads();
    const TailItem x = item_s;
    const uint32_t go = go_s;
    __syncthreads();
    if (!go) return;
    if (x.kind == TAIL_HASH) {
      // 1. the BIP143 per-tx hashes (lanes hash-major, so a wave mostly
      //    shares its hash). Every tx of the batch is hashed, and the block
      //    kernel built index rows only for the txs its inputs reference (a
      //    block's coinbase has none), so each lane re-derives its tx's row
      //    from the offsets — a stale row of an earlier call would point the
      //    hash outside the tx — and writes back only the hash words.
      const uint32_t t_ = x.idx * T + threadIdx.x;
      bool go1 = t_ < 3 * a.n_tx;
      const uint32_t t = go1 ? t_ % a.n_tx : 0, which = go1 ? t_ / a.n_tx : 0;
      uint32_t row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (go1) tx_index_row(a.txs, a.tx_off, t, row);
      if (go1 && a.hash_txs == TX_HASHES_WITNESS) go1 = (row[TXT_FLAGS] & TXF_WITNESS) != 0;
      tx_hash_word_lane(a.txs, row, a.txt + (size_t)t * TXT_WORDS, which, go1, buf);
    } else if (x.kind == TAIL_EMIT) {
      // 2. key-check and candidate records of the round's windows (global
      //    record indices from x.cw0 / x.kw0)
      const uint32_t jx = x.idx * T + threadIdx.x;
      ms_emit_lane(a.txs, a.n_tx, a.txt, a.scripts, a.scripts_len, a.jobs, jx, jx < a.n, a.forkid, a.desc, a.off,
                   a.cand, a.keyrec, x.cw0, plan.Wc, x.kw0, plan.Wk, buf);
    } else if (x.kind == TAIL_KEYS) {
      // 3a. a chunk of the round's key checks (bits at the global index)
      key_check_lane(reinterpret_cast<const uint32_t*>(a.keyrec), x.first + threadIdx.x, x.end, a.kbits, x.kw0);
    } else if (x.kind == TAIL_CAND) {
      // 3b. a pair-form group of 32 of the round's candidates on this
      //     workgroup's own scratch slots [sbase, sbase + 32): pair_group
      //     indexes records and verdict words by slot, so both are handed
      //     over shifted — the verdict words by base - sbase (base = the
      //     group's global index), the records by base - cw0 - sbase (their
      //     place in the window) — which is negative when the group lies
      //     below the slot (a queue hands any group to any workgroup):
      //     formed on the 64-bit address as an integer, never as an
      //     out-of-range pointer, and every access lands at a record and a
      //     verdict word of the group
      const int64_t shift = (int64_t)x.base - (int64_t)sbase;  // a multiple of 32
      const int64_t rshift = shift - (int64_t)x.cw0;
      uint32_t* recs = reinterpret_cast<uint32_t*>(reinterpret_cast<uintptr_t>(a.cand) +
                                                   (uintptr_t)(rshift * (int64_t)(REC_WORDS * 4)));
      uint32_t* bits = reinterpret_cast<uint32_t*>(reinterpret_cast<uintptr_t>(a.cbits) +
                                                   (uintptr_t)(shift / 32 * 4));
      // slot sbase + i is record base + i: valid iff i < x.valid (1..32: the
      // plan has no group past the round's end)
      pair_group<false>(sbase, a.im, sbase + x.valid, slots, a.gtab, bits, 0xFFFFFFFFu, a.aux, recs,
                        HKV_MODE_HASKOIN, nullptr, none, qlds, hlds, xch, buf);
    } else {
      // 4. the countMulSig walk
      const uint32_t jx = x.idx * T + threadIdx.x;
      ms_resolve_lane(a.desc, a.off, jx, jx < a.n, a.cbits, a.kbits, a.out_bits);
    }
    publish_count(&q[TQ_DONE]);
  }
}


}  // namespace hkv

// ---------------------------------------------------------------------------
// launch wrappers (called by hkv_api.cpp). Which kernels a batch runs, their
// grids and strides are decided in hkv_launch_plan.h: the wrappers of a
// verify switch on the plan's shape and choose nothing themselves.
// ---------------------------------------------------------------------------
namespace hkv {

static inline uint32_t ceil_div(size_t a, uint32_t b) { return (uint32_t)((a + b - 1) / b); }

hipError_t launch_prologue(const RecPlan& p, const RecOps& r, hipStream_t st) {
  hipLaunchKernelGGL(hkv_prologue_kernel, dim3(ceil_div(p.n_pad, WG)), dim3(WG), 0, st, (const uint32_t*)r.recs, r.n,
                     p.n_pad, r.mode, r.im);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hkv_inv_kernel, dim3(ceil_div(p.inv_stride, WG)), dim3(WG), 0, st, p.n_pad, p.inv_stride, r.im);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hkv_glv_kernel, dim3(ceil_div(p.n_pad, WG)), dim3(WG), 0, st, p.n_pad, r.im);
  return hipGetLastError();
}
// TableChain (2a): the table and chain launches of part k of the plan (a
// multiple of WG signatures), its tables and Zg slots in the part's slot of qs
hipError_t launch_table_chain(const RecPlan& p, const RecOps& r, uint32_t k, hipStream_t st) {
  if (p.shape != Shape::TableChain || k >= p.n_parts) return hipErrorInvalidValue;
  const uint32_t i0 = p.part(k).i0, cn = p.part(k).cn, slot = p.qs_slots == 2 ? RecPlan::part_slot(k) : 0u;
  if (cn < (uint32_t)WG || cn % WG != 0) return hipErrorInvalidValue;
  uint32_t* qs = r.qs + p.slot_quads(slot) * 4;
  hipLaunchKernelGGL(hkv_qtable_kernel, dim3(cn / WG), dim3(WG), 0, st, (const uint32_t*)r.im, r.n, p.n_pad, i0, cn, qs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hkv_chain_kernel, dim3(cn / WG), dim3(WG), 0, st, r.im, r.n, p.n_pad, i0, cn, (const uint32_t*)qs,
                     i0 == 0 ? r.clk : nullptr);
  return hipGetLastError();
}
static StdArgs std_args(const StdOps& o) {
  return StdArgs{o.txs, o.n_tx, o.txt, o.scripts, o.scripts_len, o.jobs, o.forkid, nullptr, nullptr, nullptr, nullptr};
}
// (the standard-input instance of the mid-size kernel: defined below
// launch_gtable, so that this file's first uses of the kernel templates, which
// order their instances in the code object, stay in the order they had)
static hipError_t launch_mid_std(const RecPlan& p, const RecOps& r, const StdOps& o, hipStream_t st);
hipError_t launch_ecmult(const RecPlan& p, const RecOps& r, const StdOps* std_pro, hipStream_t st) {
  if (std_pro != nullptr && p.shape != Shape::Mid) return hipErrorInvalidValue;  // (the lane prologue is a mid-size form)
  uint32_t* rw = const_cast<uint32_t*>((const uint32_t*)r.recs);
  switch (p.shape) {
    case Shape::Block:  // (record batches: no std operands)
      hipLaunchKernelGGL(hkv_block_kernel<false>, dim3(p.grid), dim3(BLK_TPB), 0, st, r.im, r.n, p.n_pad, r.gtab, r.qs,
                         r.bits, r.n_words, r.aux, rw, r.mode, r.clk, StdArgs{});
      break;
    case Shape::Pair:
      hipLaunchKernelGGL(hkv_pair_split_kernel<false>, dim3(p.grid), dim3(PAIR_TPB), 0, st, r.im, r.n, p.n_pad, r.gtab,
                         r.bits, r.n_words, r.aux, rw, r.mode, r.clk, StdArgs{});
      break;
    case Shape::Mid:
      if (std_pro != nullptr) return launch_mid_std(p, r, *std_pro, st);
      hipLaunchKernelGGL((hkv_ecmult_kernel<true, false>), dim3(p.grid), dim3(WG), 0, st, r.im, r.n, p.n_pad, r.qs,
                         r.clk, StdArgs{});
      break;
    default: return hipErrorInvalidValue;  // (TableChain: launch_table_chain, part by part)
  }
  return hipGetLastError();
}
// Block and Pair chunks of standard inputs: parse, the Q chains, the script
// checks, the sighash and the verdict in one launch (hkv_block_kernel<true> or
// hkv_pair_split_kernel<true>, which reads the batch's prebuilt tx index rows)
hipError_t launch_std_verify_split(const StdPlan& p, const StdOps& o, const RecOps& r, const MsScan* ms,
                                   const uint32_t* tx_off, hipStream_t st) {
  StdArgs sa = std_args(o);
  uint32_t* rw = const_cast<uint32_t*>((const uint32_t*)r.recs);
  switch (p.shape) {
    case Shape::Block:
      if (ms != nullptr) {
        sa.ms_desc = ms->desc;
        sa.ms_off = ms->off;
        sa.ms_ctr = reinterpret_cast<unsigned long long*>(ms->counters);
      }
      sa.tx_off = tx_off;  // the block kernel builds its own rows
      hipLaunchKernelGGL(hkv_block_kernel<true>, dim3(p.n_pad / BLK_SIGS), dim3(BLK_TPB), 0, st, r.im, r.n, p.n_pad,
                         r.gtab, r.qs, r.bits, r.n_words, r.aux, rw, (uint32_t)HKV_MODE_HASKOIN, r.clk, sa);
      break;
    case Shape::Pair:
      if (tx_off != nullptr) return hipErrorInvalidValue;  // the pair kernel reads prebuilt rows
      hipLaunchKernelGGL(hkv_pair_split_kernel<true>, dim3(p.n_pad / PAIR_SIGS), dim3(PAIR_TPB), 0, st, r.im, r.n,
                         p.n_pad, r.gtab, r.bits, r.n_words, r.aux, rw, (uint32_t)HKV_MODE_HASKOIN, r.clk, sa);
      break;
    default: return hipErrorInvalidValue;  // (larger chunks: the extraction, then launch_ecmult)
  }
  return hipGetLastError();
}
uint32_t ms_tail_slots(uint32_t n_cu) { return n_cu * PAIR_SIGS; }
hipError_t launch_ms_tail(const MsTail& a, uint32_t grid, hipStream_t st) {
  hipLaunchKernelGGL(hkv_ms_tail_kernel, dim3(grid), dim3(PAIR_TPB), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_gtable(uint32_t* gtab, hipStream_t st) {
  hipLaunchKernelGGL(hkv_gtable_kernel, dim3(ceil_div((size_t)GTAB_TABLES * GTAB_ENTRIES, WG)), dim3(WG), 0, st,
                     gtab);
  return hipGetLastError();
}
static hipError_t launch_mid_std(const RecPlan& p, const RecOps& r, const StdOps& o, hipStream_t st) {
  hipLaunchKernelGGL((hkv_ecmult_kernel<true, true>), dim3(p.grid), dim3(WG), 0, st, r.im, r.n, p.n_pad, r.qs, r.clk,
                     std_args(o));
  return hipGetLastError();
}
hipError_t launch_finish(const RecPlan& p, const RecOps& r, RecChunk w, uint32_t* rare_ctr, const void* late_recs,
                         hipStream_t st) {
  if (p.shape != Shape::Mid && p.shape != Shape::TableChain) return hipErrorInvalidValue;
  const uint32_t i0 = w.i0, cn = w.cn;
  if (cn < (uint32_t)WG || cn % WG != 0 || i0 % WG != 0 || (uint64_t)i0 + cn > p.n_pad) return hipErrorInvalidValue;
  const bool paired = p.shape == Shape::Mid;  // (the paired-product instance)
  const uint32_t* lr = static_cast<const uint32_t*>(late_recs);
  const dim3 g(cn / WG), b(WG);
  if (paired && lr)
    hipLaunchKernelGGL((hkv_finish_kernel<true, true>), g, b, 0, st, r.im, r.n, p.n_pad, i0, cn, r.gtab, rare_ctr, lr);
  else if (paired)
    hipLaunchKernelGGL((hkv_finish_kernel<true, false>), g, b, 0, st, r.im, r.n, p.n_pad, i0, cn, r.gtab, rare_ctr, lr);
  else if (lr)
    hipLaunchKernelGGL((hkv_finish_kernel<false, true>), g, b, 0, st, r.im, r.n, p.n_pad, i0, cn, r.gtab, rare_ctr, lr);
  else
    hipLaunchKernelGGL((hkv_finish_kernel<false, false>), g, b, 0, st, r.im, r.n, p.n_pad, i0, cn, r.gtab, rare_ctr, lr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hkv_rare_kernel, g, b, 0, st, r.im, p.n_pad, i0, cn, (const uint32_t*)rare_ctr);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint32_t stride = verdict_stride_of(cn);  // (the whole batch as one window: p.verdict_stride)
  hipLaunchKernelGGL(hkv_yverdict_kernel, dim3(stride / WG), b, 0, st, r.im, p.n_pad, i0, cn, stride, r.bits,
                     r.n_words, rare_ctr);
  return hipGetLastError();
}
hipError_t launch_gen_pool(uint64_t seed, uint32_t npool, uint32_t* pool, hipStream_t st) {
  hipLaunchKernelGGL(hkv_gen_pool_kernel, dim3(ceil_div(npool, WG)), dim3(WG), 0, st, seed, npool, pool);
  return hipGetLastError();
}
hipError_t launch_gen_records(uint64_t seed, uint64_t index0, uint32_t n, const uint32_t* pool, uint32_t npool,
                              uint32_t unc_permille, uint32_t invalid_permille, void* recs, uint32_t* labels,
                              hipStream_t st) {
  hipLaunchKernelGGL(hkv_gen_records_kernel, dim3(ceil_div(n, WG)), dim3(WG), 0, st, seed, index0, n, pool, npool,
                     unc_permille, invalid_permille, (uint8_t*)recs, labels);
  return hipGetLastError();
}
hipError_t launch_debug(uint32_t op, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* out,
                        hipStream_t st) {
  if (op >= HKV_DBG_GEJ_DOUBLE) {  // two rows per lane
    if (n < 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hkv_debug_group_kernel, dim3(ceil_div(n / 2, WG)), dim3(WG), 0, st, op, n / 2, a, b, out);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(hkv_debug_kernel, dim3(ceil_div(n, WG)), dim3(WG), 0, st, op, n, a, b, out);
  return hipGetLastError();
}
hipError_t launch_gen_keys(uint64_t seed, uint32_t n, uint8_t* priv, uint8_t* pub, uint8_t* h160, hipStream_t st) {
  hipLaunchKernelGGL(hkv_gen_keys_kernel, dim3(ceil_div(n, WG)), dim3(WG), 0, st, seed, n, priv, pub, h160);
  return hipGetLastError();
}
hipError_t launch_gen_sign(uint64_t seed, uint32_t n, const uint8_t* priv, const uint32_t* key_idx,
                           const uint8_t* msg, uint32_t msg_stride, uint8_t* sig, hipStream_t st) {
  hipLaunchKernelGGL(hkv_gen_sign_kernel, dim3(ceil_div(n, WG)), dim3(WG), 0, st, seed, n, priv, key_idx, msg,
                     msg_stride, sig);
  return hipGetLastError();
}
// The resident grid (Geometry::grid_max = blocks per CU x CUs) sets the
// plan's thresholds between the shapes (hkv_launch_plan.h).
// It is defined by the 4-wave allocation of the full-grid chain, 128 VGPRs:
// HKV_ECMULT_WAVES blocks of 4 waves per CU. The query only confirms that
// the chain kernel reaches it; a chain kernel that could hold more (fewer
// registers) must not move the thresholds, so the answer is capped.
hipError_t ecmult_max_blocks_per_cu(int* out) {
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(out, hkv_chain_kernel, WG, 0);
  if (e == hipSuccess && *out > HKV_ECMULT_WAVES) *out = HKV_ECMULT_WAVES;
  return e;
}

}  // namespace hkv
