// hkv_chainctx.h — the chain-context rule of hkv_chain_context_device: what
// haskoin-core connectBlocks [dep] checks of a header against its actual
// ancestors (median time past, the future-time limit, nextWorkRequired with
// the 2016-block retarget and the testnet minimum-difficulty walk,
// validVersion, checkpoints) and the accumulated chain work, for the device
// (hkv_chainctx.hip) and, compiled as plain C++, for the host test
// (tests/chainctx_host.cpp). Nothing here touches a HIP builtin, and no
// register array is indexed by a run-time value (every such access is an
// unrolled select), so the device build needs no scratch.
//
// The rule (include/hkv.h states it in full). Header i of a batch has height
// H = height0 + i; its parent P is header i - 1, or the context's tip.
//   mtp[i]   element c / 2 of the ascending sort of the c = min(11, i +
//            n_prev_times) timestamps before header i (unsigned compare)
//   want[i]  Bitcoin's GetNextWorkRequired: bits(P) off a period boundary
//            (or, with CHAIN_MIN_DIFFICULTY, the limit after a gap above
//            min_diff_spacing and real(P) otherwise); at a boundary the
//            retarget of target(P) by the period's clamped time span, in exact
//            integers, capped at pow_limit (bits(P) with CHAIN_NO_RETARGET)
//   work[i]  parent_work + the sum of floor(2^256 / (target + 1)) up to i,
//            mod 2^256; a negative, overflowing or zero compact adds 0
//   flags    CHN_* below
// BCH's EDA / DAA / ASERT difficulty rules are not here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef HKV_DEV
#if defined(__HIPCC__)
#define HKV_DEV __device__ __forceinline__
#else
#define HKV_DEV inline
#endif
#endif

// the two functions the C ABI also runs on the host (the limit's compact form)
#if defined(__HIPCC__)
#define HKV_HOST_DEV __host__ __device__ __forceinline__
#else
#define HKV_HOST_DEV inline
#endif

namespace hkv {

// HKV_CHN_* and HKV_CHAIN_* of include/hkv.h
constexpr uint32_t CHN_TIME_OK = 0x01, CHN_NOT_FUTURE = 0x02, CHN_BITS_OK = 0x04, CHN_VERSION_OK = 0x08,
                   CHN_CHECKPOINT_OK = 0x10, CHN_ALL = 0x1F;
constexpr uint32_t CHAIN_NO_RETARGET = 1u, CHAIN_MIN_DIFFICULTY = 2u;
constexpr uint32_t CHAIN_MTP_SPAN = 11;        // timestamps in a full median window
constexpr uint64_t CHAIN_FUTURE_LIMIT = 7200;  // seconds a header's time may lie past `now`
constexpr uint32_t CHAIN_TILE = 256;           // headers per workgroup: the unit of the two scans
constexpr uint32_t CHAIN_TILE_WORDS = 10;      // a tile's scan element: 8 work limbs, the real-bits value, its defined flag
constexpr uint32_t CHAIN_MAX_TIMESPAN = 1u << 30;  // 4 * target_timespan fits 32 bits below it
constexpr uint32_t CHAIN_CP_NONE = 0xFFFFFFFFu;

// decode flags
constexpr uint32_t CC_NEGATIVE = 1u, CC_OVERFLOW = 2u, CC_ZERO = 4u;

// hkv_chain_ctx with the two 256-bit numbers as limbs and the limit's compact
// form worked out once on the host
struct ChainCtx {
  uint32_t height0;
  uint32_t n_prev_times;
  uint32_t prev_times[CHAIN_MTP_SPAN];
  uint32_t parent_bits;
  uint32_t period_first_time;
  uint32_t period_real_bits;
  uint32_t parent_work[8];
  uint64_t now;
  uint32_t pow_limit[8];
  uint32_t limit_bits;
  uint32_t interval;
  uint32_t target_timespan;
  uint32_t min_diff_spacing;
  uint32_t bip34_height, bip66_height, bip65_height;
  uint32_t flags;
};

// scratch of n headers, in 32-bit words: time, bits and version of every
// header, then per tile the tile's scan element and its exclusive prefix
inline size_t chain_tiles(size_t n) { return (n + CHAIN_TILE - 1) / CHAIN_TILE; }
inline size_t chain_scratch_words(size_t n) { return 3 * n + 2 * CHAIN_TILE_WORDS * chain_tiles(n); }

// decodeCompact: the magnitude as 8 little-endian limbs where it fits
HKV_DEV uint32_t cc_decode_compact(uint32_t bits, uint32_t t[8]) {
  const uint32_t size = bits >> 24;
  const uint32_t w0 = bits & 0x007FFFFFu;
  const uint32_t word = size <= 3 ? (w0 >> (8 * (3 - size))) : w0;
  uint32_t fl = 0;
  if (word != 0 && (bits & 0x00800000u)) fl |= CC_NEGATIVE;
  if (word != 0 && (size > 34 || (word > 0xFFu && size > 33) || (word > 0xFFFFu && size > 32))) fl |= CC_OVERFLOW;
  if (word == 0) fl |= CC_ZERO;
  const uint32_t s = size > 3 ? 8u * (size - 3u) : 0u;
  const uint64_t v = (uint64_t)word << (s & 31u);
  const uint32_t li = s >> 5;
  for (uint32_t j = 0; j < 8; ++j) t[j] = (j == li) ? (uint32_t)v : (j == li + 1) ? (uint32_t)(v >> 32) : 0u;
  return fl;
}

HKV_HOST_DEV uint32_t cc_bit_length(const uint32_t t[8]) {
  uint32_t bl = 0;
  for (int j = 7; j >= 0; --j)
    if (bl == 0 && t[j] != 0) bl = 32u * (uint32_t)j + 32u - (uint32_t)__builtin_clz(t[j]);
  return bl;
}

// encodeCompact (Bitcoin's GetCompact of a non-negative number)
HKV_HOST_DEV uint32_t cc_encode_compact(const uint32_t t[8]) {
  uint32_t size = (cc_bit_length(t) + 7u) >> 3;
  uint32_t word;
  if (size <= 3) {
    word = t[0] << (8u * (3u - size));
  } else {
    const uint32_t sb = size - 3u, li = sb >> 2, sh = 8u * (sb & 3u);
    uint32_t lo = 0, hi = 0;
    for (uint32_t j = 0; j < 8; ++j) {
      if (j == li) lo = t[j];
      if (j == li + 1) hi = t[j];
    }
    word = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh) & 0x00FFFFFFu;
  }
  if (word & 0x00800000u) {
    word >>= 8;
    ++size;
  }
  return (size << 24) | word;
}

HKV_DEV void cc_add256(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) {
  uint64_t c = 0;
  for (int j = 0; j < 8; ++j) {
    c += (uint64_t)a[j] + b[j];
    r[j] = (uint32_t)c;
    c >>= 32;
  }
}

// a > b
HKV_DEV bool cc_gt256(const uint32_t a[8], const uint32_t b[8]) {
  bool gt = false, decided = false;
  for (int j = 7; j >= 0; --j) {
    gt = decided ? gt : (a[j] > b[j]);
    decided = decided || (a[j] != b[j]);
  }
  return gt;
}

// headerWork: floor(2^256 / (target + 1)), 0 for a compact that is negative,
// overflowing or zero. A restoring division that starts below the divisor's
// top bit: d = target + 1 has k bits (2 <= k <= 256), the quotient 258 - k at
// most, so a mainnet header takes about 35 steps and a regtest header 3.
HKV_DEV void cc_header_work(uint32_t bits, uint32_t q[8]) {
  uint32_t d[8], r[8];
  const uint32_t fl = cc_decode_compact(bits, d);
  for (int j = 0; j < 8; ++j) q[j] = 0;
  if (fl) return;
  uint32_t carry = 1;  // d = target + 1 (target < 2^256 - 1: no wrap)
  for (int j = 0; j < 8; ++j) {
    d[j] += carry;
    carry = (carry && d[j] == 0) ? 1u : 0u;
  }
  const uint32_t k = cc_bit_length(d);
  // the first k bits of 2^256: 2^(k - 1)
  for (uint32_t j = 0; j < 8; ++j) r[j] = (j == ((k - 1u) >> 5)) ? (1u << ((k - 1u) & 31u)) : 0u;
  uint32_t top = 0;  // bit 256 of r, set by a shift when k = 256
  const uint32_t steps = 258u - k;
  for (uint32_t it = 0; it < steps; ++it) {
    if (it) {
      top = r[7] >> 31;
      for (int j = 7; j > 0; --j) r[j] = (r[j] << 1) | (r[j - 1] >> 31);
      r[0] <<= 1;
    }
    uint32_t s[8];
    uint64_t borrow = 0;
    for (int j = 0; j < 8; ++j) {
      const uint64_t x = (uint64_t)r[j] - d[j] - borrow;
      s[j] = (uint32_t)x;
      borrow = (x >> 32) & 1u;
    }
    const uint32_t ge = (top | (borrow ? 0u : 1u)) & 1u;
    for (int j = 0; j < 8; ++j) r[j] = ge ? s[j] : r[j];
    for (int j = 7; j > 0; --j) q[j] = (q[j] << 1) | (q[j - 1] >> 31);
    q[0] = (q[0] << 1) | ge;
  }
}

// The retarget at a period boundary: target(P) * span / target_timespan in
// exact integers (a nine-limb product, divided limb by limb), capped at
// pow_limit, as compact bits. span is the signed 64-bit difference of the two
// times clamped to [target_timespan / 4, 4 * target_timespan]. A parent compact
// that overflows gives 0 and sets overflow.
HKV_DEV uint32_t cc_retarget(const ChainCtx& x, uint32_t parent_bits, uint32_t parent_time, uint32_t first_time,
                             bool& overflow) {
  uint32_t t[8];
  overflow = (cc_decode_compact(parent_bits, t) & CC_OVERFLOW) != 0;
  if (overflow) return 0;
  const int64_t lo = (int64_t)(x.target_timespan / 4u), hi = 4 * (int64_t)x.target_timespan;
  int64_t span = (int64_t)parent_time - (int64_t)first_time;
  span = span < lo ? lo : span > hi ? hi : span;
  uint32_t p[9];
  uint64_t c = 0;
  for (int j = 0; j < 8; ++j) {
    c += (uint64_t)t[j] * (uint32_t)span;
    p[j] = (uint32_t)c;
    c >>= 32;
  }
  p[8] = (uint32_t)c;
  uint64_t rem = 0;
  for (int j = 8; j >= 0; --j) {
    const uint64_t cur = (rem << 32) | p[j];
    p[j] = (uint32_t)(cur / x.target_timespan);  // (rem < target_timespan: the quotient fits a limb)
    rem = cur % x.target_timespan;
  }
  if (p[8] != 0 || cc_gt256(p, x.pow_limit))
    for (int j = 0; j < 8; ++j) p[j] = x.pow_limit[j];
  return cc_encode_compact(p);
}

HKV_DEV void cc_cmpswap(uint32_t& a, uint32_t& b) {
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// Element c / 2 of the ascending sort of w[0, c): the caller fills w[c, 11)
// with 0xFFFFFFFF, which sorts behind every real element (or ties with it).
// A fixed 35-comparator network for 11 keys (tests/chainctx_host.cpp checks
// it on all 2^11 zero-one inputs).
HKV_DEV uint32_t cc_median(uint32_t w[CHAIN_MTP_SPAN], uint32_t c) {
#define HKV_CC_CS(i, j) cc_cmpswap(w[i], w[j])
  HKV_CC_CS(0, 9); HKV_CC_CS(1, 6); HKV_CC_CS(2, 4); HKV_CC_CS(3, 7); HKV_CC_CS(5, 8);
  HKV_CC_CS(0, 1); HKV_CC_CS(3, 5); HKV_CC_CS(4, 10); HKV_CC_CS(6, 9); HKV_CC_CS(7, 8);
  HKV_CC_CS(1, 3); HKV_CC_CS(2, 5); HKV_CC_CS(4, 7); HKV_CC_CS(8, 10);
  HKV_CC_CS(0, 4); HKV_CC_CS(1, 2); HKV_CC_CS(3, 7); HKV_CC_CS(5, 9); HKV_CC_CS(6, 8);
  HKV_CC_CS(0, 1); HKV_CC_CS(2, 6); HKV_CC_CS(4, 5); HKV_CC_CS(7, 8); HKV_CC_CS(9, 10);
  HKV_CC_CS(2, 4); HKV_CC_CS(3, 6); HKV_CC_CS(5, 7); HKV_CC_CS(8, 9);
  HKV_CC_CS(1, 2); HKV_CC_CS(3, 4); HKV_CC_CS(5, 6); HKV_CC_CS(7, 8);
  HKV_CC_CS(2, 3); HKV_CC_CS(4, 5); HKV_CC_CS(6, 7);
#undef HKV_CC_CS
  uint32_t m = 0;
  for (uint32_t j = 0; j <= CHAIN_MTP_SPAN / 2; ++j)
    if (j == c / 2u) m = w[j];
  return m;
}

// validVersion: the version as a signed number
HKV_DEV bool cc_version_ok(const ChainCtx& x, uint32_t version, uint32_t H) {
  const int32_t v = (int32_t)version;
  return !((v < 2 && H >= x.bip34_height) || (v < 3 && H >= x.bip66_height) || (v < 4 && H >= x.bip65_height));
}

// the index of the checkpoint at height H in the ascending heights, or CHAIN_CP_NONE
HKV_DEV uint32_t cc_checkpoint_at(const uint32_t* heights, uint32_t n_cp, uint32_t H) {
  uint32_t lo = 0, hi = n_cp;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (heights[mid] < H) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n_cp && heights[lo] == H) ? lo : CHAIN_CP_NONE;
}

// The scan element of the minimum-difficulty walk: (1 << 32) | bits where a
// header's own bits are "real" (a period start, or not the limit), else 0;
// combined by "the later defined value wins".
HKV_DEV uint64_t cc_real_of(const ChainCtx& x, uint32_t H, uint32_t bits) {
  return (H % x.interval == 0 || bits != x.limit_bits) ? ((1ull << 32) | bits) : 0ull;
}
HKV_DEV uint64_t cc_real_join(uint64_t earlier, uint64_t later) { return (later >> 32) ? later : earlier; }

// What one header's verdict reads beside the context: itself, its parent, the
// period's first block when it stands on a boundary, real(P), its median
// window (newest first, padded with 0xFFFFFFFF past c elements) and its
// checkpoint's outcome.
struct ChainIn {
  uint32_t H, version, time, bits;
  uint32_t parent_time, parent_bits;
  uint32_t first_time;   // time of the block at H - interval (read at a boundary only)
  uint32_t parent_real;  // real(P) (read with CHAIN_MIN_DIFFICULTY only)
  uint32_t window[CHAIN_MTP_SPAN];
  uint32_t c;
  bool checkpoint_ok;  // no checkpoint at H, or its hash equals the header's
};

// -> the CHN_* flags; mtp and want are the two outputs beside them
HKV_DEV uint32_t chain_verdict(const ChainCtx& x, ChainIn& in, uint32_t& mtp, uint32_t& want) {
  uint32_t fl = 0;
  mtp = cc_median(in.window, in.c);
  if (in.time > mtp) fl |= CHN_TIME_OK;
  if ((uint64_t)in.time <= x.now + CHAIN_FUTURE_LIMIT) fl |= CHN_NOT_FUTURE;
  bool overflow = false;
  if (in.H % x.interval != 0) {
    if (x.flags & CHAIN_MIN_DIFFICULTY)
      want = (uint64_t)in.time > (uint64_t)in.parent_time + x.min_diff_spacing ? x.limit_bits : in.parent_real;
    else
      want = in.parent_bits;
  } else if (x.flags & CHAIN_NO_RETARGET) {
    want = in.parent_bits;
  } else {
    want = cc_retarget(x, in.parent_bits, in.parent_time, in.first_time, overflow);
  }
  if (!overflow && in.bits == want) fl |= CHN_BITS_OK;
  if (cc_version_ok(x, in.version, in.H)) fl |= CHN_VERSION_OK;
  if (in.checkpoint_ok) fl |= CHN_CHECKPOINT_OK;
  return fl;
}

}  // namespace hkv
