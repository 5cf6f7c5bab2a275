// hkv_tail_plan.h — the multisig tail's work-queue arithmetic (hkv_kernels.hip
// 2e, hkv_ms_tail_kernel) and the host's sizes of the verdict words it writes
// (hkv_api.cpp enqueue_std_chunk), in one place. Pure C++ (no HIP include):
// the kernel and tests/tail_plan.cpp compile this same text, the latter on
// the CPU under ASan and UBSan, where every item of a launch can be walked
// against a model of the buffers.
//
// The queue: n1 hash chunks; then per round r its n2 emit chunks, the key
// chunks of its key window and the candidate groups of its candidate window;
// then n2 resolve chunks. Round r's windows hold the records
//   candidates [r * Wc, r * Wc + c_r),  c_r = clamp(n_cand - r * Wc, 0, Wc)
//   key checks [r * Wk, r * Wk + k_r),  k_r = clamp(n_keys - r * Wk, 0, Wk)
// and the round has ceil(k_r / T) key chunks and ceil(c_r / group) candidate
// groups — none for an empty window, so no item has an empty range. Only the
// last non-empty round of each kind differs from a full one, so a round's
// first item index is a closed form (tail_round_start) and an item's round is
// found in at most four steps over the spans of rounds with equal counts.
//
// Counts are 32-bit: a launch has at most 2^20 inputs (HKV_STD_CHUNK), hence
// at most 136 * 2^20 candidates, and e4 < 2^32 for every window >= 64.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HKV_TP_FN __host__ __device__ inline
#else
#define HKV_TP_FN inline
#endif

namespace hkv {

// the 16-of-16 bound: candidate and key-check records per input
enum : uint32_t { MS_CAND_PER_INPUT = 136, MS_KEYS_PER_INPUT = 16 };

// 32-bit words of candidate / key-check verdict bits for a chunk of n inputs
// (the bound rounded up to a wave's ballot: a key chunk's wave stores 2 words)
HKV_TP_FN uint64_t ms_cbits_words(uint64_t n) { return (n * MS_CAND_PER_INPUT + 63) / 64 * 2; }
HKV_TP_FN uint64_t ms_kbits_words(uint64_t n) { return (n * MS_KEYS_PER_INPUT + 63) / 64 * 2; }

// the record windows' budget (records; multiples of 64): ~512 MiB of 168-B records
#ifndef HKV_MS_WIN_CAND
#define HKV_MS_WIN_CAND 2752512u  // 43,008 x 64 candidate records (441 MiB)
#endif
#ifndef HKV_MS_WIN_KEYS
#define HKV_MS_WIN_KEYS 442368u   // 6,912 x 64 key-check records (71 MiB)
#endif
// a window's capacity in records: the whole bound when it fits win, else win
HKV_TP_FN uint64_t ms_window_records(uint64_t bound, uint64_t win) {
  return ((bound < win ? bound : win) + 63) / 64 * 64;
}

enum : uint32_t { TAIL_HASH = 0, TAIL_EMIT = 1, TAIL_KEYS = 2, TAIL_CAND = 3, TAIL_RESOLVE = 4 };

struct TailPlan {
  uint32_t n1, n2;          // hash chunks; emit chunks per round (= resolve chunks)
  uint32_t n_cand, n_keys;  // the scan's totals
  uint32_t Wc, Wk, T, group;
  uint32_t rc, rk, rounds;  // non-empty candidate rounds, non-empty key rounds, max of both
  uint32_t gf, gl;          // candidate groups of a full round / of round rc - 1
  uint32_t kf, kl;          // key chunks of a full round / of round rk - 1
  uint32_t e1, e3, e4;      // first item of round 0 / of the resolve phase / past the last item
};

struct TailItem {
  uint32_t kind;   // TAIL_*
  uint32_t round;  // (TAIL_EMIT, TAIL_KEYS, TAIL_CAND)
  uint32_t idx;    // index within the kind (and round)
  uint32_t start;  // first item index of this item's stage: every item before it must have completed
  uint32_t cw0, kw0;  // the round's window origins (global record indices); past every record when empty
  // TAIL_CAND: records [base, end) of the group, valid = end - base <= group;
  // TAIL_KEYS: first = the chunk's first record, end = the round's last + 1
  uint32_t base, first, end, valid;
};

HKV_TP_FN uint32_t tail_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
HKV_TP_FN uint32_t tail_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
HKV_TP_FN uint32_t tail_ceil(uint32_t a, uint32_t b) { return a / b + (a % b ? 1u : 0u); }

// records of round r in a window of W records over n records
HKV_TP_FN uint32_t tail_round_records(uint32_t n, uint32_t W, uint32_t r, uint32_t n_rounds) {
  return r >= n_rounds ? 0u : tail_min(W, n - r * W);
}
// candidate groups / key chunks of round r
HKV_TP_FN uint32_t tail_round_groups(const TailPlan& p, uint32_t r) {
  return r + 1 < p.rc ? p.gf : (r + 1 == p.rc ? p.gl : 0u);
}
HKV_TP_FN uint32_t tail_round_kchunks(const TailPlan& p, uint32_t r) {
  return r + 1 < p.rk ? p.kf : (r + 1 == p.rk ? p.kl : 0u);
}
// the first item index of round r (r <= rounds; r == rounds: e3)
HKV_TP_FN uint32_t tail_round_start(const TailPlan& p, uint32_t r) {
  const uint32_t g = p.rc == 0 ? 0u : tail_min(r, p.rc - 1) * p.gf + (r >= p.rc ? p.gl : 0u);
  const uint32_t k = p.rk == 0 ? 0u : tail_min(r, p.rk - 1) * p.kf + (r >= p.rk ? p.kl : 0u);
  return p.e1 + r * p.n2 + g + k;
}

// n inputs, n_hash_chunks hash items, the scan's totals, the windows (> 0),
// T lanes per chunk, group candidates per group
HKV_TP_FN TailPlan tail_plan(uint32_t n, uint32_t n_hash_chunks, uint32_t n_cand, uint32_t n_keys, uint32_t Wc,
                             uint32_t Wk, uint32_t T, uint32_t group) {
  TailPlan p;
  p.n1 = n_hash_chunks;
  p.n2 = tail_ceil(n, T);
  p.n_cand = n_cand;
  p.n_keys = n_keys;
  p.Wc = Wc;
  p.Wk = Wk;
  p.T = T;
  p.group = group;
  p.rc = tail_ceil(n_cand, Wc);
  p.rk = tail_ceil(n_keys, Wk);
  p.rounds = tail_max(p.rc, p.rk);
  p.gf = tail_ceil(tail_min(Wc, n_cand), group);
  p.gl = p.rc ? tail_ceil(n_cand - (p.rc - 1) * Wc, group) : 0u;
  p.kf = tail_ceil(tail_min(Wk, n_keys), T);
  p.kl = p.rk ? tail_ceil(n_keys - (p.rk - 1) * Wk, T) : 0u;
  p.e1 = p.n1;
  p.e3 = tail_round_start(p, p.rounds);
  p.e4 = p.e3 + p.n2;
  return p;
}

// item it < e4 of the queue
HKV_TP_FN TailItem tail_item(const TailPlan& p, uint32_t it) {
  TailItem x;
  x.kind = TAIL_HASH;
  x.round = x.idx = x.start = x.cw0 = x.kw0 = x.base = x.first = x.end = x.valid = 0;
  if (it < p.e1) {
    x.idx = it;
    return x;
  }
  if (it >= p.e3) {
    x.kind = TAIL_RESOLVE;
    x.idx = it - p.e3;
    x.start = p.e3;
    return x;
  }
  // the round: rounds of equal item counts lie in at most four spans, bounded
  // by the last non-empty round of each kind
  const uint32_t lo_r = tail_min(p.rc, p.rk), hi_r = p.rounds;
  const uint32_t bound[4] = {lo_r ? lo_r - 1 : 0u, lo_r, tail_max(hi_r ? hi_r - 1 : 0u, lo_r), hi_r};
  uint32_t r = 0, s = p.e1;  // s = the first item of round r
  for (int k = 0; k < 4; ++k) {
    if (bound[k] <= r) continue;
    const uint32_t per = p.n2 + tail_round_kchunks(p, r) + tail_round_groups(p, r);
    const uint32_t span = (bound[k] - r) * per;
    if (it - s < span) {
      const uint32_t dr = (it - s) / per;
      r += dr;
      s += dr * per;
      break;
    }
    s += span;
    r = bound[k];
  }
  const uint32_t k0 = it - s, nk = tail_round_kchunks(p, r);
  x.round = r;
  x.cw0 = tail_min(r, p.rc) * p.Wc;
  x.kw0 = tail_min(r, p.rk) * p.Wk;
  if (k0 < p.n2) {
    x.kind = TAIL_EMIT;
    x.idx = k0;
    x.start = s;
  } else if (k0 - p.n2 < nk) {
    x.kind = TAIL_KEYS;
    x.idx = k0 - p.n2;
    x.start = s + p.n2;
    x.first = x.kw0 + x.idx * p.T;
    x.end = x.kw0 + tail_round_records(p.n_keys, p.Wk, r, p.rk);
  } else {
    x.kind = TAIL_CAND;
    x.idx = k0 - p.n2 - nk;
    x.start = s + p.n2;
    x.base = x.cw0 + x.idx * p.group;
    x.end = x.cw0 + tail_round_records(p.n_cand, p.Wc, r, p.rc);
    x.valid = tail_min(p.group, x.end - x.base);
  }
  return x;
}

}  // namespace hkv
