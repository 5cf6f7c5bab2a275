// Host test of haskoin-node_amd/csrc/hkv_tail_plan.h (the multisig tail's
// work-queue arithmetic: hkv_ms_tail_kernel takes its rounds, item counts and
// ranges from it, hkv_api.cpp its verdict-word and window sizes), built by
// tests/test_tail_plan.py with -fsanitize=address,undefined: the same header
// the kernel compiles. For every case the queue is walked item by item
// against a model of the buffers enqueue_std_chunk allocates — the candidate
// and key-check verdict words and the two record windows, each an exactly
// sized heap array — doing what the kernel does with each item's numbers.
// Prints "ok <cases>" or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#ifndef TAIL_PLAN_HEADER
#define TAIL_PLAN_HEADER "../haskoin-node_amd/csrc/hkv_tail_plan.h"
#endif
#include TAIL_PLAN_HEADER

using hkv::TailItem;
using hkv::TailPlan;

static const uint32_t T = 256, GROUP = 32;  // hkv_layout.h PAIR_TPB, PAIR_SIGS

struct Case {
  uint32_t n, n_tx_hash;  // inputs; txs the fused path hashes first (0: the extraction path)
  uint32_t n_cand, n_keys;
  uint32_t win_c, win_k;  // hkv_debug_ms_window's (0 = default)
};

#define CHECK(c, ...)                                                                                  \
  do {                                                                                                 \
    if (!(c)) {                                                                                        \
      std::printf("FAIL: n=%u n_tx_hash=%u n_cand=%u n_keys=%u win=(%u, %u) item %u: ", cs.n,          \
                  cs.n_tx_hash, cs.n_cand, cs.n_keys, cs.win_c, cs.win_k, it);                         \
      std::printf(__VA_ARGS__);                                                                        \
      std::printf("  [%s]\n", #c);                                                                     \
      return false;                                                                                    \
    }                                                                                                  \
  } while (0)

static uint64_t ceil64(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

static bool walk(const Case& cs) {
  uint32_t it = 0;
  // the sizes, exactly as enqueue_std_chunk computes them
  const uint64_t all_cand = (uint64_t)cs.n * hkv::MS_CAND_PER_INPUT, all_keys = (uint64_t)cs.n * hkv::MS_KEYS_PER_INPUT;
  const uint64_t cap_cand = hkv::ms_window_records(all_cand, cs.win_c ? cs.win_c : HKV_MS_WIN_CAND);
  const uint64_t cap_keys = hkv::ms_window_records(all_keys, cs.win_k ? cs.win_k : HKV_MS_WIN_KEYS);
  const uint64_t cwords = hkv::ms_cbits_words(cs.n), kwords = hkv::ms_kbits_words(cs.n);
  CHECK(cwords == (all_cand + 63) / 64 * 64 / 32 && kwords == (all_keys + 63) / 64 * 64 / 32, "verdict word sizes");
  CHECK(cs.n_cand <= all_cand && cs.n_keys <= all_keys && cs.n_keys > 0, "case outside the 16-of-16 bound");
  const uint32_t Wc = (uint32_t)cap_cand, Wk = (uint32_t)cap_keys;
  const uint32_t n1 = (uint32_t)ceil64(3ull * cs.n_tx_hash, T);
  const TailPlan p = hkv::tail_plan(cs.n, n1, cs.n_cand, cs.n_keys, Wc, Wk, T, GROUP);

  // the plan's totals against a plain per-round sum in 64 bits
  const uint64_t rounds = ceil64(cs.n_cand, Wc) > ceil64(cs.n_keys, Wk) ? ceil64(cs.n_cand, Wc) : ceil64(cs.n_keys, Wk);
  const uint64_t n2 = ceil64(cs.n, T);
  uint64_t verify_items = 0;
  for (uint64_t r = 0; r < rounds; ++r) {
    const uint64_t c_r = r * Wc >= cs.n_cand ? 0 : (cs.n_cand - r * Wc < Wc ? cs.n_cand - r * Wc : Wc);
    const uint64_t k_r = r * Wk >= cs.n_keys ? 0 : (cs.n_keys - r * Wk < Wk ? cs.n_keys - r * Wk : Wk);
    verify_items += ceil64(c_r, GROUP) + ceil64(k_r, T);
  }
  const uint64_t want_e4 = n1 + rounds * n2 + verify_items + n2;
  CHECK(p.rounds == rounds && p.n2 == n2 && p.e1 == n1, "rounds %u n2 %u e1 %u", p.rounds, p.n2, p.e1);
  CHECK(want_e4 < (1ull << 32) && p.e4 == want_e4 && p.e3 == want_e4 - n2, "e3 %u e4 %u, want e4 %llu", p.e3, p.e4,
        (unsigned long long)want_e4);

  // the buffers: heap arrays of exactly the allocated sizes (ASan sees any
  // access past them); verdict words count their stores, window records
  // their reads (small cases slot by slot, every case by range)
  std::vector<uint8_t> cbits(cwords, 0), kbits(kwords, 0);
  const bool slots = cs.n_cand <= 40000;
  std::vector<uint8_t> cand_win(slots ? cap_cand : 0, 0), key_win(slots ? cap_keys : 0, 0);
  std::vector<uint8_t> cand_seen(slots ? cs.n_cand : 0, 0), key_seen(slots ? cs.n_keys : 0, 0);

  uint32_t stage = 0xFFFFFFFFu, stage_first = 0, prev_start = 0;
  uint32_t next_cand = 0, next_key = 0;  // records covered so far (the queue runs them in order)
  uint32_t n_hash = 0, n_emit = 0, n_resolve = 0, in_stage = 0;
  uint64_t n_verify = 0;
  for (it = 0; it < p.e4; ++it) {
    const TailItem x = hkv::tail_item(p, it);
    CHECK(x.kind <= hkv::TAIL_RESOLVE, "kind %u", x.kind);
    // stages in queue order: hash, then per round emit and verify, then resolve
    const bool in_round = x.kind == hkv::TAIL_EMIT || x.kind == hkv::TAIL_KEYS || x.kind == hkv::TAIL_CAND;
    CHECK(!in_round || x.round < p.rounds, "round %u of %u", x.round, p.rounds);
    const uint32_t st = x.kind == hkv::TAIL_HASH ? 0u
                        : x.kind == hkv::TAIL_RESOLVE ? 1u + 2u * p.rounds
                                                      : 1u + 2u * x.round + (x.kind == hkv::TAIL_EMIT ? 0u : 1u);
    if (st != stage) {
      // (no stage is skipped or revisited: round r's emits follow round
      // r - 1's verifies, its verifies its emits, the resolve the last round)
      CHECK(stage == 0xFFFFFFFFu ? st == (n1 ? 0u : 1u) : st == stage + 1, "stage %u after stage %u", st, stage);
      stage = st;
      stage_first = it;
      in_stage = 0;
    }
    // start: at most it, never decreasing, and past every item of an earlier
    // stage — with the stages in order that is the stage's first item
    CHECK(x.start <= it, "start %u", x.start);
    CHECK(x.start >= prev_start, "start %u after %u", x.start, prev_start);
    CHECK(x.start == stage_first, "start %u, the stage begins at %u", x.start, stage_first);
    prev_start = x.start;
    if (x.kind == hkv::TAIL_HASH) {
      CHECK(x.idx == n_hash && x.idx < n1, "hash chunk %u", x.idx);
      ++n_hash;
    } else if (x.kind == hkv::TAIL_EMIT) {
      CHECK(x.idx == in_stage && x.idx < n2, "emit chunk %u", x.idx);
      // the windows the emit writes through: origin r * W where the round has
      // records, at or past the last record where it has none
      const uint64_t cw = (uint64_t)x.round * Wc, kw = (uint64_t)x.round * Wk;
      CHECK(cw < cs.n_cand ? x.cw0 == cw : x.cw0 >= cs.n_cand, "candidate window origin %u", x.cw0);
      CHECK(kw < cs.n_keys ? x.kw0 == kw : x.kw0 >= cs.n_keys, "key window origin %u", x.kw0);
      CHECK((uint64_t)x.cw0 + Wc < (1ull << 32) && (uint64_t)x.kw0 + Wk < (1ull << 32), "window end wraps");
      ++n_emit;
    } else if (x.kind == hkv::TAIL_CAND) {
      const uint64_t cw = (uint64_t)x.round * Wc;
      const uint64_t lim = cw + Wc < cs.n_cand ? cw + Wc : cs.n_cand;
      CHECK(x.cw0 == cw, "cw0 %u in round %u", x.cw0, x.round);
      CHECK(x.base % 32 == 0, "base %u", x.base);
      CHECK(x.cw0 <= x.base && x.base < x.end && x.end <= lim, "group [%u, %u) of window %u, limit %llu", x.base, x.end,
            x.cw0, (unsigned long long)lim);
      CHECK(x.valid == (x.end - x.base < GROUP ? x.end - x.base : GROUP) && x.valid >= 1, "valid %u of [%u, %u)", x.valid,
            x.base, x.end);
      CHECK(x.base == next_cand, "group at %u, candidates covered to %u", x.base, next_cand);
      next_cand = x.base + x.valid;
      // pair_group stores the group's verdict word, unconditionally
      CHECK(x.base / 32 < cwords, "verdict word %u of %llu", x.base / 32, (unsigned long long)cwords);
      CHECK(cbits[x.base / 32]++ == 0, "verdict word %u stored twice", x.base / 32);
      // ... and reads the window record of every valid slot
      CHECK((uint64_t)x.base - x.cw0 + x.valid <= cap_cand, "record %u of a window of %llu", x.base - x.cw0 + x.valid - 1,
            (unsigned long long)cap_cand);
      if (slots)
        for (uint32_t s = 0; s < x.valid; ++s) {
          cand_win[x.base - x.cw0 + s] = 1;
          CHECK(cand_seen[x.base + s]++ == 0, "candidate %u in two groups", x.base + s);
        }
      ++n_verify;
    } else if (x.kind == hkv::TAIL_KEYS) {
      const uint64_t kw = (uint64_t)x.round * Wk;
      const uint64_t lim = kw + Wk < cs.n_keys ? kw + Wk : cs.n_keys;
      CHECK(x.kw0 == kw && x.end == lim, "key window %u end %u in round %u", x.kw0, x.end, x.round);
      CHECK(x.first < x.end && x.first % 64 == 0, "key chunk at %u, round end %u", x.first, x.end);
      CHECK(x.first == next_key, "key chunk at %u, keys covered to %u", x.first, next_key);
      const uint32_t last = x.end - x.first < T ? x.end : x.first + T;
      next_key = last;
      // key_check_lane: lane i = first + t reads record i - kw0 when i < end;
      // each wave with wbase < end stores two ballot words
      CHECK((uint64_t)last - x.kw0 <= cap_keys, "key record %u of a window of %llu", last - x.kw0 - 1,
            (unsigned long long)cap_keys);
      for (uint32_t w = 0; w < T / 64; ++w) {
        const uint32_t wbase = (x.first + 64 * w) & ~63u;
        if (wbase >= x.end) continue;
        CHECK(wbase / 32 + 1 < kwords, "ballot words %u, %u of %llu", wbase / 32, wbase / 32 + 1,
              (unsigned long long)kwords);
        CHECK(kbits[wbase / 32]++ == 0 && kbits[wbase / 32 + 1]++ == 0, "ballot words at %u stored twice", wbase / 32);
      }
      if (slots)
        for (uint32_t i = x.first; i < last; ++i) {
          key_win[i - x.kw0] = 1;
          CHECK(key_seen[i]++ == 0, "key %u in two chunks", i);
        }
      ++n_verify;
    } else {
      CHECK(x.idx == n_resolve && x.idx < n2, "resolve chunk %u", x.idx);
      ++n_resolve;
    }
    ++in_stage;
  }
  CHECK(stage == 1u + 2u * p.rounds, "the walk ends in stage %u", stage);
  CHECK(n_hash == n1 && n_emit == rounds * n2 && n_resolve == n2, "chunks: %u hash, %u emit, %u resolve", n_hash, n_emit,
        n_resolve);
  CHECK(next_cand == cs.n_cand, "candidates covered to %u", next_cand);
  CHECK(next_key == cs.n_keys, "keys covered to %u", next_key);
  // minimality: nothing verified twice, nothing stale, no empty item
  CHECK(n_verify == verify_items, "%llu verify items, want %llu", (unsigned long long)n_verify,
        (unsigned long long)verify_items);
  for (it = 0; slots && it < cs.n_cand; ++it) CHECK(cand_seen[it] == 1, "candidate %u in no group", it);
  for (it = 0; slots && it < cs.n_keys; ++it) CHECK(key_seen[it] == 1, "key %u in no chunk", it);
  return true;
}

static void around(std::set<uint64_t>& s, uint64_t W, uint64_t bound, const int* d, int nd) {
  const uint64_t ks[3] = {1, 2, bound / W};
  for (uint64_t k : ks)
    for (int j = 0; j < nd; ++j) {
      const int64_t v = (int64_t)(k * W) + d[j];
      if (k >= 1 && v >= 1 && (uint64_t)v <= bound) s.insert((uint64_t)v);
    }
}

int main() {
  size_t cases = 0;
  const uint32_t ns[] = {1, 31, 32, 33, 64, 255, 256, 257, 4096};
  const uint32_t wins[] = {64, 128, 1024, 4096, 0};
  const int dc[] = {0, 1, -1, 31, -31, 32, -32}, dk[] = {0, 1, -1};
  for (uint32_t n : ns)
    for (uint32_t wc : wins)
      for (uint32_t wk : wins) {
        const uint64_t bc = 136ull * n, bk = 16ull * n;
        const uint64_t Wc = hkv::ms_window_records(bc, wc ? wc : HKV_MS_WIN_CAND);
        const uint64_t Wk = hkv::ms_window_records(bk, wk ? wk : HKV_MS_WIN_KEYS);
        // per-input density at the extremes and in between, and every residue
        // of the count against the window and the group
        std::set<uint64_t> cands = {0, n, 16ull * n, 135ull * n, bc, bc - 1}, keys = {n, bk};
        around(cands, Wc, bc, dc, 7);
        around(keys, Wk, bk, dk, 3);
        for (uint64_t c : cands)
          for (uint64_t k : keys)
            for (uint32_t n_tx_hash : {0u, n}) {
              if (!walk(Case{n, n_tx_hash, (uint32_t)c, (uint32_t)k, wc, wk})) return 1;
              ++cases;
            }
      }
  // a 30,000-input chunk of 16-of-16 inputs at the default windows; a full
  // 131,072-input chunk of 1-of-16; and the shapes of
  // tests/test_gpu_ms_window.py's dense cases (inputs, candidates, keys, windows)
  const Case extra[] = {
      {30000, 0, 136u * 30000u, 16u * 30000u, 0, 0},
      {131072, 0, 16u * 131072u, 16u * 131072u, 0, 0},
      {64, 0, 1024, 1024, 4096, 64},     // key-only rounds
      {32, 0, 4352, 512, 64, 4096},      // candidate-only rounds
      {31, 0, 4216, 496, 1024, 64},      // ragged last round
      {31, 0, 4081, 481, 1024, 1024},    // residues: 17 / 31 / 32 valid slots in the last group
      {45, 0, 4095, 495, 1024, 1024},
      {46, 0, 4096, 496, 1024, 1024},
      {96, 0, 9916, 1536, 4096, 64},     // dense mix, no signature dropped
      {96, 0, 9916, 1536, 0, 0},
      {96, 0, 9914, 1536, 4096, 64},     // ... with one signature of a 15-of-16 input dropped
      {96, 0, 9914, 1536, 0, 0},
      {5500, 0, 9916, 1536, 1024, 64},   // dense mix among ~5,400 single-signature inputs
      {5500, 0, 9914, 1536, 1024, 64},
  };
  for (const Case& e : extra)
    for (uint32_t n_tx_hash : {0u, e.n}) {
      Case c = e;
      c.n_tx_hash = n_tx_hash;
      if (!walk(c)) return 1;
      ++cases;
    }
  std::printf("ok %zu\n", cases);
  return 0;
}
