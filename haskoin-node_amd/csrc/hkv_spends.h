// hkv_spends.h — the spend rule of hkv_block_spends_device: the first spender of
// every outpoint of a batch and each tx's value balance, for the device
// (hkv_spends.hip) and, compiled as plain C++, for the host test
// (tests/spends_host.cpp). Nothing here touches a HIP builtin: the two atomic
// operations of the table build come in through the policy type of
// hkv_blocktx.h (Ops::cas, Ops::min).
//
// The rule (include/hkv.h states it in full). Input i of tx t is
// g = input_first[t] + i; a tx that does not parse has no inputs.
//   spender[g]  the smallest g' whose 36-byte wire outpoint equals input g's
//               (g itself when it is the first). Bytes only: whether either
//               input resolved does not matter. The null outpoint (32 zero
//               bytes, index 0xFFFFFFFF) is never indexed: spender[g] = g.
//   flags[t]    SPEND_* below, from the inputs' src, spender and amount
//               (job.value) and the outputs' LE64 amounts on the wire;
//   sums[2t]    the exact input sum, sums[2t + 1] the exact output sum, each
//               UINT64_MAX once an amount or the running sum exceeds max_money.
//
// The spender comes from an open-addressing table over the batch's inputs:
// n_slots uint32_t slots (a power of two, >= 2 n and >= 64, so a linear probe
// always meets an empty slot), empty = 0xFFFFFFFF, a slot holding the smallest
// input index of one outpoint. The key of input u is the 36 bytes at
// T + input_off[u], wherever they lie in the tx bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "hkv_blocktx.h"
#include "hkv_stdtx.h"

namespace hkv {

constexpr uint32_t SPEND_EMPTY = 0xFFFFFFFFu;  // an empty slot; spender of a slot past the input total
constexpr size_t SPEND_MIN_SLOTS = 64;
constexpr size_t SPEND_MAX_SLOTS = (size_t)1 << 31;
constexpr uint64_t SPEND_MONEY_LIMIT = 1ull << 63;  // max_money lies below it: an in-range sum plus an in-range amount cannot wrap
constexpr uint64_t SPEND_SUM_NONE = ~0ull;          // a sum whose RANGE flag is clear

// HKV_SPEND_* of include/hkv.h
constexpr uint8_t SPEND_RESOLVED = 0x01, SPEND_FIRST = 0x02, SPEND_IN_RANGE = 0x04, SPEND_OUT_RANGE = 0x08,
                  SPEND_BALANCED = 0x10, SPEND_COINBASE = 0x20;

// the sizing rule: the smallest power of two >= 2 n and >= 64; 0 when that
// would exceed 2^31 slots
inline size_t spend_table_slots(size_t n) {
  if (n > SPEND_MAX_SLOTS / 2) return 0;
  size_t s = SPEND_MIN_SLOTS;
  while (s < 2 * n) s <<= 1;
  return s;
}

// 32 zero bytes, then 0xFFFFFFFF: the outpoint of a coinbase input
HKV_DEV bool outpoint_is_null(const uint8_t* p) {
  uint32_t any = ~outpoint_word(p, 8);
  for (uint32_t k = 0; k < 8; ++k) any |= outpoint_word(p, k);
  return any == 0;
}

// The slot hash: txid_hash's salted finaliser over outpoint words 0 and 1 with
// the LE32 index mixed in before it (the 2,000 inputs that spend one parent's
// 2,000 outputs share their hash words: without the index they would form one
// probe chain), ANDed with the same debug mask (hkv_debug_txid_hash_mask).
HKV_DEV uint32_t spend_hash(const uint8_t* p, uint64_t salt, uint32_t mask) {
  uint64_t z = ((uint64_t)outpoint_word(p, 0) | ((uint64_t)outpoint_word(p, 1) << 32)) ^ salt;
  z += (uint64_t)outpoint_word(p, 8) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return ((uint32_t)z ^ (uint32_t)(z >> 32)) & mask;
}

// what the table build and every lookup of one call share
struct SpendTable {
  const uint8_t* T;           // the batch's tx bytes
  const uint32_t* input_off;  // input u's outpoint lies at T + input_off[u]
  uint32_t n;                 // the inputs indexed: input_off[0, n) is written
  uint32_t* slots;
  uint32_t n_slots;  // spend_table_slots(n) or a larger power of two
  uint64_t salt;
  uint32_t mask;
};

// Insert input g < tb.n: txid_insert (hkv_blocktx.h) with the outpoint as the
// key. A slot only ever holds indices of one outpoint (it leaves empty once, by
// the cas, and changes afterwards only through min by a lane whose outpoint
// equals the holder's), so comparing with whichever index is present is sound,
// and every lane of one outpoint stops at the same slot.
template <class Ops>
HKV_DEV void spend_insert(const SpendTable& tb, uint32_t g) {
  const uint8_t* mine = tb.T + tb.input_off[g];
  if (outpoint_is_null(mine)) return;
  uint32_t s = spend_hash(mine, tb.salt, tb.mask) & (tb.n_slots - 1u);
  // (n_slots >= 2 n: an empty slot is met within n_slots steps; the bound only
  // keeps a table that breaks the sizing rule from spinning)
  for (uint32_t step = 0; step < tb.n_slots; ++step) {
    const uint32_t u = Ops::cas(tb.slots + s, SPEND_EMPTY, g);
    if (u == SPEND_EMPTY) return;
    if (u < tb.n && outpoint_eq(tb.T + tb.input_off[u], mine)) {
      Ops::min(tb.slots + s, g);
      return;
    }
    s = txid_next_slot(s, tb.n_slots);
  }
}

// The smallest indexed u whose outpoint is the 36 bytes at q, or SPEND_EMPTY.
// Reads a finished table. A slot value that is no input index ends the probe
// like an empty slot and the probe is bounded by the slot count: a table that
// was not built by spend_insert gives wrong answers, never a wild read or an
// endless loop.
HKV_DEV uint32_t spend_lookup(const SpendTable& tb, const uint8_t* q) {
  if (outpoint_is_null(q)) return SPEND_EMPTY;
  uint32_t s = spend_hash(q, tb.salt, tb.mask) & (tb.n_slots - 1u);
  for (uint32_t step = 0; step < tb.n_slots; ++step) {
    const uint32_t u = tb.slots[s];
    if (u >= tb.n) return SPEND_EMPTY;
    if (outpoint_eq(tb.T + tb.input_off[u], q)) return u;
    s = txid_next_slot(s, tb.n_slots);
  }
  return SPEND_EMPTY;
}

// spender[g] of an indexed input g < tb.n: itself for the null outpoint (and
// for an outpoint the table does not hold, which a table built over the same
// inputs never leaves out)
HKV_DEV uint32_t first_spender(const SpendTable& tb, uint32_t g) {
  const uint32_t u = spend_lookup(tb, tb.T + tb.input_off[g]);
  return u == SPEND_EMPTY ? g : u;
}

// an exact sum of amounts while every amount and the sum stay <= max_money
// (< 2^63, so adding one in-range amount to an in-range sum cannot wrap); once
// either bound is exceeded it sticks at out of range
struct RangeSum {
  uint64_t sum;
  bool in_range;
};
HKV_DEV void range_add(RangeSum& s, uint64_t v, uint64_t max_money) {
  if (!s.in_range || v > max_money) {
    s.in_range = false;
    return;
  }
  s.sum += v;
  s.in_range = s.sum <= max_money;
}
HKV_DEV uint64_t range_value(const RangeSum& s) { return s.in_range ? s.sum : SPEND_SUM_NONE; }

// what the walk of one tx reports beside the offsets it writes
struct TxWalk {
  uint64_t out_sum;  // range_value of the outputs' amounts
  uint8_t flags;     // SPEND_OUT_RANGE, SPEND_COINBASE
};

// The walk of the validated tx at start, whose inputs are [first, first + its
// count) of the batch: input i's outpoint offset, counted from T, goes to
// input_off[first + i] where that slot exists (< cap), then the outputs'
// amounts are summed. It stops behind the last output: the witness stacks and
// the lock time of a BIP144 tx are not read.
HKV_DEV TxWalk spend_walk(const uint8_t* T, uint32_t start, uint32_t first, uint32_t cap, uint32_t* input_off,
                          uint64_t max_money) {
  uint32_t nin;
  uint32_t off = tx_inputs_start(T, start, nin);
  const bool coinbase = nin == 1u && outpoint_is_null(T + off);
  for (uint32_t i = 0; i < nin; ++i) {
    if (first + i < cap) input_off[first + i] = off;
    off = next_input(T, off);
  }
  const uint32_t nout = varint_at(T, off);
  RangeSum out{0, true};
  for (uint32_t j = 0; j < nout; ++j) {
    uint64_t v;
    memcpy(&v, T + off, 8);  // (LE64 at any alignment; the targets are little-endian)
    range_add(out, v, max_money);
    off += 8u;
    const uint32_t sl = varint_at(T, off);
    off += sl;
  }
  TxWalk w;
  w.out_sum = range_value(out);
  w.flags = (uint8_t)((out.in_range ? SPEND_OUT_RANGE : 0) | (coinbase ? SPEND_COINBASE : 0));
  return w;
}

// one input's amount as the fold reads it: the value field of an hkv_input_job
// (24 bytes, 8-byte aligned: tx, input, script_off, script_len, value), by its
// place among the job's three 64-bit words so that this header needs no
// include/hkv.h
constexpr size_t SPEND_JOB_WORDS = 3, SPEND_JOB_VALUE = 2;
HKV_DEV uint64_t job_value(const uint64_t* jobs, uint32_t g) { return jobs[(size_t)g * SPEND_JOB_WORDS + SPEND_JOB_VALUE]; }

// The per-tx fold over the inputs [b, e), e > b: the input sum and its range,
// RESOLVED from src, FIRST from spender, then the flag byte from them and the
// walk's (out_sum, SPEND_OUT_RANGE | SPEND_COINBASE). Returns the flags;
// in_sum gets range_value of the inputs.
HKV_DEV uint8_t spend_fold(const uint64_t* jobs, const uint32_t* src, const uint32_t* spender, uint32_t b, uint32_t e,
                           uint64_t max_money, uint64_t out_sum, uint8_t walk_flags, uint64_t& in_sum) {
  RangeSum in{0, true};
  bool resolved = true, first = true;
  for (uint32_t g = b; g < e; ++g) {
    range_add(in, job_value(jobs, g), max_money);
    resolved = resolved && src[g] != SRC_NONE;
    first = first && spender[g] == g;
  }
  in_sum = range_value(in);
  const bool out_range = (walk_flags & SPEND_OUT_RANGE) != 0;
  const bool balanced = resolved && in.in_range && out_range && in.sum >= out_sum;
  return (uint8_t)((resolved ? SPEND_RESOLVED : 0) | (first ? SPEND_FIRST : 0) | (in.in_range ? SPEND_IN_RANGE : 0) |
                   (out_range ? SPEND_OUT_RANGE : 0) | (balanced ? SPEND_BALANCED : 0) |
                   (walk_flags & SPEND_COINBASE));
}

}  // namespace hkv
