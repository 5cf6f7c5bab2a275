// hkv_blocktx.h — the in-batch prevout rule of hkv_verify_block_txs*, for the
// device (hkv_blocktx.hip) and, compiled as plain C++, for the host test
// (tests/blocktx_host.cpp). Nothing here touches a HIP builtin: the two atomic
// operations of the table build come in through a policy type.
//
// The rule (include/hkv.h states it in full). For input i of a tx t that
// parses, with outpoint (h, k) as wire bytes:
//   1. tx t's own prevout list, by match_prevout (hkv_stdtx.h), unchanged:
//      src = SRC_LIST;
//   2. otherwise p = the smallest u such that tx u parses and txHash(tx u) == h;
//      the input resolves only if p exists, p < t and k < the output count of
//      tx p, and then takes output k of tx p where it lies in the tx bytes:
//      src = p;
//   3. otherwise nothing: src = SRC_NONE, script_len 0.
//
// Step 2's p comes from an open-addressing table over the batch's txids:
// n_slots uint32_t slots (a power of two, >= 2 n_tx and >= 64, so a linear probe
// always meets an empty slot), empty = 0xFFFFFFFF, a slot holding the smallest
// tx index of one txid. All-zero txids (txs that do not parse) are not indexed.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "hkv_stdtx.h"

namespace hkv {

constexpr uint32_t TXID_EMPTY = 0xFFFFFFFFu;  // an empty slot; also "no such txid" of a lookup
constexpr uint32_t SRC_NONE = 0xFFFFFFFFu;    // HKV_SRC_NONE
constexpr uint32_t SRC_LIST = 0xFFFFFFFEu;    // HKV_SRC_LIST
constexpr size_t TXID_MIN_SLOTS = 64;

// the sizing rule: the smallest power of two >= 2 n_tx and >= 64
inline size_t txid_table_slots(size_t n_tx) {
  size_t s = TXID_MIN_SLOTS;
  while (s < 2 * n_tx) s <<= 1;
  return s;
}

// a txid as the two 16-byte halves it is loaded by (txids are 16-byte aligned)
struct alignas(16) TxidHalf {
  uint32_t w[4];
};
struct Txid {
  TxidHalf lo, hi;
};
HKV_DEV Txid txid_load(const uint32_t* txids, uint32_t u) {
  const TxidHalf* p = reinterpret_cast<const TxidHalf*>(txids + (size_t)u * 8);
  Txid r;
  r.lo = p[0];
  r.hi = p[1];
  return r;
}
// 32 bytes at any alignment (an outpoint's hash inside the tx bytes, a query)
HKV_DEV Txid txid_load_bytes(const uint8_t* p) {
  Txid r;
  for (uint32_t k = 0; k < 4; ++k) r.lo.w[k] = outpoint_word(p, k), r.hi.w[k] = outpoint_word(p, 4 + k);
  return r;
}
HKV_DEV bool txid_eq(const Txid& a, const Txid& b) {
  uint32_t diff = 0;
  for (uint32_t k = 0; k < 4; ++k) diff |= (a.lo.w[k] ^ b.lo.w[k]) | (a.hi.w[k] ^ b.hi.w[k]);
  return diff == 0;
}
HKV_DEV bool txid_is_zero(const Txid& a) {
  uint32_t any = 0;
  for (uint32_t k = 0; k < 4; ++k) any |= a.lo.w[k] | a.hi.w[k];
  return any == 0;
}

// The slot hash: txid words 0 and 1 xored with the context's salt, through a
// 64-bit finaliser (splitmix64's), folded to 32 bits, ANDed with the debug
// mask (hkv_debug_txid_hash_mask: 0xFFFFFFFF unless a test narrows it). Without
// the salt a peer who grinds txid prefixes could line a block's txs up in one
// probe chain; with it the chain a set of txids forms is not known outside the
// process.
HKV_DEV uint32_t txid_hash(const Txid& a, uint64_t salt, uint32_t mask) {
  uint64_t z = ((uint64_t)a.lo.w[0] | ((uint64_t)a.lo.w[1] << 32)) ^ salt;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return ((uint32_t)z ^ (uint32_t)(z >> 32)) & mask;
}
HKV_DEV uint32_t txid_first_slot(const Txid& a, uint64_t salt, uint32_t mask, uint32_t n_slots) {
  return txid_hash(a, salt, mask) & (n_slots - 1u);
}
// the probe step: the next slot, around the end
HKV_DEV uint32_t txid_next_slot(uint32_t s, uint32_t n_slots) { return (s + 1u) & (n_slots - 1u); }

// what the table build and every lookup of one call share
struct TxidTable {
  const uint32_t* txids;  // n_tx * 8 words, 16-byte aligned
  uint32_t n_tx;
  uint32_t* slots;
  uint32_t n_slots;  // txid_table_slots(n_tx) or a larger power of two
  uint64_t salt;
  uint32_t mask;
};

// Insert tx t. Ops::cas(slot, expected, desired) returns the slot's value
// before it, Ops::min(slot, v) lowers the slot to v: atomicCAS / atomicMin on
// the device, plain code in the sequential host build. A slot only ever holds
// indices of one txid (it leaves empty once, by the cas, and changes afterwards
// only through min by a lane whose txid equals the holder's), so comparing with
// whichever index is present is sound, and every lane of one txid stops at the
// same slot: the first on its probe path that was empty or held its txid.
template <class Ops>
HKV_DEV void txid_insert(const TxidTable& tb, uint32_t t) {
  const Txid mine = txid_load(tb.txids, t);
  if (txid_is_zero(mine)) return;
  uint32_t s = txid_first_slot(mine, tb.salt, tb.mask, tb.n_slots);
  // (n_slots >= 2 n_tx: an empty slot is met within n_slots steps; the bound
  // only keeps a table that breaks the sizing rule from spinning)
  for (uint32_t step = 0; step < tb.n_slots; ++step) {
    const uint32_t u = Ops::cas(tb.slots + s, TXID_EMPTY, t);
    if (u == TXID_EMPTY) return;
    if (u < tb.n_tx && txid_eq(txid_load(tb.txids, u), mine)) {
      Ops::min(tb.slots + s, t);
      return;
    }
    s = txid_next_slot(s, tb.n_slots);
  }
}

// The smallest indexed u with txids[u] == q, or TXID_EMPTY. Reads a finished
// table. A slot value that is no tx index ends the probe like an empty slot,
// and the probe is bounded by the slot count, so a table the caller did not
// build with hkv_txid_index_device gives wrong answers, never a wild read or
// an endless loop.
HKV_DEV uint32_t txid_lookup(const TxidTable& tb, const Txid& q) {
  if (txid_is_zero(q)) return TXID_EMPTY;
  uint32_t s = txid_first_slot(q, tb.salt, tb.mask, tb.n_slots);
  for (uint32_t step = 0; step < tb.n_slots; ++step) {
    const uint32_t u = tb.slots[s];
    if (u >= tb.n_tx) return TXID_EMPTY;
    if (txid_eq(txid_load(tb.txids, u), q)) return u;
    s = txid_next_slot(s, tb.n_slots);
  }
  return TXID_EMPTY;
}

// a varint of a tx whose structure is already validated (counts and lengths
// < 2^32). This is get_varint of hkv_sighash_dev.h, restated because that
// header does not compile for the host; the two must stay in step.
HKV_DEV uint32_t varint_at(const uint8_t* T, uint32_t& off) {
  const uint32_t t = T[off];
  if (t < 0xFDu) {
    off += 1;
    return t;
  }
  if (t == 0xFDu) {
    const uint32_t v = (uint32_t)T[off + 1] | ((uint32_t)T[off + 2] << 8);
    off += 3;
    return v;
  }
  const uint32_t v = (uint32_t)T[off + 1] | ((uint32_t)T[off + 2] << 8) | ((uint32_t)T[off + 3] << 16) |
                     ((uint32_t)T[off + 4] << 24);
  off += t == 0xFEu ? 5u : 9u;
  return v;
}

// the offset of the first input of the validated tx starting at start, and its
// input count: the version, the BIP144 marker rule and the count as
// tx_index_row (hkv_sighash_dev.h) reads them and hkv_stdtx_jobs_kernel
// (hkv_stdtx.hip) repeats them; a change of the parse rule changes all three
HKV_DEV uint32_t tx_inputs_start(const uint8_t* T, uint32_t start, uint32_t& nin) {
  uint32_t off = start + 4u;
  if (T[off] == 0u && T[off + 1] == 1u) off += 2u;  // BIP144 marker and flag
  nin = varint_at(T, off);
  return off;
}

// what an input was resolved to: a job's script reference and amount, and src
struct Prevout {
  uint32_t script_off, script_len;
  uint64_t value;
  uint32_t src;
};

// Output k of the validated tx at start: false when k >= its output count.
// The walk skips the inputs with next_input, reads the output-count varint,
// then steps k outputs: O(inputs + k) dependent byte reads.
HKV_DEV bool tx_output_at(const uint8_t* T, uint32_t start, uint32_t k, Prevout& out) {
  uint32_t nin;
  uint32_t off = tx_inputs_start(T, start, nin);
  for (uint32_t j = 0; j < nin; ++j) off = next_input(T, off);
  const uint32_t nout = varint_at(T, off);
  if (k >= nout) return false;
  for (uint32_t j = 0; j < k; ++j) {
    off += 8u;
    const uint32_t sl = varint_at(T, off);
    off += sl;
  }
  uint64_t v;
  memcpy(&v, T + off, 8);  // (LE64 at any alignment; the targets are little-endian)
  off += 8u;
  out.value = v;
  out.script_len = varint_at(T, off);
  out.script_off = off;
  return true;
}

// Step 2 of the rule for the input at in_off of tx t: the in-batch parent's
// output, as a reference into the tx bytes, or SRC_NONE.
HKV_DEV Prevout resolve_in_batch(const uint8_t* T, const uint32_t* tx_off, uint32_t t, uint32_t in_off,
                                 const TxidTable& tb) {
  Prevout r;
  r.script_off = 0, r.script_len = 0, r.value = 0, r.src = SRC_NONE;
  const uint32_t p = txid_lookup(tb, txid_load_bytes(T + in_off));
  if (p == TXID_EMPTY || p >= t) return r;  // no such tx, a later tx, or itself
  Prevout o;
  if (!tx_output_at(T, tx_off[p], outpoint_word(T + in_off, 8), o)) return r;
  o.src = p;
  return o;
}

// Step 1's reference: list entry (off, len) of the caller's pool, which starts
// pool_base bytes after the tx bytes, as a reference from the tx bytes. The
// verify reads through a view wider than the pool, so the entry is checked
// against the pool here; one that overruns it gets script_len 0 (and offset
// 0), the verdict such an entry has under hkv_verify_std_txs*.
HKV_DEV Prevout list_prevout(uint32_t off, uint32_t len, uint64_t value, uint32_t pool_base, uint32_t pool_len) {
  Prevout r;
  const bool inside = off <= pool_len && len <= pool_len - off;
  r.script_off = inside ? pool_base + off : 0u;
  r.script_len = inside ? len : 0u;
  r.value = value;
  r.src = SRC_LIST;
  return r;
}

}  // namespace hkv
