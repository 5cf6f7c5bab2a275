// hkv_stdtx.h — the prevout matching rule of batch verifyStdTx, for the device
// (hkv_stdtx.hip) and, compiled as plain C++, for the host test
// (tests/stdtx_host.cpp). Nothing here touches a HIP builtin.
//
// haskoin-core verifyStdTx [dep, haskoin-core-1.1.0 Haskoin.Transaction.Builder]
// pairs a tx's inputs with an unordered prevout list through matchTemplate:
//
//   matchTemplate as (b:bs) f = case break (`f` b) as of
//       (l, r:rs) -> Just r  : matchTemplate (l ++ rs) bs f   -- first match, consumed
//       _         -> Nothing : matchTemplate as bs f
//
// with f = equal outpoints. Inputs are served in input order and an entry is
// consumed by the input that takes it, so the entries with one given outpoint
// go, in list order, to the inputs with that outpoint, in input order; entries
// with another outpoint never interfere. Hence the closed form one lane can
// evaluate alone: if d earlier inputs of the tx carry input i's 36-byte
// outpoint, input i takes the (d + 1)-th entry with that outpoint, or nothing.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef HKV_DEV
#if defined(__HIPCC__)
#define HKV_DEV __device__ __forceinline__
#else
#define HKV_DEV inline
#endif
#endif

namespace hkv {

constexpr uint32_t OUTPOINT_BYTES = 36;        // 32 hash bytes as in the tx, then the LE32 index
constexpr uint32_t NO_PREVOUT = 0xFFFFFFFFu;   // match_prevout: no entry is left for the input

// a 32-bit word at any alignment (outpoints sit at odd offsets of the tx buffer)
HKV_DEV uint32_t outpoint_word(const uint8_t* p, uint32_t k) {
  uint32_t w;
  memcpy(&w, p + 4 * k, 4);
  return w;
}

// equal 36-byte outpoints: the index and the first hash word decide nearly
// every unequal pair, so they are compared before the other seven words
HKV_DEV bool outpoint_eq(const uint8_t* a, const uint8_t* b) {
  if (outpoint_word(a, 8) != outpoint_word(b, 8) || outpoint_word(a, 0) != outpoint_word(b, 0)) return false;
  uint32_t diff = 0;
  for (uint32_t k = 1; k < 8; ++k) diff |= outpoint_word(a, k) ^ outpoint_word(b, k);
  return diff == 0;
}

// the input after the one at off, in a tx whose structure is already
// validated (one step of hkv_sighash_dev.h walk_input: outpoint, scriptSig
// length varint, scriptSig, sequence)
HKV_DEV uint32_t next_input(const uint8_t* T, uint32_t off) {
  const uint32_t o = off + OUTPOINT_BYTES;
  const uint32_t t = T[o];
  if (t < 0xFDu) return o + 1 + t + 4;
  if (t == 0xFDu) return o + 3 + ((uint32_t)T[o + 1] | ((uint32_t)T[o + 2] << 8)) + 4;
  const uint32_t v = (uint32_t)T[o + 1] | ((uint32_t)T[o + 2] << 8) | ((uint32_t)T[o + 3] << 16) | ((uint32_t)T[o + 4] << 24);
  return o + (t == 0xFEu ? 5u : 9u) + v + 4;
}

// The entry input i of a validated tx takes. T: the batch's tx bytes; ins: the
// offset of the tx's first input; i < the tx's input count. entries: n_entries
// outpoints of 36 bytes, the tx's own prevout list in list order. Returns the
// entry's index in [0, n_entries) or NO_PREVOUT; in_off gets input i's offset.
HKV_DEV uint32_t match_prevout(const uint8_t* T, uint32_t ins, uint32_t i, const uint8_t* entries, uint32_t n_entries,
                               uint32_t& in_off) {
  uint32_t off = ins;
  for (uint32_t j = 0; j < i; ++j) off = next_input(T, off);
  in_off = off;
  const uint8_t* mine = T + off;
  // d: earlier inputs with this outpoint, each of which consumed one entry
  uint32_t d = 0, at = ins;
  for (uint32_t j = 0; j < i; ++j) {
    d += outpoint_eq(T + at, mine) ? 1u : 0u;
    at = next_input(T, at);
  }
  for (uint32_t e = 0; e < n_entries; ++e) {
    if (!outpoint_eq(entries + (size_t)e * OUTPOINT_BYTES, mine)) continue;
    if (d == 0) return e;
    --d;
  }
  return NO_PREVOUT;
}

}  // namespace hkv
