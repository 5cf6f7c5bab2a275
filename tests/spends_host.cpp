// Host test of haskoin-node_amd/csrc/hkv_spends.h (the spend rule of
// hkv_block_spends_device), built by tests/test_spends_model.py with
// -fsanitize=address,undefined: the same header the device kernels compile,
// with the table built sequentially (plain code in place of the two atomics),
// run on the batch tests/spends_model.py emits and checked against the model:
// the sizing rule, the range sums on their edges, and for the batch every
// input's outpoint offset and first spender, every tx's two sums and its flag
// byte. The tx bytes and every per-input array sit in heap blocks of their
// exact size, so a read or write past any of them is an AddressSanitizer
// report; the walk is also run with one slot too few, as the device runs it
// when the caller's input total is too small. The whole run repeats for the
// hash masks 0xFFFFFFFF, 0xF and 0, two salts and both insertion orders (the
// descending one takes the min path); the answers must not depend on them.
// Prints "ok <inputs> <txs>" or the first failure and exits 1.
//
// The case file (little-endian): tests/spends_model.py emit_cases.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../haskoin-node_amd/csrc/hkv_spends.h"

namespace {

struct Reader {
  const std::vector<uint8_t>& b;
  size_t at = 0;
  bool ok = true;
  uint32_t u32() {
    if (b.size() - at < 4) {
      ok = false;
      return 0;
    }
    uint32_t v;
    std::memcpy(&v, b.data() + at, 4);
    at += 4;
    return v;
  }
  uint64_t u64() {
    const uint64_t lo = u32();
    return lo | ((uint64_t)u32() << 32);
  }
  const uint8_t* bytes(size_t n) {
    if (b.size() - at < n) {
      ok = false;
      return nullptr;
    }
    const uint8_t* p = b.data() + at;
    at += n;
    return p;
  }
};

// the table build without atomics: one input after the other
struct SeqSlotOps {
  static uint32_t cas(uint32_t* slot, uint32_t expected, uint32_t desired) {
    const uint32_t old = *slot;
    if (old == expected) *slot = desired;
    return old;
  }
  static void min(uint32_t* slot, uint32_t v) {
    if (v < *slot) *slot = v;
  }
};

// an exact-size heap block
template <class T>
struct Block {
  T* p;
  explicit Block(size_t n) : p(static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1))) {
    if (!p) std::abort();
  }
  ~Block() { std::free(p); }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
};

bool sizing_rule() {
  const size_t ns[] = {0, 1, 31, 32, 33, 64, 1000, (size_t)1 << 20, ((size_t)1 << 20) + 1, (size_t)1 << 30};
  for (size_t n : ns) {
    const size_t s = hkv::spend_table_slots(n);
    if (s < 64 || s < 2 * n || (s & (s - 1)) != 0 || (s > 64 && s / 2 >= 2 * n) || s > ((size_t)1 << 31)) {
      std::printf("FAIL: %zu slots for %zu inputs\n", s, n);
      return false;
    }
  }
  if (hkv::spend_table_slots(((size_t)1 << 30) + 1) != 0 || hkv::spend_table_slots(0xFFFFFF00u) != 0) {
    std::printf("FAIL: a table past 2^31 slots\n");
    return false;
  }
  return true;
}

bool range_sums() {
  const uint64_t m = 2100000000000000ull, top = ~0ull;
  struct Case {
    uint64_t max, a, b, c, sum;
    bool in_range;
  };
  const Case cases[] = {
      {m, m - 5, 5, 0, m, true},         {m, m, 1, 0, top, false},         {m, 1, top, 1, top, false},
      {m, m + 1, 0, 0, top, false},      {m, 0, 0, 0, 0, true},            {(1ull << 63) - 1, 1ull << 62, 1ull << 62, 0, top, false},
      {(1ull << 63) - 1, (1ull << 62) - 1, 1ull << 62, 0, (1ull << 63) - 1, true},
      {(1ull << 63) - 1, 1ull << 63, 1ull << 63, 1, top, false},
  };
  for (const Case& k : cases) {
    hkv::RangeSum s{0, true};
    hkv::range_add(s, k.a, k.max);
    hkv::range_add(s, k.b, k.max);
    hkv::range_add(s, k.c, k.max);
    if (hkv::range_value(s) != k.sum || s.in_range != k.in_range) {
      std::printf("FAIL: range sum of %llu %llu %llu\n", (unsigned long long)k.a, (unsigned long long)k.b,
                  (unsigned long long)k.c);
      return false;
    }
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: spends_host <case file>\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> blob;
  uint8_t buf[65536];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + n);
  std::fclose(f);
  if (!sizing_rule() || !range_sums()) return 1;

  Reader r{blob};
  const uint32_t n_tx = r.u32();
  std::vector<uint32_t> tx_off(n_tx + 1);
  for (uint32_t& o : tx_off) o = r.u32();
  if (!r.ok) return 1;
  const uint32_t n_bytes = tx_off[n_tx];
  const uint8_t* txp = r.bytes(n_bytes);
  std::vector<uint32_t> first(n_tx + 1);
  for (uint32_t& o : first) o = r.u32();
  const uint64_t max_money = r.u64();
  if (!r.ok) return 1;
  const uint32_t n = first[n_tx];
  std::vector<uint32_t> want_off(n), want_spender(n);
  // exact-size copies: the header must not read or write a byte beyond them
  Block<uint8_t> txs(n_bytes);
  std::memcpy(txs.p, txp, n_bytes);
  Block<uint64_t> jobs((size_t)n * hkv::SPEND_JOB_WORDS);
  Block<uint32_t> src(n), off(n), spender(n), short_off(n ? n - 1 : 0);
  for (uint32_t g = 0; g < n; ++g) {
    jobs.p[(size_t)g * 3] = jobs.p[(size_t)g * 3 + 1] = 0;
    jobs.p[(size_t)g * 3 + 2] = r.u64();
    src.p[g] = r.u32();
    want_off[g] = r.u32();
    want_spender[g] = r.u32();
  }
  std::vector<uint64_t> want_in(n_tx), want_out(n_tx);
  std::vector<uint32_t> want_flags(n_tx);
  for (uint32_t t = 0; t < n_tx; ++t) want_in[t] = r.u64(), want_out[t] = r.u64(), want_flags[t] = r.u32();
  if (!r.ok || r.at != blob.size()) {
    std::printf("FAIL: malformed case file\n");
    return 1;
  }

  // the walk: offsets, output sums, the two walk flags
  std::vector<hkv::TxWalk> walked(n_tx);
  for (uint32_t t = 0; t < n_tx; ++t) {
    walked[t].out_sum = 0, walked[t].flags = 0;
    if (first[t + 1] == first[t]) continue;
    walked[t] = hkv::spend_walk(txs.p, tx_off[t], first[t], n, off.p, max_money);
    const hkv::TxWalk again = hkv::spend_walk(txs.p, tx_off[t], first[t], n ? n - 1 : 0, short_off.p, max_money);
    if (again.out_sum != walked[t].out_sum || again.flags != walked[t].flags) return 1;
    if (walked[t].out_sum != want_out[t] ||
        walked[t].flags != (want_flags[t] & (hkv::SPEND_OUT_RANGE | hkv::SPEND_COINBASE))) {
      std::printf("FAIL: tx %u: out_sum %llu flags %02x (want %llu %02x)\n", t, (unsigned long long)walked[t].out_sum,
                  walked[t].flags, (unsigned long long)want_out[t], want_flags[t]);
      return 1;
    }
  }
  for (uint32_t g = 0; g < n; ++g)
    if (off.p[g] != want_off[g] || (g + 1 < n && short_off.p[g] != want_off[g])) {
      std::printf("FAIL: input %u: offset %u (want %u)\n", g, off.p[g], want_off[g]);
      return 1;
    }

  const uint32_t n_slots = (uint32_t)hkv::spend_table_slots(n);
  Block<uint32_t> slots(n_slots);
  const uint32_t masks[] = {0xFFFFFFFFu, 0xFu, 0u};
  const uint64_t salts[] = {0ull, 0x9E3779B97F4A7C15ull};
  for (uint64_t salt : salts)
    for (uint32_t mask : masks)
      for (int descending = 0; descending < 2; ++descending) {
        for (uint32_t s = 0; s < n_slots; ++s) slots.p[s] = hkv::SPEND_EMPTY;
        const hkv::SpendTable tb{txs.p, off.p, n, slots.p, n_slots, salt, mask};
        for (uint32_t k = 0; k < n; ++k) hkv::spend_insert<SeqSlotOps>(tb, descending ? n - 1 - k : k);
        for (uint32_t s = 0; s < n_slots; ++s)
          if (slots.p[s] != hkv::SPEND_EMPTY && (slots.p[s] >= n || want_spender[slots.p[s]] != slots.p[s])) {
            std::printf("FAIL: mask %08x slot %u holds %u\n", mask, s, slots.p[s]);
            return 1;
          }
        for (uint32_t g = 0; g < n; ++g) {
          spender.p[g] = hkv::first_spender(tb, g);
          if (spender.p[g] != want_spender[g]) {
            std::printf("FAIL: mask %08x input %u: spender %u (want %u)\n", mask, g, spender.p[g], want_spender[g]);
            return 1;
          }
        }
        for (uint32_t t = 0; t < n_tx; ++t) {
          uint64_t in_sum = 0, out_sum = 0;
          uint8_t flags = 0;
          if (first[t + 1] > first[t]) {
            out_sum = walked[t].out_sum;
            flags = hkv::spend_fold(jobs.p, src.p, spender.p, first[t], first[t + 1], max_money, out_sum,
                                    walked[t].flags, in_sum);
          }
          if (in_sum != want_in[t] || out_sum != want_out[t] || flags != want_flags[t]) {
            std::printf("FAIL: tx %u: in %llu out %llu flags %02x (want %llu %llu %02x)\n", t, (unsigned long long)in_sum,
                        (unsigned long long)out_sum, flags, (unsigned long long)want_in[t],
                        (unsigned long long)want_out[t], want_flags[t]);
            return 1;
          }
        }
      }
  std::printf("ok %u %u\n", n, n_tx);
  return 0;
}
