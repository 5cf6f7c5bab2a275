// Host test of haskoin-node_amd/csrc/hkv_blocktx.h (the in-batch prevout rule
// of hkv_verify_block_txs*), built by tests/test_blocktx_model.py with
// -fsanitize=address,undefined: the same header the device kernels compile,
// with the table built sequentially (plain code in place of the two atomics),
// run on the batch tests/blocktx_model.py emits and checked against the
// model: the sizing rule, every direct lookup (each txid, near misses, zero),
// and for every input of every parsing tx the parent index, the script
// offset, the script length and the amount of step 2 of the rule. The tx
// bytes, the txids and the table sit in heap blocks of their exact size, so a
// read past any of them is an AddressSanitizer report. The whole run repeats
// for the hash masks 0xFFFFFFFF, 0x3 and 0 and two salts; the answers must
// not depend on them. Prints "ok <inputs> <lookups>" or the first failure and
// exits 1.
//
// The case file (little-endian): tests/blocktx_model.py emit_cases.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../haskoin-node_amd/csrc/hkv_blocktx.h"

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

// the table build without atomics: one tx after the other
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

// an exact-size heap block, 16-byte aligned (the txids are loaded 16 bytes at a time)
template <class T>
struct Block {
  T* p;
  explicit Block(size_t n) : p(nullptr) {
    void* q = nullptr;
    if (posix_memalign(&q, 16, n ? n * sizeof(T) : 1) != 0) std::abort();
    p = static_cast<T*>(q);
  }
  ~Block() { std::free(p); }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
};

struct Want {
  uint32_t src, off, len;
  uint64_t value;
};

bool sizing_rule() {
  const size_t ns[] = {0, 1, 31, 32, 33, 64, 1000, (size_t)1 << 20, ((size_t)1 << 20) + 1};
  for (size_t n : ns) {
    const size_t s = hkv::txid_table_slots(n);
    if (s < 64 || s < 2 * n || (s & (s - 1)) != 0 || (s > 64 && s / 2 >= 2 * n)) {
      std::printf("FAIL: %zu slots for %zu txs\n", s, n);
      return false;
    }
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: blocktx_host <case file>\n");
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
  if (!sizing_rule()) return 1;

  Reader r{blob};
  const uint32_t n_tx = r.u32();
  std::vector<uint32_t> tx_off(n_tx + 1);
  for (uint32_t& o : tx_off) o = r.u32();
  if (!r.ok) return 1;
  const uint32_t n_bytes = tx_off[n_tx];
  const uint8_t* txp = r.bytes(n_bytes);
  const uint8_t* idp = r.bytes((size_t)n_tx * 32);
  std::vector<uint32_t> nin(n_tx);
  for (uint32_t& c : nin) c = r.u32();
  if (!r.ok) return 1;
  std::vector<std::vector<Want>> want(n_tx);
  unsigned long long inputs = 0;
  for (uint32_t t = 0; t < n_tx; ++t)
    for (uint32_t i = 0; i < nin[t]; ++i, ++inputs) {
      Want w;
      w.src = r.u32(), w.off = r.u32(), w.len = r.u32(), w.value = r.u64();
      want[t].push_back(w);
    }
  const uint32_t n_q = r.u32();
  const uint8_t* qp = r.bytes((size_t)n_q * 36);
  if (!r.ok || r.at != blob.size()) {
    std::printf("FAIL: malformed case file\n");
    return 1;
  }

  // exact-size copies: the header must not read a byte beyond them
  Block<uint8_t> txs(n_bytes);
  std::memcpy(txs.p, txp, n_bytes);
  Block<uint32_t> ids((size_t)n_tx * 8);
  std::memcpy(ids.p, idp, (size_t)n_tx * 32);
  const uint32_t n_slots = (uint32_t)hkv::txid_table_slots(n_tx);
  Block<uint32_t> slots(n_slots);

  const uint32_t masks[] = {0xFFFFFFFFu, 0x3u, 0u};
  const uint64_t salts[] = {0ull, 0x9E3779B97F4A7C15ull};
  for (uint64_t salt : salts)
    for (uint32_t mask : masks) {
      for (uint32_t s = 0; s < n_slots; ++s) slots.p[s] = hkv::TXID_EMPTY;
      const hkv::TxidTable tb{ids.p, n_tx, slots.p, n_slots, salt, mask};
      for (uint32_t t = 0; t < n_tx; ++t) hkv::txid_insert<SeqSlotOps>(tb, t);
      // at most one slot per distinct txid, never an index out of range
      uint32_t used = 0;
      for (uint32_t s = 0; s < n_slots; ++s) {
        if (slots.p[s] == hkv::TXID_EMPTY) continue;
        if (slots.p[s] >= n_tx) {
          std::printf("FAIL: slot %u holds %u\n", s, slots.p[s]);
          return 1;
        }
        ++used;
      }
      if (used > n_tx) return 1;
      for (uint32_t q = 0; q < n_q; ++q) {
        uint32_t exp;
        std::memcpy(&exp, qp + (size_t)q * 36 + 32, 4);
        const uint32_t got = hkv::txid_lookup(tb, hkv::txid_load_bytes(qp + (size_t)q * 36));
        if (got != exp) {
          std::printf("FAIL: mask %08x query %u: %u (want %u)\n", mask, q, got, exp);
          return 1;
        }
      }
      for (uint32_t t = 0; t < n_tx; ++t) {
        if (nin[t] == 0) continue;
        uint32_t count;
        uint32_t off = hkv::tx_inputs_start(txs.p, tx_off[t], count);
        if (count != nin[t]) {
          std::printf("FAIL: tx %u: %u inputs (want %u)\n", t, count, nin[t]);
          return 1;
        }
        for (uint32_t i = 0; i < count; ++i) {
          const hkv::Prevout p = hkv::resolve_in_batch(txs.p, tx_off.data(), t, off, tb);
          const Want& w = want[t][i];
          if (p.src != w.src || p.script_off != w.off || p.script_len != w.len || p.value != w.value) {
            std::printf("FAIL: mask %08x tx %u input %u: src %u off %u len %u value %llu (want %u %u %u %llu)\n", mask, t,
                        i, p.src, p.script_off, p.script_len, (unsigned long long)p.value, w.src, w.off, w.len,
                        (unsigned long long)w.value);
            return 1;
          }
          off = hkv::next_input(txs.p, off);
        }
      }
    }
  // list references: rebased inside the pool, zeroed when they overrun it
  {
    const hkv::Prevout a = hkv::list_prevout(10, 20, 7, 1000, 30), b = hkv::list_prevout(11, 20, 7, 1000, 30),
                       c = hkv::list_prevout(31, 0, 7, 1000, 30), d = hkv::list_prevout(0xFFFFFFF0u, 0x20, 7, 1000, 30),
                       e = hkv::list_prevout(30, 0, 7, 1000, 30);
    if (a.script_off != 1010 || a.script_len != 20 || b.script_off != 0 || b.script_len != 0 || c.script_len != 0 ||
        c.script_off != 0 || d.script_off != 0 || d.script_len != 0 || e.script_off != 1030 || e.script_len != 0 ||
        a.src != hkv::SRC_LIST || b.src != hkv::SRC_LIST || b.value != 7) {
      std::printf("FAIL: list_prevout\n");
      return 1;
    }
  }
  std::printf("ok %llu %u\n", inputs, n_q);
  return 0;
}
