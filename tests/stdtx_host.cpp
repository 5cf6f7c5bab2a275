// Host test of haskoin-node_amd/csrc/hkv_stdtx.h (the prevout matching rule of
// batch verifyStdTx), built by tests/test_stdtx_model.py with
// -fsanitize=address,undefined: the same header the job-builder kernel
// compiles, run on the cases tests/stdtx_model.py emits (random txs whose
// outpoints repeat, entry lists shuffled, truncated and padded) and checked
// per input against the entry the model's matchTemplate chose. Every tx and
// every entry list sits in a heap block of its exact size, so a read past
// either end is an AddressSanitizer report. Prints "ok <inputs>" or the first
// failure and exits 1.
//
// The case file (little-endian): u32 n_cases, then per case
//   u32 tx_len | tx | u32 ins | u32 nin | u32 n_entries | 36-byte entries |
//   nin x u32 expected entry (0xFFFFFFFF: none).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../haskoin-node_amd/csrc/hkv_stdtx.h"

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

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: stdtx_host <case file>\n");
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

  Reader r{blob};
  const uint32_t n_cases = r.u32();
  unsigned long long inputs = 0;
  for (uint32_t c = 0; c < n_cases && r.ok; ++c) {
    const uint32_t tx_len = r.u32();
    const uint8_t* txp = r.bytes(tx_len);
    const uint32_t ins = r.u32(), nin = r.u32(), n_entries = r.u32();
    const uint8_t* entp = r.bytes((size_t)n_entries * hkv::OUTPOINT_BYTES);
    if (!r.ok) break;
    // exact-size copies: the header must not read a byte beyond them
    const std::unique_ptr<uint8_t[]> tx_copy(new uint8_t[tx_len ? tx_len : 1]);
    const std::unique_ptr<uint8_t[]> ent_copy(new uint8_t[n_entries ? (size_t)n_entries * hkv::OUTPOINT_BYTES : 1]);
    uint8_t *tx = tx_copy.get(), *ent = ent_copy.get();
    std::memcpy(tx, txp, tx_len);
    if (n_entries) std::memcpy(ent, entp, (size_t)n_entries * hkv::OUTPOINT_BYTES);
    uint32_t walk = ins;
    for (uint32_t i = 0; i < nin; ++i) {
      const uint32_t want = r.u32();
      if (!r.ok) break;
      uint32_t in_off = 0;
      const uint32_t got = hkv::match_prevout(tx, ins, i, ent, n_entries, in_off);
      if (got != want || in_off != walk) {
        std::printf("FAIL: case %u input %u: entry %u (want %u), offset %u (want %u)\n", c, i, got, want, in_off, walk);
        return 1;
      }
      // the entry it names really carries the input's outpoint
      if (got != hkv::NO_PREVOUT && std::memcmp(ent + (size_t)got * hkv::OUTPOINT_BYTES, tx + in_off, 36) != 0) {
        std::printf("FAIL: case %u input %u: entry %u has another outpoint\n", c, i, got);
        return 1;
      }
      walk = hkv::next_input(tx, walk);
      ++inputs;
    }
    // the walk over every input ends inside the tx (the output count follows)
    if (walk >= tx_len) {
      std::printf("FAIL: case %u: the input walk ends at %u of %u bytes\n", c, walk, tx_len);
      return 1;
    }
  }
  if (!r.ok || r.at != blob.size()) {
    std::printf("FAIL: malformed case file\n");
    return 1;
  }
  std::printf("ok %llu\n", inputs);
  return 0;
}
