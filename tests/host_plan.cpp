// Host test of haskoin-node_amd/csrc/hkv_plan.h (the shard planning, bitmap
// merge and device failover of hkv_api.cpp verify_from_host), built by
// tests/test_host_plan.py with -fsanitize=address,undefined: the same header
// the library compiles, driven by mock devices whose enqueue / join fail on
// a random schedule; then the host-batch chunk schedule (host_chunks) and the
// staging layout (Layout) of the same header, and the prevout staging plan of
// the verifyStdTx host forms (plan_prevouts) against the arithmetic it
// replaced. Prints "ok <cases>" or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "../haskoin-node_amd/csrc/hkv_plan.h"

static uint32_t verdict(size_t i) {  // a deterministic stand-in for a verdict bit
  uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull;
  z ^= z >> 29;
  return (uint32_t)(z & 1u);
}

#define CHECK(c, ...)                    \
  do {                                   \
    if (!(c)) {                          \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
      return false;                      \
    }                                    \
  } while (0)

static bool check_plan(size_t lo, size_t hi, int nd) {
  std::vector<int> devs;
  for (int k = 0; k < nd; ++k) devs.push_back(k * 3 + 1);
  const std::vector<hkv::Shard> p = hkv::plan_shards(lo, hi, devs);
  size_t at = lo;
  for (size_t k = 0; k < p.size(); ++k) {
    CHECK(p[k].lo == at, "plan gap lo=%zu hi=%zu nd=%d", lo, hi, nd);
    CHECK(p[k].hi > p[k].lo, "empty shard");
    CHECK((p[k].lo - lo) % 64 == 0, "unaligned start");
    CHECK(k == 0 || p[k].dev > p[k - 1].dev, "device order");
    at = p[k].hi;
  }
  CHECK(at == (hi > lo ? hi : lo), "plan does not cover [%zu, %zu)", lo, hi);
  CHECK(p.size() <= (size_t)nd, "too many shards");
  return true;
}

// one failover run: nd mock devices; fail_at[d] = round in which device d
// fails (-1: never), fail_join[d] = it fails at join rather than at enqueue
static bool check_failover(std::mt19937_64& rng, size_t n, int nd) {
  std::vector<int> fail_at(nd, -1);
  std::vector<bool> fail_join(nd, false);
  int n_fail = 0;
  for (int d = 0; d < nd; ++d)
    if (rng() % 3 == 0) {
      fail_at[d] = (int)(rng() % 3);
      fail_join[d] = rng() & 1;
      ++n_fail;
    }
  std::vector<bool> healthy(nd, true);
  std::vector<std::vector<uint32_t>> staging(nd);  // per-device verdict words (d.hbits)
  std::vector<int> round_of(nd, 0), pending(nd, 0), verified(n, 0), fails(nd, 0);
  std::vector<uint32_t> out((n + 31) / 32 + 1, 0xDEADBEEFu);
  const size_t out_words = (n + 31) / 32;
  auto enqueue = [&](const hkv::Shard& s) {
    if (s.dev < 0 || s.dev >= nd || !healthy[(size_t)s.dev]) return 99;  // enqueue on an unhealthy device
    if (pending[(size_t)s.dev]) return 98;  // two shards in flight on one device
    const int r = round_of[(size_t)s.dev]++;
    if (fail_at[(size_t)s.dev] == r && !fail_join[(size_t)s.dev]) return -4;
    std::vector<uint32_t>& w = staging[(size_t)s.dev];
    w.assign((s.hi - s.lo + 31) / 32, 0);
    for (size_t i = s.lo; i < s.hi; ++i) w[(i - s.lo) / 32] |= verdict(i) << ((i - s.lo) % 32);
    pending[(size_t)s.dev] = 1;
    return 0;
  };
  auto join = [&](const hkv::Shard& s) {
    pending[(size_t)s.dev] = 0;
    if (fail_at[(size_t)s.dev] == round_of[(size_t)s.dev] - 1 && fail_join[(size_t)s.dev]) return -4;
    if (!hkv::merge_shard_words(out.data(), out_words, staging[(size_t)s.dev].data(), s)) return 97;
    for (size_t i = s.lo; i < s.hi; ++i) ++verified[i];
    return 0;
  };
  auto on_fail = [&](int dev, int) { ++fails[(size_t)dev]; };
  const int rc = hkv::run_with_failover(n, healthy, enqueue, join, on_fail);
  CHECK(rc != 97 && rc != 98 && rc != 99, "harness violation rc=%d", rc);
  bool any_left = false;
  for (int d = 0; d < nd; ++d) {
    CHECK(fails[d] <= 1, "device reported twice");
    CHECK(healthy[d] == (fails[d] == 0), "health flag vs reports");
    any_left = any_left || healthy[d];
  }
  if (rc == 0) {
    for (size_t i = 0; i < n; ++i) {
      CHECK(verified[i] == 1, "record %zu verified %d times (n=%zu nd=%d)", i, verified[i], n, nd);
      CHECK(((out[i / 32] >> (i % 32)) & 1u) == verdict(i), "verdict bit %zu", i);
    }
    CHECK(out[out_words] == 0xDEADBEEFu, "write past the bitmap");
  } else {
    CHECK(!any_left, "failed with healthy devices left (rc=%d)", rc);
    for (size_t i = 0; i < n; ++i) CHECK(verified[i] <= 1, "record %zu verified twice", i);
  }
  return true;
}

// the chunk schedule as enqueue_host_shard stepped it before host_chunks: an
// independent transcription, kept here to compare against
static std::vector<size_t> chunks_by_stepping(size_t len, size_t grid_lanes, size_t first_div, size_t max_grids) {
  std::vector<size_t> out;
  const size_t first = len >= 2 * grid_lanes ? grid_lanes / first_div : len;
  size_t next = first, off = 0;
  while (off < len) {
    size_t cl = next < len - off ? next : len - off;
    if (len - off - cl < grid_lanes) cl = len - off;
    size_t grown = 2 * next > grid_lanes ? 2 * next : grid_lanes;
    next = grown < max_grids * grid_lanes ? grown : max_grids * grid_lanes;
    out.push_back(cl);
    off += cl;
  }
  return out;
}

static bool check_chunks(size_t len, size_t grid_lanes, size_t first_div, size_t max_grids) {
  CHECK(hkv::host_chunks_ok(grid_lanes, first_div), "host_chunks_ok(%zu, %zu)", grid_lanes, first_div);
  const std::vector<size_t> c = hkv::host_chunks(len, grid_lanes, first_div, max_grids);
  size_t at = 0;
  for (size_t k = 0; k < c.size(); ++k) {
    CHECK(at % 32 == 0, "chunk %zu starts at %zu (len=%zu grid=%zu)", k, at, len, grid_lanes);
    CHECK(c[k] > 0, "empty chunk %zu (len=%zu grid=%zu)", k, len, grid_lanes);
    CHECK(k == 0 || c[k] >= grid_lanes, "chunk %zu of %zu is under one grid (len=%zu grid=%zu)", k, c[k], len,
          grid_lanes);
    CHECK(c[k] <= (max_grids + 1) * grid_lanes, "chunk %zu of %zu is over %zu grids (len=%zu grid=%zu)", k, c[k],
          max_grids + 1, len, grid_lanes);
    at += c[k];
  }
  CHECK(at == len, "chunks sum to %zu, not %zu (grid=%zu)", at, len, grid_lanes);
  CHECK(c == chunks_by_stepping(len, grid_lanes, first_div, max_grids), "schedule differs (len=%zu grid=%zu)", len,
        grid_lanes);
  return true;
}

struct Part {
  size_t bytes, align;
};
// lays parts out, checks them, and returns the total through *total
static bool check_layout(const std::vector<Part>& parts, size_t* total) {
  hkv::Layout l;
  size_t end = 0;  // of the part before
  for (size_t k = 0; k < parts.size(); ++k) {
    const size_t at = l.add(parts[k].bytes, parts[k].align);
    CHECK(at >= end, "part %zu at %zu overlaps the one before (ends %zu)", k, at, end);
    CHECK(at % parts[k].align == 0, "part %zu at %zu is not %zu-aligned", k, at, parts[k].align);
    CHECK(at - end < parts[k].align, "part %zu at %zu: more padding than its alignment after %zu", k, at, end);
    end = at + parts[k].bytes;
    CHECK(l.total >= end, "total %zu does not cover part %zu (ends %zu)", l.total, k, end);
  }
  CHECK(l.total == end, "total %zu past the last part's end %zu", l.total, end);
  *total = l.total;
  return true;
}

// The prevout staging as hkv_verify_std_txs and the block host form each wrote
// it out before plan_prevouts: the acceptance rule, then the four parts one
// behind the other (every size is a multiple of 4 and the values, 8 B each,
// come first, so no part needs padding).
struct HandStage {
  bool ok = false;
  size_t e0 = 0, n_ent = 0, o_val = 0, o_off = 0, o_scr = 0, o_op = 0, total = 0;
};
static HandStage stage_by_hand(const uint32_t* po, size_t n_tx, const uint8_t* ops, const uint32_t* scr,
                               const uint64_t* val) {
  HandStage h;
  for (size_t t = 0; t < n_tx; ++t)
    if (po[t + 1] < po[t]) return h;
  h.e0 = po[0];
  h.n_ent = po[n_tx] - h.e0;
  if (h.n_ent && (!ops || !scr || !val)) return h;
  h.o_val = 0;
  h.o_off = h.n_ent * 8;
  h.o_scr = h.o_off + (n_tx + 1) * 4;
  h.o_op = h.o_scr + h.n_ent * 8;
  h.total = h.o_op + h.n_ent * 36;
  h.ok = true;
  return h;
}

// one call: the plan against the hand staging; for an accepted call the
// layout's own properties, then the copies stage_prevouts makes, from arrays
// in heap blocks of their exact size into a block of exactly total bytes
static bool check_prevout_plan(const std::vector<uint32_t>& offsets, bool with_entries, bool want_ok) {
  const size_t n_tx = offsets.size() - 1;
  std::unique_ptr<uint32_t[]> po(new uint32_t[n_tx + 1]);
  std::copy(offsets.begin(), offsets.end(), po.get());
  const size_t end = *std::max_element(offsets.begin(), offsets.end());  // entries [0, end) exist
  std::unique_ptr<uint8_t[]> ops;
  std::unique_ptr<uint32_t[]> scr;
  std::unique_ptr<uint64_t[]> val;
  if (with_entries) {
    ops.reset(new uint8_t[end * 36]), scr.reset(new uint32_t[end * 2]), val.reset(new uint64_t[end]);
    for (size_t k = 0; k < end * 36; ++k) ops[k] = (uint8_t)(k * 7 + 1);
    for (size_t k = 0; k < end * 2; ++k) scr[k] = (uint32_t)(k * 0x9E3779B9u + 5);
    for (size_t k = 0; k < end; ++k) val[k] = (uint64_t)k * 0x9E3779B97F4A7C15ull + 9;
  }
  const hkv::PrevoutPlan p = hkv::plan_prevouts(po.get(), n_tx, with_entries);
  const HandStage h = stage_by_hand(po.get(), n_tx, ops.get(), scr.get(), val.get());
  CHECK(p.ok == h.ok && p.ok == want_ok, "acceptance: plan %d hand %d want %d (n_tx=%zu)", (int)p.ok, (int)h.ok,
        (int)want_ok, n_tx);
  if (!p.ok) return true;
  CHECK(p.e0 == h.e0 && p.n_ent == h.n_ent, "e0 %zu n_ent %zu, by hand %zu %zu", p.e0, p.n_ent, h.e0, h.n_ent);
  CHECK(p.o_val == h.o_val && p.o_off == h.o_off && p.o_scr == h.o_scr && p.o_op == h.o_op && p.total == h.total,
        "layout differs from the hand staging (n_tx=%zu e0=%zu n_ent=%zu)", n_tx, p.e0, p.n_ent);
  const size_t at[4] = {p.o_val, p.o_off, p.o_scr, p.o_op}, align[4] = {8, 4, 4, 4};
  const size_t bytes[4] = {p.n_ent * 8, (n_tx + 1) * 4, p.n_ent * 8, p.n_ent * 36};
  for (int k = 0; k < 4; ++k) {
    CHECK(at[k] % align[k] == 0, "part %d at %zu is not %zu-aligned", k, at[k], align[k]);
    CHECK(k == 0 || at[k] >= at[k - 1] + bytes[k - 1], "part %d at %zu overlaps the one before", k, at[k]);
  }
  CHECK(p.total == at[3] + bytes[3], "total %zu is not the end of the last part", p.total);
  CHECK(p.rebased.size() == n_tx + 1, "rebased holds %zu offsets", p.rebased.size());
  for (size_t t = 0; t <= n_tx; ++t)
    CHECK(p.rebased[t] == po[t] - p.e0, "rebased[%zu] = %u", t, p.rebased[t]);
  // the copies, as stage_prevouts issues them
  std::unique_ptr<uint8_t[]> stage(new uint8_t[p.total]);
  std::memcpy(stage.get() + p.o_off, p.rebased.data(), p.rebased.size() * 4);
  if (p.n_ent) {
    std::memcpy(stage.get() + p.o_op, ops.get() + p.e0 * 36, p.n_ent * 36);
    std::memcpy(stage.get() + p.o_scr, scr.get() + p.e0 * 2, p.n_ent * 8);
    std::memcpy(stage.get() + p.o_val, val.get() + p.e0, p.n_ent * 8);
  }
  // what the device then reads: entry e of tx t's list, by the staged offsets
  for (size_t t = 0; t < n_tx; ++t)
    for (size_t e = p.rebased[t]; e < p.rebased[t + 1]; ++e) {
      const size_t src = po[t] + (e - p.rebased[t]);
      CHECK(std::memcmp(stage.get() + p.o_op + e * 36, ops.get() + src * 36, 36) == 0 &&
                std::memcmp(stage.get() + p.o_scr + e * 8, scr.get() + src * 2, 8) == 0 &&
                std::memcmp(stage.get() + p.o_val + e * 8, val.get() + src, 8) == 0,
            "staged entry %zu of tx %zu is not the caller's entry %zu", e, t, src);
    }
  return true;
}

static bool check_prevout_plans(std::mt19937_64& rng, size_t* cases) {
  for (size_t n_tx : {1ul, 2ul, 33ul})
    for (uint32_t e0 : {0u, 1u, 7u}) {
      for (int it = 0; it < 20; ++it) {
        // it 0: every list empty; it 1: every list one entry; then lists of 0 to 3
        std::vector<uint32_t> po(n_tx + 1, e0);
        for (size_t t = 0; t < n_tx; ++t) po[t + 1] = po[t] + (it == 0 ? 0u : it == 1 ? 1u : (uint32_t)(rng() % 4));
        const bool any = po[n_tx] != e0;
        if (!check_prevout_plan(po, true, true)) return false;
        if (!check_prevout_plan(po, false, !any)) return false;  // null entry arrays: only with no entry named
        ++*cases;
        if (it != 1) continue;
        // one step down, at the first, a middle and the last position
        for (size_t t : {(size_t)0, n_tx / 2, n_tx - 1}) {
          std::vector<uint32_t> bad = po;
          bad[t] = bad[t + 1] + 1;
          if (!check_prevout_plan(bad, true, false)) return false;
          ++*cases;
        }
      }
    }
  // sizes near the largest entry count, nothing allocated: no wrap, the hand sum
  static_assert(sizeof(size_t) == 8, "the staging sizes need 64 bits");
  for (uint32_t e0 : {0u, 1u}) {
    const uint32_t po[2] = {e0, 0xFFFFFFFFu};
    const hkv::PrevoutPlan p = hkv::plan_prevouts(po, 1, true);
    const size_t n_ent = (size_t)0xFFFFFFFFu - e0;
    CHECK(p.ok && p.e0 == e0 && p.n_ent == n_ent, "largest entry count: e0 %zu n_ent %zu", p.e0, p.n_ent);
    CHECK(p.o_val == 0 && p.o_off == n_ent * 8 && p.o_scr == n_ent * 8 + 8 && p.o_op == n_ent * 16 + 8 &&
              p.total == n_ent * 52 + 8 && p.total > (size_t)0xFFFFFFFFu * 50,
          "largest entry count: total %zu", p.total);
    CHECK(p.rebased.size() == 2 && p.rebased[0] == 0 && p.rebased[1] == n_ent, "largest entry count: rebased");
    CHECK(!hkv::plan_prevouts(po, 1, false).ok, "largest entry count without entry arrays");
    ++*cases;
  }
  return true;
}

int main() {
  std::mt19937_64 rng(0x504C414E);
  size_t cases = 0;
  {
    std::mt19937_64 prev_rng(0x50524556);  // (its own: the schedules below keep theirs)
    if (!check_prevout_plans(prev_rng, &cases)) return 1;
  }
  // the host-batch chunk schedule
  {
    const std::vector<size_t> pinned = {65536, 262144, 720896};
    if (hkv::host_chunks(1048576, 262144, 4, 8) != pinned) {
      std::printf("FAIL: pinned chunk schedule\n");
      return 1;
    }
    if (hkv::host_chunks(0, 262144, 4, 8).size() != 0 || hkv::host_chunks_ok(0, 4) || hkv::host_chunks_ok(64, 4) ||
        hkv::host_chunks_ok(3, 4) || hkv::host_chunks_ok(262144, 0) || !hkv::host_chunks_ok(128, 4)) {
      std::printf("FAIL: host_chunks edge cases\n");
      return 1;
    }
    for (size_t grid_lanes : {128ul, 256ul, 384ul, 1280ul, 65536ul, 262144ul})
      for (int it = 0; it < 2000; ++it) {
        // lengths around the schedule's turns (whole grids, the doubling, the cap) and anywhere up to 40 grids
        const size_t grids = rng() % 40, len = it % 2 ? rng() % (40 * grid_lanes) : grids * grid_lanes + rng() % 3 - 1;
        if (len > 40 * grid_lanes) continue;  // (0 grids - 1)
        if (!check_chunks(len, grid_lanes, 4, 8) || !check_chunks(len, grid_lanes, 1, 1 + rng() % 8)) return 1;
        ++cases;
      }
  }
  // the staging layout
  {
    for (size_t n : {1ul, 300ul}) {  // hkv_check_headers: limit | prev | headers | hashes | status
      size_t total = 0;
      if (!check_layout({{32, 4}, {32, 4}, {n * 80, 4}, {n * 32, 16}, {n, 1}}, &total)) return 1;
      if (total > 64 + n * 113 + (4 - 1) * 3 + (16 - 1)) {
        std::printf("FAIL: header layout of %zu takes %zu bytes\n", n, total);
        return 1;
      }
    }
    for (int it = 0; it < 2000; ++it) {
      std::vector<Part> parts(1 + rng() % 8);
      for (Part& p : parts) p = {(size_t)(rng() % 1000), (size_t)1 << (rng() % 5)};
      size_t total = 0;
      if (!check_layout(parts, &total)) return 1;
      ++cases;
    }
  }
  for (int nd = 1; nd <= 9; ++nd)
    for (size_t n : {0ul, 1ul, 31ul, 32ul, 63ul, 64ul, 65ul, 127ul, 128ul, 129ul, 1000ul, 4097ul}) {
      for (size_t lo : {0ul, 64ul, 640ul})
        if (!check_plan(lo, lo + n, nd)) return 1;
      ++cases;
    }
  for (int it = 0; it < 20000; ++it) {
    const int nd = 1 + (int)(rng() % 8);
    const size_t n = (rng() % 4) == 0 ? rng() % 70 : rng() % 6000;
    if (!check_failover(rng, n, nd)) return 1;
    ++cases;
  }
  // every device fails: an error, never a partial success
  {
    std::vector<bool> healthy(3, true);
    int fails = 0;
    const int rc = hkv::run_with_failover(
        1000, healthy, [](const hkv::Shard&) { return -4; }, [](const hkv::Shard&) { return 0; },
        [&](int, int) { ++fails; });
    if (rc != -4 || fails != 3) {
      std::printf("FAIL: all-fail rc=%d fails=%d\n", rc, fails);
      return 1;
    }
    // an allocation failure (HKV_E_OOM = -3) on one device ends the call with
    // that error but takes no device out of service: nothing is re-sharded,
    // the shards already started are joined, and the next call uses every
    // device again (one OOM must not cascade over the context)
    for (int fail_dev = 0; fail_dev < 3; ++fail_dev) {
      std::vector<bool> h3(3, true);
      int reported = 0, enq = 0, joins = 0;
      std::vector<int> in_flight(3, 0);
      const int rc2 = hkv::run_with_failover(
          5000, h3,
          [&](const hkv::Shard& s) {
            if (s.dev == fail_dev) return -3;
            ++enq;
            in_flight[(size_t)s.dev] = 1;
            return 0;
          },
          [&](const hkv::Shard& s) {
            ++joins;
            in_flight[(size_t)s.dev] = 0;
            return 0;
          },
          [&](int, int) { ++reported; });
      if (rc2 != -3 || reported != 0 || !(h3[0] && h3[1] && h3[2]) || joins != enq || in_flight[0] + in_flight[1] + in_flight[2]) {
        std::printf("FAIL: alloc failure dev=%d rc=%d reported=%d enq=%d joins=%d\n", fail_dev, rc2, reported, enq,
                    joins);
        return 1;
      }
      int used = 0;
      if (hkv::run_with_failover(5000, h3, [&](const hkv::Shard&) { ++used; return 0; },
                                 [](const hkv::Shard&) { return 0; }, [](int, int) {}) != 0 || used != 3) {
        std::printf("FAIL: devices not reused after an allocation failure\n");
        return 1;
      }
      // the same at join: the error is returned, every started shard joined
      std::vector<bool> h4(3, true);
      int joined = 0;
      const int rc3 = hkv::run_with_failover(
          5000, h4, [](const hkv::Shard&) { return 0; },
          [&](const hkv::Shard& s) { ++joined; return s.dev == fail_dev ? -3 : 0; }, [](int, int) {});
      if (rc3 != -3 || joined != 3 || !(h4[0] && h4[1] && h4[2])) {
        std::printf("FAIL: alloc failure at join dev=%d rc=%d joined=%d\n", fail_dev, rc3, joined);
        return 1;
      }
    }
    std::vector<bool> none(2, false);
    if (hkv::run_with_failover(10, none, [](const hkv::Shard&) { return 0; }, [](const hkv::Shard&) { return 0; },
                               [](int, int) {}) != -2) {
      std::printf("FAIL: no healthy device\n");
      return 1;
    }
  }
  std::printf("ok %zu\n", cases);
  return 0;
}
