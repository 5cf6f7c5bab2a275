// Host test of the part plan in haskoin-node_amd/csrc/hkv_launch_plan.h (the
// parts a table / chain batch runs in, two at a time on two streams), built by
// tests/test_pipe_plan.py with -fsanitize=address,undefined: the same header
// the library compiles. Over the four device geometries of
// tests/launch_plan.cpp, each with the parts off and at seven part lengths,
// and every n up to two resident grids plus a workgroup, plus 2^24:
//   - every field the plan had before the parts equals the plan with parts off;
//   - the parts are an exact, ordered, disjoint cover of [0, n_pad);
//   - a two-slot plan's part length is a multiple of WG and of
//     VERDICT_BATCH * 32, no longer than a chunk, and both slots lie inside
//     qs_quads; a one-slot plan's parts are its chunks;
//   - two slots are taken exactly when that is possible;
//   - each part's verdict stride is whole workgroups, at most the part, at
//     least min(part, MIN_INV_LANES), and VERDICT_BATCH strides cover the part;
//   - in a model of the pipeline (table, chain, finish per part, each on the
//     part's stream, streams ordered only by their own order between the fork
//     and the join) no part's table launch comes before the chain launch of
//     the slot's previous user, and neighbouring parts share neither stream
//     nor slot.
// Prints "ok <cases>" or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../haskoin-node_amd/csrc/hkv_launch_plan.h"

#define CHECK(c, ...)                    \
  do {                                   \
    if (!(c)) {                          \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
      return false;                      \
    }                                    \
  } while (0)

static size_t g_cases = 0, g_piped = 0, g_parts = 0;

constexpr size_t SLOT_SIG_QUADS = hkv::QTAB_QUADS + hkv::QTAB_ZG_QUADS;

// the fields the plan had before the parts
static bool same_as_off(const hkv::RecPlan& p, const hkv::RecPlan& off, size_t n) {
  CHECK(p.shape == off.shape && p.n_pad == off.n_pad && p.grid == off.grid, "n=%zu: shape / n_pad / grid", n);
  CHECK(p.prologue == off.prologue && p.aux == off.aux, "n=%zu: prologue / aux", n);
  CHECK(p.inv_stride == off.inv_stride && p.verdict_stride == off.verdict_stride, "n=%zu: strides", n);
  CHECK(p.qs_quads == off.qs_quads, "n=%zu: qs_quads %zu, off %zu", n, p.qs_quads, off.qs_quads);
  CHECK(p.chunk_len == off.chunk_len && p.n_chunks == off.n_chunks, "n=%zu: chunks", n);
  for (uint32_t k = 0; k < p.n_chunks; k += (p.n_chunks > 64 ? p.n_chunks / 64 : 1))
    CHECK(p.chunk(k).i0 == off.chunk(k).i0 && p.chunk(k).cn == off.chunk(k).cn, "n=%zu: chunk %u", n, k);
  return true;
}

static bool check_stride(uint32_t cn, size_t n) {
  const uint32_t s = hkv::verdict_stride_of(cn);
  const uint32_t least = cn < hkv::MIN_INV_LANES ? cn : hkv::MIN_INV_LANES;
  CHECK(s % hkv::WG == 0 && s > 0 && s <= cn, "n=%zu: verdict stride %u of a window of %u", n, s, cn);
  CHECK(s >= least, "n=%zu: verdict stride %u below %u lanes", n, s, least);
  CHECK((uint64_t)s * hkv::VERDICT_BATCH >= cn, "n=%zu: %u strides of %u do not cover %u", n, hkv::VERDICT_BATCH, s, cn);
  return true;
}

// the parts as a cover, and the slot schedule
static bool check_parts(const hkv::RecPlan& p, size_t n) {
  struct Use {
    bool used;
    uint32_t stream;
    size_t chain_at;  // position of the slot's last chain launch in its stream
  };
  Use slot[2] = {{false, 0, 0}, {false, 0, 0}};
  size_t at_stream[2] = {0, 0};  // launches so far per stream, after the fork
  uint64_t at = 0;
  for (uint32_t k = 0; k < p.n_parts; ++k) {
    const hkv::RecChunk w = p.part(k);
    CHECK(w.i0 == at && w.cn > 0 && w.cn % hkv::WG == 0 && w.cn <= p.part_len, "n=%zu: part %u cover", n, k);
    CHECK(k + 1 == p.n_parts || w.cn == p.part_len, "n=%zu: part %u is short but not last", n, k);
    at += w.cn;
    if (k < 3 || k + 2 >= p.n_parts)
      if (!check_stride(w.cn, n)) return false;
    if (p.qs_slots != 2) continue;
    CHECK(w.i0 % hkv::PART_ALIGN == 0, "n=%zu: part %u starts inside a verdict group", n, k);
    const uint32_t st = hkv::RecPlan::part_stream(k), sl = hkv::RecPlan::part_slot(k);
    CHECK(st < 2 && sl < 2, "n=%zu: part %u stream / slot", n, k);
    CHECK(p.slot_quads(sl) + (size_t)w.cn * SLOT_SIG_QUADS <= p.qs_quads, "n=%zu: part %u past qs", n, k);
    if (k > 0)
      CHECK(st != hkv::RecPlan::part_stream(k - 1) && sl != hkv::RecPlan::part_slot(k - 1),
            "n=%zu: parts %u and %u cannot overlap", n, k - 1, k);
    // table, chain, finish (+ rare, verdict) in the part's stream
    const size_t table_at = at_stream[st], chain_at = table_at + 1;
    at_stream[st] += 3;
    if (slot[sl].used)
      CHECK(slot[sl].stream == st && slot[sl].chain_at < table_at,
            "n=%zu: part %u's table launch is not ordered after slot %u's last chain", n, k, sl);
    slot[sl] = Use{true, st, chain_at};
    ++g_parts;
  }
  CHECK(at == p.n_pad, "n=%zu: parts end at %llu of %u", n, (unsigned long long)at, p.n_pad);
  return true;
}

static bool check_n(const hkv::Geometry& g, size_t n, bool walk) {
  using hkv::Shape;
  hkv::Geometry g_off = g;
  g_off.rec_part = 0;
  const hkv::RecPlan off = hkv::plan_records(g_off, n), p = hkv::plan_records(g, n);
  if (!same_as_off(p, off, n)) return false;
  CHECK(p.verdict_stride == hkv::verdict_stride_of(p.n_pad), "n=%zu: the batch's stride is not its window's", n);
  CHECK(off.qs_slots == 1 && off.part_len == off.chunk_len && off.n_parts == off.n_chunks, "n=%zu: parts off", n);
  const size_t want = (g.rec_part + hkv::PART_ALIGN - 1) / hkv::PART_ALIGN * hkv::PART_ALIGN;
  const bool can = p.shape == Shape::TableChain && g.rec_part != 0 && want < p.n_pad && want <= p.chunk_len &&
                   2 * want * SLOT_SIG_QUADS <= p.qs_quads;
  CHECK((p.qs_slots == 2) == can, "n=%zu: %u slots, two %s fit", n, p.qs_slots, can ? "would" : "do not");
  if (p.qs_slots == 2) {
    CHECK(p.shape == Shape::TableChain && p.n_parts > 1, "n=%zu: two slots for one part", n);
    CHECK(p.part_len == want, "n=%zu: part length %u, asked %zu", n, p.part_len, want);
    CHECK(p.part_len % hkv::WG == 0 && p.part_len % (hkv::VERDICT_BATCH * 32) == 0, "n=%zu: part alignment", n);
    CHECK(p.part_len <= p.chunk_len, "n=%zu: a part longer than a chunk", n);
    CHECK(2 * (size_t)p.part_len * SLOT_SIG_QUADS <= p.qs_quads, "n=%zu: two slots do not fit qs", n);
    CHECK(p.slot_quads(0) == 0 && p.slot_quads(1) == (size_t)p.part_len * SLOT_SIG_QUADS, "n=%zu: slot bases", n);
    CHECK(p.n_parts == (p.n_pad + (uint64_t)p.part_len - 1) / p.part_len, "n=%zu: part count", n);
    ++g_piped;
  } else {
    CHECK(p.qs_slots == 1 && p.part_len == p.chunk_len && p.n_parts == p.n_chunks, "n=%zu: one slot", n);
    CHECK(p.slot_quads(0) == 0, "n=%zu: slot base", n);
  }
  if (walk) {
    if (!check_parts(p, n) || !check_parts(off, n)) return false;
    for (uint32_t k = 0; k < off.n_parts; ++k)
      CHECK(off.part(k).i0 == off.chunk(k).i0 && off.part(k).cn == off.chunk(k).cn, "n=%zu: part %u is not chunk", n, k);
  }
  ++g_cases;
  return true;
}

int main() {
  const hkv::Geometry geos[] = {
      {256, 1024, (size_t)1 << 20, (size_t)1 << 20, 0},  // MI355X
      {256, 1024, 98304, 196608, 0},                     // ... with the two chunk hooks the suite uses
      {32, 128, (size_t)1 << 20, (size_t)1 << 20, 0},    // a small partition
      {256, 256, (size_t)1 << 20, (size_t)1 << 20, 0},   // one block per CU
  };
  // off; the shortest; one that is rounded up; two parts of the smallest
  // table / chain batch of an MI355X; half, one and two resident grids of one
  const size_t parts[] = {0, 1, 1000, 66048, 131072, 262144, 524288, (size_t)1 << 20};
  for (hkv::Geometry g : geos)
    for (size_t part : parts) {
      g.rec_part = part;
      const size_t grid_lanes = (size_t)g.grid_max * hkv::WG;
      // (a plan depends on n through n_pad: the parts are walked at both ends of every n_pad)
      for (size_t n = 1; n <= 2 * grid_lanes + hkv::WG; ++n)
        if (!check_n(g, n, n % hkv::WG <= 1)) return 1;
      if (!check_n(g, (size_t)1 << 24, true)) return 1;
      if (!check_n(g, 0xFFFFFF00ull, part == 0 || part >= 65536)) return 1;
    }
  if (g_piped == 0 || g_parts == 0) {
    std::printf("FAIL: no two-slot plan was checked\n");
    return 1;
  }
  std::printf("ok %zu %zu %zu\n", g_cases, g_piped, g_parts);
  return 0;
}
