// Host test of haskoin-node_amd/csrc/hkv_launch_plan.h (which launches a
// batch of records or of standard inputs runs, and with which grids), built by
// tests/test_launch_plan.py with -fsanitize=address,undefined: the same header
// the library compiles, checked field by field against the expressions it
// replaced — restated below as they stood in hkv_api.cpp and at the end of
// hkv_kernels.hip — over every n up to two resident grids on four device
// geometries and near the 32-bit end of the index range; then the edges by
// value and the plan's structural properties. Prints "ok <cases>" or the first
// failure and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
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

// ---- the stepping the plan replaced ----------------------------------------
namespace was {

constexpr int WG = 256, BLK_SIGS = 16, PAIR_SIGS = 32, BATCH_INV = 16, VERDICT_BATCH = 16;
constexpr int QTAB_QUADS = hkv::QTAB_QUADS, QTAB_ZG_QUADS = hkv::QTAB_ZG_QUADS;
#define HKV_SPLIT_DIV 8
#define HKV_BLOCK_ROWS 1
#define HKV_STD_OVERLAP 1
enum : uint32_t { TX_HASHES_NONE = 0, TX_HASHES_NETWORK = 7 };  // (7: std_tx_hashes(forkid), either value)

struct DevCtx {
  int n_cu;
  uint32_t grid_max;
  size_t rec_chunk, std_chunk;
};

size_t round_up(size_t a, size_t b) { return (a + b - 1) / b * b; }
uint32_t ceil_div(size_t a, uint32_t b) { return (uint32_t)((a + b - 1) / b); }

// hkv_api.cpp
bool split_batch(const DevCtx& d, size_t n) { return round_up(n, WG) <= (size_t)d.grid_max * WG / HKV_SPLIT_DIV; }
bool mid_batch(const DevCtx& d, size_t n) {
  return !split_batch(d, n) && round_up(n, WG) <= (size_t)d.grid_max * WG / 2;
}
// hkv_kernels.hip
bool block_batch(uint32_t n_pad, uint32_t n_cu) { return n_pad <= (uint32_t)BLK_SIGS * n_cu; }

struct Rec {
  bool split, mid, block;
  uint32_t n_pad, blocks, block_grid, pair_grid, inv_stride, verdict_stride;
  bool prologue, aux;
  size_t quads;
  std::vector<std::pair<uint32_t, uint32_t>> chunks;  // launch_table_chain's (i0, cn)
};

Rec records(const DevCtx& d, size_t n) {
  Rec r;
  // enqueue_verify
  const size_t n_pad = round_up(n, WG);
  const bool split = split_batch(d, n);
  const bool mid = mid_batch(d, n);
  r.split = split, r.mid = mid, r.n_pad = (uint32_t)n_pad;
  r.prologue = !split;  // (and no std_pro, the caller's)
  r.aux = split;
  r.blocks = split ? 0u : (uint32_t)std::min<size_t>(n_pad / WG, mid ? d.grid_max / 2 : d.grid_max);
  // launch_ecmult
  r.block = split && block_batch((uint32_t)n_pad, (uint32_t)d.n_cu);
  r.block_grid = (uint32_t)n_pad / BLK_SIGS;
  r.pair_grid = (uint32_t)n_pad / PAIR_SIGS;
  // launch_prologue
  {
    uint32_t stride = ceil_div(n_pad, BATCH_INV);
    stride = stride > 65536u ? stride : (n_pad < 65536u ? (uint32_t)n_pad : 65536u);
    r.inv_stride = stride;
  }
  // launch_finish
  {
    uint32_t stride = ceil_div(ceil_div(n_pad, VERDICT_BATCH), WG) * WG;
    const uint32_t min_lanes = n_pad < 65536u ? (uint32_t)n_pad : 65536u;
    if (stride < min_lanes) stride = min_lanes;
    r.verdict_stride = stride;
  }
  // ensure_dev_buffers
  {
    const size_t lanes = (size_t)d.grid_max * WG;
    size_t quads = lanes * QTAB_QUADS;
    if (n_pad > lanes / 2) quads = std::max(quads, std::min(n_pad, d.rec_chunk) * (QTAB_QUADS + QTAB_ZG_QUADS));
    r.quads = quads;
  }
  // launch_table_chain
  if (!split && !mid) {
    const uint32_t chunk = (uint32_t)d.rec_chunk, np = (uint32_t)n_pad;
    for (uint64_t next = 0; next < np; next += chunk) {
      const uint32_t i0 = (uint32_t)next, cn = np - i0 < chunk ? np - i0 : chunk;
      r.chunks.push_back({i0, cn});
    }
  }
  return r;
}

struct Std {
  bool fused, fused_scan, rows, overlap;
  bool index_first;
  uint32_t index_hashes, tail_hashes;
  int scan;  // 0 in the kernel, 1 on st, 2 on the hash stream
};

Std std_chunk(const DevCtx& d, size_t n) {
  Std s;
  // enqueue_std_chunk
  const bool fused = split_batch(d, n);
  const bool fused_scan = fused && block_batch((uint32_t)round_up(n, WG), (uint32_t)d.n_cu);
  const bool overlap = !fused && HKV_STD_OVERLAP && mid_batch(d, n);
  const bool rows = fused_scan && HKV_BLOCK_ROWS;
  s.fused = fused, s.fused_scan = fused_scan, s.overlap = overlap, s.rows = rows;
  if (fused) {
    s.index_first = !rows;
    s.index_hashes = TX_HASHES_NONE;
  } else if (overlap) {
    s.index_first = true;
    s.index_hashes = TX_HASHES_NONE;
  } else {
    s.index_first = true;  // enqueue_std_inputs
    s.index_hashes = TX_HASHES_NETWORK;
  }
  // enqueue_std_rest, tail_args
  s.scan = fused_scan ? 0 : overlap ? 2 : 1;
  s.tail_hashes = fused ? TX_HASHES_NETWORK : TX_HASHES_NONE;
  return s;
}

// enqueue_verify_std_inputs
size_t std_chunk_len(const DevCtx& d, size_t n) {
  const size_t grid_lanes = (size_t)d.grid_max * WG;
  return n > grid_lanes ? d.std_chunk : grid_lanes / 2;
}

}  // namespace was

// ---- plan against restatement, and the structural properties ---------------
static size_t g_cases = 0;

static bool check_n(const hkv::Geometry& g, size_t n) {
  using hkv::Shape;
  const was::DevCtx d{(int)g.n_cu, g.grid_max, g.rec_chunk, g.std_chunk};
  const was::Rec w = was::records(d, n);
  const hkv::RecPlan p = hkv::plan_records(g, n);
  const Shape shape = w.block ? Shape::Block : w.split ? Shape::Pair : w.mid ? Shape::Mid : Shape::TableChain;
  CHECK(p.shape == shape, "records n=%zu: shape %u, was %u", n, (unsigned)p.shape, (unsigned)shape);
  CHECK(p.n_pad == w.n_pad, "records n=%zu: n_pad", n);
  const uint32_t grid = w.block ? w.block_grid : w.split ? w.pair_grid : w.mid ? w.blocks : 0u;
  CHECK(p.grid == grid, "records n=%zu: grid %u, was %u", n, p.grid, grid);
  CHECK(p.prologue == w.prologue && p.aux == w.aux, "records n=%zu: prologue / aux", n);
  CHECK(p.inv_stride == w.inv_stride, "records n=%zu: s^-1 stride %u, was %u", n, p.inv_stride, w.inv_stride);
  CHECK(p.verdict_stride == w.verdict_stride, "records n=%zu: verdict stride", n);
  CHECK(p.verdict_stride % hkv::WG == 0, "records n=%zu: verdict stride not whole workgroups", n);
  CHECK(p.qs_quads == w.quads, "records n=%zu: quads %zu, was %zu", n, p.qs_quads, w.quads);
  CHECK(p.qs_quads >= (size_t)g.grid_max * hkv::WG * hkv::QTAB_QUADS, "records n=%zu: below the resident grid", n);
  if (shape == Shape::TableChain) {
    CHECK(p.n_chunks == w.chunks.size(), "records n=%zu: %u chunks, was %zu", n, p.n_chunks, w.chunks.size());
    CHECK(p.chunk_len >= (uint32_t)hkv::WG && p.chunk_len % hkv::WG == 0, "records n=%zu: chunk length", n);
    CHECK((size_t)p.chunk_len * (hkv::QTAB_QUADS + hkv::QTAB_ZG_QUADS) <= p.qs_quads, "records n=%zu: chunk scratch", n);
  } else {
    CHECK(p.n_chunks == 1 && p.chunk_len == p.n_pad, "records n=%zu: one chunk", n);
  }
  uint64_t at = 0;  // chunks: whole workgroups, covering [0, n_pad) in order without overlap
  for (uint32_t k = 0; k < p.n_chunks; ++k) {
    const hkv::RecChunk c = p.chunk(k);
    if (shape == Shape::TableChain)
      CHECK(c.i0 == w.chunks[k].first && c.cn == w.chunks[k].second, "records n=%zu: chunk %u", n, k);
    CHECK(c.i0 == at && c.cn > 0 && c.cn % hkv::WG == 0 && c.cn <= p.chunk_len, "records n=%zu: chunk %u cover", n, k);
    at += c.cn;
  }
  CHECK(at == p.n_pad, "records n=%zu: chunks end at %llu", n, (unsigned long long)at);

  const was::Std ws = was::std_chunk(d, n);
  const hkv::StdPlan s = hkv::plan_std_chunk(g, n);
  const Shape sshape = ws.fused_scan ? Shape::Block : ws.fused ? Shape::Pair : ws.overlap ? Shape::Mid : Shape::TableChain;
  CHECK(s.shape == sshape && s.n_pad == w.n_pad, "std n=%zu: shape / n_pad", n);
  CHECK(s.shape == p.shape, "std n=%zu: the record verify of the chunk takes another shape", n);
  CHECK(s.scan_in_kernel == ws.fused_scan && s.rows_in_kernel == ws.rows && s.overlap == ws.overlap, "std n=%zu: flags", n);
  CHECK(s.index_first == ws.index_first, "std n=%zu: index first", n);
  CHECK(!s.index_first || (s.index_hashes ? was::TX_HASHES_NETWORK : was::TX_HASHES_NONE) == ws.index_hashes,
        "std n=%zu: index hashes", n);
  CHECK((s.tail_hashes ? was::TX_HASHES_NETWORK : was::TX_HASHES_NONE) == ws.tail_hashes, "std n=%zu: tail hashes", n);
  CHECK((int)s.scan == ws.scan, "std n=%zu: scan on %u, was %d", n, (unsigned)s.scan, ws.scan);
  CHECK(!s.rows_in_kernel || s.scan_in_kernel, "std n=%zu: rows without scan", n);
  CHECK(!s.scan_in_kernel || s.shape == Shape::Block, "std n=%zu: scan outside the block kernel", n);
  CHECK(!s.overlap || s.shape == Shape::Mid, "std n=%zu: overlap outside the mid-size form", n);
  CHECK(hkv::std_chunk_len(g, n) == was::std_chunk_len(d, n), "std n=%zu: chunk length", n);
  ++g_cases;
  return true;
}

static bool check_geometry(const hkv::Geometry& g) {
  const size_t grid_lanes = (size_t)g.grid_max * hkv::WG;
  for (size_t n = 1; n <= 2 * grid_lanes + hkv::WG; ++n)
    if (!check_n(g, n)) return false;
  // the 64-bit stepping: n within two chunks below the largest batch (every
  // 1021st n, and each of the last 600)
  const size_t top = 0xFFFFFF00ull, from = top - 2 * g.rec_chunk;
  for (size_t n = from; n < top - 600; n += 1021)
    if (!check_n(g, n)) return false;
  for (size_t n = top - 600; n <= top; ++n)
    if (!check_n(g, n)) return false;
  return true;
}

// the edges by value on an MI355X (256 CUs, 4 blocks per CU)
static bool check_edges(const hkv::Geometry& g) {
  using hkv::Shape;
  struct RecEdge {
    size_t n;
    Shape shape;
    uint32_t n_pad, grid, n_chunks, first, last;
  };
  const RecEdge rec[] = {
      {4096, Shape::Block, 4096, 256, 1, 4096, 4096},
      {4097, Shape::Pair, 4352, 136, 1, 4352, 4352},
      {32768, Shape::Pair, 32768, 1024, 1, 32768, 32768},
      {32769, Shape::Mid, 33024, 129, 1, 33024, 33024},
      {131072, Shape::Mid, 131072, 512, 1, 131072, 131072},
      {131073, Shape::TableChain, 131328, 0, 1, 131328, 131328},
      {1048576, Shape::TableChain, 1048576, 0, 1, 1048576, 1048576},
      {1048577, Shape::TableChain, 1048832, 0, 2, 1048576, 256},
  };
  for (const RecEdge& e : rec) {
    const hkv::RecPlan p = hkv::plan_records(g, e.n);
    CHECK(p.shape == e.shape && p.n_pad == e.n_pad && p.grid == e.grid, "edge records n=%zu: shape %u n_pad %u grid %u",
          e.n, (unsigned)p.shape, p.n_pad, p.grid);
    CHECK(p.n_chunks == e.n_chunks && p.chunk(0).cn == e.first && p.chunk(p.n_chunks - 1).cn == e.last,
          "edge records n=%zu: chunks", e.n);
    ++g_cases;
  }
  struct StdEdge {
    size_t n;
    Shape shape;
    bool scan, rows, overlap;
    size_t chunk;
  };
  const StdEdge st[] = {
      {4096, Shape::Block, true, true, false, 131072},        {4097, Shape::Pair, false, false, false, 131072},
      {32769, Shape::Mid, false, false, true, 131072},        {131072, Shape::Mid, false, false, true, 131072},
      {131073, Shape::TableChain, false, false, false, 131072}, {262145, Shape::TableChain, false, false, false, 0},
  };
  for (const StdEdge& e : st) {
    const hkv::StdPlan p = hkv::plan_std_chunk(g, e.n);
    CHECK(p.shape == e.shape && p.scan_in_kernel == e.scan && p.rows_in_kernel == e.rows && p.overlap == e.overlap,
          "edge std n=%zu", e.n);
    CHECK(hkv::std_chunk_len(g, e.n) == (e.chunk ? e.chunk : g.std_chunk), "edge std n=%zu: chunk length", e.n);
    ++g_cases;
  }
  return true;
}

int main() {
  const hkv::Geometry geos[] = {
      {256, 1024, (size_t)1 << 20, (size_t)1 << 20},  // MI355X
      {256, 1024, 98304, 196608},                     // ... with the two test hooks the suite uses
      {32, 128, (size_t)1 << 20, (size_t)1 << 20},    // a small partition
      {256, 256, (size_t)1 << 20, (size_t)1 << 20},   // one block per CU
  };
  for (const hkv::Geometry& g : geos)
    if (!check_geometry(g)) return 1;
  if (!check_edges(geos[0])) return 1;
  std::printf("ok %zu\n", g_cases);
  return 0;
}
