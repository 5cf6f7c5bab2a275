// hkv_launch_plan.h — which launches a batch runs, and with which grids: the
// one place that turns "n records (or standard inputs) on this device" into
// a launch shape. hkv_api.cpp computes a plan first and reads everything else
// from it; the launch wrappers at the end of hkv_kernels.hip switch on its
// shape and decide nothing themselves. Pure C++ (no HIP), so
// tests/launch_plan.cpp drives exactly this code under ASan and UBSan on the
// CPU, against the expressions it replaced.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hkv_layout.h"

namespace hkv {

// The device facts fixed at hkv_open (hkv_api.cpp init_device).
struct Geometry {
  uint32_t n_cu = 0;
  uint32_t grid_max = 0;  // the resident grid: ecmult blocks of WG lanes (blocks per CU x CUs)
  // signatures per table / chain launch pair of a record batch above the
  // mid-size range (default HKV_REC_CHUNK; env HKV_REC_CHUNK at open, for
  // tests: a multiple of WG)
  size_t rec_chunk = 0;
  // standard inputs per chunk of a batch past one resident grid (default
  // 2^20; env HKV_STD_CHUNK at open, for tests: a multiple of 64)
  size_t std_chunk = 0;
  // signatures per part of a table / chain batch that runs as a two-stream
  // pipeline (RecPlan::part_len; default HKV_REC_PART; env HKV_REC_PART at
  // open, for tests: rounded up to PART_ALIGN). 0: no parts, every chunk runs
  // whole on the caller's stream
  size_t rec_part = 0;
};

// Part boundaries are whole workgroups and whole groups of VERDICT_BATCH
// verdict words, so no verdict word and no batched-inversion group of a
// windowed launch straddles two parts.
constexpr size_t PART_ALIGN = (size_t)VERDICT_BATCH * 32 % WG == 0 ? (size_t)VERDICT_BATCH * 32
                                                                   : (size_t)VERDICT_BATCH * 32 * WG;
static_assert(PART_ALIGN % WG == 0 && PART_ALIGN % ((size_t)VERDICT_BATCH * 32) == 0, "part alignment");

// A batch of at most 1 / SPLIT_DIV of the resident grid (half a wave per SIMD)
// runs a small-batch kernel: a shorter dependency chain where latency, not
// issue, bounds the launch. Above that the duplicated doublings cost more than
// the chain saves (measured: a 115k batch at ~1.8 waves/SIMD took 2.1 ms split
// vs 1.5 ms unsplit; the bound re-measured in profiles/r02_split_threshold.log).
constexpr size_t SPLIT_DIV = 8;
// smaller batches keep at least this many lanes (or one per signature) in the
// two batched-inversion kernels, so the latency of their sequential per-lane
// products does not dominate
constexpr uint32_t MIN_INV_LANES = 65536;

enum class Shape : uint32_t {
  Block = 1,       // at most BLK_SIGS signatures per CU: hkv_block_kernel, one launch
  Pair = 2,        // up to 1 / SPLIT_DIV of the resident grid: hkv_pair_split_kernel, one launch
  Mid = 3,         // up to half the resident grid (2 waves per SIMD): the paired-form ecmult instance
  TableChain = 4,  // above: a table and a chain launch per chunk of rec_chunk signatures
};

struct RecChunk {
  uint32_t i0, cn;  // signatures [i0, i0 + cn) of the padded batch
};

struct RecPlan {
  Shape shape;
  uint32_t n_pad;  // n rounded up to WG
  // the main launch's blocks: n_pad / BLK_SIGS, n_pad / PAIR_SIGS, the
  // mid-size instance's n_pad / WG (never above grid_max / 2, which the min
  // below restates); 0 for the table / chain launches (chunk(k).cn / WG each)
  uint32_t grid;
  // Mid and TableChain only: the prologue launches before the main one (a
  // mid-size standard-input batch runs its lane prologue inside the main
  // launch instead) and the finish launches after it
  bool prologue;
  bool aux;  // Block and Pair: the in-kernel join reads aux (AUX_WORDS per signature)
  // lanes of the s^-1 kernel (BATCH_INV signatures per lane at large n) and of
  // the verdict kernel (VERDICT_BATCH per lane; a multiple of WG, as n_pad is)
  uint32_t inv_stride, verdict_stride;
  // Q-table scratch, in quads (16 B): one table per lane of the resident grid
  // for every shape up to the mid-size one and the multisig tail; above it, a
  // table and a Zg slot per signature of one chunk (800 B each: 839 MB at the
  // default 2^20, whatever n) when that is more
  size_t qs_quads;
  // TableChain: chunk(0 .. n_chunks) cover [0, n_pad) in order; else one chunk, the batch
  uint32_t chunk_len, n_chunks;
  RecChunk chunk(uint32_t k) const {
    const uint64_t i0 = (uint64_t)k * chunk_len;  // (64-bit: n_pad may be within a chunk of 2^32)
    const uint64_t left = n_pad - i0;
    return RecChunk{(uint32_t)i0, (uint32_t)(left < chunk_len ? left : chunk_len)};
  }
  // TableChain: part(0 .. n_parts) cover [0, n_pad) in order, each through
  // table, chain, finish, rare and verdict launches of its own window. With
  // qs_slots == 2 the parts cut the batch, not a chunk, every part_len
  // signatures (a multiple of PART_ALIGN), and part k runs on stream
  // part_stream(k) with its tables and Zg slots in slot part_slot(k) of qs,
  // part_len * (QTAB_QUADS + QTAB_ZG_QUADS) quads each, beside part k + 1 in
  // the other. With one slot the parts are the chunks, one after another on
  // the caller's stream, and the finish launches take the whole batch as one
  // window. Other shapes: one part, the batch.
  uint32_t part_len, n_parts, qs_slots;
  RecChunk part(uint32_t k) const {
    const uint64_t i0 = (uint64_t)k * part_len;
    const uint64_t left = n_pad - i0;
    return RecChunk{(uint32_t)i0, (uint32_t)(left < part_len ? left : part_len)};
  }
  // the stream (0 the caller's, 1 the pipe stream) and the qs slot of part k
  // of a two-slot plan. Both alternate, so the part that overwrites a slot
  // follows the slot's last chain launch in its own stream's order: the
  // pipeline (hkv_api.cpp enqueue_table_chain) checks that per part, and
  // tests/pipe_plan.cpp models it
  static constexpr uint32_t part_stream(uint32_t k) { return k & 1u; }
  static constexpr uint32_t part_slot(uint32_t k) { return k & 1u; }
  size_t slot_quads(uint32_t slot) const { return (size_t)slot * part_len * (QTAB_QUADS + QTAB_ZG_QUADS); }
};

namespace plan_detail {
inline size_t round_up(size_t a, size_t b) { return (a + b - 1) / b * b; }
inline size_t grid_lanes(const Geometry& g) { return (size_t)g.grid_max * WG; }
inline Shape shape_of(const Geometry& g, size_t n_pad) {
  if (n_pad > grid_lanes(g) / 2) return Shape::TableChain;
  if (n_pad > grid_lanes(g) / SPLIT_DIV) return Shape::Mid;
  return n_pad <= (size_t)BLK_SIGS * g.n_cu ? Shape::Block : Shape::Pair;
}
}  // namespace plan_detail

// The verdict kernel's lanes for a window of cn signatures (a multiple of WG):
// VERDICT_BATCH per lane, whole workgroups, at least MIN_INV_LANES (or one per
// signature). At most cn, so every lane's first signature lies in the window.
inline uint32_t verdict_stride_of(size_t cn) {
  const size_t min_lanes = cn < MIN_INV_LANES ? cn : MIN_INV_LANES;
  const size_t ver = plan_detail::round_up((cn + VERDICT_BATCH - 1) / VERDICT_BATCH, WG);
  return (uint32_t)(ver < min_lanes ? min_lanes : ver);
}

// A batch of n records (1 <= n <= 0xFFFFFF00) at once on this device.
inline RecPlan plan_records(const Geometry& g, size_t n) {
  using namespace plan_detail;
  const size_t n_pad = round_up(n, WG);
  RecPlan p{};
  p.shape = shape_of(g, n_pad);
  p.n_pad = (uint32_t)n_pad;
  const bool small = p.shape == Shape::Block || p.shape == Shape::Pair;
  p.prologue = !small;
  p.aux = small;
  const size_t blocks = n_pad / WG;
  switch (p.shape) {
    case Shape::Block: p.grid = (uint32_t)(n_pad / BLK_SIGS); break;
    case Shape::Pair: p.grid = (uint32_t)(n_pad / PAIR_SIGS); break;
    case Shape::Mid: p.grid = (uint32_t)(blocks < g.grid_max / 2 ? blocks : g.grid_max / 2); break;
    case Shape::TableChain: p.grid = 0; break;
  }
  const size_t min_lanes = n_pad < MIN_INV_LANES ? n_pad : MIN_INV_LANES;
  const size_t inv = (n_pad + BATCH_INV - 1) / BATCH_INV;
  p.inv_stride = (uint32_t)(inv > MIN_INV_LANES ? inv : min_lanes);
  p.verdict_stride = verdict_stride_of(n_pad);
  p.qs_quads = grid_lanes(g) * QTAB_QUADS;
  p.chunk_len = p.n_pad;
  p.n_chunks = 1;
  if (p.shape == Shape::TableChain) {
    const size_t chunk = n_pad < g.rec_chunk ? n_pad : g.rec_chunk;
    const size_t quads = chunk * (QTAB_QUADS + QTAB_ZG_QUADS);
    if (quads > p.qs_quads) p.qs_quads = quads;
    p.chunk_len = (uint32_t)chunk;
    p.n_chunks = (uint32_t)((n_pad + chunk - 1) / chunk);
  }
  p.part_len = p.chunk_len;
  p.n_parts = p.n_chunks;
  p.qs_slots = 1;
  if (p.shape == Shape::TableChain && g.rec_part != 0) {
    // two parts in flight: more than one part, none longer than a chunk, and
    // both slots inside the scratch the plan reserves anyway
    const size_t part = round_up(g.rec_part, PART_ALIGN);
    if (part < n_pad && part <= p.chunk_len && 2 * part * (QTAB_QUADS + QTAB_ZG_QUADS) <= p.qs_quads) {
      p.part_len = (uint32_t)part;
      p.n_parts = (uint32_t)((n_pad + part - 1) / part);
      p.qs_slots = 2;
    }
  }
  return p;
}

// Where the multisig scan of a chunk of standard inputs runs.
enum class ScanOn : uint32_t {
  Kernel = 0,      // on the block kernel's signature wave
  MainStream = 1,  // hkv_ms_scan_kernel on the caller's stream
  HashStream = 2,  // ... on the hash stream, beside the Q chains
};

struct StdPlan {
  Shape shape;
  uint32_t n_pad;
  // Block: the kernel runs the multisig scan on its signature wave and builds
  // the index rows of its inputs' txs itself (kernel 2d txc_fill)
  bool scan_in_kernel, rows_in_kernel;
  // Mid: the hash half (BIP143 per-tx hashes, script checks, sighashes, the
  // multisig scan) runs on the hash stream beside the parse half and the Q
  // chains, and the main stream joins it before the finish launches
  bool overlap;
  // what follows from them
  bool index_first;   // a tx index launch comes before everything else (all but Block)
  // whether that launch computes the BIP143 per-tx hashes the network allows
  // (TableChain: the plain extraction) or none (TX_HASHES_NONE), and whether
  // the multisig tail computes them first (Block and Pair: their index hashed
  // nothing); at Mid the hash stream's own launch computes them
  bool index_hashes, tail_hashes;
  ScanOn scan;
};

// One chunk of n standard inputs (std_chunk_len) on this device.
inline StdPlan plan_std_chunk(const Geometry& g, size_t n) {
  using namespace plan_detail;
  const size_t n_pad = round_up(n, WG);
  StdPlan p{};
  p.shape = shape_of(g, n_pad);
  p.n_pad = (uint32_t)n_pad;
  p.scan_in_kernel = p.rows_in_kernel = p.shape == Shape::Block;
  p.overlap = p.shape == Shape::Mid;
  p.index_first = !p.rows_in_kernel;
  p.index_hashes = p.shape == Shape::TableChain;
  p.tail_hashes = p.shape == Shape::Block || p.shape == Shape::Pair;
  p.scan = p.scan_in_kernel ? ScanOn::Kernel : p.overlap ? ScanOn::HashStream : ScanOn::MainStream;
  return p;
}

// The chunk length of a batch of n standard inputs: at most one resident grid
// runs in half-grid chunks (131,072 inputs on an MI355X: the overlapped
// mid-size form), a larger batch in chunks of std_chunk through the plain
// extraction and the table / chain launches. (Round 6: 1,007,894 inputs in
// 128k chunks took 15.96 ms, 63 M inputs/s, profiles/r06y/.)
inline size_t std_chunk_len(const Geometry& g, size_t n) {
  return n > plan_detail::grid_lanes(g) ? g.std_chunk : plan_detail::grid_lanes(g) / 2;
}

}  // namespace hkv
