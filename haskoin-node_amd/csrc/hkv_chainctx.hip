// hkv_chainctx.hip — the chain-context stage behind hkv_check_headers*: the
// rest of haskoin-core connectBlocks [dep] (hkv_chainctx.h states the rule).
// Every check is a function of a header's actual ancestors, not of earlier
// verdicts, so the stage is three data-parallel launches and a reduction:
//
//   hkv_chain_facts_kernel    one lane per header, a tile of 256 headers per
//                             workgroup staged through LDS by coalesced dword
//                             loads: time, bits and version go to scratch
//                             (structure of arrays), headerWork (an exact
//                             256-bit division) is scanned over the tile and
//                             its inclusive sums go to work_out; the tile's
//                             work total and its last "real bits" value (or
//                             none) go to the tile array.
//   hkv_chain_scan_kernel     one workgroup: the exclusive scan of the tile
//                             elements under both operators (256-bit add with
//                             carry; the later defined value wins), seeded
//                             with the context's parent_work and
//                             period_real_bits, 256 tiles per round.
//   hkv_chain_verdict_kernel  one lane per header: the tile's carry-in added
//                             to work_out in place, real(i) re-scanned with
//                             the carry-in, the tile's times with an
//                             11-header halo and its bits with a 1-header
//                             halo staged in LDS, the median window sorted by
//                             a fixed network, time[i - interval] gathered and
//                             the nine-limb retarget run on boundary lanes, the
//                             checkpoints binary-searched; mtp, want and the
//                             flag byte out.
//   hkv_chain_first_bad_kernel  at most 256 workgroups, each over a contiguous
//                             chunk in ascending steps up to its first failing
//                             header: one atomicMin per workgroup at most.
//
// No workgroup waits for another: stream order is the only synchronisation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hkv_chainctx.h"
#include "hkv_internal.h"
#include "hkv_layout.h"
#include "../../include/hkv.h"

namespace hkv {

static_assert(CHAIN_TILE == (uint32_t)WG, "one lane per header of a tile");
static_assert(CHN_TIME_OK == HKV_CHN_TIME_OK && CHN_NOT_FUTURE == HKV_CHN_NOT_FUTURE &&
                  CHN_BITS_OK == HKV_CHN_BITS_OK && CHN_VERSION_OK == HKV_CHN_VERSION_OK &&
                  CHN_CHECKPOINT_OK == HKV_CHN_CHECKPOINT_OK && CHN_ALL == HKV_CHN_ALL &&
                  CHAIN_NO_RETARGET == HKV_CHAIN_NO_RETARGET && CHAIN_MIN_DIFFICULTY == HKV_CHAIN_MIN_DIFFICULTY,
              "hkv_chainctx.h restates the HKV_CHN_* and HKV_CHAIN_* flags");

namespace {

constexpr int CHAIN_HDR_WORDS = 20;
constexpr uint32_t WAVES = WG / 64;

// the scan element: a 256-bit work sum and a real-bits value
struct ChainSum {
  uint32_t w[8];
  uint64_t real;
};

__device__ __forceinline__ void chain_join(ChainSum& later, const ChainSum& earlier) {
  cc_add256(later.w, later.w, earlier.w);
  later.real = cc_real_join(earlier.real, later.real);
}

// The workgroup's inclusive scan of one element per lane: six shuffle steps
// inside each wave, then the totals of the waves before it from LDS. wave_tot
// holds WAVES elements; the barrier at the end leaves it free for reuse.
__device__ __forceinline__ void chain_block_scan(ChainSum& v, ChainSum* wave_tot) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    ChainSum o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.w[j] = __shfl_up(v.w[j], d, 64);
    o.real = __shfl_up((unsigned long long)v.real, d, 64);
    if (lane >= d) chain_join(v, o);
  }
  if (lane == 63) wave_tot[wave] = v;
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k + 1 < WAVES; ++k) {
    // the totals of the waves before this one, the nearest first: each lies
    // before everything joined so far (the add commutes; the real value stays
    // the latest defined one)
    const uint32_t src = WAVES - 2 - k;
    if (src < wave) chain_join(v, wave_tot[src]);
  }
  __syncthreads();
}

__device__ __forceinline__ void store_sum(uint32_t* p, const ChainSum& v) {
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = v.w[j];
  p[8] = (uint32_t)v.real;
  p[9] = (uint32_t)(v.real >> 32);
}
__device__ __forceinline__ ChainSum load_sum(const uint32_t* p) {
  ChainSum v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v.w[j] = p[j];
  v.real = (uint64_t)p[8] | ((uint64_t)p[9] << 32);
  return v;
}

}  // namespace

__global__ void __launch_bounds__(WG) hkv_chain_facts_kernel(const uint32_t* __restrict__ hdrs, uint32_t n, ChainCtx x,
                                                             uint32_t* __restrict__ times,
                                                             uint32_t* __restrict__ bits_a,
                                                             uint32_t* __restrict__ vers,
                                                             uint32_t* __restrict__ work_out,
                                                             uint32_t* __restrict__ tile_tot) {
  __shared__ uint32_t lds[WG * CHAIN_HDR_WORDS];
  __shared__ ChainSum wave_tot[WAVES];
  const uint32_t t = threadIdx.x;
  const uint32_t base = blockIdx.x * CHAIN_TILE;
  const uint32_t cnt = min(CHAIN_TILE, n - base);
  const uint32_t* src = hdrs + (size_t)base * CHAIN_HDR_WORDS;
  for (uint32_t k = t; k < cnt * CHAIN_HDR_WORDS; k += WG) lds[k] = src[k];
  __syncthreads();
  const uint32_t i = base + t;
  const bool own = t < cnt;
  ChainSum v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v.w[j] = 0;
  v.real = 0;
  if (own) {
    const uint32_t version = lds[t * CHAIN_HDR_WORDS], time = lds[t * CHAIN_HDR_WORDS + 17],
                   bits = lds[t * CHAIN_HDR_WORDS + 18];
    times[i] = time;
    bits_a[i] = bits;
    vers[i] = version;
    cc_header_work(bits, v.w);
    v.real = cc_real_of(x, x.height0 + i, bits);
  }
  chain_block_scan(v, wave_tot);
  if (own) {
    uint32_t* out = work_out + (size_t)i * 8;
    *reinterpret_cast<uint4*>(out) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    *reinterpret_cast<uint4*>(out + 4) = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]);
  }
  // (lanes past cnt added nothing: the last lane holds the tile's element)
  if (t == WG - 1) store_sum(tile_tot + (size_t)blockIdx.x * CHAIN_TILE_WORDS, v);
}

// tile_pre[b] = the context's (parent_work, period_real_bits) joined with tiles
// [0, b). first_bad (or null) is armed with n for the reduction behind the stage.
__global__ void __launch_bounds__(WG) hkv_chain_scan_kernel(const uint32_t* __restrict__ tile_tot, uint32_t n_tiles,
                                                            ChainCtx x, uint32_t* __restrict__ tile_pre,
                                                            uint32_t* __restrict__ first_bad, uint32_t n) {
  __shared__ ChainSum wave_tot[WAVES];
  __shared__ ChainSum incl[WG];
  const uint32_t t = threadIdx.x;
  if (t == 0 && first_bad) *first_bad = n;
  ChainSum carry;
#pragma unroll
  for (int j = 0; j < 8; ++j) carry.w[j] = x.parent_work[j];
  carry.real = (1ull << 32) | x.period_real_bits;
  for (uint32_t c0 = 0; c0 < n_tiles; c0 += WG) {  // n_tiles is workgroup-uniform: every barrier is reached by all lanes
    const uint32_t b = c0 + t;
    ChainSum v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v.w[j] = 0;
    v.real = 0;
    if (b < n_tiles) v = load_sum(tile_tot + (size_t)b * CHAIN_TILE_WORDS);
    chain_block_scan(v, wave_tot);
    incl[t] = v;
    __syncthreads();
    ChainSum pre = carry;
    if (t) {
      pre = incl[t - 1];
      chain_join(pre, carry);
    }
    if (b < n_tiles) store_sum(tile_pre + (size_t)b * CHAIN_TILE_WORDS, pre);
    ChainSum all = incl[WG - 1];
    chain_join(all, carry);
    carry = all;
    __syncthreads();  // incl is rewritten by the next round
  }
}

__global__ void __launch_bounds__(WG) hkv_chain_verdict_kernel(uint32_t n, ChainCtx x,
                                                               const uint32_t* __restrict__ times,
                                                               const uint32_t* __restrict__ bits_a,
                                                               const uint32_t* __restrict__ vers,
                                                               const uint32_t* __restrict__ tile_pre,
                                                               const uint32_t* __restrict__ hashes,
                                                               const uint32_t* __restrict__ cp_heights,
                                                               const uint32_t* __restrict__ cp_hashes, uint32_t n_cp,
                                                               uint32_t* __restrict__ mtp_out,
                                                               uint32_t* __restrict__ bits_out, uint32_t* work_out,
                                                               uint8_t* __restrict__ status) {
  __shared__ uint32_t lt[WG + CHAIN_MTP_SPAN];  // slot k: the time of header base - 11 + k
  __shared__ uint32_t lb[WG + 1];               // slot k: the bits of header base - 1 + k
  __shared__ uint64_t lr[WG];                   // real(i) of the tile's lanes
  __shared__ ChainSum wave_tot[WAVES];
  const uint32_t t = threadIdx.x;
  const uint32_t base = blockIdx.x * CHAIN_TILE;
  const uint32_t cnt = min(CHAIN_TILE, n - base);
  for (uint32_t k = t; k < cnt + CHAIN_MTP_SPAN; k += WG) {
    const int64_t h = (int64_t)base + k - CHAIN_MTP_SPAN;
    uint32_t v = 0xFFFFFFFFu;  // before the context's oldest time: the window's padding
    if (h >= 0) {
      v = times[h];
    } else if (-h <= (int64_t)x.n_prev_times) {
      const uint32_t idx = x.n_prev_times - (uint32_t)(-h);
#pragma unroll
      for (uint32_t j = 0; j < CHAIN_MTP_SPAN; ++j)
        if (j == idx) v = x.prev_times[j];
    }
    lt[k] = v;
  }
  for (uint32_t k = t; k < cnt + 1; k += WG) lb[k] = (base + k) ? bits_a[base + k - 1] : x.parent_bits;
  __syncthreads();
  const uint32_t i = base + t;
  const bool own = t < cnt;
  const ChainSum pre = load_sum(tile_pre + (size_t)blockIdx.x * CHAIN_TILE_WORDS);

  ChainIn in;
  in.H = x.height0 + i;
  in.time = lt[own ? t + CHAIN_MTP_SPAN : 0];
  in.bits = lb[own ? t + 1 : 0];
  in.version = own ? vers[i] : 0;

  // real(i): the tile's scan again, with the carry-in (the work sums of the
  // tile came from the facts launch: only the carry-in is added)
  ChainSum v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v.w[j] = 0;
  v.real = own ? cc_real_of(x, in.H, in.bits) : 0;
  chain_block_scan(v, wave_tot);
  lr[t] = cc_real_join(pre.real, v.real);
  __syncthreads();
  if (!own) return;

  uint32_t* wp = work_out + (size_t)i * 8;
  const uint4 a = *reinterpret_cast<const uint4*>(wp), b = *reinterpret_cast<const uint4*>(wp + 4);
  uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  cc_add256(w, w, pre.w);
  *reinterpret_cast<uint4*>(wp) = make_uint4(w[0], w[1], w[2], w[3]);
  *reinterpret_cast<uint4*>(wp + 4) = make_uint4(w[4], w[5], w[6], w[7]);

  in.parent_time = lt[t + CHAIN_MTP_SPAN - 1];
  in.parent_bits = lb[t];
  in.parent_real = (uint32_t)(t ? lr[t - 1] : pre.real);
  in.first_time = x.period_first_time;
  if (in.H % x.interval == 0 && i >= x.interval) in.first_time = times[i - x.interval];
#pragma unroll
  for (uint32_t j = 0; j < CHAIN_MTP_SPAN; ++j) in.window[j] = lt[t + CHAIN_MTP_SPAN - 1 - j];
  const uint64_t before = (uint64_t)i + x.n_prev_times;
  in.c = before < CHAIN_MTP_SPAN ? (uint32_t)before : CHAIN_MTP_SPAN;
  in.checkpoint_ok = true;
  if (n_cp) {
    const uint32_t c = cc_checkpoint_at(cp_heights, n_cp, in.H);
    if (c != CHAIN_CP_NONE) {
      uint32_t diff = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) diff |= hashes[(size_t)i * 8 + j] ^ cp_hashes[(size_t)c * 8 + j];
      in.checkpoint_ok = diff == 0;
    }
  }
  uint32_t mtp, want;
  const uint32_t fl = chain_verdict(x, in, mtp, want);
  mtp_out[i] = mtp;
  bits_out[i] = want;
  status[i] = (uint8_t)fl;
}

// first_bad = min(first_bad, the smallest i whose chain flags are not all set
// or whose header status lacks POW_OK or LINK_OK); armed with n by the scan
// launch. At most FIRST_BAD_GROUPS workgroups, each over one contiguous chunk
// of the batch (a multiple of WG headers) in ascending steps of WG: it stops at
// the first step that holds a failing header and sends that step's minimum with
// one atomicMin. So the word sees at most FIRST_BAD_GROUPS atomics whatever
// fails, and a chunk is read only up to its first failure.
constexpr uint32_t FIRST_BAD_GROUPS = 256;

__global__ void __launch_bounds__(WG) hkv_chain_first_bad_kernel(const uint8_t* __restrict__ hdr_status,
                                                                 const uint8_t* __restrict__ chain_status, uint32_t n,
                                                                 uint32_t chunk, uint32_t* first_bad) {
  __shared__ uint32_t wave_min[WAVES];
  const uint32_t begin = blockIdx.x * chunk;  // < n: the grid is ceil(n / chunk)
  const uint32_t end = n - begin < chunk ? n : begin + chunk;
  // (base + WG cannot wrap: base < n <= 0xFFFFFF00)
  for (uint32_t base = begin; base < end; base += WG) {
    const uint32_t i = base + threadIdx.x;
    uint32_t v = 0xFFFFFFFFu;
    if (i < end) {
      const uint32_t need = HKV_HDR_POW_OK | HKV_HDR_LINK_OK;
      if ((chain_status[i] & CHN_ALL) != CHN_ALL || (hdr_status[i] & need) != need) v = i;
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, 64));
    if ((threadIdx.x & 63u) == 0) wave_min[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t m = wave_min[0];
#pragma unroll
    for (uint32_t k = 1; k < WAVES; ++k) m = min(m, wave_min[k]);
    __syncthreads();  // wave_min is rewritten by the next step
    if (m != 0xFFFFFFFFu) {  // m is the same in every lane: the whole workgroup leaves
      if (threadIdx.x == 0) atomicMin(first_bad, m);
      return;
    }
  }
}

hipError_t launch_chain_context(const ChainStage& s, uint32_t stages, hipStream_t st) {
  if (s.n == 0) return hipSuccess;
  const uint32_t tiles = (uint32_t)chain_tiles(s.n);
  uint32_t* times = s.scratch;
  uint32_t* bits_a = times + s.n;
  uint32_t* vers = bits_a + s.n;
  uint32_t* tile_tot = vers + s.n;
  uint32_t* tile_pre = tile_tot + (size_t)tiles * CHAIN_TILE_WORDS;
  if (stages & CHAIN_STAGE_FACTS) {
    hipLaunchKernelGGL(hkv_chain_facts_kernel, dim3(tiles), dim3(WG), 0, st,
                       reinterpret_cast<const uint32_t*>(s.headers), s.n, s.ctx, times, bits_a, vers, s.work, tile_tot);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (stages & CHAIN_STAGE_SCAN) {
    hipLaunchKernelGGL(hkv_chain_scan_kernel, dim3(1), dim3(WG), 0, st, tile_tot, tiles, s.ctx, tile_pre, s.first_bad,
                       s.n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (stages & CHAIN_STAGE_VERDICT) {
    hipLaunchKernelGGL(hkv_chain_verdict_kernel, dim3(tiles), dim3(WG), 0, st, s.n, s.ctx, times, bits_a, vers,
                       tile_pre, reinterpret_cast<const uint32_t*>(s.hashes), s.cp_heights,
                       reinterpret_cast<const uint32_t*>(s.cp_hashes), s.n_cp, s.mtp, s.bits, s.work, s.status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (s.first_bad && (stages & CHAIN_STAGE_FIRST_BAD)) {
    const uint32_t groups = tiles < FIRST_BAD_GROUPS ? tiles : FIRST_BAD_GROUPS;
    const uint32_t chunk = (tiles + groups - 1) / groups * WG;  // a multiple of WG; groups * chunk >= n
    hipLaunchKernelGGL(hkv_chain_first_bad_kernel, dim3((s.n + chunk - 1) / chunk), dim3(WG), 0, st, s.hdr_status,
                       s.status, s.n, chunk, s.first_bad);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace hkv
