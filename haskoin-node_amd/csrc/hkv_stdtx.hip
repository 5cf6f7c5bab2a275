// hkv_stdtx.hip — batch verifyStdTx around the standard-input verify: the
// prevout provider before it and the per-tx reduction after it.
//
// haskoin-core verifyStdTx [dep, haskoin-core-1.1.0 Haskoin.Transaction.Builder]
//
//   verifyStdTx net ctx tx xs =
//       not (null tx.inputs) && all go (zip (matchTemplate xs tx.inputs f) [0..])
//     where f (_,_,o) txin = o == txin.outpoint
//           go (Just (so,val,_), i) = verifyStdInput net ctx tx i so val
//           go _                    = False
//
// takes a decoded tx and an unordered prevout list keyed by outpoint. Here the
// txs are the wire bytes of an hkv_txs batch and tx t's list is the entries
// [prev_off[t], prev_off[t+1]) of three plain arrays (36-byte outpoints,
// (offset, length) script references into the batch's script pool, amounts):
//
//   hkv_stdtx_count_kernel   one lane per tx: its input count from
//                            tx_index_row, 0 for a tx that does not parse.
//   hkv_stdtx_scan_kernel    the counts' exclusive prefix sum in tx order, in
//                            place: input g of the batch is input i of tx t in
//                            tx-major order, so slots cannot be handed out by
//                            an atomic counter. One workgroup walks the array
//                            in tiles (8 counts per lane, a wave scan by
//                            shuffles, the 16 wave sums through LDS, a running
//                            carry): no other workgroup to wait for and no
//                            scratch, at 2 x 4 bytes of traffic per tx.
//   hkv_stdtx_jobs_kernel    one lane per input: binary search of the prefix
//                            sums for its tx, then the matching rule of
//                            hkv_stdtx.h (the walk to its input, the rank among
//                            equal outpoints, the scan of the tx's entries) and
//                            one hkv_input_job.
//   hkv_tx_verdict_kernel    one lane per tx: all of its inputs' verdict bits,
//                            word-wise with head and tail masks; 64 tx bits
//                            per wave by ballot.
//
// All four are small and latency-bound (dependent byte reads of the tx walk);
// none uses LDS beyond the scan's 16 words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hkv_sighash_dev.h"
#include "hkv_stdtx.h"
#include "hkv_internal.h"
#include "../../include/hkv.h"

namespace hkv {

constexpr int SCAN_WG = 1024;                   // the scan's one workgroup: 16 waves
constexpr int SCAN_PER_LANE = 8;                // consecutive counts a lane scans serially
constexpr int SCAN_TILE = SCAN_WG * SCAN_PER_LANE;

__global__ void __launch_bounds__(WG) hkv_stdtx_count_kernel(const uint8_t* __restrict__ txs,
                                                             const uint32_t* __restrict__ tx_off, uint32_t n_tx,
                                                             uint32_t* __restrict__ input_first) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= n_tx) return;
  uint32_t row[8];
  tx_index_row(txs, tx_off, t, row);
  input_first[t] = (row[TXT_FLAGS] & TXF_OK) ? row[TXT_NIN] : 0u;
}

// a[0, n) counts -> their exclusive prefix sums, a[n] = the total; the total
// is compared with the caller's n_inputs
__global__ void __launch_bounds__(SCAN_WG) hkv_stdtx_scan_kernel(uint32_t* __restrict__ a, uint32_t n,
                                                                 uint32_t n_inputs, uint32_t* __restrict__ status) {
  __shared__ uint32_t wave_sum[SCAN_WG / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t carry = 0;
  // the lane's words of the tile at base, loaded without a branch: an index
  // past the counts reads a[n] (the slot of the total, never a count) and is
  // masked when it is used, so the loads stay in flight until then
  auto load_tile = [&](uint64_t base, uint32_t (&c)[SCAN_PER_LANE]) {
    const uint64_t at = base + (uint64_t)tid * SCAN_PER_LANE;
#pragma unroll
    for (int k = 0; k < SCAN_PER_LANE; ++k) c[k] = a[at + k < n ? at + k : (uint64_t)n];
  };
  uint32_t cur[SCAN_PER_LANE], nxt[SCAN_PER_LANE];
  load_tile(0, cur);
  for (uint64_t base = 0; base < n; base += SCAN_TILE) {
    // the next tile's loads are issued before this one is scanned (the tiles
    // are a serial chain). Measured, this hides little: a tile's time is in its
    // 32-byte lane stride, DESIGN.md §4.7
    load_tile(base + SCAN_TILE, nxt);
    const uint64_t at = base + (uint64_t)tid * SCAN_PER_LANE;
    uint32_t v[SCAN_PER_LANE], mine = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_LANE; ++k) {
      v[k] = mine;  // exclusive within the lane
      mine += at + k < n ? cur[k] : 0u;
    }
    uint32_t incl = mine;  // inclusive over the wave's lanes
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t up = __shfl_up(incl, s);
      if (lane >= (uint32_t)s) incl += up;
    }
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = carry, tile = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WG / 64; ++w) {
      const uint32_t s = wave_sum[w];
      before += (uint32_t)w < wave ? s : 0u;
      tile += s;
    }
    before += incl - mine;
#pragma unroll
    for (int k = 0; k < SCAN_PER_LANE; ++k)
      if (at + k < n) a[at + k] = before + v[k];
    carry += tile;
    __syncthreads();  // (wave_sum is rewritten by the next tile)
#pragma unroll
    for (int k = 0; k < SCAN_PER_LANE; ++k) cur[k] = nxt[k];
  }
  if (tid == 0) {
    a[n] = carry;
    if (carry != n_inputs) atomicOr(status, HKV_STATUS_INPUT_COUNT);
  }
}

__global__ void __launch_bounds__(WG) hkv_stdtx_jobs_kernel(const uint8_t* __restrict__ txs,
                                                            const uint32_t* __restrict__ tx_off, uint32_t n_tx,
                                                            const uint32_t* __restrict__ input_first,
                                                            const uint32_t* __restrict__ prev_off,
                                                            const uint8_t* __restrict__ prev_outpoints,
                                                            const uint32_t* __restrict__ prev_scripts,
                                                            const uint64_t* __restrict__ prev_values,
                                                            uint32_t n_inputs, hkv_input_job* __restrict__ jobs) {
  const uint32_t g = blockIdx.x * WG + threadIdx.x;
  if (g >= n_inputs) return;  // nothing is written past the caller's capacity
  hkv_input_job jb;
  jb.tx = 0xFFFFFFFFu;  // a surplus slot: no such tx, the job never verifies
  jb.input = 0;
  jb.script_off = 0;
  jb.script_len = 0;
  jb.value = 0;
  if (g < input_first[n_tx]) {
    // the last t with input_first[t] <= g: input_first[t + 1] > g, so tx t has inputs
    uint32_t lo = 0, hi = n_tx;
    while (hi - lo > 1u) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (input_first[mid] <= g) lo = mid;
      else hi = mid;
    }
    const uint32_t t = lo, i = g - input_first[t];
    // the tx parsed (its count is not 0): its inputs start as tx_index_row found them
    uint32_t off = tx_off[t] + 4u;
    if (txs[off] == 0u && txs[off + 1] == 1u) off += 2u;
    (void)get_varint(txs, off);
    const uint32_t e0 = prev_off[t], e1 = prev_off[t + 1];
    uint32_t in_off;
    const uint32_t e = match_prevout(txs, off, i, prev_outpoints + (size_t)e0 * OUTPOINT_BYTES,
                                     e1 > e0 ? e1 - e0 : 0u, in_off);
    jb.tx = t;
    jb.input = i;
    if (e != NO_PREVOUT) {  // (an unmatched input keeps script_len 0: no template, verifies false)
      jb.script_off = prev_scripts[2 * ((size_t)e0 + e)];
      jb.script_len = prev_scripts[2 * ((size_t)e0 + e) + 1];
      jb.value = prev_values[(size_t)e0 + e];
    }
  }
  jobs[g] = jb;
}

// tx bit t = its input range is not empty and every input bit in it is 1.
// status (the composed call; else null): a batch whose input count differed
// from the caller's has no verdicts — its ranges do not describe input_bits
__global__ void __launch_bounds__(WG) hkv_tx_verdict_kernel(const uint32_t* __restrict__ input_first, uint32_t n_tx,
                                                            const uint32_t* __restrict__ input_bits,
                                                            const uint32_t* __restrict__ status,
                                                            uint32_t* __restrict__ tx_bits) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  bool ok = false;
  if (t < n_tx && !(status != nullptr && (*status & HKV_STATUS_INPUT_COUNT))) {
    const uint32_t b = input_first[t], e = input_first[t + 1];
    ok = e > b;
    if (ok) {
      const uint32_t w0 = b >> 5, w1 = (e - 1u) >> 5;
      for (uint32_t w = w0; w <= w1; ++w) {
        uint32_t mask = 0xFFFFFFFFu;
        if (w == w0) mask &= 0xFFFFFFFFu << (b & 31u);
        if (w == w1) mask &= 0xFFFFFFFFu >> (31u - ((e - 1u) & 31u));
        ok = ok && (input_bits[w] & mask) == mask;
      }
    }
  }
  const unsigned long long word = __ballot(ok);
  const uint32_t first = t & ~63u;  // the wave's first tx
  if ((threadIdx.x & 63u) == 0 && first < n_tx) {
    tx_bits[2 * (size_t)(first >> 6)] = (uint32_t)word;
    tx_bits[2 * (size_t)(first >> 6) + 1] = (uint32_t)(word >> 32);
  }
}

hipError_t launch_stdtx_counts(const uint8_t* txs, const uint32_t* tx_off, uint32_t n_tx, uint32_t n_inputs,
                               uint32_t* input_first, uint32_t* status, hipStream_t st) {
  if (n_tx != 0) {
    hipLaunchKernelGGL(hkv_stdtx_count_kernel, dim3((n_tx + WG - 1) / WG), dim3(WG), 0, st, txs, tx_off, n_tx,
                       input_first);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(hkv_stdtx_scan_kernel, dim3(1), dim3(SCAN_WG), 0, st, input_first, n_tx, n_inputs, status);
  return hipGetLastError();
}

hipError_t launch_stdtx_jobs(const uint8_t* txs, const uint32_t* tx_off, uint32_t n_tx, const uint32_t* input_first,
                             const StdPrevouts& p, uint32_t n_inputs, hkv_input_job* jobs, hipStream_t st) {
  if (n_inputs == 0) return hipSuccess;
  hipLaunchKernelGGL(hkv_stdtx_jobs_kernel, dim3((n_inputs + WG - 1) / WG), dim3(WG), 0, st, txs, tx_off, n_tx,
                     input_first, p.offsets, p.outpoints, p.scripts, p.values, n_inputs, jobs);
  return hipGetLastError();
}

hipError_t launch_tx_verdicts(const uint32_t* input_first, uint32_t n_tx, const uint32_t* input_bits,
                              const uint32_t* status, uint32_t* tx_bits, hipStream_t st) {
  if (n_tx == 0) return hipSuccess;
  hipLaunchKernelGGL(hkv_tx_verdict_kernel, dim3((n_tx + WG - 1) / WG), dim3(WG), 0, st, input_first, n_tx,
                     input_bits, status, tx_bits);
  return hipGetLastError();
}

}  // namespace hkv
