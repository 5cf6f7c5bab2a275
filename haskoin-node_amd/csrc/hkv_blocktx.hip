// hkv_blocktx.hip — prevouts created earlier in the same batch, resolved on
// the device from device-computed txids (hkv_verify_block_txs*): the join
// between hkv_txid_kernel and the prevout provider of batch verifyStdTx.
//
//   hkv_txid_table_kernel    one lane per tx: its index into an open-addressing
//                            table keyed by its txid (hkv_blocktx.h
//                            txid_insert: atomicCAS on an empty slot, atomicMin
//                            on a slot of the same txid, the next slot
//                            otherwise). The table is cleared to 0xFF bytes by a
//                            memset on the same stream before the launch.
//   hkv_txid_lookup_kernel   one lane per 32-byte query: the smallest tx index
//                            with that txid, or 0xFFFFFFFF.
//   hkv_blocktx_jobs_kernel  one lane per input, the launch shape of
//                            hkv_stdtx_jobs_kernel: binary search of the prefix
//                            sums, match_prevout on the tx's own list, and on a
//                            miss the lookup and the walk to the parent's
//                            output; one hkv_input_job and one src word.
//
// All three are latency-bound: a probe is a dependent chain of a slot load and
// two 16-byte txid loads (at load factor <= 1/2 about 1.5 probes per hit), the
// output walk a chain of byte reads through the parent, O(parent inputs + k).
// The atomics are one CAS per tx on slots the hash spreads over the table (4
// bytes each, no two lanes of a wave on one slot but for equal txids or a
// collision), far below any rate that would matter. No LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hkv_blocktx.h"
#include "hkv_internal.h"
#include "hkv_layout.h"
#include "../../include/hkv.h"

namespace hkv {

struct DeviceSlotOps {
  static __device__ __forceinline__ uint32_t cas(uint32_t* slot, uint32_t expected, uint32_t desired) {
    return atomicCAS(slot, expected, desired);
  }
  static __device__ __forceinline__ void min(uint32_t* slot, uint32_t v) { atomicMin(slot, v); }
};

__global__ void __launch_bounds__(WG) hkv_txid_table_kernel(TxidTable tb) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= tb.n_tx) return;
  txid_insert<DeviceSlotOps>(tb, t);
}

__global__ void __launch_bounds__(WG) hkv_txid_lookup_kernel(TxidTable tb, const uint8_t* __restrict__ queries,
                                                             uint32_t n_q, uint32_t* __restrict__ found) {
  const uint32_t q = blockIdx.x * WG + threadIdx.x;
  if (q >= n_q) return;
  found[q] = txid_lookup(tb, txid_load_bytes(queries + (size_t)q * 32));
}

// pool_base: where the caller's script pool starts, in bytes from txs (the
// verify reads every reference from txs); pool_len: the pool's length
__global__ void __launch_bounds__(WG) hkv_blocktx_jobs_kernel(const uint8_t* __restrict__ txs,
                                                              const uint32_t* __restrict__ tx_off, uint32_t n_tx,
                                                              const uint32_t* __restrict__ input_first,
                                                              const uint32_t* __restrict__ prev_off,
                                                              const uint8_t* __restrict__ prev_outpoints,
                                                              const uint32_t* __restrict__ prev_scripts,
                                                              const uint64_t* __restrict__ prev_values,
                                                              uint32_t pool_base, uint32_t pool_len, TxidTable tb,
                                                              uint32_t n_inputs, hkv_input_job* __restrict__ jobs,
                                                              uint32_t* __restrict__ input_src) {
  const uint32_t g = blockIdx.x * WG + threadIdx.x;
  if (g >= n_inputs) return;  // nothing is written past the caller's capacity
  hkv_input_job jb;
  jb.tx = 0xFFFFFFFFu;  // a surplus slot: no such tx, the job never verifies
  jb.input = 0;
  jb.script_off = 0;
  jb.script_len = 0;
  jb.value = 0;
  uint32_t src = SRC_NONE;
  if (g < input_first[n_tx]) {
    // the last t with input_first[t] <= g: input_first[t + 1] > g, so tx t has inputs
    uint32_t lo = 0, hi = n_tx;
    while (hi - lo > 1u) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (input_first[mid] <= g) lo = mid;
      else hi = mid;
    }
    const uint32_t t = lo, i = g - input_first[t];
    uint32_t nin;
    const uint32_t ins = tx_inputs_start(txs, tx_off[t], nin);  // (the tx parsed: its count is not 0)
    const uint32_t e0 = prev_off[t], e1 = prev_off[t + 1];
    uint32_t in_off;
    const uint32_t e = match_prevout(txs, ins, i, prev_outpoints + (size_t)e0 * OUTPOINT_BYTES,
                                     e1 > e0 ? e1 - e0 : 0u, in_off);
    const Prevout p = e != NO_PREVOUT
                          ? list_prevout(prev_scripts[2 * ((size_t)e0 + e)], prev_scripts[2 * ((size_t)e0 + e) + 1],
                                         prev_values[(size_t)e0 + e], pool_base, pool_len)
                          : resolve_in_batch(txs, tx_off, t, in_off, tb);
    jb.tx = t;
    jb.input = i;
    jb.script_off = p.script_off;
    jb.script_len = p.script_len;
    jb.value = p.value;
    src = p.src;
  }
  jobs[g] = jb;
  input_src[g] = src;
}

hipError_t launch_txid_table(const TxidTable& tb, hipStream_t st) {
  // empty = 0xFFFFFFFF in every slot
  const hipError_t e = hipMemsetAsync(tb.slots, 0xFF, (size_t)tb.n_slots * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  if (tb.n_tx == 0) return hipSuccess;
  hipLaunchKernelGGL(hkv_txid_table_kernel, dim3((tb.n_tx + WG - 1) / WG), dim3(WG), 0, st, tb);
  return hipGetLastError();
}

hipError_t launch_txid_lookup(const TxidTable& tb, const uint8_t* queries, uint32_t n_q, uint32_t* found,
                              hipStream_t st) {
  if (n_q == 0) return hipSuccess;
  hipLaunchKernelGGL(hkv_txid_lookup_kernel, dim3((n_q + WG - 1) / WG), dim3(WG), 0, st, tb, queries, n_q, found);
  return hipGetLastError();
}

hipError_t launch_blocktx_jobs(const uint8_t* txs, const uint32_t* tx_off, uint32_t n_tx, const uint32_t* input_first,
                               const StdPrevouts& p, uint32_t pool_base, uint32_t pool_len, const TxidTable& tb,
                               uint32_t n_inputs, hkv_input_job* jobs, uint32_t* input_src, hipStream_t st) {
  if (n_inputs == 0) return hipSuccess;
  hipLaunchKernelGGL(hkv_blocktx_jobs_kernel, dim3((n_inputs + WG - 1) / WG), dim3(WG), 0, st, txs, tx_off, n_tx,
                     input_first, p.offsets, p.outpoints, p.scripts, p.values, pool_base, pool_len, tb, n_inputs, jobs,
                     input_src);
  return hipGetLastError();
}

}  // namespace hkv
