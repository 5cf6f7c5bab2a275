// hkv_spends.hip — whole-block spend checks behind hkv_verify_block_txs*: the
// first spender of every outpoint of the batch and each tx's value balance
// (hkv_block_spends_device), from what the block call leaves in HBM: the tx
// bytes, the input prefix sums, the resolved amount of every input and its src.
//
//   hkv_spend_walk_kernel    one lane per tx with inputs: the offset of every
//                            input's outpoint, then on over the outputs for
//                            their exact sum (hkv_spends.h spend_walk). Lane 0
//                            compares the device's input total with the
//                            caller's and ORs HKV_STATUS_INPUT_COUNT in.
//   hkv_spend_table_kernel   one lane per input: its index into an
//                            open-addressing table keyed by its 36-byte outpoint
//                            (spend_insert: atomicCAS on an empty slot,
//                            atomicMin on a slot of the same outpoint, the next
//                            slot otherwise). The table is cleared to 0xFF bytes
//                            by a memset on the same stream before the launch.
//   hkv_spender_kernel       one lane per input slot: the smallest input index
//                            with its outpoint, by a lookup in the finished
//                            table; 0xFFFFFFFF past the device's input total.
//   hkv_tx_spend_kernel      one lane per tx: the fold over its inputs (amount,
//                            src, spender) into the flag byte and the two sums.
//
// Stream order is the only synchronisation between them. All four are
// latency-bound chains of dependent loads (the byte reads of the tx walk; a
// probe is a slot load, an offset load and up to nine unaligned words of the
// holder's outpoint); none uses LDS. One lane walks one tx and folds one tx's
// inputs: a tx of 100,000 inputs is one lane's serial chain.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hkv_spends.h"
#include "hkv_internal.h"
#include "hkv_layout.h"
#include "../../include/hkv.h"

namespace hkv {

static_assert(sizeof(hkv_input_job) == SPEND_JOB_WORDS * 8 && offsetof(hkv_input_job, value) == SPEND_JOB_VALUE * 8,
              "job_value reads hkv_input_job::value");
static_assert(SPEND_RESOLVED == HKV_SPEND_RESOLVED && SPEND_FIRST == HKV_SPEND_FIRST &&
                  SPEND_IN_RANGE == HKV_SPEND_IN_RANGE && SPEND_OUT_RANGE == HKV_SPEND_OUT_RANGE &&
                  SPEND_BALANCED == HKV_SPEND_BALANCED && SPEND_COINBASE == HKV_SPEND_COINBASE &&
                  HKV_SPEND_OK == (SPEND_RESOLVED | SPEND_FIRST | SPEND_IN_RANGE | SPEND_OUT_RANGE | SPEND_BALANCED),
              "hkv_spends.h restates the HKV_SPEND_* flags");

namespace {
struct DeviceSpendOps {
  static __device__ __forceinline__ uint32_t cas(uint32_t* slot, uint32_t expected, uint32_t desired) {
    return atomicCAS(slot, expected, desired);
  }
  static __device__ __forceinline__ void min(uint32_t* slot, uint32_t v) { atomicMin(slot, v); }
};
}  // namespace

// a tx with an empty input range is not walked (it was not validated): flags
// and output sum 0. The fold reads both back from tx_flags / tx_sums.
__global__ void __launch_bounds__(WG) hkv_spend_walk_kernel(const uint8_t* __restrict__ txs,
                                                            const uint32_t* __restrict__ tx_off, uint32_t n_tx,
                                                            const uint32_t* __restrict__ input_first,
                                                            uint32_t n_inputs, uint64_t max_money,
                                                            uint32_t* __restrict__ input_off,
                                                            uint64_t* __restrict__ tx_sums,
                                                            uint8_t* __restrict__ tx_flags,
                                                            uint32_t* __restrict__ status) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= n_tx) return;
  if (t == 0 && input_first[n_tx] != n_inputs) atomicOr(status, HKV_STATUS_INPUT_COUNT);
  const uint32_t b = input_first[t], e = input_first[t + 1];
  TxWalk w;
  w.out_sum = 0;
  w.flags = 0;
  // (nothing is written past the caller's n_inputs slots of input_off)
  if (e > b) w = spend_walk(txs, tx_off[t], b, n_inputs, input_off, max_money);
  tx_sums[2 * (size_t)t + 1] = w.out_sum;
  tx_flags[t] = w.flags;
}

// tb.n arrives as the caller's n_inputs; the inputs indexed are those the
// device counted, as far as the caller's arrays hold them
__global__ void __launch_bounds__(WG) hkv_spend_table_kernel(SpendTable tb, const uint32_t* __restrict__ total) {
  const uint32_t g = blockIdx.x * WG + threadIdx.x;
  tb.n = *total < tb.n ? *total : tb.n;
  if (g >= tb.n) return;
  spend_insert<DeviceSpendOps>(tb, g);
}

__global__ void __launch_bounds__(WG) hkv_spender_kernel(SpendTable tb, const uint32_t* __restrict__ total,
                                                         uint32_t* __restrict__ spender) {
  const uint32_t g = blockIdx.x * WG + threadIdx.x;
  const uint32_t n_inputs = tb.n;
  if (g >= n_inputs) return;  // nothing is written past the caller's capacity
  tb.n = *total < tb.n ? *total : tb.n;
  spender[g] = g < tb.n ? first_spender(tb, g) : SPEND_EMPTY;
}

// status is read first, as hkv_tx_verdict_kernel reads it: a batch whose input
// count differed from the caller's has no flags and no sums (its ranges do not
// describe the per-input arrays, none of which is read then)
__global__ void __launch_bounds__(WG) hkv_tx_spend_kernel(const uint32_t* __restrict__ input_first, uint32_t n_tx,
                                                          const uint64_t* __restrict__ jobs,
                                                          const uint32_t* __restrict__ input_src,
                                                          const uint32_t* __restrict__ spender, uint32_t n_inputs,
                                                          uint64_t max_money, const uint32_t* __restrict__ status,
                                                          uint64_t* tx_sums, uint8_t* tx_flags) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= n_tx) return;
  const bool mismatch = (*status & HKV_STATUS_INPUT_COUNT) != 0 || input_first[n_tx] != n_inputs;
  uint64_t in_sum = 0, out_sum = 0;
  uint8_t flags = 0;
  if (!mismatch) {
    const uint32_t b = input_first[t], e = input_first[t + 1];
    if (e > b) {
      out_sum = tx_sums[2 * (size_t)t + 1];
      flags = spend_fold(jobs, input_src, spender, b, e, max_money, out_sum, tx_flags[t], in_sum);
    }
  }
  tx_sums[2 * (size_t)t] = in_sum;
  tx_sums[2 * (size_t)t + 1] = out_sum;
  tx_flags[t] = flags;
}

hipError_t launch_block_spends(const SpendStage& s, uint32_t stages, hipStream_t st) {
  if (s.n_tx == 0) return hipSuccess;
  const uint32_t* total = s.input_first + s.n_tx;
  const SpendTable tb{s.txs, s.input_off, s.n_inputs, s.slots, s.n_slots, s.salt, s.mask};
  const dim3 per_tx((s.n_tx + WG - 1) / WG), per_input((s.n_inputs + WG - 1) / WG);
  if (stages & SPEND_STAGE_WALK) {
    hipLaunchKernelGGL(hkv_spend_walk_kernel, per_tx, dim3(WG), 0, st, s.txs, s.tx_off, s.n_tx, s.input_first,
                       s.n_inputs, s.max_money, s.input_off, s.tx_sums, s.tx_flags, s.status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (s.n_inputs != 0 && (stages & SPEND_STAGE_TABLE)) {
    // empty = 0xFFFFFFFF in every slot
    hipError_t e = hipMemsetAsync(s.slots, 0xFF, (size_t)s.n_slots * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hkv_spend_table_kernel, per_input, dim3(WG), 0, st, tb, total);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (s.n_inputs != 0 && (stages & SPEND_STAGE_SPENDER)) {
    hipLaunchKernelGGL(hkv_spender_kernel, per_input, dim3(WG), 0, st, tb, total, s.spender);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (stages & SPEND_STAGE_FOLD) {
    hipLaunchKernelGGL(hkv_tx_spend_kernel, per_tx, dim3(WG), 0, st, s.input_first, s.n_tx,
                       reinterpret_cast<const uint64_t*>(s.jobs), s.input_src, s.spender, s.n_inputs, s.max_money,
                       s.status, s.tx_sums, s.tx_flags);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace hkv
