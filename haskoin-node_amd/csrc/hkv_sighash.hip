// hkv_sighash.hip — on-device signature hashes and standard-input extraction
// for gfx950.
//
// A batch is a buffer of serialised transactions (wire form, with or without
// BIP144 witnesses) plus per-signature jobs. The kernels, one lane each:
//   1. hkv_tx_index_kernel   — per tx: bounds-checked parse of the wire form
//      into a 128-byte row (input / output / locktime offsets) and, when
//      asked, the three BIP143 per-tx hashes (hashPrevouts, hashSequence,
//      hashOutputs), computed once per tx and shared by its inputs.
//   1c. hkv_txid_kernel      — per tx: haskoin-core txHash (SHA-256d of the
//      witness-stripped re-serialisation), the leaves of the merkle kernels.
//   2. hkv_sighash_kernel    — per job: haskoin-core txSigHash (legacy) or
//      txSigHashForkId (BIP143) -> 32-byte msg32, written with a caller
//      stride (stride 168 writes straight into verify records).
//   3. hkv_std_input_kernel  — per input: the non-ECDSA half of
//      verifyStdInput for P2PK / P2PKH / P2WPKH / P2SH-P2WPKH prevouts (template match,
//      strict DER decode + low S + hashtype, HASH160 check, sighash) -> one
//      168-byte verify record; a failed check writes an all-zero record, which
//      the verify kernels reject (pubkey length 0).
//
// Preimages are never materialised. Each lane runs a small generator that
// emits its preimage as "pieces" (a byte range of the tx / script buffers, or
// an up-to-8-byte literal such as a re-encoded varint, a zeroed sequence or a
// stored hash), and sha256_stream absorbs them block-synchronously through a
// per-lane 64-byte LDS slot. Varints that haskoin re-serialises (input and
// output counts, script lengths) are always re-emitted canonically, so
// non-canonical encodings in the input hash exactly as the reference does.
//
// Reference semantics restated [dep; haskoin-core-1.1.0 pinned at
// /root/reference/stack.yaml:10]: Haskoin.Script.SigHash txSigHash /
// txSigHashForkId / decodeTxSig, Haskoin.Crypto.Signature decodeStrictSig
// (libsecp256k1 secp256k1_ecdsa_signature_parse_der), Haskoin.Transaction.
// Builder verifyStdInput; CPU restatement: oracle/sighash_oracle.py.
#include "hkv_hash.h"
#include "hkv_scalar.h"
#include "hkv_layout.h"
#include "hkv_internal.h"
#include "../../include/hkv.h"

#include "hkv_sighash_dev.h"

namespace hkv {

__global__ void __launch_bounds__(WG) hkv_tx_index_kernel(const uint8_t* __restrict__ txs,
                                                          const uint32_t* __restrict__ tx_off, uint32_t n_tx,
                                                          uint32_t* __restrict__ txt) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= n_tx) return;
  uint32_t row[8];
  tx_index_row(txs, tx_off, t, row);
#pragma unroll
  for (int k = 0; k < 8; ++k) txt[(size_t)t * TXT_WORDS + k] = row[k];
}

// 1b. the three BIP143 per-tx hashes, one lane per (tx, hash): blockIdx.y
// selects hashPrevouts / hashSequence / hashOutputs (wave-uniform), so the
// three SHA-256d streams of a tx run side by side instead of one after the
// other (a block's index is latency-bound: one wave per 64 txs).
// Each lane parses its tx itself (the three blockIdx.y lanes of a tx repeat
// the cheap walk; y = 0 writes the row), so the index costs no launch of its own.
// witness_only: hash only the txs with witness data (the others' rows keep
// stale hash words, which no standard input on a network without a fork id reads)
__global__ void __launch_bounds__(WG) hkv_tx_hash_kernel(const uint8_t* __restrict__ txs,
                                                         const uint32_t* __restrict__ tx_off, uint32_t n_tx,
                                                         uint32_t witness_only, uint32_t write_rows,
                                                         uint32_t* __restrict__ txt) {
  __shared__ uint32_t buf[16 * WG];
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t which = blockIdx.y;  // 0 prevouts, 1 sequences, 2 outputs
  uint32_t row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (t < n_tx) {
    tx_index_row(txs, tx_off, t, row);
    if (which == 0 && write_rows) {
#pragma unroll
      for (int k = 0; k < 8; ++k) txt[(size_t)t * TXT_WORDS + k] = row[k];
    }
  }
  const bool go = t < n_tx && (row[TXT_FLAGS] & TXF_OK) && (!witness_only || (row[TXT_FLAGS] & TXF_WITNESS));
  Gen g;
  uint32_t h[8], d[8];
  gen_clear(g);
  g.T = txs;
  if (which == 2) {  // hashOutputs (each output re-serialised canonically)
    g.ooff = row[TXT_OUTS_FIRST]; g.ocnt = row[TXT_NOUT]; g.ret = PH_DONE; g.phase = PH_O_VAL;
  } else {
    g.nin = row[TXT_NIN]; g.ioff = row[TXT_INS]; g.j = 0; g.phase = which == 0 ? PH_P_IN : PH_S_IN;
  }
  sha256_stream(h, g, go, buf);
  sha256d_finish(d, h);
  if (go) {
    const int slot = which == 0 ? TXT_HP : (which == 1 ? TXT_HS : TXT_HO);
#pragma unroll
    for (int k = 0; k < 8; ++k) txt[(size_t)t * TXT_WORDS + slot + k] = d[k];
  }
}

// ---------------------------------------------------------------------------
// 1c. txHash: SHA-256d of the tx re-serialised without witness data
// ---------------------------------------------------------------------------
// haskoin-core txHash = doubleSHA256 (runPutS (serialize tx{witness = []}))
// [dep]: the decoded tx, not its wire bytes, so the segwit marker / flag and
// the witness stacks are dropped and the four kinds of varint haskoin
// re-serialises (input count, scriptSig lengths, output count, output script
// lengths) are re-emitted canonically. CPU restatement:
// sha256d(tx_serialize(tx_parse(raw), with_witness=False)), oracle/sighash_oracle.py.
//
// A generator of its own (see hkv_sighash_dev.h on why not new phases of
// Gen's switch); its output walker restates PH_O_VAL / PH_O_LEN / PH_O_SCRIPT.
enum : uint32_t {
  // (0 = PH_DONE) whole ranges of a tx whose varints are canonical already
  TP_MID = 1, TP_LOCK,
  // the piecewise re-serialisation
  TP_NIN, TP_IN_OP, TP_IN_SLEN, TP_IN_REST, TP_NOUT, TP_O_VAL, TP_O_LEN, TP_O_SCRIPT,
};

struct TxGen {
  const uint8_t* src;  // current piece: byte range (src != null) or literal
  uint64_t lit;
  uint32_t rem;
  uint32_t phase;
  const uint8_t* T;    // tx buffer (absolute offsets below)
  uint32_t mid, mid_len, lock;
  uint32_t nin, nout, j, ioff, sl, scr;
  uint32_t ooff, ocnt, osl, oscr;
};

HKV_DEV void txgen_clear(TxGen& g) {
  g.src = nullptr; g.lit = 0; g.rem = 0; g.phase = PH_DONE; g.T = nullptr;
  g.mid = g.mid_len = g.lock = 0;
  g.nin = g.nout = g.j = g.ioff = g.sl = g.scr = 0;
  g.ooff = g.ocnt = g.osl = g.oscr = 0;
}

HKV_DEV void gen_advance(TxGen& g) {
  const uint8_t* T = g.T;
  switch (g.phase) {
    case TP_MID: piece_copy(g, T + g.mid, g.mid_len); g.phase = TP_LOCK; break;
    case TP_LOCK: piece_copy(g, T + g.lock, 4); g.phase = PH_DONE; break;
    case TP_NIN: piece_varint(g, g.nin); g.j = 0; g.phase = TP_IN_OP; break;
    case TP_IN_OP: {
      if (g.j == g.nin) {
        g.phase = TP_NOUT;
        break;
      }
      piece_copy(g, T + g.ioff, 36);
      uint32_t o = g.ioff + 36;
      g.sl = get_varint(T, o);
      g.scr = o;
      g.phase = TP_IN_SLEN;
      break;
    }
    case TP_IN_SLEN: piece_varint(g, g.sl); g.phase = TP_IN_REST; break;
    case TP_IN_REST:  // scriptSig and sequence are adjacent: one range
      piece_copy(g, T + g.scr, g.sl + 4);
      g.ioff = g.scr + g.sl + 4;
      g.j += 1;
      g.phase = TP_IN_OP;
      break;
    case TP_NOUT: piece_varint(g, g.nout); g.ocnt = g.nout; g.phase = TP_O_VAL; break;
    case TP_O_VAL: {
      if (g.ocnt == 0) {
        g.phase = TP_LOCK;
        break;
      }
      piece_copy(g, T + g.ooff, 8);
      uint32_t o = g.ooff + 8;
      g.osl = get_varint(T, o);
      g.oscr = o;
      g.phase = TP_O_LEN;
      break;
    }
    case TP_O_LEN: piece_varint(g, g.osl); g.phase = TP_O_SCRIPT; break;
    case TP_O_SCRIPT:
      piece_copy(g, T + g.oscr, g.osl);
      g.ooff = g.oscr + g.osl;
      g.ocnt -= 1;
      g.phase = TP_O_VAL;
      break;
    default: g.phase = PH_DONE; break;
  }
}

// bytes of the canonical varint of v
HKV_DEV uint32_t varint_canon_len(uint32_t v) { return v < 0xFDu ? 1u : (v <= 0xFFFFu ? 3u : 5u); }

// Every varint txHash re-serialises is canonical on the wire (walk over a tx
// tx_index_row accepted): the stripped serialisation is then whole ranges of it.
HKV_DEV bool tx_varints_canonical(const uint8_t* T, const uint32_t row[8]) {
  const uint32_t nin = row[TXT_NIN], nout = row[TXT_NOUT];
  const uint32_t nin_at = row[TXT_START] + 4 + ((row[TXT_FLAGS] & TXF_WITNESS) ? 2u : 0u);
  bool canon = row[TXT_INS] - nin_at == varint_canon_len(nin);
  uint32_t o = row[TXT_INS];
  for (uint32_t j = 0; j < nin; ++j) {
    o += 36;
    const uint32_t at = o;
    const uint32_t sl = get_varint(T, o);
    canon = canon && o - at == varint_canon_len(sl);
    o += sl + 4;
  }
  canon = canon && row[TXT_OUTS_FIRST] - o == varint_canon_len(nout);
  o = row[TXT_OUTS_FIRST];
  for (uint32_t k = 0; k < nout; ++k) {
    o += 8;
    const uint32_t at = o;
    const uint32_t sl = get_varint(T, o);
    canon = canon && o - at == varint_canon_len(sl);
    o += sl;
  }
  return canon;
}

HKV_DEV void txgen_setup(TxGen& g, const uint8_t* T, const uint32_t row[8]) {
  txgen_clear(g);
  g.T = T;
  const uint32_t start = row[TXT_START], lock = row[TXT_LOCK];
  const bool wit = (row[TXT_FLAGS] & TXF_WITNESS) != 0;
  g.lock = lock;
  if (tx_varints_canonical(T, row)) {
    if (!wit) {  // the wire bytes are the message
      piece_copy(g, T + start, lock + 4 - start);
      g.phase = PH_DONE;
    } else {     // version | counts, inputs, outputs | locktime
      piece_copy(g, T + start, 4);
      g.mid = start + 6;
      g.mid_len = row[TXT_OUTS_END] - (start + 6);
      g.phase = TP_MID;
    }
    return;
  }
  piece_copy(g, T + start, 4);
  g.nin = row[TXT_NIN];
  g.nout = row[TXT_NOUT];
  g.ioff = row[TXT_INS];
  g.ooff = row[TXT_OUTS_FIRST];
  g.phase = TP_NIN;
}

// sha256_stream for txHash messages (chosen over the template for a TxGen):
// the same block-synchronous loop, but a lane with 64 or more bytes left in a
// byte range fetches the whole block by 64 independent loads into registers,
// instead of 16 dependent rounds of gen_word through its LDS slot. txHash
// messages are long ranges, and a long tx is one lane's serial chain.
HKV_DEV void sha256_stream(uint32_t h[8], TxGen& g, bool live, uint32_t* buf) {
  sha256_init(h);
  const uint32_t tid = threadIdx.x;
  uint32_t st = live ? 0u : 3u;  // 0 message, 1 padding (0x80 written), 3 done
  uint64_t len = 0;
  while (__any(st != 3u)) {
    if (st != 3u) {
      uint32_t w[16];
      bool last = false;
      if (st == 0u && g.src != nullptr && g.rem >= 64u) {
        const uint8_t* s = g.src;
#pragma unroll
        for (int k = 0; k < 16; ++k)
          w[k] = ((uint32_t)s[4 * k] << 24) | ((uint32_t)s[4 * k + 1] << 16) | ((uint32_t)s[4 * k + 2] << 8) |
                 (uint32_t)s[4 * k + 3];
        g.src += 64;
        g.rem -= 64u;
        len += 64;
      } else {
        bool fits = st == 1u;  // a block after the 0x80 block always has room
#pragma unroll 1
        for (uint32_t k = 0; k < 16u; ++k) {
          uint32_t v = 0;
          if (st == 0u) {
            const uint32_t nb = gen_word(g, v);
            len += nb;
            if (nb < 4u) {
              v |= 0x80u << (24 - 8 * nb);
              st = 1u;
              fits = k < 14u;
            }
          }
          buf[k * WG + tid] = v;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = buf[k * WG + tid];
        last = st == 1u && fits;
        if (last) {
          const uint64_t bits = len << 3;
          w[14] = (uint32_t)(bits >> 32);
          w[15] = (uint32_t)bits;
        }
      }
      sha256_compress(h, w);
      if (last) st = 3u;
    }
  }
}

// One lane per tx; stateless (the lane parses its tx itself: no index rows,
// no context scratch). A tx tx_index_row rejects gets an all-zero txid and
// status HKV_TXID_BAD_TX. Latency is bounded below by the batch's longest
// tx: SHA-256 is one serial chain per message and a tx is one lane's.
__global__ void __launch_bounds__(WG) hkv_txid_kernel(const uint8_t* __restrict__ txs,
                                                      const uint32_t* __restrict__ tx_off, uint32_t n_tx,
                                                      uint32_t* __restrict__ txids, uint8_t* __restrict__ status) {
  __shared__ uint32_t buf[16 * WG];
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (t < n_tx) tx_index_row(txs, tx_off, t, row);
  const bool live = t < n_tx && (row[TXT_FLAGS] & TXF_OK);
  TxGen g;
  uint32_t h[8], d[8];
  if (live) txgen_setup(g, txs, row);
  else txgen_clear(g);
  sha256_stream(h, g, live, buf);
  sha256d_finish(d, h);
  if (t < n_tx) {
    uint4* o = reinterpret_cast<uint4*>(txids + (size_t)t * 8);
    o[0] = live ? make_uint4(d[0], d[1], d[2], d[3]) : make_uint4(0, 0, 0, 0);
    o[1] = live ? make_uint4(d[4], d[5], d[6], d[7]) : make_uint4(0, 0, 0, 0);
    if (status) status[t] = live ? (uint8_t)HKV_TXID_OK : (uint8_t)HKV_TXID_BAD_TX;
  }
}

// ---------------------------------------------------------------------------
// 2. sighash jobs
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(WG) hkv_sighash_kernel(const uint8_t* __restrict__ txs, uint32_t n_tx,
                                                         const uint32_t* __restrict__ txt,
                                                         const uint8_t* __restrict__ scripts, uint32_t scripts_len,
                                                         const hkv_sighash_job* __restrict__ jobs, uint32_t n,
                                                         int32_t forkid, uint8_t* __restrict__ out, uint32_t stride,
                                                         uint8_t* __restrict__ status) {
  __shared__ uint32_t buf[16 * WG];
  const uint32_t jx = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = jx < n;
  uint32_t stc = HKV_SH_BAD_REF;
  JobCtx c;
  c.forkid_form = false; c.one = false; c.single_hash = false;
  const uint32_t* row = txt;
  const uint8_t* code = scripts;
  uint32_t code_len = 0;
  uint64_t value = 0;
  uint32_t* o32 = reinterpret_cast<uint32_t*>(out + (size_t)jx * stride);
  if (in_range) {
    const hkv_sighash_job jb = jobs[jx];
    const bool ref_ok = jb.tx < n_tx && jb.script_off <= scripts_len && scripts_len - jb.script_off >= jb.script_len &&
                        jb.kind <= HKV_SIGHASH_FORKID;
    if (ref_ok) {
      row = txt + (size_t)jb.tx * TXT_WORDS;
      if (!(row[TXT_FLAGS] & TXF_OK)) stc = HKV_SH_BAD_TX;
      else if (jb.input >= row[TXT_NIN]) stc = HKV_SH_BAD_INPUT;
      else stc = HKV_SH_OK;
    }
    if (stc == HKV_SH_OK) {
      job_setup(c, txs, row, jb.input, jb.sighash, jb.kind == HKV_SIGHASH_FORKID, forkid);
      code = scripts + jb.script_off;
      code_len = jb.script_len;
      value = jb.value;
    }
  }
  const bool ok = in_range && stc == HKV_SH_OK;
  Gen g;
  uint32_t h[8], d[8];
  // BIP143 SINGLE: hashOutputs = SHA-256d(output i), parked in the job's output slot
  const bool need_single = ok && c.single_hash;
  if (__any(need_single)) {
    gen_clear(g);
    g.T = txs; g.ooff = c.single_off; g.ocnt = 1; g.ret = PH_DONE; g.phase = PH_O_VAL;
    sha256_stream(h, g, need_single, buf);
    sha256d_finish(d, h);
    if (need_single) {
#pragma unroll
      for (int k = 0; k < 8; ++k) o32[k] = d[k];
    }
  }
  const bool live = ok && !c.one;
  if (live) gen_job(g, c, txs, row, code, code_len, false, value, o32);
  else gen_clear(g);
  sha256_stream(h, g, live, buf);
  sha256d_finish(d, h);
  if (in_range) {
#pragma unroll
    for (int k = 0; k < 8; ++k) o32[k] = live ? d[k] : ((ok && c.one && k == 0) ? 1u : 0u);
    if (status) status[jx] = (uint8_t)stc;
  }
}

__global__ void __launch_bounds__(WG) hkv_std_input_kernel(const uint8_t* __restrict__ txs, uint32_t n_tx,
                                                           const uint32_t* __restrict__ txt,
                                                           const uint8_t* __restrict__ scripts, uint32_t scripts_len,
                                                           const hkv_input_job* __restrict__ jobs, uint32_t n,
                                                           int32_t forkid, uint8_t* __restrict__ recs) {
  __shared__ uint32_t buf[16 * WG];
  const uint32_t jx = blockIdx.x * blockDim.x + threadIdx.x;
  StdIn x;
  std_parse(x, txs, n_tx, txt, scripts, scripts_len, jobs, jx, n, forkid);
  uint32_t* r32 = reinterpret_cast<uint32_t*>(recs + (size_t)jx * REC_SIZE);
  uint32_t d[8];
  const bool live = std_hash(x, txs, forkid, r32, buf, d);
  if (jx >= n) return;
  std_write_record(r32, x, live, d);
}

// 4. multisig inputs: the scan (hkv_sighash_dev.h ms_scan_lane), candidate
//    records, the countMulSig walk
__global__ void __launch_bounds__(WG) hkv_ms_scan_kernel(const uint8_t* __restrict__ txs, uint32_t n_tx,
                                                         const uint32_t* __restrict__ txt,
                                                         const uint8_t* __restrict__ scripts, uint32_t scripts_len,
                                                         const hkv_input_job* __restrict__ jobs, uint32_t n,
                                                         int32_t forkid, uint32_t* __restrict__ desc,
                                                         uint64_t* __restrict__ off,
                                                         unsigned long long* __restrict__ counters) {
  __shared__ uint32_t buf[16 * WG];
  const uint32_t jx = blockIdx.x * WG + threadIdx.x;
  ms_scan_lane(txs, n_tx, txt, scripts, scripts_len, jobs, jx, jx < n, forkid, desc, off, counters, buf);
}

}  // namespace hkv

// ---------------------------------------------------------------------------
// launch wrappers (called by hkv_api.cpp)
// ---------------------------------------------------------------------------
namespace hkv {

static inline uint32_t blocks_for(size_t n) { return (uint32_t)((n + WG - 1) / WG); }

hipError_t launch_tx_index(const uint8_t* txs, const uint32_t* tx_off, uint32_t n_tx, uint32_t hashes,
                           uint32_t* txt, hipStream_t st) {
  if (n_tx == 0) return hipSuccess;
  if (hashes != TX_HASHES_NONE)
    hipLaunchKernelGGL(hkv_tx_hash_kernel, dim3((n_tx + xtpb_for(n_tx) - 1) / xtpb_for(n_tx), 3), dim3(xtpb_for(n_tx)), 0, st,
                       txs, tx_off, n_tx, hashes == TX_HASHES_WITNESS ? 1u : 0u, 1u, txt);
  else
    hipLaunchKernelGGL(hkv_tx_index_kernel, dim3(blocks_for(n_tx)), dim3(WG), 0, st, txs, tx_off, n_tx, txt);
  return hipGetLastError();
}
hipError_t launch_tx_hashes_only(const uint8_t* txs, const uint32_t* tx_off, uint32_t n_tx, uint32_t hashes,
                                 uint32_t* txt, hipStream_t st) {
  if (n_tx == 0 || hashes == TX_HASHES_NONE) return hipSuccess;
  hipLaunchKernelGGL(hkv_tx_hash_kernel, dim3((n_tx + xtpb_for(n_tx) - 1) / xtpb_for(n_tx), 3), dim3(xtpb_for(n_tx)), 0,
                     st, txs, tx_off, n_tx, hashes == TX_HASHES_WITNESS ? 1u : 0u, 0u, txt);
  return hipGetLastError();
}
hipError_t launch_txids(const uint8_t* txs, const uint32_t* tx_off, uint32_t n_tx, uint8_t* txids, uint8_t* status,
                        hipStream_t st) {
  if (n_tx == 0) return hipSuccess;
  hipLaunchKernelGGL(hkv_txid_kernel, dim3((n_tx + xtpb_for(n_tx) - 1) / xtpb_for(n_tx)), dim3(xtpb_for(n_tx)), 0, st,
                     txs, tx_off, n_tx, reinterpret_cast<uint32_t*>(txids), status);
  return hipGetLastError();
}
hipError_t launch_sighash(const uint8_t* txs, uint32_t n_tx, const uint32_t* txt, const uint8_t* scripts,
                          uint32_t scripts_len, const hkv_sighash_job* jobs, uint32_t n, int32_t forkid, uint8_t* out,
                          uint32_t stride, uint8_t* status, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(hkv_sighash_kernel, dim3((n + xtpb_for(n) - 1) / xtpb_for(n)), dim3(xtpb_for(n)), 0, st, txs, n_tx, txt, scripts, scripts_len,
                     jobs, n, forkid, out, stride, status);
  return hipGetLastError();
}
hipError_t launch_std_inputs(const StdOps& o, uint32_t n, uint8_t* recs, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(hkv_std_input_kernel, dim3((n + xtpb_for(n) - 1) / xtpb_for(n)), dim3(xtpb_for(n)), 0, st, o.txs,
                     o.n_tx, o.txt, o.scripts, o.scripts_len, o.jobs, n, o.forkid, recs);
  return hipGetLastError();
}

}  // namespace hkv

// ---------------------------------------------------------------------------
// multisig launch wrappers
// ---------------------------------------------------------------------------
namespace hkv {

// per-input desc words and record offsets; *ms.counters (the call's parity
// word, zeroed by the call before) ends as the number of candidate records |
// key-check records << 32 (the tail kernel reads it, stream-ordered after the
// scan)
hipError_t launch_ms_scan(const StdOps& o, uint32_t n, const MsScan& ms, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(hkv_ms_scan_kernel, dim3(blocks_for(n)), dim3(WG), 0, st, o.txs, o.n_tx, o.txt, o.scripts,
                     o.scripts_len, o.jobs, n, o.forkid, ms.desc, ms.off,
                     reinterpret_cast<unsigned long long*>(ms.counters));
  return hipGetLastError();
}

}  // namespace hkv
