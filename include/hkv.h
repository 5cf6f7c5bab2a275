/*
 * hkv.h — C ABI of libhkv: MI355X batch secp256k1 ECDSA verification.
 *
 * Drop-in boundary for the signature-check hot path of a haskoin-node based
 * validator. What each entry point replaces:
 *
 *   hkv_verify / hkv_verify_device
 *       replaces N per-input calls of haskoin-core
 *       `verifyHashSig :: Ctx -> Hash256 -> Sig -> PubKey -> Bool`
 *       (Haskoin.Crypto.Signature, haskoin-core-1.1.0 pinned at
 *       /root/reference/stack.yaml:10) in mode HKV_HASKOIN, and of
 *       secp256k1-haskell `verifySig` -> FFI `secp256k1_ecdsa_verify`
 *       (secp256k1-haskell-1.2.0, /root/reference/stack.yaml:9) in mode
 *       HKV_LIBSECP. Per-record parsing replaces `importPubKey`
 *       (secp256k1_ec_pubkey_parse) and `importCompactSig`
 *       (secp256k1_ecdsa_signature_parse_compact) so raw/adversarial bytes
 *       get exact reject parity. The reference itself never verifies; the
 *       batch is fed from the node's block/tx events
 *       (/root/reference/src/Haskoin/Node.hs:151-174, Peer.hs:309-344).
 *   hkv_open / hkv_close
 *       replaces secp256k1-haskell `createContext`/`withContext` (one
 *       shared read-only context per process).
 *   hkv_sighash / hkv_sighash_device
 *       replaces N calls of haskoin-core
 *       `txSigHash :: Network -> Tx -> Script -> Word64 -> Int -> SigHash -> Hash256`
 *       and `txSigHashForkId` (Haskoin.Script.SigHash) — the producer of
 *       every msg32 verifyHashSig checks.
 *   hkv_verify_std_inputs / hkv_verify_std_inputs_device
 *       replaces N calls of haskoin-core
 *       `verifyStdInput :: Network -> Ctx -> Tx -> Int -> ScriptOutput -> Word64 -> Bool`
 *       (Haskoin.Transaction.Builder) for P2PK / P2PKH / P2WPKH / multisig
 *       prevouts, bare or behind P2SH / P2WSH / P2SH-P2WSH: decodeTxSig
 *       (strict DER, low S, hashtype), the HASH160 / SHA-256 script checks,
 *       legacy or BIP143 sighash, verifyHashSig and the countMulSig walk,
 *       all on device.
 *   hkv_verify_std_txs / hkv_verify_std_txs_device
 *       replaces N calls of haskoin-core
 *       `verifyStdTx :: Network -> Ctx -> Tx -> [(ScriptOutput, Word64, OutPoint)] -> Bool`
 *       (Haskoin.Transaction.Builder): matchTemplate of each tx's unordered
 *       prevout list against its inputs by outpoint, verifyStdInput per
 *       matched input, one verdict per tx. hkv_std_tx_jobs_device is the
 *       matching alone (the prevout provider), hkv_tx_verdicts_device the
 *       per-tx `all`.
 *   hkv_verify_block_txs / hkv_verify_block_txs_device
 *       replaces the same N calls of `verifyStdTx` for the txs of whole blocks
 *       and the host work in front of them: a prevout created earlier in the
 *       same batch (which no UTXO provider has yet) is found on the device from
 *       the device-computed `txHash`, where the caller of hkv_verify_std_txs
 *       must parse and hash every tx, build a txid map and copy each parent
 *       output into the prevout lists. hkv_block_tx_jobs_device is that
 *       provider alone; hkv_txid_index_device / hkv_txid_lookup_device the
 *       `HashMap TxHash Int` it stands on.
 *   hkv_block_spends_device / hkv_verify_block_txs_spends
 *       replaces the host work a validator does around `verifyStdTx` when it
 *       connects a block: the outpoints of every input in a `HashMap OutPoint`
 *       (a second spender of an outpoint within the batch is a double spend)
 *       and the sums of input and output amounts against `maxSatoshi`, from
 *       what hkv_verify_block_txs* leaves on the device.
 *   hkv_check_headers / hkv_check_headers_device
 *       replaces the per-header part of haskoin-core `connectBlocks` reached
 *       from importHeaders (/root/reference/src/Haskoin/Node/Chain.hs:500-520):
 *       headerHash, isValidPOW (decodeCompact) and the prev-hash link.
 *   hkv_connect_headers / hkv_connect_headers_device / hkv_chain_context_device
 *       replaces the rest of that `connectBlocks` call: median time past, the
 *       future-time limit, nextWorkRequired, validVersion, checkpoints and the
 *       chain work, and the count of leading headers that connect.
 *   hkv_tx_ids / hkv_tx_ids_device
 *       replaces N calls of haskoin-core `txHash :: Tx -> TxHash`
 *       (SHA-256d of the tx re-serialised without witness data).
 *   hkv_check_blocks / hkv_check_blocks_device
 *       replaces the reference's block assertion on getBlocks results
 *       (Peer.hs:309-344; test/Haskoin/NodeSpec.hs:185-193):
 *       b.header.merkle == buildMerkleRoot (txHash <$> b.txs), per block.
 *
 * Streams: device-form calls enqueue on the caller's stream; calls on one
 * device share its scratch buffers, so each call is ordered after the
 * previous call on that device (an event wait), whatever stream either used.
 *
 * Conventions: no C++ exceptions cross this boundary; every function that
 * can fail returns 0 (HKV_OK) or a negative hkv_err. A verdict is never an
 * error: malformed records simply get bit 0. Verdict bit i of the output is
 * bit (i % 32) of word (i / 32); 1 = accept.
 *
 * Record layout (HKV_RECORD_SIZE = 168 bytes, 8-byte aligned array):
 *   [0,32)    msg32   (the Hash256 bytes as secp256k1 `msg32`, no reversal)
 *   [32,64)   r       big-endian (compact signature first half)
 *   [64,96)   s       big-endian
 *   [96]      pubkey length in bytes (33 or 65 are the only valid ones)
 *   [97,162)  pubkey  SEC1 bytes (02/03 compressed, 04 uncompressed,
 *                     06/07 hybrid), zero padded
 *   [162,168) zero padding
 */
#ifndef HKV_H
#define HKV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HKV_RECORD_SIZE 168

/* verify modes */
#define HKV_LIBSECP 0u /* secp256k1_ecdsa_verify: high-S rejected        */
#define HKV_HASKOIN 1u /* verifyHashSig: normalize to low-S, then verify */

enum hkv_err {
  HKV_OK = 0,
  HKV_E_ARG = -1,      /* bad argument (NULL, n > capacity, bad mode)   */
  HKV_E_NODEV = -2,    /* no usable gfx950 device                       */
  HKV_E_OOM = -3,      /* device or pinned host allocation failed       */
  HKV_E_HIP = -4,      /* HIP runtime error (see hkv_last_hip_error)     */
  HKV_E_INTERNAL = -5, /* self-check failed at open                      */
};

typedef struct hkv_ctx hkv_ctx;
typedef struct hkv_batch hkv_batch;

/* open flags */
#define HKV_OPEN_NO_SELFCHECK 1u /* skip the known-answer self-check at open */

/* Open a context on the first n_gpus visible devices (n_gpus <= 0: all).
 * Builds the fixed-base tables on every device and, unless flags has
 * HKV_OPEN_NO_SELFCHECK, verifies 256 generated signatures per device
 * (HKV_E_INTERNAL if any is rejected). */
int hkv_open(int n_gpus, uint32_t flags, hkv_ctx** out);
/* Open on an explicit list of HIP device ordinals (one process per GPU:
 * pass {LOCAL_RANK}). Context device index k refers to device_ids[k]. */
int hkv_open_devices(const int* device_ids, int n_ids, uint32_t flags, hkv_ctx** out);
void hkv_close(hkv_ctx* ctx);
int hkv_ctx_num_devices(const hkv_ctx* ctx);
/* Device k of the context still takes host-batch shards (1) or has failed
 * one with a device fault (0); negative on a bad argument. */
int hkv_device_healthy(hkv_ctx* ctx, int dev);
/* Give device k host-batch shards again (after the caller has decided it
 * recovered, e.g. a hipDeviceReset or a passing probe batch). */
int hkv_device_reset_health(hkv_ctx* ctx, int dev);
/* Host-batch shards device k has failed (0 or 1: a failed device gets no
 * more shards); negative on a bad argument. */
int hkv_device_failures(hkv_ctx* ctx, int dev);
/* Test hook: device k's next host-batch shard fails — HKV_FAIL_ENQUEUE
 * before anything is enqueued, HKV_FAIL_JOIN after its work completed — as a
 * HIP error would, exercising the failover of hkv_verify / hkv_verify_host;
 * HKV_FAIL_ALLOC as a staging allocation would (HKV_E_OOM: the call fails,
 * the device stays healthy). */
#define HKV_FAIL_NONE 0u
#define HKV_FAIL_ENQUEUE 1u
#define HKV_FAIL_JOIN 2u
#define HKV_FAIL_ALLOC 3u
/* HKV_FAIL_TAIL: the next multisig tail launch on device k gives up the
 * first wait of its work queue at a phase transition (the timeout branch of a
 * wait for the phase before, taken at once without looking at the count), so
 * the fault reporting below can be tested; deterministic for any batch with a
 * multisig input. */
#define HKV_FAIL_TAIL 4u
int hkv_debug_fail_device(hkv_ctx* ctx, int dev, uint32_t when);
/* Test hooks of the multisig record windows (hkv_verify_std_inputs*): the
 * tail runs a chunk's candidate and key-check records in rounds through two
 * windows of at most 2,752,512 + 442,368 records (~512 MiB); _window sets
 * smaller capacities for device dev's later calls (records, rounded up to
 * 64; 0 = the default), so tests can force many rounds on small batches;
 * _scratch reports the bytes the windows hold allocated on device dev. */
int hkv_debug_ms_window(hkv_ctx* ctx, int dev, uint32_t cand_records, uint32_t key_records);
int hkv_debug_ms_scratch(hkv_ctx* ctx, int dev, size_t* bytes);
/* Read-only test hook: the bytes of Q-table scratch device dev holds (one
 * table per lane of the resident grid from hkv_open on; it grows once to 800 B
 * per signature of a chunk with the first batch above half that grid) and the
 * chunk, in signatures, in which such batches run (2^20; HKV_REC_CHUNK, read
 * at hkv_open, sets a smaller multiple of 256: a test hook). */
int hkv_debug_q_scratch(hkv_ctx* ctx, int dev, size_t* bytes, size_t* chunk);
/* Read-only test hook: the launch shape a batch of n (1..0xFFFFFF00) would
 * take on device dev, from the plan the verify entry points run on; nothing is
 * launched. kind 0: n records; kind 1: n standard inputs. out[0] = the shape
 * of the first chunk (1 the block kernel, 2 the pair kernel, 3 the mid-size
 * instance, 4 the table and chain launches); out[1] = for standard inputs,
 * bit 0 the multisig scan runs in the kernel, bit 1 the kernel builds its tx
 * index rows, bit 2 the hash half overlaps the Q chains (0 for records);
 * out[2] = the first chunk's length (records: padded to 256; the chunk of the
 * table and chain launches); out[3] = the number of chunks. */
int hkv_debug_launch_shape(hkv_ctx* ctx, int dev, uint32_t kind, size_t n, uint32_t out[4]);
/* Read-only test hook: the parts a batch of n records would run in on device
 * dev, from the same plan; nothing is launched. A batch of shape 4 whose plan
 * holds two parts at a time (the env hook HKV_REC_PART at open sets their
 * length) runs its table, chain, finish and verdict launches part by part on
 * two streams: *part_len = the parts' length (the last may be shorter),
 * *n_parts > 1 their number. Otherwise the parts are the chunks of
 * hkv_debug_launch_shape, or the batch. */
int hkv_debug_rec_parts(hkv_ctx* ctx, int dev, size_t n, uint32_t* part_len, uint32_t* n_parts);
/* Read-only test hook: what device dev's last multisig tail launch saw and
 * did, read after every call enqueued so far has completed. out[0] = the
 * scan's total it ran on (candidate records | key-check records << 32),
 * out[1] = work-queue items claimed (each workgroup's final claim past the
 * last item included), out[2] = items completed. All 0 before the first
 * call. Changes no state. */
int hkv_debug_ms_tail_counts(hkv_ctx* ctx, int dev, uint64_t out[3]);

/* Pinned host record buffer with room for max_n records. */
int hkv_batch_alloc(hkv_ctx* ctx, size_t max_n, hkv_batch** out);
void hkv_batch_free(hkv_batch* b);
uint8_t* hkv_batch_records(hkv_batch* b);
size_t hkv_batch_capacity(const hkv_batch* b);

/* Verify records [0, n) of the batch. Shards contiguous 64-aligned index
 * ranges across the context's healthy devices; writes ceil(n/32) words.
 * Blocking. Failover: when a device's shard fails with a device fault (a
 * HIP error while enqueueing or while waiting for it: HKV_E_HIP), that device
 * is marked unhealthy until hkv_device_reset_health and its shard is
 * re-verified on the devices still healthy; the call fails only when none is
 * left (the last error, or HKV_E_NODEV once every device of the context is
 * unhealthy). An allocation failure (HKV_E_OOM) is returned as is: no device
 * changes health and nothing is re-sharded. */
int hkv_verify(hkv_ctx* ctx, hkv_batch* b, size_t n, uint32_t mode, uint32_t* verdict_bits);

/* Same, from any host memory (copied through the context's staging). */
int hkv_verify_host(hkv_ctx* ctx, const uint8_t* records, size_t n, uint32_t mode, uint32_t* verdict_bits);

/* Device-resident form: d_records (n * 168 bytes) and d_bits
 * (>= ceil(n/64)*2 words) live in HBM of the context's device `dev`; work is
 * enqueued on `hip_stream` and NOT synchronised. In every *_device entry point
 * NULL means the null (default) stream, which is ordered against the
 * blocking streams of the process, e.g. PyTorch's default stream.
 * Used by one-process-per-GPU sharding (bench.py) and by zero-copy callers. */
int hkv_verify_device(hkv_ctx* ctx, int dev, const void* d_records, size_t n, uint32_t mode,
                      uint32_t* d_bits, void* hip_stream);

/* Synthetic valid records (keyless construction) written
 * to device memory: pubkeys from a pool of `pool_size` keys, a per-mille
 * share of uncompressed keys, all signatures low-S. Enqueued on hip_stream. */
int hkv_gen_records_device(hkv_ctx* ctx, int dev, uint64_t seed, size_t n, uint32_t pool_size,
                           uint32_t uncompressed_permille, void* d_records, void* hip_stream);
/* A slice of one synthetic batch: records [index0, index0 + n) of the batch
 * `seed` (record k depends on (seed, k) only, and the key pool on seed only,
 * so ranks generating contiguous slices produce exactly the one-process
 * batch; BASELINE configs[4]). invalid_permille of the records are mutated
 * into a class that rejects in both modes: a flipped bit of msg32, r or s,
 * another key of the pool, or the negated key. d_labels (NULL or
 * ceil(n/64)*2 words): bit i = record index0 + i is valid by construction.
 * hkv_gen_records_device is this call with index0 = 0, invalid_permille = 0.
 * CPU restatement (test infrastructure): oracle/hkv_oracle.c hkvo_gen_batch. */
int hkv_gen_batch_device(hkv_ctx* ctx, int dev, uint64_t seed, uint64_t index0, size_t n, uint32_t pool_size,
                         uint32_t uncompressed_permille, uint32_t invalid_permille, void* d_records,
                         uint32_t* d_labels, void* hip_stream);

/* ------------------------------------------------------------------------
 * Signature hashes and standard inputs on device (SURVEY.md §8(a) a7-a9,
 * §8(f) row 2).
 *
 * A tx batch is a buffer of serialised transactions (wire form, BIP144
 * witness form allowed) with n_tx + 1 byte offsets (tx t occupies
 * bytes[offsets[t], offsets[t+1])), plus a pool of scripts the jobs refer to
 * by (offset, length). In the *_device entry points every pointer of the
 * hkv_txs and the job / output arrays live in HBM of device `dev`.
 * ------------------------------------------------------------------------ */
typedef struct hkv_txs {
  const uint8_t* bytes;
  const uint32_t* offsets; /* n_tx + 1 entries, non-decreasing, < 2^32 */
  uint32_t n_tx;
  const uint8_t* scripts;
  uint32_t scripts_len;
} hkv_txs;

#define HKV_SIGHASH_LEGACY 0u /* haskoin-core txSigHash                  */
#define HKV_SIGHASH_FORKID 1u /* haskoin-core txSigHashForkId (BIP143)   */
#define HKV_NO_FORKID (-1)    /* network without a fork id (BTC)         */

/* One call of txSigHash / txSigHashForkId:
 *   txSigHash net tx scriptCode value input sighash
 * scriptCode = scripts[script_off, script_off + script_len). 32 bytes. */
typedef struct hkv_sighash_job {
  uint32_t tx;
  uint32_t input;
  uint32_t script_off;
  uint32_t script_len;
  uint64_t value;   /* prevout amount (BIP143 form) */
  uint32_t sighash; /* SigHash word */
  uint32_t kind;    /* HKV_SIGHASH_LEGACY / HKV_SIGHASH_FORKID */
} hkv_sighash_job;

/* per-job status (hkv_sighash*): the hash of a failed job is all zero */
#define HKV_SH_OK 0u
#define HKV_SH_BAD_TX 1u    /* the tx does not parse within its bounds   */
#define HKV_SH_BAD_INPUT 2u /* input index >= number of inputs           */
#define HKV_SH_BAD_REF 3u   /* tx index or script range out of the batch */

/* One standard input for verifyStdInput: input `input` of tx `tx` spends a
 * prevout with scriptPubKey = scripts[script_off, +script_len) and amount
 * `value`. Templates (haskoin verifyStdInput): P2PK (21 <33> ac / 41 <65> ac),
 * P2PKH, P2WPKH, multisig (OP_m <keys> OP_n OP_CHECKMULTISIG, keys as direct
 * 21 / 41 pushes), each of P2PK / P2PKH / P2WPKH / P2WSH / multisig behind
 * P2SH, and P2PK / P2PKH / multisig behind P2WSH (native or P2SH-nested);
 * any other prevout script verifies false. 24 bytes. */
typedef struct hkv_input_job {
  uint32_t tx;
  uint32_t input;
  uint32_t script_off;
  uint32_t script_len;
  uint64_t value;
} hkv_input_job;

/* Batch txSigHash / txSigHashForkId (forkid: HKV_NO_FORKID or the network's
 * fork id, e.g. 0 for BCH). out32: n * 32 bytes; status: n bytes or NULL.
 * Host memory; runs on the context's first device. Blocking. */
int hkv_sighash(hkv_ctx* ctx, const hkv_txs* txs, const hkv_sighash_job* jobs, size_t n, int32_t forkid,
                uint8_t* out32, uint8_t* status);
/* Device form: hash j goes to d_out + j * out_stride (out_stride % 4 == 0;
 * 168 writes the msg32 field of verify records in place). Enqueued on
 * hip_stream, not synchronised. */
int hkv_sighash_device(hkv_ctx* ctx, int dev, const hkv_txs* d_txs, const hkv_sighash_job* d_jobs, size_t n,
                       int32_t forkid, uint8_t* d_out, size_t out_stride, uint8_t* d_status, void* hip_stream);
/* The non-ECDSA half of verifyStdInput on device: one 168-byte verify record
 * per single-signature input (all-zero when the template / DER / HASH160
 * checks fail, and for multisig inputs, which only the verify entry points
 * below resolve). */
int hkv_std_inputs_device(hkv_ctx* ctx, int dev, const hkv_txs* d_txs, const hkv_input_job* d_jobs, size_t n,
                          int32_t forkid, void* d_records, void* hip_stream);
/* Full batch verifyStdInput: extraction + ECDSA (HKV_HASKOIN semantics).
 * d_records: scratch of n * 168 bytes; verdict bit i in d_bits
 * (>= ceil(n/64)*2 words). Multisig inputs follow haskoin-core countMulSig:
 * every (signature j, key k >= j) pair the walk could compare is verified as
 * its own record, every key of the script is parse-checked, and the walk is
 * replayed on device (count == m and all keys valid).
 * ASYNCHRONOUS: everything is enqueued on hip_stream and the call returns
 * without waiting for any of it (the batch's multisig record count stays on
 * the device: the tail, one launch after the verify on every path, reads it
 * and does nothing when it is 0), so a
 * caller may enqueue block k+1 while block k verifies, and hip_stream may be
 * gated on events recorded after the call. A batch of at most one resident
 * grid (262,144 inputs on an MI355X) runs in chunks of half a grid (131,072),
 * a larger one in chunks of up to 2^20 inputs (the environment variable
 * HKV_STD_CHUNK, read at hkv_open, overrides the 2^20: a test hook). Multisig
 * scratch per chunk: the verdict bits by the 16-of-16 bound
 * (136 candidate + 16 key-check bits per input) and the 168-B records in two
 * windows, the bound or at most 2,752,512 + 442,368 records (~512 MiB), which
 * the tail runs in rounds when a chunk's records exceed them: ~0.1 GB for a
 * 4,000-input block, ~512 MiB for any larger chunk, multisig or not,
 * allocated on first use and kept.
 * A multisig tail whose work-queue wait gave up leaves its multisig
 * verdicts at 0 and reports HKV_STATUS_TAIL_FAULT (below) — this form only
 * through hkv_device_fault; use the _status form to get it per call.
 * n <= 0xFFFFFF00. */
int hkv_verify_std_inputs_device(hkv_ctx* ctx, int dev, const hkv_txs* d_txs, const hkv_input_job* d_jobs, size_t n,
                                 int32_t forkid, void* d_records, uint32_t* d_bits, void* hip_stream);
/* Status bits a verify call reports (hkv_verify_std_inputs_device_status,
 * hkv_device_fault). HKV_STATUS_TAIL_FAULT: a wait of the multisig tail's
 * work queue gave up (seconds; the queue needs no co-residency, so only a
 * hung or preempted workgroup, or the HKV_FAIL_TAIL test hook, causes it):
 * some multisig inputs of the batch were left rejected whatever their
 * signatures. Never a false accept. */
#define HKV_STATUS_TAIL_FAULT 1u
/* hkv_verify_std_inputs_device with a status word: d_status (device memory
 * of `dev`, or NULL) gets the call's HKV_STATUS_* bits ORed in on hip_stream,
 * so an asynchronous caller learns of a fault when it reads its verdicts.
 * The caller zeroes it. */
int hkv_verify_std_inputs_device_status(hkv_ctx* ctx, int dev, const hkv_txs* d_txs, const hkv_input_job* d_jobs,
                                        size_t n, int32_t forkid, void* d_records, uint32_t* d_bits,
                                        uint32_t* d_status, void* hip_stream);
/* Read and clear device dev's sticky fault latch: HKV_STATUS_* bits of every
 * verify call on the device since the last read (any entry point). Waits for
 * the device's enqueued calls. */
int hkv_device_fault(hkv_ctx* ctx, int dev, uint32_t* fault);
/* Host-memory form of the above; writes ceil(n/32) verdict words. Blocking.
 * Same bound on n. HKV_E_INTERNAL if this call's multisig tail reported
 * HKV_STATUS_TAIL_FAULT (some multisig verdicts stayed 0). */
int hkv_verify_std_inputs(hkv_ctx* ctx, const hkv_txs* txs, const hkv_input_job* jobs, size_t n, int32_t forkid,
                          uint32_t* verdict_bits);

/* ---------------------------------------------------------------------------
 * Batch verifyStdTx: whole transactions against outpoint-keyed prevout lists.
 *
 *   verifyStdTx net ctx tx xs =
 *       not (null tx.inputs) && all go (zip (matchTemplate xs tx.inputs f) [0..])
 *     where f (_,_,o) txin = o == txin.outpoint
 *           go (Just (so,val,_), i) = verifyStdInput net ctx tx i so val
 *           go _                    = False
 *
 * The prevouts of a batch are four plain arrays. Tx t owns the entries
 * [prev_offsets[t], prev_offsets[t+1]) (n_tx + 1 non-decreasing entry
 * indices: one list per tx, as verifyStdTx takes it), in list order. Entry e:
 *   outpoint      prev_outpoints[36e, 36e + 36), wire form: the 32 hash bytes
 *                 as they appear in the tx, then the LE32 index;
 *   scriptPubKey  scripts[prev_scripts[2e], + prev_scripts[2e + 1]) of the
 *                 batch's script pool (hkv_txs);
 *   amount        prev_values[e].
 * matchTemplate: inputs are served in input order and input i takes the first
 * entry in list order, not yet taken, whose outpoint equals its own. So when d
 * earlier inputs of the tx carry the same outpoint, input i gets the (d+1)-th
 * entry with that outpoint, or none. A tx is false when an input finds no
 * entry, when it has no inputs, and when it does not parse (it then counts as
 * having no inputs); entries no input takes are ignored.
 * ------------------------------------------------------------------------ */
/* HKV_STATUS_INPUT_COUNT: the batch's txs hold another number of inputs than
 * the caller's n_inputs (hkv_std_tx_jobs_device, hkv_verify_std_txs_device). */
#define HKV_STATUS_INPUT_COUNT 2u
/* The prevout provider alone. Every pointer in HBM of device `dev`
 * (d_prev_offsets, d_prev_scripts, d_input_first, d_status 4-byte aligned;
 * d_prev_values, d_jobs 8-byte aligned); the caller vouches for
 * d_prev_offsets as for the tx offsets. Writes d_input_first[n_tx + 1], the
 * exclusive prefix sums of the txs' input counts (0 for a tx that does not
 * parse; the last entry is the batch's total), and exactly n_inputs jobs into
 * d_jobs, input i of tx t at d_input_first[t] + i: (t, i, the matched entry's
 * script and amount), for an input without an entry (t, i, script_len 0),
 * which no template matches. n_inputs is the caller's total and d_jobs's
 * capacity: when the txs hold another number of inputs HKV_STATUS_INPUT_COUNT
 * is ORed into d_status (the caller zeroes it), the jobs that fit are written
 * and slots past the device's total get jobs that never verify
 * (tx = 0xFFFFFFFF). Enqueued on hip_stream, not synchronised; stateless as
 * hkv_tx_ids_device. n_inputs <= 0xFFFFFF00. */
int hkv_std_tx_jobs_device(hkv_ctx* ctx, int dev, const hkv_txs* d_txs, const uint32_t* d_prev_offsets,
                           const uint8_t* d_prev_outpoints, const uint32_t* d_prev_scripts,
                           const uint64_t* d_prev_values, size_t n_inputs, uint32_t* d_input_first,
                           hkv_input_job* d_jobs, uint32_t* d_status, void* hip_stream);
/* The per-tx reduction alone: tx bit t = 1 iff [d_input_first[t],
 * d_input_first[t+1]) is not empty and every bit of d_input_bits in it is 1.
 * Writes ceil(n_tx/64)*2 words to d_tx_bits. The caller vouches that
 * d_input_bits holds d_input_first[n_tx] bits. Enqueued, stateless. */
int hkv_tx_verdicts_device(hkv_ctx* ctx, int dev, const uint32_t* d_input_first, size_t n_tx,
                           const uint32_t* d_input_bits, uint32_t* d_tx_bits, void* hip_stream);
/* Batch verifyStdTx on device: hkv_std_tx_jobs_device, then
 * hkv_verify_std_inputs_device_status on the jobs it built, then
 * hkv_tx_verdicts_device, all enqueued on hip_stream with no host wait
 * (ASYNCHRONOUS as hkv_verify_std_inputs_device). The caller supplies its
 * input total n_inputs and the scratch: d_input_first (n_tx + 1 words), d_jobs
 * (n_inputs jobs), d_records (n_inputs * 168 bytes), d_input_bits
 * (ceil(n_inputs/64)*2 words). Out: d_tx_bits (ceil(n_tx/64)*2 words) and
 * d_status (zeroed by the caller; HKV_STATUS_* ORed in). d_input_first and
 * d_input_bits stay readable: input i of tx t is bit d_input_first[t] + i.
 * With HKV_STATUS_INPUT_COUNT set every tx bit is 0. */
int hkv_verify_std_txs_device(hkv_ctx* ctx, int dev, const hkv_txs* d_txs, const uint32_t* d_prev_offsets,
                              const uint8_t* d_prev_outpoints, const uint32_t* d_prev_scripts,
                              const uint64_t* d_prev_values, int32_t forkid, size_t n_inputs,
                              uint32_t* d_input_first, hkv_input_job* d_jobs, void* d_records,
                              uint32_t* d_input_bits, uint32_t* d_tx_bits, uint32_t* d_status, void* hip_stream);
/* Host-memory form; writes ceil(n_tx/32) words of tx verdicts. First device,
 * blocking. The inputs are counted on the device and the 4-byte total is read
 * back (the one synchronisation this form adds) to size the scratch of the
 * composed call. HKV_E_ARG for decreasing prev_offsets or tx offsets;
 * HKV_E_INTERNAL as hkv_verify_std_inputs on a multisig tail fault. */
int hkv_verify_std_txs(hkv_ctx* ctx, const hkv_txs* txs, const uint32_t* prev_offsets,
                       const uint8_t* prev_outpoints, const uint32_t* prev_scripts, const uint64_t* prev_values,
                       int32_t forkid, uint32_t* tx_verdict_bits);

/* ---------------------------------------------------------------------------
 * Header batches: the data-parallel part of
 * importHeaders (/root/reference/src/Haskoin/Node/Chain.hs:500-520), which
 * hands up to 2,000 headers per peer message to haskoin-core connectBlocks
 * [dep]. Per header: headerHash (SHA-256d of the 80-byte wire form) and
 * isValidPOW net h = target > 0 && !overflow && target <= powLimit &&
 * headerPOW h <= target, with (target, overflow) = decodeCompact h.bits;
 * plus the batch linkage connectBlocks relies on (prev field of header i
 * == headerHash of header i-1). The chain-context checks (median time past,
 * retarget / nextWorkRequired, checkpoints, validVersion, chain work) are the
 * stage below (hkv_chain_context_device, hkv_connect_headers*).
 * ------------------------------------------------------------------------ */
#define HKV_HDR_POW_OK 0x01u           /* isValidPOW                               */
#define HKV_HDR_LINK_OK 0x02u          /* prev == hash of the previous header      */
#define HKV_HDR_NEGATIVE 0x04u         /* decodeCompact sign bit with nonzero word */
#define HKV_HDR_OVERFLOW 0x08u         /* decodeCompact overflow                   */
#define HKV_HDR_ZERO_TARGET 0x10u      /* target == 0                              */
#define HKV_HDR_ABOVE_LIMIT 0x20u      /* target > powLimit                        */
#define HKV_HDR_HASH_ABOVE 0x40u       /* headerPOW > target                       */

/* headers: n * 80 wire bytes. pow_limit: 32 bytes, little-endian integer
 * (the network's powLimit). prev_hash: 32 bytes in internal (digest) order,
 * the hash header 0 must extend, or NULL (header 0 then counts as linked).
 * hashes_out: n * 32 bytes (digest order, i.e. headerHash's serialisation);
 * status: n bytes of HKV_HDR_* flags. Host memory, first device, blocking. */
int hkv_check_headers(hkv_ctx* ctx, const uint8_t* headers, size_t n, const uint8_t* pow_limit,
                      const uint8_t* prev_hash, uint8_t* hashes_out, uint8_t* status);
/* Device form: every pointer in HBM of device `dev`; enqueued on hip_stream,
 * not synchronised. */
int hkv_check_headers_device(hkv_ctx* ctx, int dev, const uint8_t* d_headers, size_t n, const uint8_t* d_pow_limit,
                             const uint8_t* d_prev_hash, uint8_t* d_hashes, uint8_t* d_status, void* hip_stream);

/* ---------------------------------------------------------------------------
 * Header chain context: the rest of connectBlocks [dep] behind the per-header
 * checks above, so that a `headers` message goes in and connectBlocks' answer
 * comes out (importHeaders, reference src/Haskoin/Node/Chain.hs:500-520):
 * how many leading headers connect, and each header's height-dependent facts.
 * Every check is a function of a header's actual ancestors (the batch's earlier
 * headers, then the context), never of an earlier verdict: a header's flags
 * presume that its ancestors are as given.
 *
 * Header i of the batch has height H = height0 + i. Its parent P is header
 * i - 1, or the context's tip when i = 0. With limit_bits =
 * encodeCompact(pow_limit):
 *   mtp[i]    element c / 2 of the ascending sort of the c = min(11, i +
 *             n_prev_times) timestamps before header i (the batch's, then the
 *             context's; unsigned compare).
 *   want[i]   Bitcoin's GetNextWorkRequired.
 *             H mod interval != 0: bits(P); with HKV_CHAIN_MIN_DIFFICULTY,
 *             limit_bits when time[i] > time(P) + min_diff_spacing (64 bits),
 *             else real(P), where real(b) = bits(b) if height(b) mod interval
 *             = 0 or bits(b) != limit_bits, else real(parent of b); real(tip)
 *             is period_real_bits.
 *             H mod interval == 0: bits(P) with HKV_CHAIN_NO_RETARGET; else
 *             encodeCompact(min(pow_limit, target(P) * span /
 *             target_timespan)) in exact integers, span = time(P) - time(F)
 *             (signed, 64 bits) clamped to [target_timespan / 4,
 *             4 * target_timespan], F the block at height H - interval
 *             (header i - interval, or period_first_time when i < interval),
 *             target(P) decodeCompact's magnitude. A parent compact that
 *             overflows gives want = 0 and clears BITS_OK.
 *   work[i]   parent_work + the sum over j <= i of headerWork(j), mod 2^256,
 *             32 little-endian bytes; headerWork = floor(2^256 / (target + 1)),
 *             and 0 for a compact that is negative, overflowing or zero.
 *   HKV_CHN_TIME_OK        time[i] > mtp[i]
 *   HKV_CHN_NOT_FUTURE     time[i] <= now + 7200 (64 bits)
 *   HKV_CHN_BITS_OK        bits[i] == want[i]
 *   HKV_CHN_VERSION_OK     validVersion: the version read as a signed number;
 *                          below 2 needs H < bip34_height, below 3 needs
 *                          H < bip66_height, below 4 needs H < bip65_height
 *   HKV_CHN_CHECKPOINT_OK  no checkpoint has height H, or its hash equals
 *                          headerHash(i) as hkv_check_headers* wrote it (the
 *                          BIP34 block is one more checkpoint of the caller's)
 *   HKV_CHN_ALL            the five together
 * BCH's EDA / DAA / ASERT difficulty rules are not covered, nor afterLastCP
 * (it depends on the store's best block).
 * ------------------------------------------------------------------------ */
#define HKV_CHN_TIME_OK 0x01u
#define HKV_CHN_NOT_FUTURE 0x02u
#define HKV_CHN_BITS_OK 0x04u
#define HKV_CHN_VERSION_OK 0x08u
#define HKV_CHN_CHECKPOINT_OK 0x10u
#define HKV_CHN_ALL 0x1Fu
#define HKV_CHAIN_NO_RETARGET 1u    /* regtest: a boundary keeps bits(P)             */
#define HKV_CHAIN_MIN_DIFFICULTY 2u /* testnet: the minimum-difficulty rule and walk */
/* What header 0 stands on, and the network's constants. Read on the host when a
 * call is enqueued and passed to the kernels by value. */
typedef struct hkv_chain_ctx {
  uint32_t height0;            /* header 0's height, >= 1                                        */
  uint32_t n_prev_times;       /* 1..11                                                          */
  uint32_t prev_times[11];     /* header 0's nearest ancestors' times, oldest first, the parent's last */
  uint32_t parent_bits;
  uint32_t period_first_time;  /* time of the block at (height0-1) - ((height0-1) mod interval)  */
  uint32_t period_real_bits;   /* real(tip), see want[i]                                         */
  uint8_t parent_work[32];     /* the tip's chain work, little-endian                            */
  uint64_t now;                /* seconds, below 2^63                                            */
  uint8_t pow_limit[32];       /* little-endian                                                  */
  uint32_t interval;           /* 2016; not 0                                                    */
  uint32_t target_timespan;    /* 1,209,600; within [4, 2^30)                                    */
  uint32_t min_diff_spacing;   /* 1,200                                                          */
  uint32_t bip34_height, bip66_height, bip65_height;
  uint32_t flags;              /* HKV_CHAIN_*                                                    */
} hkv_chain_ctx;
/* The scratch of the stage for n headers, in 32-bit words (3 per header and 20
 * per tile of 256 headers). */
size_t hkv_chain_scratch_words(size_t n);
/* The stage on device (replaces the caller's walk of connectBlocks' context
 * checks: medianTime, nextWorkRequired, validVersion, the checkpoint test and the
 * chain work of haskoin-core Haskoin.Block.Headers [dep]).
 * Stateless and without a lock as hkv_block_spends_device; three launches on
 * hip_stream, enqueued and not synchronised. In: d_headers (n * 80 bytes,
 * 4-aligned), d_hashes (n * 32 bytes as hkv_check_headers_device wrote them on
 * the same stream, 16-aligned; NULL is allowed when n_cp == 0), the
 * checkpoints d_cp_heights (n_cp words, ascending: the caller vouches for the
 * order here, the host form checks it) and d_cp_hashes (n_cp * 32 bytes, digest
 * order, 4-aligned). Out: d_mtp and d_bits (= want; n words each), d_work
 * (n * 32 bytes, 16-aligned), d_status (n bytes of HKV_CHN_*). d_scratch:
 * hkv_chain_scratch_words(n) words. HKV_E_ARG for height0 == 0, height0 + n
 * above 2^32 - 1, n_prev_times outside 1..11, interval == 0, target_timespan
 * outside [4, 2^30), checkpoints without d_hashes, a NULL or misaligned
 * pointer. HKV_OK for n == 0, with nothing launched. */
int hkv_chain_context_device(hkv_ctx* ctx, int dev, const uint8_t* d_headers, size_t n, const uint8_t* d_hashes,
                             const hkv_chain_ctx* chain, const uint32_t* d_cp_heights, const uint8_t* d_cp_hashes,
                             size_t n_cp, uint32_t* d_mtp, uint32_t* d_bits, uint8_t* d_work, uint8_t* d_status,
                             uint32_t* d_scratch, void* hip_stream);
/* connectBlocks on device (replaces the connectBlocks call of importHeaders):
 * hkv_check_headers_device (d_pow_limit, d_prev_hash, d_hashes, d_hdr_status
 * as there; d_pow_limit holds chain->pow_limit), then the stage, then a
 * reduction into *d_first_bad: the smallest i whose chain flags are not
 * HKV_CHN_ALL or whose header status lacks HKV_HDR_POW_OK or HKV_HDR_LINK_OK,
 * n when there is none: the number of headers connectBlocks would connect.
 * Five launches on hip_stream, enqueued and not synchronised. d_hashes is
 * always needed here. With n == 0 nothing is launched and *d_first_bad is
 * not written. */
int hkv_connect_headers_device(hkv_ctx* ctx, int dev, const uint8_t* d_headers, size_t n, const uint8_t* d_pow_limit,
                               const uint8_t* d_prev_hash, const hkv_chain_ctx* chain, const uint32_t* d_cp_heights,
                               const uint8_t* d_cp_hashes, size_t n_cp, uint8_t* d_hashes, uint8_t* d_hdr_status,
                               uint32_t* d_mtp, uint32_t* d_bits, uint8_t* d_work, uint8_t* d_status,
                               uint32_t* d_scratch, uint32_t* d_first_bad, void* hip_stream);
/* Host-memory form of the same (replaces connectBlocks net ... headers): every
 * pointer in host memory, first device, blocking. prev_hash as
 * hkv_check_headers. Any of mtp_out, bits_out, work_out, chain_status may be
 * NULL; hashes_out, hdr_status and n_ok may not. *n_ok = first_bad. Also
 * HKV_E_ARG for checkpoint heights that are not strictly ascending. n == 0
 * succeeds with *n_ok = 0. */
int hkv_connect_headers(hkv_ctx* ctx, const uint8_t* headers, size_t n, const uint8_t* prev_hash,
                        const hkv_chain_ctx* chain, const uint32_t* cp_heights, const uint8_t* cp_hashes, size_t n_cp,
                        uint8_t* hashes_out, uint8_t* hdr_status, uint32_t* mtp_out, uint32_t* bits_out,
                        uint8_t* work_out, uint8_t* chain_status, size_t* n_ok);
/* Measurement hook (no reference counterpart): device dev's later chain-context
 * calls run only the launches named in stages (bit 0 the facts, bit 1 the tile
 * scan, bit 2 the verdicts, bit 3 the first_bad reduction; default 15), so a
 * bench can time each on scratch a full call filled before. Results of a
 * partial call mean nothing. */
int hkv_debug_chain_stages(hkv_ctx* ctx, int dev, uint32_t stages);

/* ---------------------------------------------------------------------------
 * Block merkle roots: haskoin-core buildMerkleRoot [dep, haskoin-core-1.1.0
 * Haskoin.Block.Merkle], as the reference's block test applies it
 * (/root/reference/test/Haskoin/NodeSpec.hs:185-193: b.header.merkle ==
 * buildMerkleRoot (txHash <$> b.txs)) to blocks from getBlocks
 * (src/Haskoin/Node/Peer.hs:309-344). Batched over many blocks.
 * txids: offsets[n_blocks] * 32 bytes, digest order (txHash serialisation);
 * block b owns txids [offsets[b], offsets[b+1]). roots_out: n_blocks * 32
 * (an empty block gets 32 zero bytes). mutated: n_blocks bytes, 1 when two
 * equal hashes are paired at some level (CVE-2012-2459 duplicate-tx form).
 * Host memory, first device, blocking. */
int hkv_merkle_roots(hkv_ctx* ctx, const uint8_t* txids, const uint32_t* offsets, size_t n_blocks,
                     uint8_t* roots_out, uint8_t* mutated);
/* Device form: every pointer in HBM of device `dev`; d_scratch holds
 * offsets[n_blocks] * 32 bytes and may alias nothing else; 16-byte aligned
 * txids / scratch / roots. Enqueued on hip_stream, not synchronised. */
int hkv_merkle_roots_device(hkv_ctx* ctx, int dev, const uint8_t* d_txids, const uint32_t* d_offsets,
                            size_t n_blocks, uint8_t* d_scratch, uint8_t* d_roots, uint8_t* d_mutated,
                            void* hip_stream);

/* ---------------------------------------------------------------------------
 * Transaction hashes and whole-block merkle checks.
 *
 * hkv_tx_ids / hkv_tx_ids_device replace N calls of haskoin-core
 * `txHash :: Tx -> TxHash` [dep, haskoin-core-1.1.0 Haskoin.Transaction.Common]
 * = doubleSHA256 (runPutS (serialize tx{witness = []})): the hash of the
 * decoded and re-serialised tx, not of its wire bytes. The segwit marker and
 * flag and every witness stack are dropped, and the varints haskoin
 * re-serialises (input count, scriptSig lengths, output count, output script
 * lengths) are re-emitted canonically, as in hkv_sighash. The 32 bytes are in
 * digest order, the order hkv_merkle_roots takes and header bytes [36,68)
 * hold. A tx that does not parse (it does not fill its [offsets[t],
 * offsets[t+1]) range exactly, is truncated, is shorter than 10 bytes or has a
 * count or length >= 2^32) gets an all-zero txid and status HKV_TXID_BAD_TX.
 * wtxids and the BIP141 witness commitment are not computed.
 * ------------------------------------------------------------------------ */
#define HKV_TXID_OK 0u
#define HKV_TXID_BAD_TX 1u
/* txHash of every tx of the batch (scripts pool unused, may be NULL/0).
 * txids_out: n_tx * 32 bytes, digest order; status: n_tx bytes or NULL.
 * Host memory, first device, blocking; offsets must be non-decreasing
 * (HKV_E_ARG). */
int hkv_tx_ids(hkv_ctx* ctx, const hkv_txs* txs, uint8_t* txids_out, uint8_t* status);
/* Device form: every pointer (those of d_txs included) in HBM of device
 * `dev`; d_txids 16-byte aligned; d_status n_tx bytes or NULL. Enqueued on
 * hip_stream, not synchronised. Stateless: it uses none of the device's
 * scratch, so it is not ordered against other calls on the device. */
int hkv_tx_ids_device(hkv_ctx* ctx, int dev, const hkv_txs* d_txs, uint8_t* d_txids, uint8_t* d_status,
                      void* hip_stream);

/* hkv_check_blocks / hkv_check_blocks_device replace, for a batch of blocks,
 * the reference's block assertion on getBlocks results
 * (test/Haskoin/NodeSpec.hs:185-193 on blocks from src/Haskoin/Node/Peer.hs:309-344):
 *   b.header.merkle == buildMerkleRoot (txHash <$> b.txs)
 * as hkv_tx_ids, then hkv_merkle_roots, then the comparison with header bytes
 * [36,68), without the txids leaving the device. Per-block status flags: */
#define HKV_BLK_MERKLE_OK 0x01u /* header merkle == buildMerkleRoot (txHash <$> txs) */
#define HKV_BLK_MUTATED 0x02u   /* two equal hashes paired at some level (CVE-2012-2459) */
#define HKV_BLK_BAD_TX 0x04u    /* a tx of the block does not parse; MERKLE_OK is never set */
#define HKV_BLK_EMPTY 0x08u     /* no tx; root all zero; MERKLE_OK is never set */
/* Block b owns txs [block_offsets[b], block_offsets[b+1]) of the batch
 * (n_blocks + 1 tx indices, block_offsets[0] == 0, non-decreasing, last <= n_tx;
 * HKV_E_ARG otherwise); headers: n_blocks * 80 wire bytes. txids_out (n_tx*32)
 * and roots_out (n_blocks*32) may be NULL in the host form; status: n_blocks
 * bytes. The root of a block with a tx that does not parse is computed over
 * the txids as written, that tx's 32 zero bytes included (two such txs paired
 * in the tree also set HKV_BLK_MUTATED): HKV_BLK_BAD_TX is the verdict, the root
 * means nothing. Host memory, first device, blocking. */
int hkv_check_blocks(hkv_ctx* ctx, const hkv_txs* txs, const uint32_t* block_offsets, size_t n_blocks,
                     const uint8_t* headers, uint8_t* txids_out, uint8_t* roots_out, uint8_t* status);
/* Device form: every pointer in HBM of device `dev`, none NULL; d_txids and
 * d_scratch n_tx * 32 bytes each, 16-byte aligned as d_roots (n_blocks * 32),
 * d_scratch aliasing nothing else; d_headers and d_block_offsets 4-byte
 * aligned; d_mutated and d_status n_blocks bytes. The caller vouches for
 * d_block_offsets. Enqueued on hip_stream, not synchronised; stateless as
 * hkv_tx_ids_device. */
int hkv_check_blocks_device(hkv_ctx* ctx, int dev, const hkv_txs* d_txs, const uint32_t* d_block_offsets,
                            size_t n_blocks, const uint8_t* d_headers, uint8_t* d_txids, uint8_t* d_scratch,
                            uint8_t* d_roots, uint8_t* d_mutated, uint8_t* d_status, void* hip_stream);

/* ---------------------------------------------------------------------------
 * Batch verifyStdTx for whole blocks: prevouts created earlier in the batch.
 *
 * hkv_verify_std_txs* takes every prevout from the caller. A block input may
 * spend an output created earlier in the same block, and during initial block
 * download an output of an earlier block of the same batch; no UTXO provider
 * has those yet. hkv_verify_block_txs* finds them itself. The caller hands
 * over the raw txs in block order and, per tx, the prevouts it does have.
 *
 * For input i of a tx t that parses, whose outpoint is (h, k) as wire bytes:
 *  1. The list first, unchanged. Tx t's own prevout list is consulted by the
 *     matchTemplate rule above exactly as in hkv_verify_std_txs*. A hit gives
 *     the entry's script reference and amount, and src = HKV_SRC_LIST.
 *  2. Otherwise the batch. Let p be the smallest index u such that tx u parses
 *     and txHash(tx u) == h, txHash being what hkv_tx_ids computes (digest
 *     order, witness stripped, varints re-emitted canonically). Input i
 *     resolves only if p exists, p < t, and k < the output count of tx p. It
 *     then takes output k of tx p: the scriptPubKey bytes where they lie in
 *     the transaction buffer, and the LE64 amount. src = p.
 *  3. Otherwise nothing. src = HKV_SRC_NONE and the job keeps script_len = 0.
 *     No template matches a zero-length script, so the input is false and so
 *     is the transaction.
 * Consequences:
 *  - A transaction cannot spend a later transaction. It cannot spend itself.
 *  - A parent that does not parse has an all-zero txid and is never indexed.
 *    A coinbase input (32 zero bytes, index 0xFFFFFFFF) therefore finds
 *    nothing, and its transaction is 0, as under verifyStdTx.
 *  - Transactions with equal txids have equal outputs, so the choice of p
 *    affects only src.
 *  - Two inputs that take the same in-batch output both resolve: this call
 *    gives signature verdicts only. Double spends within the batch and each
 *    tx's value balance are what hkv_block_spends_device (below) adds, on the
 *    arrays this call leaves in HBM; spends against the caller's UTXO set
 *    stay with the caller.
 *  - A batch with all-empty lists is legal.
 *  - A batch with no in-batch spends gives exactly the verdicts of
 *    hkv_verify_std_txs*.
 *
 * Script references without copies. The per-input verify reads a prevout
 * script as scripts + job.script_off. The device entry points below therefore
 * require the script pool to follow the tx bytes in one address range:
 * d_txs->scripts >= d_txs->bytes and (scripts - bytes) + scripts_len <=
 * 0xFFFFFFFF (HKV_E_ARG otherwise), and the caller vouches that the pool
 * starts at or after the end of the last tx, as it vouches for the offsets.
 * scripts is also the only bound these entry points have on the tx bytes, so
 * it is never NULL: a batch without a pool (all lists empty) passes
 * scripts_len 0 and any scripts at or after the end of the last tx, e.g.
 * bytes + offsets[n_tx] (HKV_E_ARG for NULL). The jobs they write count from d_txs->bytes:
 * a list entry's reference is rebased by scripts - bytes, an in-batch
 * reference is the offset of the output's script within the tx bytes, and the
 * verify runs on the view {scripts = bytes, scripts_len = (scripts - bytes) +
 * scripts_len}. A list entry whose (offset, length) overruns the caller's
 * scripts_len gets script_off 0 and script_len 0 (its amount and
 * src = HKV_SRC_LIST stay): the verdict such an entry has under
 * hkv_verify_std_txs*. The host form takes any two host buffers and stages
 * them so (the tx bytes rounded up to 4, then the pool).
 *
 * The walk to output k of a parent is O(parent inputs + k) dependent byte
 * reads by the child's lane: a parent of 2,000 outputs with 2,000 children in
 * the batch is about 4 M steps.
 * ------------------------------------------------------------------------ */
#define HKV_SRC_NONE 0xFFFFFFFFu /* the input found no prevout                  */
#define HKV_SRC_LIST 0xFFFFFFFEu /* the prevout came from the tx's own list     */
/* The txid table: open addressing over n_tx txids, uint32_t slots holding the
 * smallest tx index of a txid, 0xFFFFFFFF when empty. This is the slot count
 * for n_tx txids: the smallest power of two >= 2 * n_tx and >= 64 (0 for
 * n_tx >= 0xFFFFFF00). Replaces sizing a `HashMap TxHash Int`. */
size_t hkv_txid_table_slots(size_t n_tx);
/* Build the table (replaces HashMap.fromListWith min (zip txids [0..])):
 * d_txids n_tx * 32 bytes as hkv_tx_ids_device writes them, 16-byte aligned;
 * d_table n_slots words, n_slots a power of two >= hkv_txid_table_slots(n_tx)
 * and <= 2^31. All-zero txids are skipped. The slot hash is salted per
 * context at hkv_open. Enqueued on hip_stream (a memset of the table, then
 * one launch), not synchronised; stateless as hkv_tx_ids_device. */
int hkv_txid_index_device(hkv_ctx* ctx, int dev, const uint8_t* d_txids, size_t n_tx, uint32_t* d_table,
                          size_t n_slots, void* hip_stream);
/* Look n_q 32-byte txids (any alignment) up in a table hkv_txid_index_device
 * built from the same d_txids, n_tx and n_slots on this context (replaces n_q
 * calls of HashMap.lookup): d_found[q] = the smallest tx index with that
 * txid, or 0xFFFFFFFF. Enqueued, stateless. */
int hkv_txid_lookup_device(hkv_ctx* ctx, int dev, const uint8_t* d_txids, size_t n_tx, const uint32_t* d_table,
                           size_t n_slots, const uint8_t* d_queries32, size_t n_q, uint32_t* d_found,
                           void* hip_stream);
/* The prevout provider alone (replaces the caller's parse, txHash, txid map
 * and output copy in front of verifyStdTx): hkv_tx_ids_device into d_txids,
 * hkv_txid_index_device into d_table, the input counts and their prefix sums
 * as hkv_std_tx_jobs_device, then one job and one src word per input by the
 * rule above. Arguments as hkv_std_tx_jobs_device, plus d_txids (n_tx * 32
 * bytes, 16-byte aligned), d_table / n_slots as above and d_input_src
 * (n_inputs words: HKV_SRC_LIST, HKV_SRC_NONE or the parent's tx index;
 * HKV_SRC_NONE in slots past the device's total). HKV_STATUS_INPUT_COUNT and
 * the surplus slots behave as there. Enqueued, stateless: no context scratch,
 * no lock. n_inputs <= 0xFFFFFF00. */
int hkv_block_tx_jobs_device(hkv_ctx* ctx, int dev, const hkv_txs* d_txs, const uint32_t* d_prev_offsets,
                             const uint8_t* d_prev_outpoints, const uint32_t* d_prev_scripts,
                             const uint64_t* d_prev_values, size_t n_inputs, uint8_t* d_txids, uint32_t* d_table,
                             size_t n_slots, uint32_t* d_input_first, hkv_input_job* d_jobs, uint32_t* d_input_src,
                             uint32_t* d_status, void* hip_stream);
/* Batch verifyStdTx with in-batch prevouts, on device (replaces N calls of
 * verifyStdTx and the host work above): txids, table, count, scan, block jobs,
 * the per-input verify on the view, the per-tx reduction, all enqueued on
 * hip_stream with no host wait (ASYNCHRONOUS as hkv_verify_std_txs_device,
 * whose arguments, scratch and status word it shares). d_txids,
 * d_input_first, d_input_src and d_input_bits stay readable afterwards. */
int hkv_verify_block_txs_device(hkv_ctx* ctx, int dev, const hkv_txs* d_txs, const uint32_t* d_prev_offsets,
                                const uint8_t* d_prev_outpoints, const uint32_t* d_prev_scripts,
                                const uint64_t* d_prev_values, int32_t forkid, size_t n_inputs, uint8_t* d_txids,
                                uint32_t* d_table, size_t n_slots, uint32_t* d_input_first, hkv_input_job* d_jobs,
                                uint32_t* d_input_src, void* d_records, uint32_t* d_input_bits, uint32_t* d_tx_bits,
                                uint32_t* d_status, void* hip_stream);
/* Host-memory form (replaces the same calls); writes ceil(n_tx/32) words of tx
 * verdicts. First device, blocking, one readback of the input total as
 * hkv_verify_std_txs. Optional outputs: input_first (n_tx + 1 words, or NULL)
 * and input_src (or NULL; input_src_cap words of room: HKV_E_ARG when the
 * batch holds more inputs; an input is at least 41 bytes of its tx). HKV_E_ARG
 * for decreasing prev_offsets or tx offsets; HKV_E_INTERNAL on a multisig tail
 * fault. */
int hkv_verify_block_txs(hkv_ctx* ctx, const hkv_txs* txs, const uint32_t* prev_offsets,
                         const uint8_t* prev_outpoints, const uint32_t* prev_scripts, const uint64_t* prev_values,
                         int32_t forkid, uint32_t* tx_verdict_bits, uint32_t* input_first, uint32_t* input_src,
                         size_t input_src_cap);
/* Test hook in the style of hkv_debug_ms_window (no reference counterpart):
 * the slot hash of the txid table is ANDed with mask in device dev's later
 * calls (default 0xFFFFFFFF). 0 sends every key to slot 0, the longest
 * possible probe chain. The same mask is ANDed into the slot hash of the
 * spent-outpoint table of hkv_block_spends_device. Results do not depend on
 * the mask or the salt. */
int hkv_debug_txid_hash_mask(hkv_ctx* ctx, int dev, uint32_t mask);

/* ---------------------------------------------------------------------------
 * Whole-block spend checks: double spends within the batch and value balance.
 *
 * hkv_verify_block_txs* delivers one signature verdict per tx. A block in
 * which a tx is simply repeated (the copy spends the same outputs again and
 * every signature still verifies) and a block whose txs pay out more than
 * they take in both pass it. This stage adds what a validator does around
 * verifyStdTx when it connects a block (parse every tx for its outpoints, a
 * `HashMap OutPoint` of the spent ones, the sums of the input and output
 * amounts against the Network's maxSatoshi), on the arrays the block call
 * leaves in HBM. There is no haskoin-core function of this name.
 *
 * Inputs are numbered as everywhere else: input i of tx t is
 * g = d_input_first[t] + i; a tx that does not parse has no inputs.
 *
 * Per input g, the first spender:
 *  - spender[g] is the smallest g' whose 36-byte wire outpoint equals input
 *    g's. It may be g itself.
 *  - The comparison is on bytes only. Whether either input resolved does not
 *    matter. Duplicates inside one tx count like duplicates across txs.
 *  - The null outpoint (32 zero bytes, index 0xFFFFFFFF) is never indexed.
 *    Such an input has spender[g] = g, so the coinbases of several blocks in
 *    one batch do not conflict.
 *  - Slots past the device's input total get 0xFFFFFFFF.
 *
 * Per tx t with at least one input, one flag byte and two sums, with
 * in[g] = d_jobs[g].value (the amount the block call resolved) and the
 * outputs' LE64 amounts read from the wire bytes:
 *   HKV_SPEND_RESOLVED   every input has d_input_src[g] != HKV_SRC_NONE
 *   HKV_SPEND_FIRST      every input has spender[g] == g
 *   HKV_SPEND_IN_RANGE   every in[g] <= max_money and their exact sum
 *                        <= max_money
 *   HKV_SPEND_OUT_RANGE  every output amount <= max_money and their exact sum
 *                        <= max_money (a tx with no outputs has sum 0, in
 *                        range)
 *   HKV_SPEND_BALANCED   RESOLVED, IN_RANGE, OUT_RANGE and in_sum >= out_sum
 *                        (equality is balanced: fee 0)
 *   HKV_SPEND_COINBASE   exactly one input, and its outpoint is null
 *   HKV_SPEND_OK         the first five
 *  - tx_sums[2t] is in_sum and tx_sums[2t + 1] is out_sum.
 *  - Each sum is exact when its RANGE flag is set, and UINT64_MAX otherwise.
 *  - A tx with no inputs (it does not parse, or it has none) gets flags 0 and
 *    sums 0.
 *  - max_money must be below 2^63 (HKV_E_ARG otherwise), so a running sum
 *    that is still in range cannot wrap when one in-range amount is added.
 *    Once either bound is exceeded, the sum sticks at out of range.
 *
 * Count mismatch: the stage checks d_input_first[n_tx] against the caller's
 * n_inputs itself, and honours HKV_STATUS_INPUT_COUNT if the provider already
 * set it in the same status word. On a mismatch it ORs the bit in; every tx
 * flag byte is then 0, every sum is 0, nothing is written past n_inputs slots
 * of any per-input array, and no read leaves the arrays.
 *
 * The first spender comes from an open-addressing table over the batch's
 * inputs as the txid table above: uint32_t slots holding the smallest input
 * index of one outpoint, 0xFFFFFFFF when empty, the slot hash salted per
 * context and mixed with the outpoint's index. One lane walks one tx and
 * folds one tx's inputs: a tx of 100,000 inputs is one lane's serial chain.
 * ------------------------------------------------------------------------ */
#define HKV_SPEND_RESOLVED 0x01u
#define HKV_SPEND_FIRST 0x02u
#define HKV_SPEND_IN_RANGE 0x04u
#define HKV_SPEND_OUT_RANGE 0x08u
#define HKV_SPEND_BALANCED 0x10u
#define HKV_SPEND_COINBASE 0x20u
#define HKV_SPEND_OK 0x1Fu
/* The slot count of the spent-outpoint table for n_inputs inputs: the smallest
 * power of two >= 2 * n_inputs and >= 64, and 0 when that would exceed 2^31
 * (n_inputs > 2^30). Replaces sizing a `HashMap OutPoint Int`. */
size_t hkv_spend_table_slots(size_t n_inputs);
/* The spend stage on device (replaces the caller's parse for outpoints, its
 * HashMap.fromListWith min (zip outpoints [0..]) and its amount sums). It runs
 * after hkv_block_tx_jobs_device or hkv_verify_block_txs_device on the same
 * stream, on the arrays those leave readable: d_txs, d_input_first
 * (n_tx + 1 words), d_jobs (n_inputs jobs, of which the value is read),
 * d_input_src (n_inputs words), with the same n_inputs and the same d_status.
 * Scratch: d_input_off (n_inputs words: each input's outpoint offset, counted
 * from d_txs->bytes; stays readable) and d_table (n_slots words, n_slots a
 * power of two within [hkv_spend_table_slots(n_inputs), 2^31]). Out:
 * d_input_spender (n_inputs words), d_tx_sums (2 * n_tx words, 8-byte
 * aligned), d_tx_flags (n_tx bytes), HKV_STATUS_* ORed into d_status. Four
 * launches and a memset of the table on hip_stream, enqueued and not
 * synchronised; stateless and without a lock as hkv_block_tx_jobs_device: of
 * the context it reads only the salt and the debug mask. HKV_E_ARG for a NULL
 * or misaligned pointer, max_money >= 2^63, n_inputs > 0xFFFFFF00 and an
 * n_slots outside that range. HKV_OK for n_tx == 0, with nothing launched;
 * with n_inputs == 0 only the two per-tx launches run (and the per-input
 * pointers may be NULL). */
int hkv_block_spends_device(hkv_ctx* ctx, int dev, const hkv_txs* d_txs, const uint32_t* d_input_first,
                            const hkv_input_job* d_jobs, const uint32_t* d_input_src, size_t n_inputs,
                            uint64_t max_money, uint32_t* d_input_off, uint32_t* d_table, size_t n_slots,
                            uint32_t* d_input_spender, uint64_t* d_tx_sums, uint8_t* d_tx_flags, uint32_t* d_status,
                            void* hip_stream);
/* Host-memory form: hkv_verify_block_txs, then the spend stage on the same
 * stream, with the one readback of the input total that call has, then the
 * extra copies back. Arguments as there, plus max_money, input_spender
 * (or NULL), tx_sums (2 * n_tx words, or NULL) and tx_flags (n_tx bytes, not
 * NULL). input_cap is the room of input_src and of input_spender, in words:
 * HKV_E_ARG when either is given and the batch holds more inputs.
 * tx_verdict_bits, input_first and input_src come out bit for bit as from
 * hkv_verify_block_txs. First device, blocking. */
int hkv_verify_block_txs_spends(hkv_ctx* ctx, const hkv_txs* txs, const uint32_t* prev_offsets,
                                const uint8_t* prev_outpoints, const uint32_t* prev_scripts,
                                const uint64_t* prev_values, int32_t forkid, uint64_t max_money,
                                uint32_t* tx_verdict_bits, uint32_t* input_first, uint32_t* input_src,
                                uint32_t* input_spender, size_t input_cap, uint64_t* tx_sums, uint8_t* tx_flags);
/* Measurement hook (no reference counterpart): device dev's later
 * hkv_block_spends_device calls run only the launches named in stages (bit 0
 * the walk, bit 1 the table's memset and inserts, bit 2 the spender lookup,
 * bit 3 the per-tx fold; default 15), so a bench can time each on arrays a
 * full call filled before. Results of a partial call mean nothing. */
int hkv_debug_spend_stages(hkv_ctx* ctx, int dev, uint32_t stages);

/* Synthetic-data hooks (block-mix generator, off the verify path):
 * n random private keys -> d_priv (n*32, big-endian), compressed public keys
 * d_pub (n*33) and their HASH160 d_h160 (n*20);
 * ECDSA signatures (r||s big-endian, low S, random nonces) of msg j
 * (d_msg + j*msg_stride) with key d_key_idx[j] -> d_sig (n*64). */
int hkv_gen_keys_device(hkv_ctx* ctx, int dev, uint64_t seed, size_t n, uint8_t* d_priv, uint8_t* d_pub,
                        uint8_t* d_h160, void* hip_stream);
int hkv_gen_sign_device(hkv_ctx* ctx, int dev, uint64_t seed, size_t n, const uint8_t* d_priv,
                        const uint32_t* d_key_idx, const uint8_t* d_msg, size_t msg_stride, uint8_t* d_sig,
                        void* hip_stream);

/* Known-answer hook for the tests: applies op (see hkv_internal.h) to n
 * pairs of 8-limb little-endian operands in device memory; 16 words out. */
int hkv_debug_op(hkv_ctx* ctx, int dev, uint32_t op, size_t n, const uint32_t* d_a, const uint32_t* d_b,
                 uint32_t* d_out, void* hip_stream);

/* Per-kernel timing with HIP events recorded on the launch stream around the
 * prologue and ecmult kernels of every subsequent verify (bench.py's roofline).
 * read: synchronises, returns summed milliseconds and the launch count, resets. */
int hkv_profile_enable(hkv_ctx* ctx, int on);
int hkv_profile_read(hkv_ctx* ctx, int dev, double* prologue_ms, double* ecmult_ms, uint64_t* launches);
/* Shader clock (MHz) block 0 of the last profiled ecmult launch ran at:
 * clock64() / wall_clock64() deltas around its work (so the roofline can be
 * priced at the measured clock). Synchronises the device. */
int hkv_profile_clock(hkv_ctx* ctx, int dev, double* sclk_mhz);

/* Phase stamps of workgroup 0 of the last profiled small-batch (split)
 * launch: n <= 12 constant-rate clock values (tick_ns nanoseconds per tick)
 * at its phase boundaries — 0 start, 1 k1 table built, 2 past barrier P,
 * 3 k1 chain done, 4 past barrier A, 5 join done, 6 signature parse done,
 * 7 u1 G done, 8 key sqrt done, 9 k2 table built, 10 k2 chain done.
 * Synchronises the device. */
int hkv_profile_phases(hkv_ctx* ctx, int dev, uint64_t* stamps, size_t n, double* tick_ns);

/* Per-workgroup (start, end) constant-rate clock stamps of the last profiled
 * block-kernel launch (a block: at most 16 signatures per CU): stamps[2g] =
 * workgroup g's first instruction, stamps[2g + 1] = its last; n_groups <=
 * 4096. Where the launch's span goes beyond workgroup 0's phase stamps.
 * Synchronises the device. (Measurement only; no reference counterpart.) */
int hkv_profile_group_stamps(hkv_ctx* ctx, int dev, uint64_t* stamps, size_t n_groups, double* tick_ns);

const char* hkv_strerror(int err);
const char* hkv_last_hip_error(void);
int hkv_device_count(void);
/* ABI version: (major << 16) | minor */
uint32_t hkv_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HKV_H */
