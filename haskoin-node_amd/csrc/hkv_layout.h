// hkv_layout.h — buffer layouts shared by the HIP kernels and the host API.
#pragma once
#include <stdint.h>

namespace hkv {

// Input record (AoS, include/hkv.h): msg32 | r32 | s32 | pklen u8 | pubkey[65] | pad[6]
constexpr int REC_SIZE = 168;
constexpr int REC_WORDS = REC_SIZE / 4;

// Q digit word of window w (w = 0..NWIN-1, bit position QW*w): biased Booth
//   digits, bits 0..QW d1 + QBIAS (k1, radix 2^QW, -QBIAS..QBIAS), bits
//   QW+1..2QW+1 d2 + QBIAS (k2)
// G digit word of G window j (j = 0..GWIN-1, bit position GTAB_W*j = Q
// window GSTEP*j), one per u1 half: bits 0..GTAB_W-1 |d| (0..2^(GTAB_W-1)),
// bit GTAB_W sign. Default radix 2^20: 7 windows, every fifth Q window.
// HKV_QW = 5 (radix-32 Q windows: 52 instead of 66 Q additions, 125
// doublings, a 16-entry table) is correct (GPU suite green) but measured
// 1-1.5% slower at 1M (profiles/r02_variants.log): the 400 MB of per-lane
// tables of a full grid no longer stay in the 256 MB MALL.
#ifndef HKV_QW
#define HKV_QW 4
#endif
#ifndef HKV_GTAB_W
#define HKV_GTAB_W 20
#endif
// The table-and-chain shape's chain (hkv_kernels.hip 2a) on joint radix-8
// digits over Z[lambda] (hkv_joint_digits.h): 129 doublings and 44 additions
// from an 11-entry table, where the Booth chain runs 124 and 66 from 8
// entries. A form of the radix-16 layout only. 0: the Booth chain (the A/B).
#ifndef HKV_JOINT_DIGITS
#define HKV_JOINT_DIGITS (HKV_QW == 4)
#endif
constexpr int QW = HKV_QW;                       // Booth radix 2^QW of the k1 / k2 windows
static_assert(QW == 4 || QW == 5, "radix-16 or radix-32 Q windows");
constexpr int GTAB_W = HKV_GTAB_W;            // Booth radix of the fixed-base tables
static_assert(GTAB_W % QW == 0 && GTAB_W >= 8 && GTAB_W <= 28, "G windows sit on Q window boundaries");
constexpr int NWIN = (130 + QW - 1) / QW;        // 33 / 26: |k| < 2^129 plus the Booth carry
constexpr int QBIAS = 1 << (QW - 1);             // digit range -QBIAS..QBIAS
constexpr bool JOINT_DIGITS = HKV_JOINT_DIGITS != 0;
static_assert(!JOINT_DIGITS || QW == 4, "the joint digits are rebuilt from radix-16 Booth digits");
constexpr int QDIG_BITS = QW + 1;                // width of a biased digit in the digit word
constexpr uint32_t QDIG_MASK = (1u << QDIG_BITS) - 1u;
constexpr int GWIN = (128 + GTAB_W) / GTAB_W;  // covers 129 bits with the Booth carry
constexpr int GSTEP = GTAB_W / QW;             // Q windows per G window
constexpr uint32_t GD_MAG = (1u << GTAB_W) - 1u, GD_NEG = 1u << GTAB_W;
constexpr uint32_t DIG_ZERO = (uint32_t)QBIAS | ((uint32_t)QBIAS << QDIG_BITS);

// signatures per thread in the scalar kernel (one s^-1 per BATCH_INV via
// Montgomery's trick: 3(B-1) multiplications + 1 inversion)
#ifndef HKV_BATCH_INV
#define HKV_BATCH_INV 16
#endif
constexpr int BATCH_INV = HKV_BATCH_INV;
// signatures per lane of the verdict kernel: one Fermat den^-1 (255S + 15M,
// a dependent chain) per lane, 3 multiplications per signature
#ifndef HKV_VERDICT_BATCH
#define HKV_VERDICT_BATCH 16
#endif
constexpr int VERDICT_BATCH = HKV_VERDICT_BATCH;
// signatures per workgroup of the small-batch kernels (hkv_kernels.hip 2c, 2d):
// the pair-lane split kernel takes 32 on 4 waves, the block kernel 16
constexpr int PAIR_SIGS = 32;
constexpr int BLK_SIGS = 16;

// y-free verification (every launch shape; hkv_kernels.hip §2b): the
// prologue stores w = x^3 + 7 (IM_W) instead of solving y = sqrt(w);
// ecmult runs u2 * Q' on E_w : y^2 = x^3 + 7 w^3 with Q' = (x w, w^2) and
// leaves B' = (X, Y, Z) over the Q-digit words; the finish kernel adds the
// u1 * G sum from per-window tables and reduces "x(u1 G + u2 Q) == r" to
// y_c = num / den, accepted iff y_c^2 == w with the key's y parity. Small
// batches (hkv_pair_split_kernel, §2c) run the u1 * G sum and the key's
// square root on their own waves beside the two Q chains and join exactly in
// the kernel.

// the lane's flags word (IM_FLAGS)
constexpr uint32_t FLAG_VALID = 1u;      // the signature and key parse and every check so far passed
constexpr uint32_t FLAG_NEG1 = 2u;       // the GLV half k1 is negative
constexpr uint32_t FLAG_NEG2 = 4u;       // the GLV half k2 is negative
constexpr uint32_t FLAG_GLV_OVF = 8u;    // the GLV split overflowed (unreachable; fails closed)
constexpr uint32_t FLAG_YODD = 16u;      // the key's y is odd (prefix 03/07, or the 04 key's y)
constexpr uint32_t FLAG_COMP = 32u;      // compressed key: x^3 + 7 not yet shown to be a square
constexpr uint32_t FLAG_BINF = 64u;      // B' = u2 * Q' is infinity
constexpr uint32_t FLAG_DECIDED = 128u;  // the finish kernel decided the verdict (rare cases)
constexpr uint32_t FLAG_ACCEPT = 256u;   // ... and it is accept
constexpr uint32_t FLAG_RARE = 512u;     // A or B infinity, or A = +-B: the exact slow path decides
constexpr uint32_t FLAG_AINF = 1024u;    // A = u1 * G is infinity (u1 = 0)
// the small-batch join's flags word (AUX_FLAGS), and AUX_SQ's value
constexpr uint32_t AUXF_AINF = 1u, AUXF_SQ = 2u;
constexpr uint32_t AUXF_STDOK = 4u;  // standard inputs: the script checks passed

// ---------------------------------------------------------------------------
// The verify intermediates. Every verify launch hands its results to the next
// through `im` (IM_WORDS word rows per signature); the small-batch kernels
// also use `aux` (AUX_WORDS). Both are structure-of-arrays: word k of field F
// of signature i sits at [(F.off + k) * n_pad + i], an index the SoA view of
// hkv_kernels.hip forms (and the few sites its header comment names). The
// fields of `im` alias each other by phase: the table names each once, the
// live sets below it say which hold data at each hand-off, and the
// static_asserts check that fields live together share no word row at any
// supported HKV_QW / HKV_GTAB_W (tests/test_im_layout.py compiles them all).
// ---------------------------------------------------------------------------
struct Field {
  int off, len;  // word rows [off, off + len)
};

constexpr Field IM_FLAGS = {0, 1};    // FLAG_* of the lane
constexpr Field IM_QX = {1, 8};       // affine pubkey x (normalised)
constexpr Field IM_W = {9, 8};        // w = x^3 + 7 (normalised)
constexpr Field IM_S = {17, 8};       // s after the mode's high-S policy (words 25, 26 unused)
constexpr Field IM_M = {27, 8};       // m = msg mod n
constexpr Field IM_R = {35, 8};       // r (< n)
constexpr Field IM_C = {43, 8};       // batch-inversion prefix product, then s^-1
constexpr Field IM_DIG = {51, NWIN};  // Q digit word of window w (above), NWIN <= 33
constexpr Field IM_GDIG = {84, 2 * GWIN};  // G digit words of window j: u1_lo at 2j, u1_hi at 2j + 1
constexpr int IM_WORDS = IM_GDIG.off + IM_GDIG.len;
// over the Q digits, once the chains have consumed them
constexpr Field IM_BX = {IM_DIG.off, 8};         // B' = u2 * Q' = (X, Y, Z), Jacobian on E_w
constexpr Field IM_BY = {IM_DIG.off + 8, 8};
constexpr Field IM_BZ = {IM_DIG.off + 16, 8};
constexpr Field IM_NUM = {IM_DIG.off, 8};        // common lanes: num for the candidate r,
constexpr Field IM_NUMN = {IM_DIG.off + 8, 8};   //   num for the candidate r + n,
constexpr Field IM_DEN = {IM_DIG.off + 16, 8};   //   den (y_c = num / den)
// rare lanes: A = u1 * G parked for hkv_rare_kernel over x, s and m
constexpr Field IM_AX = {IM_QX.off, 8};
constexpr Field IM_AY = {IM_S.off, 8};
constexpr Field IM_AZ = {IM_S.off + 8, 8};
// one word row indexed by rank, not by lane: entry k is the k-th rare lane's
// index (the finish kernel compacts them), so it must miss every field any
// lane still holds. It is word 6 of another lane's m: safe because nothing
// reads m after hkv_glv_kernel (the lane prologue of standard inputs never
// stores m), which the live sets from the glv hand-off on state by leaving
// IM_M out.
constexpr Field IM_RARE_LIST = {IM_AZ.off + 8, 1};

// aux: the small-batch kernels' signature and square-root waves' output for
// the in-kernel join
constexpr Field AUX_AX = {0, 8};
constexpr Field AUX_AY = {8, 8};
constexpr Field AUX_AZ = {16, 8};  // A = u1 * G, Jacobian on E
constexpr Field AUX_Y0 = {24, 8};     // the key's y0 = sqrt(w) of its parity
constexpr Field AUX_FLAGS = {32, 1};  // AUXF_AINF, AUXF_STDOK
constexpr Field AUX_SQ = {33, 1};     // AUXF_SQ: w is a square (the sqrt wave's word)
constexpr int AUX_WORDS = 34;

// What each hand-off carries. A launch may write a field only if no field of
// the live set it hands on shares its words (and it has read what it needs of
// the set it was handed).
constexpr Field LIVE_PROLOGUE_INV[] = {IM_FLAGS, IM_QX, IM_W, IM_R, IM_S, IM_M};
constexpr Field LIVE_INV_GLV[] = {IM_FLAGS, IM_QX, IM_W, IM_R, IM_S, IM_M, IM_C};
// from hkv_glv_kernel or the standard-input lane prologue to the table, chain
// and mid-size kernels (the table build is the last reader of QX; the late
// standard-input form needs C = s^-1 up to the finish kernel)
constexpr Field LIVE_GLV_ECMULT[] = {IM_FLAGS, IM_QX, IM_W, IM_R, IM_C, IM_DIG, IM_GDIG};
constexpr Field LIVE_CHAIN_FINISH[] = {IM_FLAGS, IM_W, IM_R, IM_C, IM_BX, IM_BY, IM_BZ, IM_GDIG};
// from the finish kernel to hkv_rare_kernel and hkv_yverdict_kernel, per
// lane one of the two; C is free, and the verdict kernel keeps its prefix
// products there
constexpr Field LIVE_FINISH_RARE[] = {IM_FLAGS, IM_W, IM_R, IM_RARE_LIST, IM_AX, IM_AY, IM_AZ, IM_BX, IM_BY, IM_BZ};
constexpr Field LIVE_FINISH_VERDICT[] = {IM_FLAGS, IM_W, IM_R, IM_RARE_LIST, IM_NUM, IM_NUMN, IM_DEN, IM_C};
// inside the small-batch kernels and the multisig tail's pair groups
constexpr Field LIVE_SMALL_IM[] = {IM_FLAGS, IM_R, IM_DIG, IM_GDIG};
constexpr Field LIVE_SMALL_AUX[] = {AUX_AX, AUX_AY, AUX_AZ, AUX_Y0, AUX_FLAGS, AUX_SQ};

constexpr bool fields_overlap(Field a, Field b) { return a.off < b.off + b.len && b.off < a.off + a.len; }
// every field inside [0, words) and no two sharing a word row
template <int N>
constexpr bool live_set_ok(const Field (&f)[N], int words) {
  for (int a = 0; a < N; ++a) {
    if (f[a].off < 0 || f[a].len < 1 || f[a].off + f[a].len > words) return false;
    for (int b = a + 1; b < N; ++b)
      if (fields_overlap(f[a], f[b])) return false;
  }
  return true;
}
static_assert(live_set_ok(LIVE_PROLOGUE_INV, IM_WORDS), "prologue -> inv");
static_assert(live_set_ok(LIVE_INV_GLV, IM_WORDS), "inv -> glv");
static_assert(live_set_ok(LIVE_GLV_ECMULT, IM_WORDS), "glv -> table / chain / mid-size");
static_assert(live_set_ok(LIVE_CHAIN_FINISH, IM_WORDS), "chain -> finish");
static_assert(live_set_ok(LIVE_FINISH_RARE, IM_WORDS), "finish -> rare");
static_assert(live_set_ok(LIVE_FINISH_VERDICT, IM_WORDS), "finish -> verdict");
static_assert(live_set_ok(LIVE_SMALL_IM, IM_WORDS), "small-batch im");
static_assert(live_set_ok(LIVE_SMALL_AUX, AUX_WORDS), "small-batch aux");

// Fixed-base tables in HBM: multiples j*B for j = 1..2^19, affine, 16 dwords
// per entry [x(8) | y(8)], table t at entry offset t*2^19: table 2j + h holds
// B = 2^(GTAB_W j + 128 h) G (j = 0..GWIN-1), so the u1 * G sum (finish
// kernel, split waves 4-5) takes one addition per table and no doublings.
constexpr int GTAB_ENTRIES = 1 << (GTAB_W - 1);
constexpr int GTAB_TABLES = 2 * GWIN;
constexpr size_t GTAB_DWORDS = (size_t)GTAB_TABLES * GTAB_ENTRIES * 16;

// Per-lane Q table: multiples j*Q, j = 1..QBIAS, affine on the lane's isomorphic
// curve; per entry 6 quads (16 B): x(2) | y(2) | beta*x(2); entry e of lane L
// at quad (e * n_lanes + L) * 6 (hkv_kernels.hip qtab_ptr).
constexpr int QTAB_ENTRIES = QBIAS;
constexpr int QTAB_QUADS_PER_ENTRY = 6;
constexpr int QTAB_QUADS = QTAB_ENTRIES * QTAB_QUADS_PER_ENTRY;
// The joint form of the table launch (HKV_JOINT_DIGITS, hkv_joint_digits.h)
// keeps its 11 entries (a + b lambda) Q' in the same QTAB_QUADS quads per
// signature, so the scratch and the plan do not change: per entry 4 quads,
// x(2) | y(2), entry e of lane L at quad (e * n_lanes + L) * 4; the chain forms
// beta * x by one product per window. The 4 quads per lane left over, at quad
// 44 n_lanes + 4 L, park z-ratios during the build (hkv_kernels.hip).
constexpr int JQ_ENTRIES = 11;
constexpr int JQ_QUADS_PER_ENTRY = 4;
constexpr int JQ_SPARE_QUADS = QTAB_QUADS - JQ_ENTRIES * JQ_QUADS_PER_ENTRY;
static_assert(!JOINT_DIGITS || JQ_SPARE_QUADS == 4, "the joint table and two parked z-ratios fill the Booth table's quads");

// Record batches above half the resident grid (hkv_kernels.hip 2a) build the
// tables in one launch and run the chains in the next, over chunks of at most
// this many signatures. Each signature of a chunk of cn owns table slot s
// (n_lanes = cn) and, behind the chunk's tables, 2 quads for its table scale
// Zg at quad cn * QTAB_QUADS + 2 s: 800 B per signature, 839 MB at 2^20.
#ifndef HKV_REC_CHUNK
#define HKV_REC_CHUNK (1u << 20)
#endif
// A chunk runs in parts of this many signatures, two at a time on two streams
// (hkv_launch_plan.h RecPlan::part_len): each part's tables and Zg slots take
// one of two slots inside the chunk's scratch, laid out as above with cn the
// part's length. 0: chunks run whole. Two resident grids of an MI355X per
// part, so a 2^20 chunk in two parts, measured best on the 1M batch among
// half a grid, one and two (120.8 / 122.1, 128.5 /
// 128.0 and 129.6 / 128.7 M verifies/s against 125.5 / 125.3 whole).
#ifndef HKV_REC_PART
#define HKV_REC_PART (1u << 19)
#endif
constexpr int QTAB_ZG_QUADS = 2;

constexpr int WG = 256;                // threads per workgroup (4 waves)

// Per-transaction index (hkv_sighash.hip, tx index kernel), AoS rows of
// TXT_WORDS words so a job's gather of its tx row is one 128-byte line.
// Offsets are absolute byte offsets into the batch's tx buffer. The three
// BIP143 hashes are stored in digest byte order (word k = bytes 4k..4k+3,
// little-endian), i.e. exactly as they appear in a preimage.
enum : int {
  TXT_FLAGS = 0,        // bit0 parsed ok, bit1 witness serialisation
  TXT_INS = 1,          // first input
  TXT_NIN = 2,
  TXT_NOUT = 3,
  TXT_OUTS_FIRST = 4,   // first output (after the count varint)
  TXT_OUTS_END = 5,     // end of outputs = start of the witness section
  TXT_LOCK = 6,         // locktime
  TXT_START = 7,        // first byte of the tx (version)
  TXT_HP = 8,           // hashPrevouts
  TXT_HS = 16,          // hashSequence
  TXT_HO = 24,          // hashOutputs
  TXT_WORDS = 32,
};
constexpr uint32_t TXF_OK = 1u, TXF_WITNESS = 2u;
// which txs the index pass computes the BIP143 per-tx hashes for
enum : uint32_t { TX_HASHES_NONE = 0, TX_HASHES_ALL = 1, TX_HASHES_WITNESS = 2 };

// minimum waves per SIMD the ecmult kernel's register allocation targets
#ifndef HKV_ECMULT_WAVES
#define HKV_ECMULT_WAVES 4
#endif

}  // namespace hkv
