"""The chain-context rule of hkv_chain_context_device in Python big integers
(TEST INFRASTRUCTURE ONLY): what connectBlocks checks of a header against its
actual ancestors, written as the walk a host would do — a list of ancestors,
``sorted()`` for the median, ``//`` for the two divisions, a loop back over the
chain for the minimum-difficulty rule. The device runs the same rule as three
data-parallel launches (csrc/hkv_chainctx.hip); tests/chainctx_host.cpp runs
csrc/hkv_chainctx.h against the case files this module writes.

Readings taken without haskoin-core's source (it is a dependency of the
reference and not vendored with it). Each is Bitcoin's consensus rule as
Bitcoin Core implements it, and is what the tests pin:

* ``median_of_c_over_2`` — the median time past is element c // 2 of the c <= 11
  sorted ancestor times, also for c < 11 and for even c (GetMedianTimePast).
* ``time_strictly_above_mtp`` — a header needs time > mtp, not >=.
* ``future_limit_7200`` — time <= now + 2 h, with the caller's ``now``.
* ``retarget_uses_parent_and_period_first`` — the span is time(P) − time(block
  at H − interval): 2015 intervals, Bitcoin's off-by-one.
* ``clamp_before_multiply`` — the span is clamped to [T/4, 4T] (T // 4 in
  integers) and is a signed difference, so a negative span clamps to T/4.
* ``exact_product`` — target(P) * span is not truncated to 256 bits before the
  division (Bitcoin Core's arith_uint256 would wrap; the two differ only for
  targets above 2^254, which no retargeting network has).
* ``cap_then_compact`` — the result is capped at pow_limit, then encoded.
* ``magnitude_of_parent`` — a negative parent compact retargets by its
  magnitude; an overflowing one gives want = 0 and can never match.
* ``min_difficulty_gap_strict`` — the limit applies when time > time(P) +
  2 * spacing, strictly.
* ``min_difficulty_walk`` — otherwise the bits of the nearest ancestor (the
  parent included) that stands at a period start or has bits other than the
  limit's.
* ``version_signed`` — the version thresholds compare a signed 32-bit number
  (0x80000000 is below 2).
* ``work_of_invalid_compact_is_zero`` — negative, overflowing and zero compacts
  add no work; otherwise floor(2^256 / (target + 1)) (GetBlockProof).
* ``regtest_heights`` — btcRegTest: BIP34 at 100,000,000, BIP66 at 1,251, BIP65
  at 1,351, no retargeting, minimum difficulty allowed.
"""
from __future__ import annotations

import hashlib
import random
from types import SimpleNamespace
from typing import List, Optional, Sequence, Tuple

from header_oracle import decode_compact, encode_compact

READINGS = ("median_of_c_over_2", "time_strictly_above_mtp", "future_limit_7200",
            "retarget_uses_parent_and_period_first", "clamp_before_multiply", "exact_product", "cap_then_compact",
            "magnitude_of_parent", "min_difficulty_gap_strict", "min_difficulty_walk", "version_signed",
            "work_of_invalid_compact_is_zero", "regtest_heights")

TIME_OK, NOT_FUTURE, BITS_OK, VERSION_OK, CHECKPOINT_OK, ALL = 1, 2, 4, 8, 16, 31
NO_RETARGET, MIN_DIFFICULTY = 1, 2
POW_OK, LINK_OK = 1, 2
M256 = (1 << 256) - 1


def params(pow_limit=(1 << 224) - 1, interval=2016, target_timespan=1209600, min_diff_spacing=1200,
           bip34_height=227931, bip66_height=363725, bip65_height=388381, flags=0):
    return SimpleNamespace(pow_limit=pow_limit, interval=interval, target_timespan=target_timespan,
                           min_diff_spacing=min_diff_spacing, bip34_height=bip34_height, bip66_height=bip66_height,
                           bip65_height=bip65_height, flags=flags)


def tip(height, times, bits, period_first_time, period_real_bits, work):
    return SimpleNamespace(height=height, times=tuple(times), bits=bits, period_first_time=period_first_time,
                           period_real_bits=period_real_bits, work=work)


def make_header(version: int, time: int, bits: int, prev: bytes = bytes(32), merkle: bytes = bytes(32),
                nonce: int = 0) -> bytes:
    return (version.to_bytes(4, "little") + prev + merkle + time.to_bytes(4, "little") + bits.to_bytes(4, "little") +
            nonce.to_bytes(4, "little"))


def fields(h: bytes) -> Tuple[int, int, int]:
    return int.from_bytes(h[0:4], "little"), int.from_bytes(h[68:72], "little"), int.from_bytes(h[72:76], "little")


def header_work(bits: int) -> int:
    value, neg, over = decode_compact(bits)
    if neg or over or value == 0:
        return 0
    return (1 << 256) // (value + 1)


def retarget(p, parent_bits: int, parent_time: int, first_time: int) -> Tuple[int, bool]:
    """(want, overflow) at a period boundary."""
    value, _, over = decode_compact(parent_bits)
    if over:
        return 0, True
    span = max(p.target_timespan // 4, min(4 * p.target_timespan, parent_time - first_time))
    return encode_compact(min(p.pow_limit, value * span // p.target_timespan)), False


def connect(facts: Sequence[Tuple[int, int, int]], tp, p, now: int, checkpoints=(), hashes=None):
    """facts: (version, time, bits) per header. -> (mtp, want, work, flags) lists.
    The walk of a host: every header looks back over its actual ancestors."""
    limit_bits = encode_compact(p.pow_limit)
    cps = dict(checkpoints)
    n_prev = len(tp.times)
    # ancestors as (height, time, bits); the context's carry only their times, the tip its bits too
    anc = [(tp.height - (n_prev - 1 - j), t, None) for j, t in enumerate(tp.times)]
    anc[-1] = (tp.height, tp.times[-1], tp.bits)
    first_h = tp.height - tp.height % p.interval
    mtp, want, work, flags = [], [], [], []
    total = tp.work

    def real(k):  # the walk from ancestor k of anc back to a real-bits block
        while True:
            h, _, b = anc[k]
            if h <= tp.height and k < n_prev:      # reached the context: its answer is given
                return tp.period_real_bits
            if h % p.interval == 0 or b != limit_bits:
                return b
            k -= 1

    for i, (version, time, bits) in enumerate(facts):
        H = tp.height + 1 + i
        _, ptime, pbits = anc[-1]
        window = sorted(t for _, t, _ in anc[-11:])
        m = window[len(window) // 2]
        fl = 0
        if time > m:
            fl |= TIME_OK
        if time <= now + 7200:
            fl |= NOT_FUTURE
        over = False
        if H % p.interval:
            if p.flags & MIN_DIFFICULTY:
                w = limit_bits if time > ptime + p.min_diff_spacing else real(len(anc) - 1)
            else:
                w = pbits
        elif p.flags & NO_RETARGET:
            w = pbits
        else:
            fh = H - p.interval
            ftime = tp.period_first_time if fh <= tp.height else facts[fh - tp.height - 1][1]
            assert fh > tp.height or fh == first_h
            w, over = retarget(p, pbits, ptime, ftime)
        if bits == w and not over:
            fl |= BITS_OK
        v = version - (1 << 32) if version & 0x80000000 else version
        if not ((v < 2 and H >= p.bip34_height) or (v < 3 and H >= p.bip66_height) or (v < 4 and H >= p.bip65_height)):
            fl |= VERSION_OK
        if H not in cps or (hashes is not None and cps[H] == hashes[i]):
            fl |= CHECKPOINT_OK
        total = (total + header_work(bits)) & M256
        mtp.append(m), want.append(w), work.append(total), flags.append(fl)
        anc.append((H, time, bits))
    return mtp, want, work, flags


def first_bad(chain_flags, hdr_status) -> int:
    for i, (c, h) in enumerate(zip(chain_flags, hdr_status)):
        if c != ALL or h & (POW_OK | LINK_OK) != (POW_OK | LINK_OK):
            return i
    return len(chain_flags)


def advance(tp, facts, work, n, p):
    """The model's own tip after n headers (the checker of ChainTip.advance)."""
    if n == 0:
        return tp
    limit_bits = encode_compact(p.pow_limit)
    height = tp.height + n
    start = height - height % p.interval
    ft = facts[start - tp.height - 1][1] if start > tp.height else tp.period_first_time
    real = tp.period_real_bits
    for j in range(n):
        if (tp.height + 1 + j) % p.interval == 0 or facts[j][2] != limit_bits:
            real = facts[j][2]
    return tip(height, (tuple(tp.times) + tuple(f[1] for f in facts[:n]))[-11:], facts[n - 1][2], ft, real,
               work[n - 1])


# ---------------------------------------------------------------- generators

def random_chain(seed: int, n: int, tp, p, now: int, wrong: float = 0.03, head=()):
    """n (version, time, bits): a clock that advances by block-like steps, a few
    percent of the times at or below the median or in the future; bits mostly
    what the rule wants of the actual parent, a few percent wrong (the header
    after a wrong one goes back to the last good bits, so it is wrong too);
    a few percent of old versions. `now` should lie past the whole clock.
    `head`: directed first headers the random ones follow (the clock does not
    look at their times)."""
    rng = random.Random(seed)
    facts: List[Tuple[int, int, int]] = list(head)
    limit_bits = encode_compact(p.pow_limit)
    clock = tp.times[-1]
    good, repair = tp.bits, False
    for i in range(len(facts), n):
        H = tp.height + 1 + i
        clock += rng.choice([1, 60, 600, 600, 600, 1199, 1200, 1201, 2500])
        time = clock
        r = rng.random()
        if r < wrong:
            time = max(1, clock - rng.choice([3000, 6000, 20000]))
        elif r < 2 * wrong:
            time = now + rng.choice([7199, 7200, 7201, 100000])
        w = _want_one(facts, tp, p, H, time, limit_bits)
        bits = w
        r = rng.random()
        if repair:
            bits, repair = good, False
        elif r < wrong:
            good, repair = w, True
            bits = rng.choice([w ^ 1, limit_bits ^ 2, 0x1c05a3f4, 0x03800001, 0x22000100, 0])
        elif r < 2 * wrong and p.flags & MIN_DIFFICULTY:
            bits = limit_bits
        version = rng.choice([4, 0x20000000, 3, 2, 1, 0x80000001]) if rng.random() < 3 * wrong else 0x20000000
        facts.append((version, time & 0xFFFFFFFF, bits))
    return facts


def want_next(facts, tp, p, time):
    """want of a header of the given time that follows `facts`."""
    return _want_one(facts, tp, p, tp.height + 1 + len(facts), time, encode_compact(p.pow_limit))


def _want_one(facts, tp, p, H, time, limit_bits):
    """want of the next header after `facts` (the generator's incremental form)."""
    ptime, pbits = (facts[-1][1], facts[-1][2]) if facts else (tp.times[-1], tp.bits)
    if H % p.interval:
        if not p.flags & MIN_DIFFICULTY:
            return pbits
        if time > ptime + p.min_diff_spacing:
            return limit_bits
        for j in range(len(facts) - 1, -1, -1):
            if (tp.height + 1 + j) % p.interval == 0 or facts[j][2] != limit_bits:
                return facts[j][2]
        return tp.period_real_bits
    if p.flags & NO_RETARGET:
        return pbits
    fh = H - p.interval
    ftime = tp.period_first_time if fh <= tp.height else facts[fh - tp.height - 1][1]
    return retarget(p, pbits, ptime, ftime)[0]


def fake_hash(i: int, seed: int = 0) -> bytes:
    return hashlib.sha256(b"chainctx%d:%d" % (seed, i)).digest()


# ---------------------------------------------------------------- directed cases

VECTORS = [  # (first time, last time, old bits, expected bits): Bitcoin's published retarget vectors
    (1261130161, 1262152739, 0x1d00ffff, 0x1d00d86a),
    (1231006505, 1233061996, 0x1d00ffff, 0x1d00ffff),
    (1279008237, 1279297671, 0x1c05a3f4, 0x1c0168fd),
    (1263163443, 1269211443, 0x1c387f6f, 0x1d00e1fd),
]

WORK_COMPACTS = ([(s << 24) | m for s in range(1, 33) for m in (1, 0x7fffff)] +
                 [0x220000ff, 0x1d00ffff, 0x207fffff, 0x01010000, 0x01810000, 0x04923456, 0x22000100, 0x21010000,
                  0x23000001, 0xff123456, 0, 0x00123456, 0x01003456, 0x03000000])


def boundary_case(first_time, last_time, old_bits, p=None, height0=2016 * 16):
    """One header on a boundary, the period's first block in the context."""
    p = p or params()
    tp = tip(height0 - 1, [last_time], old_bits, first_time, old_bits, 12345)
    want = retarget(p, old_bits, last_time, first_time)[0]
    return p, tp, [(4, last_time + 600, want)]


def directed_cases():
    """[(name, params, tip, facts, now, checkpoints, hashes)]: the operands of the
    CPU case file, which the GPU test also sends through the device."""
    cases = []
    T = 1209600
    for k, (ft, lt, old, new) in enumerate(VECTORS):
        p, tp, f = boundary_case(ft, lt, old)
        assert f[0][2] == new
        cases.append(("vector%d" % k, p, tp, f, lt + 10000, (), None))
    base = 1300000000
    for name, ft, lt, old in [("clamp_low", base, base + T // 4 - 5, 0x1c05a3f4), ("clamp_low_edge", base, base + T // 4, 0x1c05a3f4),
                              ("clamp_high", base, base + 4 * T + 7, 0x1c05a3f4), ("clamp_high_edge", base, base + 4 * T, 0x1c05a3f4),
                              ("negative_span", base, base - 5000, 0x1c05a3f4),
                              ("above_limit", base, base + 4 * T, 0x1d00ffff),
                              ("above_limit_nine_limbs", base, base + 4 * T, 0x1d00ffff),
                              ("overflow_parent", base, base + T, 0x22000100),
                              ("negative_parent", base, base + T, 0x1c85a3f4),
                              ("zero_parent", base, base + T, 0x1c000000)]:
        p = params(pow_limit=(1 << 255) - 1) if name == "above_limit_nine_limbs" else params()
        old_bits = 0x207fffff if name == "above_limit_nine_limbs" else old
        p, tp, f = boundary_case(ft, lt, old_bits, p)
        # (the one header carries want; a second copy with other bits fails BITS_OK)
        cases.append((name, p, tp, f + [(4, f[0][1] + 600, f[0][2] ^ 0x100)], lt + 10000, (), None))
    # headerWork of every compact shape, and the sums' carries through all eight limbs
    for name, w0 in [("work_shapes", 5), ("work_carry_all_limbs", M256), ("work_carry_top", (1 << 255) + 7)]:
        p = params(pow_limit=(1 << 255) - 1, flags=NO_RETARGET)
        compacts = WORK_COMPACTS if name == "work_shapes" else \
            [0x207fffff, 0x01010000, 0x207fffff, 0x01010000, 0x1d00ffff, 0x01010000, 0x03000001, 0x01010000]
        tp = tip(99, [base], compacts[0], base - 100, compacts[0], w0)
        f = [(4, base + 600 * (j + 1), b) for j, b in enumerate(compacts)]
        cases.append((name, p, tp, f, base + 10**6, (), None))
    # median windows of 1..11 elements with ties
    for n_prev in range(1, 12):
        times = [base + [5, 5, 9, 1, 7, 7, 7, 3, 11, 2, 5][j] for j in range(n_prev)]
        tp = tip(500 + n_prev, times, 0x1d00ffff, base, 0x1d00ffff, 1)
        f = [(4, base + t, 0x1d00ffff) for t in [5, 6, 7, 8, 2, 7, 7, 12, 3, 9, 4, 10, 11, 12]]
        cases.append(("mtp_window_%d" % n_prev, params(), tp, f, base + 10**6, (), None))
    # the version thresholds at height - 1, height, height + 1
    p = params(bip34_height=1000, bip66_height=1003, bip65_height=1006)
    vers = [1, 2, 3, 4, 0x20000000, 0x80000000]
    for h0 in (999, 1002, 1005):
        tp = tip(h0 - 1, [base], 0x1d00ffff, base, 0x1d00ffff, 1)
        for v in vers:
            f = [(v, base + 600 * (j + 1), 0x1d00ffff) for j in range(3)]
            cases.append(("version_%x_at_%d" % (v, h0), p, tp, f, base + 10**6, (), None))
    # the minimum-difficulty rule
    pm = params(flags=MIN_DIFFICULTY, interval=2016)
    lim, real_b = 0x1d00ffff, 0x1c05a3f4
    def md(name, h0, ctx_real, rows):  # rows: (gap from the parent, bits)
        t, f = base, []
        for gap, b in rows:
            t += gap
            f.append((4, t, b))
        tp = tip(h0 - 1, [base], lim if ctx_real != "parent" else real_b, base - 100,
                 real_b if ctx_real == "parent" else ctx_real, 1)
        cases.append((name, pm, tp, f, base + 10**7, (), None))
    md("md_run_ends_at_non_limit", 5000, real_b, [(600, real_b), (1201, lim), (1201, lim), (600, real_b), (600, real_b)])
    md("md_run_ends_in_context", 5000, 0x1c0168fd, [(1201, lim), (1201, lim), (600, 0x1c0168fd), (1201, lim)])
    md("md_run_ends_at_period_start", 2016 * 3 - 2, real_b, [(600, real_b), (1201, lim), (600, lim), (1201, lim), (600, lim), (600, lim)])
    md("md_gap_exact", 5000, "parent", [(1200, real_b), (1200, lim), (1201, lim), (1200, real_b)])
    # checkpoints: a hit, a miss, heights outside the batch
    p = params()
    tp = tip(299, [base], 0x1d00ffff, base, 0x1d00ffff, 1)
    f = [(4, base + 600 * (j + 1), 0x1d00ffff) for j in range(8)]
    hs = [fake_hash(j) for j in range(8)]
    cps = ((10, fake_hash(99)), (300, hs[0]), (303, fake_hash(98)), (307, hs[7]), (308, hs[7]), (5000, hs[1]))
    cases.append(("checkpoints", p, tp, f, base + 10**6, cps, hs))
    # the future limit, around now + 7200
    f = [(4, base + d, 0x1d00ffff) for d in (7199, 7200, 7201, 7300)]
    cases.append(("future", p, tip(299, [base - 600], 0x1d00ffff, base, 0x1d00ffff, 1), f, base, (), None))
    f = [(4, 0xFFFFFFFF, 0x1d00ffff), (4, 0xFFFFFFFF, 0x1d00ffff)]
    cases.append(("future_64_bit", p, tip(299, [base], 0x1d00ffff, base, 0x1d00ffff, 1), f, (1 << 32) + 5, (), None))
    return cases


def long_min_difficulty_run(n=700, h0=2016 * 5 - 300):
    """A minimum-difficulty run longer than two tiles that starts in the context
    and crosses a period start (the GPU test's directed operand)."""
    pm = params(flags=MIN_DIFFICULTY)
    lim, real_b = 0x1d00ffff, 0x1c05a3f4
    base = 1400000000
    tp = tip(h0 - 1, [base], lim, base - 5000, real_b, 77)
    facts, t = [], base
    for i in range(n):
        H = h0 + i
        if i in (290, 610):
            t += 600
            prev_real = _want_one(facts, tp, pm, H, t, lim)
            facts.append((4, t, prev_real))          # the run's end: back to the real bits
        elif H % 2016 == 0:
            t += 600
            facts.append((4, t, _want_one(facts, tp, pm, H, t, lim)))
        else:
            t += 1201
            facts.append((4, t, lim))
    return pm, tp, facts, t + 100


# ---------------------------------------------------------------- the host program's case file

def emit_case(p, tp, facts, now, checkpoints=(), hashes=None) -> str:
    """A text case for tests/chainctx_host.cpp: the context, the headers' facts
    and hashes, and what the model expects."""
    mtp, want, work, flags = connect(facts, tp, p, now, checkpoints, hashes)
    hs = hashes if hashes is not None else [bytes(32)] * len(facts)

    def limbs(x):
        return " ".join("%x" % ((x >> (32 * j)) & 0xFFFFFFFF) for j in range(8))

    out = ["%x %x %s" % (tp.height + 1, len(tp.times), " ".join("%x" % t for t in tp.times)),
           "%x %x %x %x" % (tp.bits, tp.period_first_time, tp.period_real_bits, now),
           limbs(tp.work), limbs(p.pow_limit),
           "%x %x %x %x %x %x %x" % (p.interval, p.target_timespan, p.min_diff_spacing, p.bip34_height,
                                     p.bip66_height, p.bip65_height, p.flags),
           "%x %x" % (len(facts), len(checkpoints))]
    for h, x in checkpoints:
        out.append("%x %s" % (h, limbs(int.from_bytes(x, "little"))))
    for i, (v, t, b) in enumerate(facts):
        out.append("%x %x %x %s %x %x %x %s" % (v, t, b, limbs(int.from_bytes(hs[i], "little")), mtp[i], want[i],
                                                 flags[i], limbs(work[i])))
    return "\n".join(out) + "\n"
