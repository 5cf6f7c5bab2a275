"""CPU tests of what tests/test_gpu_chosen_scalars.py feeds the GPU: the
directed set S (tests/chosen_scalars.py) reaches every digit, top window and
sign of the recoding, and the table sweeps read the entries they name. All
from tests/recoding.py, the Python restatement of glv_split, write_qdigits
and write_gdigits."""
import random

import chosen_scalars as cs
import recoding as rc
import secp256k1_oracle as o


def test_directed_set_covers_the_q_recoding():
    """Every Booth digit a window can take occurs in every window 0..30 of
    each GLV half, every merged top digit up to the largest the split's
    parallelogram allows (10 for k1, 9 for k2: the halves are bounded by
    (|a1| + |a2|) / 2 and (|b1| + |b2|) / 2), both signs of each half, and
    never a top digit outside 0..16 (the chains' window-by-window fallback)."""
    _, _, u2, _, pin = cs.directed_set()
    pinned = [k for k, p in zip(u2, pin) if p != cs.PIN_U1]
    digits, tops, signs, fallback = cs.q_coverage(pinned)
    for h in range(2):
        for w in range(31):
            # window 0 has no carry in: nibble 7 plus a carry, the digit +8, needs a window below
            want = set(range(-8, 9)) - ({8} if w == 0 else set())
            assert digits[h][w] == want, (h, w, sorted(want - digits[h][w]))
    # m = (|k| + 2^123) >> 124: the bits from 124 up plus the Booth carry of bit 123
    top_max = [((abs(a) + abs(b)) // 2 + 2**123) >> 124 for a, b in ((o.A1, o.A2), (o.B1, o.B2))]
    assert top_max == [10, 9]
    assert tops[0] == set(range(11)) and tops[1] == set(range(10))
    assert not fallback
    assert signs == [{1, -1}, {1, -1}]


def test_directed_set_starts_the_chain_at_every_window():
    """One half zero and the other a single digit at window w: the chain's
    first addition (from infinity) falls in every window 0..31, for k1 and k2."""
    first = [set(), set()]
    for name, u2 in cs.u2_families():
        if not name.startswith("nibble_"):
            continue
        m1, _, m2, _ = rc.glv_split(u2)
        if m1 and m2:
            continue
        h = 0 if m1 else 1
        d = rc.q_digits(m1 or m2)
        nz = [w for w in range(rc.NWIN) if d[w]]
        if len(nz) == 1:
            first[h].add(nz[0])
    assert first[0] >= set(range(32)) and first[1] >= set(range(32)), first


def test_directed_set_covers_the_g_recoding():
    """G digits of magnitude 1 in all seven windows of both halves of u1, the
    digit -2^19 in windows 0..5 and +2^19 in windows 1..5 (+2^19 is the window
    value 2^19 - 1 plus a carry in, which window 0 cannot have; window 6
    holds 8 bits), the largest window-6 digit 256 in both halves, and u1_hi at
    its maximum."""
    _, u1, _, _, pin = cs.directed_set()
    seen = [[set() for _ in range(rc.GWIN)] for _ in range(2)]
    for k in (k for k, p in zip(u1, pin) if p != cs.PIN_U2):
        for h, d in enumerate(rc.g_digits(k)):
            for w in range(rc.GWIN):
                seen[h][w].add(d[w])
    for h in range(2):
        for w in range(rc.GWIN):
            assert {1, -1} & seen[h][w], (h, w)
            if w < 6:
                assert -2**19 in seen[h][w], (h, w)
            if 0 < w < 6:
                assert 2**19 in seen[h][w], (h, w)
        assert max(seen[h][6]) == 256
    assert any(k >> 128 == (o.N - 1) >> 128 for k in u1)


def test_window_six_reads_at_most_entry_256():
    """A half of u1 is below 2^128, so its top window (bits 120..127 and the
    Booth carry) is a digit 0..256: tables 12 and 13 are never read past entry
    256. Entry 256 itself needs a carry from below (the half >= 2^128 - 2^119),
    so it is no j 2^off: 256 2^120 = 2^128 is entry 1 of table 1. The sweeps
    of tables 12 and 13 reach it with the halves 2^128 - 1 and 2^128 - 2."""
    for v in range(512):  # the window sees bits 119..127
        for low in (0, 2**119 - 1):
            d = rc.booth(v << 119 | low, rc.GTAB_W, rc.GWIN)[6]
            assert d == (v + 1) >> 1 and 0 <= d <= 256
    assert rc.table_reads(256 << 120) == {1: 1}
    assert rc.table_reads(cs.ENTRY_256[12]) == {0: -1, 12: 256}
    assert rc.table_reads(cs.ENTRY_256[13]) == {1: -2, 13: 256} and cs.ENTRY_256[13] < o.N


def test_table_sweep_scalars_read_the_named_entry():
    """u1 = j 2^off reads entry j of table t and nothing else (at j = 2^19 the
    digit is -2^19 with a carry: entry 1 of table t + 2 as well); the negative
    form (2^20 - j) 2^off reads entry j negated and entry 1 of table t + 2."""
    rng = random.Random(0x5357)
    for t in range(14):
        off = rc.GTAB_W * (t // 2) + 128 * (t % 2)
        last = rc.GTAB_ENTRIES if t < 12 else 255
        for j in [1, 2, last - 1, last] + [rng.randrange(1, last) for _ in range(500)]:
            assert j << off < o.N
            want = {t: j} if j < rc.GTAB_ENTRIES else {t: -j, t + 2: 1}
            assert rc.table_reads(j << off) == want, (t, j)
            if t < 12 and j < rc.GTAB_ENTRIES:
                assert rc.table_reads((2**20 - j) << off) == {t: -j, t + 2: 1}, (t, j)
