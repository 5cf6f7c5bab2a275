"""GPU tests (MI355X) of the sum scans fe_mul_sum (a b + c d) and
fe_sqrmul_sum (a^2 + c d), of the complement negation fe_neg_compl, and of the
group formulas that use them, in the pattern of test_gpu_primitives.py: the
debug op on rows, against a limb model written here. The raw (weak-form) limbs
must match the model bit for bit and the normalised value the mathematical one.

The model follows the generated scan (tools/gen_mul_asm.py reduced_sum_scan)
column by column: with L the sum of the limb products of columns 0..7 (not
reduced mod 2^256) and H the sum of columns 8..14 (9 limbs, H < 2^257),
    o + T 2^256 = L + H C,      C = 2^32 + 977,
and fe_fold_top(o, T) follows (field_cases.fold_top). The square term's
columns are those of the doubled-operand lists (43 products), whose split
between L and H differs from the plain product's by the bits that the
doubling moves one limb up.

Lane i of ops 38 / 39 takes (a, b) from row i and its second term from row
(i + 1) mod n: a b + next a * next b, and a^2 + b * next a. The directed rows
are therefore built as chains: lane i's kind fixes one operand of row i + 1."""
import math
import random

import numpy as np
import pytest

import field_cases as fc
import secp256k1_oracle as o
from field_cases import C, M, N, P

pytestmark = pytest.mark.gpu

OP = dict(FE_MUL_SUM=38, FE_SQRMUL_SUM=39, FE_NEG_COMPL=40, FE_MUL_SUM_RA=41, FE_MUL_SUM_RD=42,
          FE_SQRMUL_SUM_RA=43, FE_SQRMUL_SUM_RD=44, FE_MUL_SUM_RB=45, GEJ_DOUBLE=64, GEJ_ACCUMULATE=66)
W32 = 2**32 - 1
# T is monotone in every limb, so its maximum is at all operands 2^256 - 1; the generated comment states
# T < 2^37 (L < (2^36 + 15) 2^256, H C < (2 C + 1) 2^256), fe_fold_top takes T < 2^40
T_BOUND = 2**37


# ---------------------------------------------------------------------------
# the limb model
# ---------------------------------------------------------------------------
def limbs(x):
    return [(x >> (32 * i)) & W32 for i in range(8)]


def mul_cols(a, b):
    a, b = limbs(a), limbs(b)
    return [[(a[i], b[k - i]) for i in range(8) if 0 <= k - i < 8] for k in range(15)]


def sqr_cols(a):
    """Row i multiplies a_i by a_i, e[i + 1] = a_{i+1} << 1 and d[j] = (a_j << 1) | (a_{j-1} >> 31), j = i + 2 .. 8."""
    a = limbs(a)
    e = [(x << 1) & W32 for x in a]
    d = [0, 0] + [((a[j] << 1) | (a[j - 1] >> 31)) & W32 for j in range(2, 8)] + [a[7] >> 31]
    cols = [[] for _ in range(16)]
    for i in range(8):
        cols[2 * i].append((a[i], a[i]))
        if i <= 6:
            cols[2 * i + 1].append((a[i], e[i + 1]))
        for j in range(i + 2, 9):
            cols[i + j].append((a[i], d[j]))
    assert not cols[15] and sum(map(len, cols)) == 43
    return cols[:15]


def sum_scan(cols1, cols2):
    """-> (o, T, h8) of the scan over the concatenated column lists"""
    L = sum(x * y << (32 * k) for k in range(8) for x, y in cols1[k] + cols2[k])
    H = sum(x * y << (32 * (k - 8)) for k in range(8, 15) for x, y in cols1[k] + cols2[k])
    assert H < 2**257
    v = L + H * C
    return v & (M - 1), v >> 256, H >> 256, L + (H << 256)


def fe_mul_sum(a, b, c, d):
    """-> (r, rare, wrap, h8, T)"""
    lo, T, h8, total = sum_scan(mul_cols(a, b), mul_cols(c, d))
    assert total == a * b + c * d and T < T_BOUND
    return fc.fold_top(lo, T) + (h8, T)


def fe_sqrmul_sum(a, c, d):
    lo, T, h8, total = sum_scan(sqr_cols(a), mul_cols(c, d))
    assert total == a * a + c * d and T < T_BOUND
    return fc.fold_top(lo, T) + (h8, T)


def lane_mul(rows, i):
    (a, b), (c, d) = rows[i], rows[(i + 1) % len(rows)]
    return (a, b, c, d), fe_mul_sum(a, b, c, d), (a * b + c * d) % P


def lane_sqrmul(rows, i):
    (a, b), (an, _) = rows[i], rows[(i + 1) % len(rows)]
    return (a, b, an), fe_sqrmul_sum(a, b, an), (a * a + b * an) % P


LANE = {"FE_MUL_SUM": lane_mul, "FE_SQRMUL_SUM": lane_sqrmul}


# ---------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def ver(torch):
    import hkv
    v = hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1))  # HKV_OPEN_NO_SELFCHECK
    yield v
    v.close()


@pytest.fixture(scope="module")
def dbg(torch, ver):
    def run(op, a_rows, b_rows):
        n = len(a_rows)
        assert n == len(b_rows) and n > 0
        a = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in a_rows), dtype=np.int32).reshape(n, 8)
        b = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in b_rows), dtype=np.int32).reshape(n, 8)
        da, db = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
        out = torch.zeros((n, 16), dtype=torch.int32, device="cuda")
        ver.debug_op(0, OP[op], n, da.data_ptr(), db.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        raw = out.cpu().numpy().view(np.uint32).tobytes()
        return [(int.from_bytes(raw[64 * i:64 * i + 32], "little"), int.from_bytes(raw[64 * i + 32:64 * i + 64], "little"))
                for i in range(n)]
    return run


def check_rows(dbg, op, rows, dev_op=None):
    """Every lane of the rows against the model; -> the model's flags per lane."""
    out = dbg(dev_op or op, [r[0] for r in rows], [r[1] for r in rows])
    flags = []
    for i, (raw, norm) in enumerate(out):
        ops, (r, rare, wrap, h8, T), value = LANE[op](rows, i)
        assert norm == value, (dev_op or op, i, [hex(x) for x in ops], hex(norm))
        assert raw == r, (dev_op or op, i, [hex(x) for x in ops], hex(raw))
        flags.append((rare, wrap, h8, T))
    return flags


def rand256(rng):
    return rng.randrange(M)


# ---------------------------------------------------------------------------
# broad operands: random tuples, boundary pairs, the ninth limb, aliasing
# ---------------------------------------------------------------------------
def edge_rows():
    E = fc.FE_EDGES
    pairs = [(a, b) for a in E for b in E]
    # a second order (a stride coprime to 100), so that each pair meets other neighbours as the second term
    return pairs + [pairs[(37 * i) % len(pairs)] for i in range(len(pairs))]


TURN_J = (0, 30, 33, 34, 35, 36, 37, 40)      # h[8] turns from 0 to 1 between 2^34 and 2^36 (the model says where)
TURN_K = (-2, 0, 2, 4, 6)                     # and between s and s + 4 * 2^32, s = isqrt(2^511)


def directed_rows(op):
    """Two rows per tuple — (a, b | c, d) for a b + c d, (a, b | c, .) for
    a^2 + b c; the odd lanes in between are checked too. -> (rows, tuples)"""
    rng = random.Random(0x5C4)
    r4 = [rand256(rng) for _ in range(4)]
    s = math.isqrt(2**511)
    tuples = [(M - 1, M - 1, M - 1, M - 1)]                       # h[8] = 1, the largest T
    tuples += [(M - 1, M - 1, M - 1, 2**j) if op == "FE_MUL_SUM" else (M - 1, M - 1, 2**j, 0) for j in TURN_J]
    tuples += [(s + k * 2**32,) * 4 for k in TURN_K]               # 2 s^2 around 2^512
    tuples += [(M - 1, M - 2, M - 2, M - 1), (M - 2, M - 2, M - 2, M - 2), (P, P, P, P), (P - 1, P - 1, P - 1, P - 1)]
    tuples += [(0, r4[1], r4[2], r4[3]), (r4[0], 0, r4[2], r4[3]), (r4[0], r4[1], 0, r4[3]), (r4[0], r4[1], r4[2], 0),
               (0, 0, r4[2], r4[3]), (r4[0], r4[1], 0, 0), (0, 0, 0, 0), (0, M - 1, M - 1, 0), (M - 1, 0, 0, M - 1)]
    rows = []
    for a, b, c, d in tuples:
        rows += [(a, b), (c, d)]
    return rows, len(tuples)


@pytest.mark.parametrize("op", ["FE_MUL_SUM", "FE_SQRMUL_SUM"])
def test_sum_scan_random_boundary_and_ninth_limb(dbg, op):
    """2,000 random tuples, every pair of the boundary values in both terms,
    zero operands in either term, and the ninth high limb: all operands
    2^256 - 1 (h[8] = 1, the largest T) and operands just below the turn."""
    rng = random.Random(OP[op])
    flags = check_rows(dbg, op, [(rand256(rng), rand256(rng)) for _ in range(2000)])
    assert sum(f[2] for f in flags) >= 100 and sum(not f[2] for f in flags) >= 100   # both values of h[8]
    check_rows(dbg, op, edge_rows())
    rows, nt = directed_rows(op)
    flags = check_rows(dbg, op, rows)[:2 * nt:2]      # the tuples' lanes
    top = flags[0]                                   # every limb of every operand all ones
    assert top[2] == 1 and top[3] == max(f[3] for f in flags) and top[3] < T_BOUND
    if op == "FE_MUL_SUM":
        assert top[3] == 2**36 + 2**33 + 1935        # the value the generator's comment states
    for turn in (flags[1:1 + len(TURN_J)], flags[1 + len(TURN_J):1 + len(TURN_J) + len(TURN_K)]):
        h8 = [f[2] for f in turn]
        assert h8[0] == 0 and h8[-1] == 1 and h8 == sorted(h8)


@pytest.mark.parametrize("op,alias", [("FE_MUL_SUM", "RA"), ("FE_MUL_SUM", "RB"), ("FE_MUL_SUM", "RD"),
                                      ("FE_SQRMUL_SUM", "RA"), ("FE_SQRMUL_SUM", "RD")])
def test_sum_scan_result_aliasing_an_operand(dbg, op, alias):
    """r aliasing a (the first operand), b (fe_mul_sum's second: the form
    gej_accumulate and gej_add_ge_core call) and d (the last, gej_double's):
    the same limbs as with a separate result, on random, boundary and
    directed rows."""
    rng = random.Random(OP[op] + 100)
    rows = [(rand256(rng), rand256(rng)) for _ in range(500)] + edge_rows() + directed_rows(op)[0]
    check_rows(dbg, op, rows, dev_op=f"{op}_{alias}")


# ---------------------------------------------------------------------------
# the directed rows (ninth limb, largest T, zero operands) in the lane layouts
# ---------------------------------------------------------------------------
def uniform_pairs():
    """Rows (x, y) that give a directed tuple in every lane when the whole
    wave holds the same row (lane i's second term is row i + 1): all ones
    (h[8] = 1, the largest T), 2 s^2 on either side of the turn of h[8], the
    values at and around p, and a zero operand in both terms."""
    rng = random.Random(0x5C5)
    s = math.isqrt(2**511)
    x = rand256(rng)
    return [(M - 1, M - 1)] + [(s + k * 2**32, s + k * 2**32) for k in TURN_K] + \
        [(M - 2, M - 1), (P, P), (P - 1, P - 1), (0, x), (x, 0), (0, 0)]


def place(op, tuples, lanes, waves, seed):
    """waves * 64 ordinary random rows with tuples[j] put at the global lanes
    `lanes[j]` (rows g and g + 1, cyclically): no two directed lanes adjacent."""
    rng = random.Random(seed)
    n = 64 * waves
    rows = [(rand256(rng), rand256(rng)) for _ in range(n)]
    taken = set()
    for (a, b, c, d), g in zip(tuples, lanes):
        assert not {g, (g + 1) % n} & taken
        taken |= {g, (g + 1) % n}
        rows[g], rows[(g + 1) % n] = (a, b), (c, d)
    return rows


def tuple_flags(op, t):
    return (fe_mul_sum(*t) if op == "FE_MUL_SUM" else fe_sqrmul_sum(t[0], t[1], t[2]))[3:]   # (h8, T)


@pytest.mark.parametrize("op", ["FE_MUL_SUM", "FE_SQRMUL_SUM"])
def test_sum_scan_directed_rows_in_lane_layouts(dbg, op):
    """The directed tuples of directed_rows — h[8] = 1 and just below, the
    largest T, zero operands — in the three lane layouts, each layout a
    launch of its own so that row i is lane i mod 64:
      every lane   whole waves of one uniform row (uniform_pairs);
      single       each tuple alone among ordinary lanes at lane 63, 32, 31
                   and 0 of four consecutive waves;
      alternating  a lane's second term is the next row's, so a directed lane's
                   neighbours share its rows: every fourth lane is directed
                   (rows g, g + 1), at offset 0 (even lanes) and 1 (odd lanes),
                   the lanes between are mixed or ordinary.
    The model confirms h[8] and T of every directed lane before the device
    runs."""
    # every lane
    seen = set()
    for x, y in uniform_pairs():
        want = tuple_flags(op, (x, y, x, y))
        flags = check_rows(dbg, op, [(x, y)] * 64)
        assert all(f[2:] == want for f in flags)
        seen.add(want[0])
    assert seen == {0, 1}
    allones = tuple_flags(op, (M - 1,) * 4)
    assert allones[0] == 1 and (op != "FE_MUL_SUM" or allones[1] == 2**36 + 2**33 + 1935)
    # single lanes
    rows, nt = directed_rows(op)
    tuples = [rows[2 * j] + rows[2 * j + 1] for j in range(nt)]
    lanes, tl = [], []
    for t in tuples:
        for lane in (63, 32, 31, 0):
            lanes.append(64 * len(lanes) + lane)
            tl.append(t)
    placed = place(op, tl, lanes, len(lanes), seed=0x51 + OP[op])
    flags = check_rows(dbg, op, placed)
    assert [g % 64 for g in lanes[:4]] == [63, 32, 31, 0]
    for t, g in zip(tl, lanes):
        assert flags[g][2:] == tuple_flags(op, t), (g, [hex(v) for v in t])
    # alternating lanes: offsets 0 and 1
    for off in (0, 1):
        lanes = list(range(off, 64 * 2, 4))
        tl = [tuples[j % nt] for j in range(len(lanes))]
        placed = place(op, tl, lanes, 2, seed=0xA1 + off + OP[op])
        flags = check_rows(dbg, op, placed)
        assert all(g % 2 == off for g in lanes)
        for t, g in zip(tl, lanes):
            assert flags[g][2:] == tuple_flags(op, t), (off, g)


# ---------------------------------------------------------------------------
# fe_fold_top's rare continuation and its wrap, in the three lane layouts
# ---------------------------------------------------------------------------
def sum_chain(op, kinds, seed):
    """Rows whose lane i is ordinary (None), rare (False) or rare with the
    second-level wrap (True): the sum's residue is chosen (field_cases.
    fold_residue) and row i + 1's free operand solved for it. The last lane's
    second term is row 0's, so it must be ordinary."""
    rng = random.Random(seed)
    n = len(kinds)
    assert kinds[-1] is None
    rows = [(rng.randrange(1, P), rng.randrange(1, P))]
    for i, kind in enumerate(kinds[:-1]):
        a, b = rows[i]
        for _ in range(fc.ATTEMPTS):
            if op == "FE_MUL_SUM":
                c = rng.randrange(1, P)
                d = rand256(rng) if kind is None else (fc.fold_residue(rng, kind) - a * b) * pow(c, -1, P) % P
                flags = fe_mul_sum(a, b, c, d)
            else:   # a^2 + b c: the next row's a is solved, its b is free
                d = rng.randrange(1, P)
                c = rng.randrange(1, M) if kind is None else (fc.fold_residue(rng, kind) - a * a) * pow(b, -1, P) % P
                flags = fe_sqrmul_sum(a, b, c) if c else (0, None, None)
            if (kind is None and flags[1] is False) or (kind is not None and flags[1] and flags[2] == kind):
                break
        else:
            raise fc.QuotaError(f"{op}: lane {i} ({kind}) not built in {fc.ATTEMPTS} attempts")
        rows.append((c, d))
    assert LANE[op](rows, n - 1)[1][1] is False   # the last lane (second term: row 0) is ordinary
    return rows


def layout_kinds():
    kinds = [False] * 64 + [True] * 64                       # every lane rare, every lane wrapping
    for lane in (0, 31, 32, 63):                             # one rare lane, its wrap variant one lane on
        w = [None] * 64
        w[lane], w[(lane + 1) % 64] = False, True
        kinds += w
    kinds += [False, None, True, None] * 16 + [None, True, None, False] * 16   # alternating lanes
    return kinds + [None] * 64


@pytest.mark.parametrize("op", ["FE_MUL_SUM", "FE_SQRMUL_SUM"])
def test_sum_scan_rare_top_fold_layouts(dbg, op):
    """Operands that take fe_fold_top_rare and its second-level wrap: whole
    waves of each, one lane at 0 / 31 / 32 / 63 among ordinary ones, and
    alternating lanes; the layout is checked against the model first."""
    kinds = layout_kinds()
    rows = sum_chain(op, kinds, seed=0x5C0 + OP[op])
    flags = check_rows(dbg, op, rows)
    for i, kind in enumerate(kinds):
        assert (flags[i][0], flags[i][1]) == ((False, False) if kind is None else (True, kind)), (i, kind)
    assert sum(f[0] and not f[1] for f in flags) >= 64 + 4 + 32 and sum(f[1] for f in flags) >= 64 + 4 + 32


# ---------------------------------------------------------------------------
# the complement negation
# ---------------------------------------------------------------------------
def check_neg(dbg, cases, model):
    out = dbg("FE_NEG_COMPL", [c[0] for c in cases], [0] * len(cases))
    for (a,), (raw, norm) in zip(cases, out):
        assert norm == -a % P, hex(a)
        assert raw == model(a)[0], hex(a)


def test_fe_neg_compl_layouts(dbg):
    """fe_neg_compl = fe_cneg's negating arm: the boundary values and 2,000
    random ones; then the values whose borrow runs past limb 1 and past limb 7
    (a > p), and the boundary values, in the three lane layouts — each layout
    a launch of its own, so that row i is lane i mod 64, and the model
    confirms which lanes are rare before the device runs."""
    rng = random.Random(40)
    model = lambda a: fc.fe_cneg(a, 1)  # noqa: E731
    check_neg(dbg, [(a,) for a in fc.FE_EDGES] + [(rand256(rng),) for _ in range(2000)], model)
    rare = [(c[0],) for c in fc.cneg_cases(False, seed=0xC4EA)]
    wrapc = [(c[0],) for c in fc.cneg_cases(True, seed=0xC4EA)]
    lay = fc.layouts(rare, wrapc, fc.ordinary(model, lambda r: (rand256(r),), 64, seed=40))
    f = {name: [model(*c)[1:] for c in rows] for name, rows in lay.items()}
    # all: a wave of rare lanes without the wrap, then a wave of wrapping lanes
    assert len(lay["all"]) == 128 and all(x == (True, False) for x in f["all"][:64])
    assert all(x == (True, True) for x in f["all"][64:])
    # single: wave j has its rare lane at 0 / 31 / 32 / 63, the wrap variant one lane on, nothing else
    assert len(lay["single"]) == 256
    for j, lane in enumerate((0, 31, 32, 63)):
        w = f["single"][64 * j:64 * j + 64]
        assert {i for i in range(64) if w[i][0]} == {lane, (lane + 1) % 64}
        assert w[lane] == (True, False) and w[(lane + 1) % 64] == (True, True)
    # alt: the even lanes of the first wave, the odd lanes of the second, rare and wrapping in turn
    assert len(lay["alt"]) == 128
    for par in (0, 1):
        w = f["alt"][64 * par:64 * par + 64]
        assert {i for i in range(64) if w[i][0]} == set(range(par, 64, 2))
        assert [w[i][1] for i in range(par, 64, 2)] == [bool(k % 2) for k in range(32)]
    for name in ("all", "single", "alt"):
        check_neg(dbg, lay[name], model)
    # the boundary values: every lane, one lane at 0 / 31 / 32 / 63 among ordinary ones, alternating lanes
    plain = fc.ordinary(model, lambda r: (rand256(r),), 64, seed=41)
    E = fc.FE_EDGES
    check_neg(dbg, [(E[i % len(E)],) for i in range(64)], model)
    single = []
    for e in E:
        for lane in (0, 31, 32, 63):
            w = list(plain)
            w[lane] = (e,)
            single += w
    assert all(single[64 * k + (0, 31, 32, 63)[k % 4]] == (E[k // 4],) for k in range(4 * len(E)))
    check_neg(dbg, single, model)
    for par in (0, 1):
        check_neg(dbg, [(E[i // 2 % len(E)],) if i % 2 == par else plain[i] for i in range(64)], model)


# ---------------------------------------------------------------------------
# the formulas: a chain of doublings and an addition
# ---------------------------------------------------------------------------
def test_doubling_and_addition_chain_keeps_the_sign(dbg):
    """64 lanes through 8 doublings, an addition and 4 doublings, one debug
    call per step chained from here: each call rebuilds the running point
    from its scalar (ecmult_simple, itself a chain of these doublings and
    additions), lifts it to a new Z != 1 and applies the step; one lane has
    T == acc at the addition. Every step against the oracle's affine
    arithmetic, y included: a Y of the wrong sign at any step fails here."""
    rng = random.Random(0x64)
    lanes = 64
    k = [rng.randrange(1, N) for _ in range(lanes)]
    k2 = [rng.randrange(1, N) for _ in range(lanes)]
    same = 37
    k2[same] = k[same] * 2**8 % N                     # T == acc after the 8 doublings
    pts = [o.point_mul(x, o.G) for x in k]
    add = [o.point_mul(x, o.G) for x in k2]

    def step(op, second):
        a_rows, b_rows = [], []
        for i in range(lanes):
            z1 = rng.choice([2, P - 1, P + 5, rng.randrange(2, P), rng.randrange(2, P)])
            a_rows += [k[i], z1]
            b_rows += [second[i], (rng.randrange(1, 2**253) << 3) | 1]   # take
        out = dbg(op, a_rows, b_rows)
        return [None if out[2 * i + 1][0] else out[2 * i] for i in range(lanes)]

    def doubling():
        got = step("GEJ_DOUBLE", [1] * lanes)
        for i in range(lanes):
            pts[i] = o.point_add(pts[i], pts[i])
            k[i] = 2 * k[i] % N
        assert got == pts

    for _ in range(8):
        doubling()
    got = step("GEJ_ACCUMULATE", k2)
    for i in range(lanes):
        pts[i] = o.point_add(pts[i], add[i])
        k[i] = (k[i] + k2[i]) % N
    assert add[same] == o.point_mul(k2[same], o.G) and got == pts
    for _ in range(4):
        doubling()
    assert pts[5] == o.point_mul(k[5], o.G)
