"""GPU tests (MI355X) of the field, scalar and group primitives underneath the
verifier, one debug op per function (hkv_internal.h), against Python integers
and the oracle's affine point arithmetic.

Every field op runs on ~2,000 random operand tuples, on every pair of boundary
values, and on the directed sets of field_cases.py — the operands that take
the fold's rare continuation (fe_fold_carry_rare, fe_fold_borrow_rare,
fe_fold_top_rare, fe_lin2's two arms, fe_fold_top2's c1 | c2 arm) and the
second-level wrap inside it — in three lane layouts: every lane of the wave
rare, one rare lane among ordinary ones at lanes 0 / 31 / 32 / 63, and
alternating lanes. The raw (weak-form) result must equal the CPU model's limb
result bit for bit and the normalised one the mathematical value."""
import random

import numpy as np
import pytest

import field_cases as fc
import secp256k1_oracle as o
from field_cases import C, M, N, P
from test_safegcd import EDGE_FIELD, EDGE_SCALARS

pytestmark = pytest.mark.gpu

OP = dict(FE_MUL=1, FE_SQR=2, FE_ADD=3, FE_SUB=4, SC_MUL=7, SC_INV=8, FE_CNEG=13, FE_CNEG_MASK=14, FE_NEG=15,
          FE_HALF=16, FE_SHL=17, FE_SHL_VAR=18, FE_MUL_SMALL=19, FE_MUL_SMALL2=20, FE_LIN2=21, FE_MUL_ADD=22,
          FE_MUL2=23, FE_SQR2=24, FE_SQRMUL=25, FE_MUL_REF=26, FE_SQR_REF=27, FE_NORMALIZE=28, FE_IS_ZERO=29,
          FE_EQUAL=30, U256_LT_P=31, SC_ADD=32, SC_SUB=33, SC_NEG=34, SC_SQR=35, SC_IS_HIGH=36, INV_MOD_P=37,
          GEJ_DOUBLE=64, GEJ_DOUBLE_ILP=65, GEJ_ACCUMULATE=66, GEJ_ACCUMULATE_ILP=67, GEJ_ADD_VAR=68,
          GEJ_ADD_AFFINE_COMPLETE=69, X_MATCHES_R=70, ECMULT=71)
NORM_FIRST = {"FE_MUL", "FE_SQR", "FE_ADD", "FE_SUB"}  # ops 1..4: normalised | raw; the others raw | normalised


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
        """op on rows of 256-bit integers -> one Python integer per 8-word half of each out row"""
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


def rand256(rng):
    return rng.randrange(M)


# ---------------------------------------------------------------------------
# field ops of one lane: (a) or (a, third operand in b)
# ---------------------------------------------------------------------------
def _pairs(rng, second):
    return [(a, b) for a in fc.FE_EDGES for b in fc.FE_EDGES] + [(rand256(rng), second(rng)) for _ in range(2000)]


def _with(rng, params, extra):
    return [(a, k) for a in fc.FE_EDGES for k in params] + [(rand256(rng), extra(rng)) for _ in range(2000)]


def _unary(rng):
    return [(a,) for a in fc.FE_EDGES] + [(rand256(rng),) for _ in range(2000)]


FIELD_OPS = {
    # op: (model, mathematical value, broad operands, directed(wrap) -> cases, an ordinary-lane maker)
    "FE_ADD": (fc.fe_add, lambda a, b: a + b, lambda r: _pairs(r, rand256), fc.add_cases,
               lambda r: (rand256(r), rand256(r))),
    "FE_SUB": (fc.fe_sub, lambda a, b: a - b, lambda r: _pairs(r, rand256), fc.sub_cases,
               lambda r: (rand256(r), rand256(r))),
    "FE_NEG": (fc.fe_neg, lambda a: -a, _unary, fc.neg_cases, lambda r: (rand256(r),)),
    "FE_CNEG": (fc.fe_cneg, lambda a, f: -a if f else a, lambda r: _with(r, [0, 1], lambda q: q.randrange(2)),
                fc.cneg_cases, lambda r: (rand256(r), r.randrange(2))),
    "FE_CNEG_MASK": (fc.fe_cneg, lambda a, f: -a if f else a,
                     lambda r: _with(r, [0, 1], lambda q: q.randrange(2)),
                     lambda wrap: fc.cneg_cases(wrap, seed=0xC4E8), lambda r: (rand256(r), r.randrange(2))),
    "FE_MUL": (fc.fe_mul, lambda a, b: a * b, lambda r: _pairs(r, rand256), fc.mul_cases,
               lambda r: (rand256(r), rand256(r))),
    "FE_MUL_REF": (fc.fe_mul_ref, lambda a, b: a * b, lambda r: _pairs(r, rand256),
                   lambda wrap: fc.mul_cases(wrap, model=fc.fe_mul_ref), lambda r: (rand256(r), rand256(r))),
    "FE_SQR": (fc.fe_sqr, lambda a: a * a, _unary, fc.sqr_cases, lambda r: (rand256(r),)),
    "FE_SQR_REF": (fc.fe_sqr_ref, lambda a: a * a, _unary, lambda wrap: fc.sqr_cases(wrap, model=fc.fe_sqr_ref),
                   lambda r: (rand256(r),)),
    "FE_MUL_SMALL": (fc.fe_mul_small, lambda a, k: a * k,
                     lambda r: _with(r, [0, 1, 2, 3, 255, 65535], lambda q: q.randrange(2**16)),
                     fc.mul_small_cases, lambda r: (rand256(r), r.randrange(2**16))),
    "FE_SHL": (fc.fe_shl, lambda a, s: a << s, lambda r: _with(r, [1, 2, 3, 16, 31], lambda q: q.randrange(1, 32)),
               lambda wrap: fc.shl_cases(wrap, shifts=(1, 1, 3, 31)), lambda r: (rand256(r), r.choice([1, 1, 3, 7]))),
    "FE_SHL_VAR": (fc.fe_shl, lambda a, s: a << s,
                   lambda r: _with(r, [1, 2, 3, 16, 31], lambda q: q.randrange(1, 32)), fc.shl_cases,
                   lambda r: (rand256(r), r.randrange(1, 32))),
}


def check_field(dbg, op, cases, model, math):
    a_rows = [c[0] for c in cases]
    b_rows = [c[1] if len(c) > 1 else 0 for c in cases]
    out = dbg(op, a_rows, b_rows)
    for c, (w0, w1) in zip(cases, out):
        raw, norm = (w1, w0) if op in NORM_FIRST else (w0, w1)
        assert norm == math(*c) % P, (op, [hex(x) for x in c], hex(norm))
        assert raw == model(*c)[0], (op, [hex(x) for x in c], hex(raw))
    return out


@pytest.mark.parametrize("op", sorted(FIELD_OPS))
def test_field_op_random_and_boundary_pairs(dbg, op):
    """fe_add, fe_sub, fe_neg, fe_cneg, fe_cneg_mask, fe_mul, fe_mul_ref,
    fe_sqr, fe_sqr_ref, fe_mul_small, fe_shl, fe_shl_var: 2,000 random tuples
    and every pairwise combination of the boundary values."""
    model, math, broad, _, _ = FIELD_OPS[op]
    check_field(dbg, op, broad(random.Random(OP[op])), model, math)


@pytest.mark.parametrize("op", sorted(FIELD_OPS))
def test_field_op_rare_branch_layouts(dbg, op):
    """The directed sets (rare continuation and its second-level wrap) of each
    op in the three lane layouts; the layout is checked against the model
    before the device runs it."""
    model, math, _, directed, plain = FIELD_OPS[op]
    rare, wrapc = directed(False), directed(True)
    lay = fc.layouts(rare, wrapc, fc.ordinary(model, plain, 64, seed=OP[op]))
    for name, cases in lay.items():
        flags = [model(*c)[1:] for c in cases]
        assert sum(bool(f[0]) for f in flags) >= {"all": 128, "single": 8, "alt": 64}[name]
        assert any(f[1] for f in flags) and any(f[0] and not f[1] for f in flags)
        check_field(dbg, op, cases, model, math)


def test_fe_half_carry_into_bit_256(dbg):
    """fe_half: random and boundary values, and the odd a with a + p >= 2^256
    (the carry becomes the top bit) in the three layouts."""
    rng = random.Random(16)
    model = lambda a: (fc.fe_half(a)[0], fc.fe_half(a)[1], False)  # noqa: E731
    half = lambda a: a * pow(2, -1, P)  # noqa: E731
    check_field(dbg, "FE_HALF", _unary(rng), model, half)
    cases = fc.half_cases()
    plain = fc.ordinary(model, lambda r: (rand256(r),), 64)
    for name, rows in fc.layouts(cases, cases[::-1], plain).items():
        check_field(dbg, "FE_HALF", rows, model, half)


def test_fe_mul_and_fe_sqr_equal_their_ref_forms(dbg):
    """fe_mul against fe_mul_ref and fe_sqr against fe_sqr_ref (the form kept
    as the reference), raw and normalised, on the random, boundary and
    directed operands above, the three lane layouts included."""
    rng = random.Random(26)
    muls = _pairs(rng, rand256) + fc.mul_cases(False) + fc.mul_cases(True)
    for name, rows in fc.layouts(fc.mul_cases(False), fc.mul_cases(True),
                                 fc.ordinary(fc.fe_mul, lambda r: (rand256(r), rand256(r)), 64)).items():
        muls += rows
    got = dbg("FE_MUL", [c[0] for c in muls], [c[1] for c in muls])
    ref = dbg("FE_MUL_REF", [c[0] for c in muls], [c[1] for c in muls])
    assert [(n, r) for n, r in got] == [(n, r) for r, n in ref]
    sqrs = _unary(rng) + fc.sqr_cases(False) + fc.sqr_cases(True)
    for name, rows in fc.layouts(fc.sqr_cases(False), fc.sqr_cases(True),
                                 fc.ordinary(fc.fe_sqr, lambda r: (rand256(r),), 64)).items():
        sqrs += rows
    got = dbg("FE_SQR", [c[0] for c in sqrs], [0] * len(sqrs))
    ref = dbg("FE_SQR_REF", [c[0] for c in sqrs], [0] * len(sqrs))
    assert [(n, r) for n, r in got] == [(n, r) for r, n in ref]
    assert all(n == c[0] * c[0] % P for c, (n, _) in zip(sqrs, got))


# ---------------------------------------------------------------------------
# ops whose third operand is the next row
# ---------------------------------------------------------------------------
def test_fe_mul_add_rare_top_fold(dbg):
    """fe_mul_add(a, b, e) with e = the next lane's a: random lanes, then whole
    waves of rare lanes, of wrapping lanes, single rare lanes at 0 / 31 / 32 /
    63 beside their wrap variant, and alternating lanes."""
    kinds = [None] * 1024 + [False] * 64 + [True] * 64
    for lane in (0, 31, 32, 63):
        w = [None] * 64
        w[lane], w[(lane + 1) % 64] = False, True
        kinds += w
    kinds += [False, None, True, None] * 16 + [None, True, None, False] * 16 + [None] * 64
    rows = fc.mul_add_chain(kinds)
    edges = [(a, b, 0) for a in fc.FE_EDGES for b in fc.FE_EDGES]
    # boundary values: a, b, e all from the list (e is the next row's a)
    a_rows = [r[0] for r in rows] + [a for a, _, _ in edges]
    b_rows = [r[1] for r in rows] + [b for _, b, _ in edges]
    n = len(a_rows)
    out = dbg("FE_MUL_ADD", a_rows, b_rows)
    taken = [0, 0]
    for i, (raw, norm) in enumerate(out):
        a, b, e = a_rows[i], b_rows[i], a_rows[(i + 1) % n]
        r, rare, wrap = fc.fe_mul_add(a, b, e)
        taken[0] += rare and not wrap
        taken[1] += wrap
        assert norm == (a * b + e) % P and raw == r, (i, hex(a), hex(b), hex(e))
    assert taken[0] >= 64 + 4 + 32 and taken[1] >= 64 + 4 + 32


LIN2_CARRY = [(9, 8), (36, 27), (2, 0), (255, 255), (255, 0), (27, 36), (8, 9)]
LIN2_BORROW = [(9, 8), (36, 27), (255, 255), (27, 36), (8, 9)]


def _lin2_plan(rng, kind):
    """kind: None, or (arm, wrap) -> a plan entry with ka > 0"""
    if kind is None:
        return None
    ka, kb = rng.choice(LIN2_CARRY if kind[0] == "carry" else LIN2_BORROW)
    return (ka, kb, kind[0], kind[1])


def test_fe_lin2_both_rare_arms(dbg):
    """fe_lin2 (ka a - kb b, per-lane ka, kb): random lanes, the callers'
    constants, and the carry and borrow arms with and without their wraps:
    whole waves of each, one rare lane at 0 / 31 / 32 / 63 beside its wrap
    variant, alternating lanes, and the ka = 0 / kb = 0 extremes."""
    rng = random.Random(21)
    arms = [("carry", False), ("carry", True), ("borrow", False), ("borrow", True)]
    plan = [None] * 1024
    for kind in arms:
        plan += [_lin2_plan(rng, kind) for _ in range(64)]
    for j, lane in enumerate((0, 31, 32, 63)):
        for arm in ("carry", "borrow"):
            w = [None] * 64
            w[lane], w[(lane + 1) % 64] = _lin2_plan(rng, (arm, False)), _lin2_plan(rng, (arm, True))
            plan += w
    plan += [_lin2_plan(rng, arms[i % 4]) if i % 2 == 0 else None for i in range(128)]
    plan += [_lin2_plan(rng, arms[i % 4]) if i % 2 == 1 else None for i in range(128)]
    # ka = 0 lanes (quad_double's -8C lane, and 255) cannot have b forced: an ordinary lane carries their constants
    for i in range(64):
        plan += [None, (0, 8 if i % 2 else 255, "borrow", i % 4 >= 2)]
    rows = fc.lin2_rows(plan)
    out = dbg("FE_LIN2", [r[0] for r in rows], [r[2] for r in rows])
    taken = {}
    for i, ((a, ka, b, kb), (raw, norm)) in enumerate(zip(rows, out)):
        r, arm, wrap = fc.fe_lin2(a, ka, b, kb)
        taken[(arm, wrap)] = taken.get((arm, wrap), 0) + 1
        assert norm == (ka * a - kb * b) % P and raw == r, (i, hex(a), ka, hex(b), kb)
    assert all(taken.get(k, 0) >= 64 for k in arms), taken
    # boundary values with the callers' constants: rows alternate so that every b carries (ka, kb)
    edge_rows, consts = [], fc.LIN2_K
    for j, (ka, kb) in enumerate(consts):
        for a in fc.FE_EDGES:
            for b in fc.FE_EDGES:
                edge_rows.append((a, (b & ~0xFFFF) | ka | (kb << 8)))
    out = dbg("FE_LIN2", [r[0] for r in edge_rows], [r[1] for r in edge_rows])
    n = len(edge_rows)
    for i, (raw, norm) in enumerate(out):
        (a, b), nb = edge_rows[i], edge_rows[(i + 1) % n][1]
        ka, kb = nb & 0xFF, (nb >> 8) & 0xFF
        assert norm == (ka * a - kb * b) % P and raw == fc.fe_lin2(a, ka, b, kb)[0], (i, hex(a), ka, hex(b), kb)


def _kinds(n, seed):
    """A row sequence over {None, False, True} (ordinary, rare, rare + wrap)
    in which every ordered pair of kinds is adjacent: lane i's first product
    is row i's, its second row i + 1's, so the rare case sits in the first
    product only, the second only and both, in the same and in different lanes."""
    rng = random.Random(seed)
    ks = [None, False, True]
    seq = [x for a in ks for b in ks for x in (a, b)]
    seq += [rng.choice(ks) for _ in range(n - len(seq) - 128)] + [False] * 64 + [True] * 64
    assert {(seq[i], seq[i + 1]) for i in range(len(seq) - 1)} == {(a, b) for a in ks for b in ks}
    return seq


def _pick(kind, rare, wrapc, plain, i):
    src = plain if kind is None else (wrapc if kind else rare)
    return src[i % len(src)]


def test_fe_mul2_rare_fold_in_either_product(dbg):
    """fe_mul2 (fe_fold_top2's c1 | c2 arm): the rare product first, second
    and both; whole waves of rare and of wrapping lanes."""
    kinds = _kinds(1024, 23)
    rare, wrapc = fc.mul_cases(False, seed=0x3B5), fc.mul_cases(True, seed=0x3B5)
    plain = fc.ordinary(fc.fe_mul, lambda r: (rand256(r), rand256(r)), 256, seed=23)
    rows = [_pick(k, rare, wrapc, plain, i) for i, k in enumerate(kinds)]
    rows += _pairs(random.Random(0x23), rand256)   # every boundary pair, 2,000 random lanes
    out = dbg("FE_MUL2", [r[0] for r in rows], [r[1] for r in rows])
    n = len(rows)
    for i, (r1, r2) in enumerate(out):
        (a, b), (c, d) = rows[i], rows[(i + 1) % n]
        assert r1 == a * b % P and r2 == c * d % P, (i, hex(a), hex(b), hex(c), hex(d))


def test_fe_sqr2_rare_fold_in_either_square(dbg):
    """fe_sqr2 (a^2, b^2) with each square ordinary, rare or wrapping."""
    rare, wrapc = fc.sqr_cases(False, seed=0x5C9), fc.sqr_cases(True, seed=0x5C9)
    plain = fc.ordinary(fc.fe_sqr, lambda r: (rand256(r),), 256, seed=24)
    ks = [None, False, True]
    rows = []
    for i in range(1152):
        k1, k2 = ks[i % 3], ks[(i // 3) % 3]
        if i >= 1024:
            k1, k2 = (i % 2 == 0), (i % 4 < 2)   # two waves with both squares rare in every lane
        rows.append((_pick(k1, rare, wrapc, plain, i)[0], _pick(k2, rare, wrapc, plain, i // 3 + 7)[0]))
    rows += _pairs(random.Random(0x24), rand256)   # every boundary pair, 2,000 random lanes
    out = dbg("FE_SQR2", [r[0] for r in rows], [r[1] for r in rows])
    for (a, b), (r1, r2) in zip(rows, out):
        assert r1 == a * a % P and r2 == b * b % P, (hex(a), hex(b))


def test_fe_sqrmul_rare_fold_in_square_or_product(dbg):
    """fe_sqrmul (a^2, b * next a): the square's kind follows the row, the
    product's is built on the next row's a. Then 2,000 random lanes, and the
    boundary values: every one squared, and every ordered pair of them as the
    product's (b, next a) — weak-form operands at and above p and the
    all-ones operand included, as gej_accumulate_ilp can pass them."""
    kinds = _kinds(1024, 25)
    rng = random.Random(25)
    rare, wrapc = fc.sqr_cases(False, seed=0x5CA), fc.sqr_cases(True, seed=0x5CA)
    plain = fc.ordinary(fc.fe_sqr, lambda r: (r.randrange(1, P),), 256, seed=25)
    a_rows = [_pick(k, rare, wrapc, plain, i)[0] for i, k in enumerate(kinds)]
    nd = len(a_rows)
    a_rows += [rand256(rng) or 1 for _ in range(2000)]
    tail_b = [rand256(rng) for _ in range(2000)]
    E = fc.FE_EDGES
    for j, (b, an) in enumerate((b, an) for b in E for an in E):
        # two rows per pair: (a = any boundary value, b), then (a = an, b = any boundary value)
        a_rows += [E[j % len(E)], an]
        tail_b += [b, E[(j // len(E) + 3) % len(E)]]
    n = len(a_rows)
    b_rows, pk = [], kinds[7:] + kinds[:7]   # the product's kinds: the same sequence, shifted
    for i in range(nd):
        nxt = a_rows[i + 1]
        for _ in range(fc.ATTEMPTS):
            b = rand256(rng) if pk[i] is None else fc.fold_residue(rng, pk[i]) * pow(nxt, -1, P) % P
            _, r, w = fc.fe_mul(b, nxt)
            if (pk[i] is None and not r) or (pk[i] is not None and r and w == pk[i]):
                break
        else:
            raise fc.QuotaError(f"fe_sqrmul row {i}")
        b_rows.append(b)
    b_rows += tail_b
    assert len(b_rows) == n
    combos = {(fc.fe_sqr(a_rows[i])[1:], fc.fe_mul(b_rows[i], a_rows[i + 1])[1:]) for i in range(nd)}
    assert len(combos) == 9
    assert {(b_rows[i], a_rows[(i + 1) % n]) for i in range(n)} >= {(b, an) for b in E for an in E}
    assert set(a_rows) >= set(E) and set(b_rows) >= set(E)
    out = dbg("FE_SQRMUL", a_rows, b_rows)
    for i, (r1, r2) in enumerate(out):
        assert r1 == a_rows[i] ** 2 % P and r2 == b_rows[i] * a_rows[(i + 1) % n] % P, i


def test_fe_mul_small2_rare_fold_in_either_multiple(dbg):
    """fe_mul_small2 (a k1, next a * k2), k <= 2^8."""
    kinds = _kinds(1024, 20)
    rare = fc.mul_small_cases(False, kmax=2**8 + 1, seed=0x5A15)
    wrapc = fc.mul_small_cases(True, kmax=2**8 + 1, seed=0x5A15)
    plain = fc.ordinary(fc.fe_mul_small, lambda r: (rand256(r), r.randrange(257)), 256, seed=20)
    rows = [_pick(k, rare, wrapc, plain, i) for i, k in enumerate(kinds)]
    rows += _with(random.Random(0x20), (0, 1, 3, 256), lambda r: r.randrange(257))   # boundary values, 2,000 random lanes
    n = len(rows)
    # limb 0 of b = this row's k (the first product), limb 1 = the next row's k (the second)
    b_rows = [rows[i][1] | (rows[(i + 1) % n][1] << 32) for i in range(n)]
    out = dbg("FE_MUL_SMALL2", [r[0] for r in rows], b_rows)
    for i, (r1, r2) in enumerate(out):
        (a, k1), (c, k2) = rows[i], rows[(i + 1) % n]
        assert r1 == a * k1 % P and r2 == c * k2 % P, (i, hex(a), k1, hex(c), k2)


# ---------------------------------------------------------------------------
# predicates and normalisation
# ---------------------------------------------------------------------------
def test_fe_is_zero_and_fe_equal(dbg):
    """fe_is_zero (0 and p only) and fe_equal on weak-form operands: (a, a),
    (a, a + p) and (a + p, a) for a < C, (0, p), (p, 0), (a, a + 1), and
    differences that pass through both borrow arms of fe_sub."""
    rng = random.Random(29)
    zs = fc.FE_EDGES + [P ^ (1 << k) for k in range(0, 256, 17)] + [1 << k for k in range(0, 256, 19)] + \
        [rand256(rng) for _ in range(500)]
    out = dbg("FE_IS_ZERO", zs, [0] * len(zs))
    assert [w[0] for w in out] == [int(z in (0, P)) for z in zs]
    small = [0, 1, 2, 976, 977, 978, 2**32, C - 2, C - 1] + [rng.randrange(C) for _ in range(200)]
    vals = fc.FE_EDGES + [rand256(rng) for _ in range(500)]
    pairs = [(a, a) for a in vals] + [(a, a + P) for a in small] + [(a + P, a) for a in small]
    pairs += [(0, P), (P, 0)] + [(a, a + 1) for a in vals if a + 1 < M] + [(a + 1, a) for a in vals if a + 1 < M]
    pairs += fc.sub_cases(False) + fc.sub_cases(True) + fc.sub_cases(False, seed=0x77) + fc.sub_cases(True, seed=0x77)
    pairs += [(a, b) for a in fc.FE_EDGES for b in fc.FE_EDGES]
    for name, rows in fc.layouts(fc.sub_cases(False), fc.sub_cases(True),
                                 fc.ordinary(fc.fe_sub, lambda r: (rand256(r), rand256(r)), 64)).items():
        pairs += rows
    out = dbg("FE_EQUAL", [p[0] for p in pairs], [p[1] for p in pairs])
    for (a, b), w in zip(pairs, out):
        assert w[0] == int((a - b) % P == 0), (hex(a), hex(b))
    assert sum(w[0] for w in out) >= len(vals) + 2 * len(small) + 2


def test_fe_normalize_and_u256_lt_p_at_the_boundary(dbg):
    """fe_normalize and u256_lt_p at p - 1, p, p + 1, 2^256 - 1 and around."""
    rng = random.Random(28)
    vals = [P - 1, P, P + 1, M - 1] + fc.FE_EDGES + [P - 2**32, P + 2**32, P + 976, P + 977, P - 2**64, 2**255] + \
        [P + rng.randrange(C) for _ in range(100)] + [P - rng.randrange(1, C) for _ in range(100)] + \
        [rand256(rng) for _ in range(500)]
    out = dbg("FE_NORMALIZE", vals, [0] * len(vals))
    assert [w[0] for w in out] == [v % P for v in vals]
    out = dbg("U256_LT_P", vals, [0] * len(vals))
    assert [w[0] for w in out] == [int(v < P) for v in vals]


# ---------------------------------------------------------------------------
# scalars
# ---------------------------------------------------------------------------
def test_scalar_ops_random_and_boundary_pairs(dbg):
    """sc_add, sc_sub, sc_neg, sc_sqr, sc_mul on reduced operands (every caller
    reduces first: msg32 by sc_cond_sub_n, r and s are rejected when >= n)."""
    rng = random.Random(32)
    pairs = [(a, b) for a in fc.SC_EDGES for b in fc.SC_EDGES] + [(rng.randrange(N), rng.randrange(N))
                                                                 for _ in range(2000)]
    xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
    for op, f in (("SC_ADD", lambda a, b: a + b), ("SC_SUB", lambda a, b: a - b), ("SC_NEG", lambda a, b: -a),
                  ("SC_SQR", lambda a, b: a * a), ("SC_MUL", lambda a, b: a * b)):
        out = dbg(op, xs, ys)
        for (a, b), w in zip(pairs, out):
            assert w[0] == f(a, b) % N, (op, hex(a), hex(b))


def test_sc_is_high_also_on_an_unreduced_s(dbg):
    """sc_is_high: the verifier's prologue calls it on s as read from the
    record, before the s < n verdict is consulted, so it must be a plain
    comparison with n / 2 on any 256-bit value."""
    rng = random.Random(36)
    vals = fc.SC_EDGES + [N, N + 1, M - 1, 2**255, 2**255 - 1] + [rand256(rng) for _ in range(1000)]
    out = dbg("SC_IS_HIGH", vals, [0] * len(vals))
    assert [w[0] for w in out] == [int(v > fc.HALF_N) for v in vals]


def test_sc_reduce512_last_fold_and_cond_sub(dbg):
    """sc_mul and sc_sqr on the operands whose reduction takes the last fold
    (c8[8] == 1) and whose sc_cond_sub_n subtracts, in the three layouts."""
    last, sub = fc.sc_mul_cases("last_fold"), fc.sc_mul_cases("cond_sub")
    plain = fc.fill("sc plain", 64, lambda r: (r.randrange(N), r.randrange(N)),
                     lambda a, b: not any(fc.sc_mul(a, b)[1:]), 7)
    for name, rows in fc.layouts(last, sub, plain).items():
        assert sum(fc.sc_mul(*c)[1] for c in rows) >= 4 and sum(fc.sc_mul(*c)[2] for c in rows) >= 4
        out = dbg("SC_MUL", [c[0] for c in rows], [c[1] for c in rows])
        assert [w[0] for w in out] == [a * b % N for a, b in rows], name
    last, sub = fc.sc_sqr_cases("last_fold"), fc.sc_sqr_cases("cond_sub")
    plain = fc.fill("sc plain", 64, lambda r: (r.randrange(N),), lambda a: not any(fc.sc_sqr(a)[1:]), 8)
    for name, rows in fc.layouts(last, sub, plain).items():
        out = dbg("SC_SQR", [c[0] for c in rows], [0] * len(rows))
        assert [w[0] for w in out] == [a * a % N for (a,) in rows], name


def _inv_layout(rng, edges, mod):
    """Lanes that finish in one or two iterations (1, 2, small powers of two)
    beside full-length values, then in waves of their own; 0 gives 0."""
    short = [1, 2, 4, 8, 16, 2**10, 2**20, 2**29, 3, 5]
    full = [x % mod for x in edges if x % mod] + [rng.randrange(1, mod) for _ in range(64)]
    xs = []
    for i in range(128):                       # short and full lanes alternate
        xs.append(short[i // 2 % len(short)] if i % 2 == 0 else full[i // 2 % len(full)])
    for lane in (0, 31, 32, 63):               # one full-length lane among short ones, and the reverse
        w = [short[i % len(short)] for i in range(64)]
        w[lane] = full[lane % len(full)]
        xs += w
        w = [full[(i + lane) % len(full)] for i in range(64)]
        w[lane] = short[lane % len(short)]
        xs += w
    xs += [short[i % len(short)] for i in range(64)]        # a wave of short lanes only
    xs += [0] * 64 + [0 if i % 2 else full[i % len(full)] for i in range(64)]
    xs += full
    return xs


def test_inv_mod_p_and_inv_mod_n_lane_mixes(dbg):
    """sgcd::inv_mod_p and inv_mod_n on the device, where the loop stops on
    __all(g == 0): a finished lane keeps iterating while its neighbours have
    not. The edge lists are test_safegcd.py's."""
    rng = random.Random(37)
    xs = _inv_layout(rng, EDGE_FIELD, P)
    out = dbg("INV_MOD_P", xs, [0] * len(xs))
    assert [w[0] for w in out] == [pow(x, -1, P) if x else 0 for x in xs]
    xs = _inv_layout(rng, EDGE_SCALARS, N)
    out = dbg("SC_INV", xs, [0] * len(xs))
    assert [w[0] for w in out] == [pow(x, -1, N) if x else 0 for x in xs]


# ---------------------------------------------------------------------------
# group ops
# ---------------------------------------------------------------------------
_POW2 = []


def jmul(k):
    """k G: Jacobian sums over a table of 2^i G, one inversion at the end
    (checked against the oracle's point_mul in test_reference_multiplier)."""
    if not _POW2:
        q = o.G
        for _ in range(256):
            _POW2.append(q)
            q = o.point_add(q, q)
    k %= N
    X = Y = Z = None
    for i in range(256):
        if not (k >> i) & 1:
            continue
        x2, y2 = _POW2[i]
        if X is None:
            X, Y, Z = x2, y2, 1
            continue
        zz = Z * Z % P
        h = (x2 * zz - X) % P
        r = (y2 * zz * Z - Y) % P
        assert h  # the partial sum is below 2^i, never +-2^i G
        hh = h * h % P
        v = X * hh % P
        hhh = hh * h % P
        X3 = (r * r - hhh - 2 * v) % P
        Y, Z = (r * (v - X3) - Y * hhh) % P, Z * h % P
        X = X3
    if X is None:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def test_reference_multiplier():
    rng = random.Random(1)
    for k in [0, 1, 2, 3, N - 1, N - 2, 2**128, o.LAMBDA] + [rng.randrange(N) for _ in range(8)]:
        assert jmul(k) == o.point_mul(k, o.G)


TAKE, AINF, BINF = 1, 2, 4


@pytest.fixture(scope="module")
def group_lanes():
    """512 lanes (k1, k2, z1, w) with their points: a wave of ordinary lanes;
    a whole wave of each degenerate case — T == acc, T == -acc, acc infinite
    on entry, take false, b infinite, both infinite; and a wave of ordinary
    lanes with one lane of each case in it (lanes 0, 63, 31, 32, ...), the
    __any(degen) path beside lanes that do not take it. Which cases are
    degenerate depends on the op: take false is an ordinary sum for
    gej_add_var, b infinite an ordinary sum for gej_accumulate."""
    rng = random.Random(64)

    def lane(kind):
        k1, k2, sel = rng.randrange(1, N), rng.randrange(1, N), TAKE
        if kind == "dbl":
            k2 = k1
        elif kind == "neg":
            k2 = N - k1
        elif kind == "ainf":
            sel |= AINF
        elif kind == "azero":
            k1 = 0
        elif kind == "notake":
            sel = 0
        elif kind == "binf":
            sel |= BINF
        elif kind == "bothinf":
            sel |= AINF | BINF
        elif kind == "dbl_notake":
            k2, sel = k1, 0
        z1 = rng.choice([1, 2, P - 1, P + 5, rng.randrange(1, P), rng.randrange(1, P), rng.randrange(1, P)])
        w = (rng.randrange(1, 2**253) << 3) | sel
        return dict(kind=kind, k1=k1, k2=k2, sel=sel, z1=z1, w=w)
    kinds = ["ord"] * 64
    for kind in ("dbl", "neg", "ainf", "notake", "binf", "bothinf"):
        kinds += [kind] * 64
    beside = ["ord"] * 64
    for lane_no, kind in ((0, "dbl"), (63, "neg"), (31, "ainf"), (32, "notake"), (5, "binf"), (40, "bothinf"),
                          (17, "azero"), (50, "dbl_notake")):
        beside[lane_no] = kind
    kinds += beside
    lanes = [lane(k) for k in kinds]
    assert len(lanes) <= 512
    for ln in lanes:
        ln["p1"], ln["p2"] = jmul(ln["k1"]), jmul(ln["k2"])
    return lanes


def run_group(dbg, op, lanes, a2=None):
    a_rows, b_rows = [], []
    for ln in lanes:
        a_rows += [ln["k1"], ln["z1"]]
        b_rows += [ln["k2"], ln["w"]]
    out = dbg(op, a_rows, b_rows)
    res = []
    for i in range(len(lanes)):
        (x, y), (flag, _) = out[2 * i], out[2 * i + 1]
        assert flag in (0, 1) and (flag == 0 or (x, y) == (0, 0))
        res.append(None if flag else (x, y))
    return res


def expect_add(ln, complete):
    """(P1, inf) += P2 under take; complete: an accumulator at infinity takes P2"""
    take = bool(ln["sel"] & TAKE)
    if ln["k1"] == 0 or ln["sel"] & AINF:
        return ln["p2"] if (complete and take) else None
    return o.point_add(ln["p1"], ln["p2"]) if take else ln["p1"]


@pytest.mark.parametrize("op", ["GEJ_ACCUMULATE", "GEJ_ACCUMULATE_ILP"])
def test_gej_accumulate_forms(dbg, group_lanes, op):
    """gej_accumulate and gej_accumulate_ilp: ordinary sums, T == acc (the
    masked doubling), T == -acc (to infinity), acc infinite on entry (left to
    the caller: stays infinite), take false; Z other than 1."""
    got = run_group(dbg, op, group_lanes)
    for ln, g in zip(group_lanes, got):
        assert g == expect_add(ln, False), (op, ln["kind"])


def test_gej_accumulate_forms_agree(dbg, group_lanes):
    assert run_group(dbg, "GEJ_ACCUMULATE", group_lanes) == run_group(dbg, "GEJ_ACCUMULATE_ILP", group_lanes)


def test_gej_add_affine_complete(dbg, group_lanes):
    """gej_add_affine_complete: as gej_accumulate, and an accumulator at
    infinity takes the point."""
    got = run_group(dbg, "GEJ_ADD_AFFINE_COMPLETE", group_lanes)
    for ln, g in zip(group_lanes, got):
        assert g == expect_add(ln, True), ln["kind"]


def test_gej_add_var(dbg, group_lanes):
    """gej_add_var: two Jacobian points with their own z; b infinite, acc
    infinite, both infinite, a == b, a == -b."""
    got = run_group(dbg, "GEJ_ADD_VAR", group_lanes)
    for ln, g in zip(group_lanes, got):
        a = None if (ln["k1"] == 0 or ln["sel"] & AINF) else ln["p1"]
        b = None if ln["sel"] & BINF else ln["p2"]
        assert g == o.point_add(a, b), ln["kind"]


def test_gej_double_and_gej_double_ilp(dbg, group_lanes):
    """gej_double returns a rescaled representative of 2a (the affine result
    absorbs the scale); gej_double_ilp must agree with it lane for lane."""
    lanes = [ln for ln in group_lanes if ln["k1"] != 0]
    a, b = run_group(dbg, "GEJ_DOUBLE", lanes), run_group(dbg, "GEJ_DOUBLE_ILP", lanes)
    assert a == b
    for ln, g in zip(lanes, a):
        if not ln["sel"] & AINF:
            assert g == o.point_add(ln["p1"], ln["p1"]), ln["kind"]


def test_x_matches_r(dbg):
    """x_matches_r(X, Z, r): r == x; the r + n branch (x >= n, r = x - n) with
    r just below and just at p - n; a non-matching r; Z other than 1."""
    rng = random.Random(70)
    pmn = P - N
    xr = []
    for _ in range(64):
        x = rng.randrange(N)
        xr += [(x, x), (x, (x + 1) % N), (x, x ^ (1 << rng.randrange(255)))]
    for x in [N, N + 1, P - 1, P - 2, N + rng.randrange(pmn), N + rng.randrange(pmn)]:
        xr += [(x, x - N), (x, x - N + 1), (x, x - N - 1 if x > N else 1)]
    xr += [(P - 1, pmn - 1), (0, pmn), (P, pmn), (1, pmn + 1), (pmn, pmn), (pmn - 1, pmn - 1), (0, 0), (P, 0),
           (N - 1, N - 1), (0, N - 1), (P - 1, N - 1), (5, 5), (P + 5, 5), (N + 5, 5), (M - 1, M - 1 - P)]
    lanes = []
    for x, r in xr:
        for z in (1, rng.randrange(1, P), rng.choice([2, P - 1, P + 3])):
            lanes.append(dict(k1=x, k2=r, z1=z, w=0))
    a_rows, b_rows = [], []
    for ln in lanes:
        a_rows += [ln["k1"], ln["z1"]]
        b_rows += [ln["k2"], 0]
    out = dbg("X_MATCHES_R", a_rows, b_rows)
    hits = 0
    for i, ln in enumerate(lanes):
        x, r = ln["k1"] % P, ln["k2"]
        exp = int(r == x or (r < pmn and r + N == x))
        hits += exp
        assert out[2 * i][0] == exp, (hex(ln["k1"]), hex(r), hex(ln["z1"]))
    assert hits >= 64 * 3 + 6 * 3


def test_ecmult_simple_two_scalars(dbg):
    """ecmult_simple(a, b, P) with b != 0 and P != G: 256 random (a, b, P),
    a = 0, b = 0, a G == -b P (infinity), a G == b P (the doubling inside
    the complete addition), a, b in {1, n - 1}."""
    rng = random.Random(71)
    cases = [(rng.randrange(N), rng.randrange(1, N), rng.randrange(2, N)) for _ in range(256)]
    for _ in range(8):
        a, b, kp = rng.randrange(1, N), rng.randrange(1, N), rng.randrange(2, N)
        cases += [(0, b, kp), (a, 0, kp), (0, 0, kp), (-b * kp % N, b, kp), (b * kp % N, b, kp)]
        cases += [(x, y, kp) for x in (1, N - 1) for y in (1, N - 1)]
    cases += [(1, 1, N - 1), (1, 1, 1), (N - 1, 1, 1), (2, N - 1, 2), (5, 0, 1)]
    a_rows, b_rows = [], []
    for a, b, kp in cases:
        a_rows += [a, kp]
        b_rows += [b, 0]
    out = dbg("ECMULT", a_rows, b_rows)
    infs = 0
    for i, (a, b, kp) in enumerate(cases):
        exp = jmul(a + b * kp)
        (x, y), (flag, _) = out[2 * i], out[2 * i + 1]
        infs += exp is None
        assert (None if flag else (x, y)) == exp and (flag == 0 or (x, y) == (0, 0)), (hex(a), hex(b), hex(kp))
    assert infs >= 17
