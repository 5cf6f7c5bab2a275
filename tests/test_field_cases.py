"""The directed operand sets of field_cases.py against its own CPU models:
every emitted case takes the branch it was built for (none skipped, every
quota filled), the model's limb result equals the mathematical value mod p
(mod n), and a build with the rare helper's body left out (skip_rare) would
be wrong on exactly these cases — which is why test_gpu_primitives.py runs
them on the device.

What the skip_rare assertions show, helper by helper (the device test
compares the same operands with the same expected values, in every lane
layout, so it fails wherever the model without the helper is wrong):

  fe_fold_carry_rare left out   test_field_op_rare_branch_layouts[FE_ADD] and
                                test_fe_lin2_both_rare_arms (carry arm) fail:
                                every case of add_cases / lin2_cases("carry")
                                loses 2^64 (test_fe_add_cases, test_fe_lin2_cases)
  fe_fold_borrow_rare left out  ...[FE_SUB], [FE_NEG], [FE_CNEG], [FE_CNEG_MASK]
                                and the borrow arm of test_fe_lin2_both_rare_arms
                                (test_fe_sub_cases, test_fe_cneg_cases)
  fe_fold_top_rare left out     ...[FE_MUL], [FE_SQR], [FE_MUL_REF], [FE_SQR_REF],
                                [FE_MUL_SMALL], [FE_SHL], [FE_SHL_VAR],
                                test_fe_mul_add_rare_top_fold and, through
                                fe_fold_top2, the four paired-form tests
                                (test_fe_mul_and_ref_cases and the like)
  sc_reduce512's last fold      test_sc_reduce512_last_fold_and_cond_sub
                                (test_sc_mul_cases, skip_last_fold)"""
import random

import pytest

import field_cases as fc
from field_cases import C, M, N, NC, P

Q = fc.QUOTA


def check(cases, model, math, rare=True, wrap=None, mod=P):
    assert len(cases) >= Q
    for ops in cases:
        r, got_rare, got_wrap = model(*ops)
        assert bool(got_rare) == rare, ops
        if wrap is not None:
            assert bool(got_wrap) == wrap, ops
        assert 0 <= r < M and r % mod == math(*ops) % mod, ops
        if rare:
            # the rare helper compiled out: the result is off by the lost carry
            assert model(*ops, skip_rare=True)[0] % mod != math(*ops) % mod, ops


@pytest.mark.parametrize("wrap", [False, True])
def test_fe_add_cases(wrap):
    cases = fc.add_cases(wrap)
    check(cases, fc.fe_add, lambda a, b: a + b, wrap=wrap)
    for a, b in cases:  # the issue's inequalities, stated on their own
        assert a + b >= M and ((a + b - M) % 2**64) + C >= 2**64
        assert (a + b - M + C >= M) == wrap
    if wrap:
        assert (M - 1, M - 1) in cases


@pytest.mark.parametrize("wrap", [False, True])
def test_fe_sub_cases(wrap):
    cases = fc.sub_cases(wrap)
    check(cases, fc.fe_sub, lambda a, b: a - b, wrap=wrap)
    for a, b in cases:
        assert a < b and (a - b + M) % 2**64 < C
        assert (a - b + M < C) == (b > P + a) == wrap
    if wrap:
        assert (0, M - 1) in cases


@pytest.mark.parametrize("wrap", [False, True])
def test_fe_cneg_cases(wrap):
    cases = fc.cneg_cases(wrap)
    check(cases, fc.fe_cneg, lambda a, neg: -a, wrap=wrap)
    for a, _ in cases:
        assert ((a ^ (M - 1)) % 2**64) < C - 1
        assert (P < a < M) == wrap
        assert fc.fe_cneg(a, 0) == (a, False, False)


def test_fe_neg_is_fe_sub_from_zero():
    for wrap in (False, True):
        cases = [(b,) for a, b in fc.sub_cases(wrap, seed=0x4E6) if a == 0]
        for (b,) in cases:
            assert fc.fe_neg(b)[0] % P == -b % P
    # a = 0 leaves only b > p for the wrap and b = M - d, d < C otherwise: b in (p, M) always wraps
    for b in (P + 1, M - 1, M - C + 5):
        assert fc.fe_neg(b)[1:] == (True, True)


@pytest.mark.parametrize("wrap", [False, True])
def test_fe_mul_and_ref_cases(wrap):
    cases = fc.mul_cases(wrap)
    check(cases, fc.fe_mul, lambda a, b: a * b, wrap=wrap)
    # fe_reduce512 as written reaches the same fold operands on these inputs
    check(cases, fc.fe_mul_ref, lambda a, b: a * b, wrap=wrap)
    for a, b in cases:
        lo, T = fc.scan_fold(a * b)
        assert (lo % 2**96) + T * C >= 2**96 and (lo + T * C >= M) == wrap
        assert fc.fe_mul_ref(a, b)[0] == fc.fe_mul(a, b)[0]


@pytest.mark.parametrize("wrap", [False, True])
def test_fe_sqr_and_ref_cases(wrap):
    cases = fc.sqr_cases(wrap)
    check(cases, fc.fe_sqr, lambda a: a * a, wrap=wrap)
    check(cases, fc.fe_sqr_ref, lambda a: a * a, wrap=wrap)


def test_fe_mul_add_chain():
    kinds = [False] * Q + [True] * Q + [None, False, True, None] * 16 + [None]
    rows = fc.mul_add_chain(kinds)
    assert len(rows) == len(kinds)
    for i, ((a, b, e), kind) in enumerate(zip(rows, kinds)):
        assert e == rows[(i + 1) % len(rows)][0]
        r, rare, wrap = fc.fe_mul_add(a, b, e)
        assert r % P == (a * b + e) % P
        if i < len(rows) - 1:
            assert (rare, wrap) == ((False, False) if kind is None else (True, kind)), i
        if rare:
            assert fc.fe_mul_add(a, b, e, skip_rare=True)[0] % P != (a * b + e) % P
    assert sum(k is False for k in kinds) >= Q and sum(k is True for k in kinds) >= Q


@pytest.mark.parametrize("wrap", [False, True])
def test_fe_mul_small_cases(wrap):
    for kmax in (2**16, 2**8 + 1):  # fe_mul_small (k < 2^16), fe_mul_small2 (k <= 2^8)
        cases = fc.mul_small_cases(wrap, kmax=kmax)
        check(cases, fc.fe_mul_small, lambda a, k: a * k, wrap=wrap)
        assert all(k < kmax for _, k in cases)
        assert any(k == 3 for _, k in cases)  # gej_double's multiple


@pytest.mark.parametrize("wrap", [False, True])
def test_fe_shl_cases(wrap):
    cases = fc.shl_cases(wrap)
    check(cases, fc.fe_shl, lambda a, s: a << s, wrap=wrap)
    ones = fc.shl_cases(wrap, shifts=(1,), seed=0x542)  # the shift every group formula uses
    check(ones, fc.fe_shl, lambda a, s: a << s, wrap=wrap)


@pytest.mark.parametrize("arm", ["carry", "borrow"])
@pytest.mark.parametrize("wrap", [False, True])
def test_fe_lin2_cases(arm, wrap):
    for ks in (fc.LIN2_K, fc.LIN2_CALLER_K):
        cases = fc.lin2_cases(arm, wrap, ks=ks)
        assert len(cases) >= Q
        for a, ka, b, kb in cases:
            r, got, w = fc.fe_lin2(a, ka, b, kb)
            assert (got, w) == (arm, wrap)
            assert r % P == (ka * a - kb * b) % P
            assert fc.fe_lin2(a, ka, b, kb, skip_rare=True)[0] % P != (ka * a - kb * b) % P
            t = ka * a + kb * (M - 1 - b)
            delta = ((t >> 256) - kb) * C + kb
            assert (delta >= 0) == (arm == "carry")
            assert ((t % 2**64) + delta >= 2**64) if arm == "carry" else ((t % 2**64) + delta < 0)
        assert len({(ka, kb) for _, ka, _, kb in cases}) >= 2


def test_fe_lin2_forced_b_bits():
    """The constants of lane i travel in the low 16 bits of lane i + 1's b."""
    rng = random.Random(5)
    got = 0
    for _ in range(4 * Q):
        c = fc.lin2_case(rng, 36, 27, "carry", False, b_low16=9 | (8 << 8))
        if c is not None and fc.fe_lin2(*c)[1] == "carry":
            assert c[2] & 0xFFFF == 9 | (8 << 8)
            got += 1
    assert got >= Q


def test_fe_half_cases():
    cases = fc.half_cases()
    assert len(cases) >= Q
    for (a,) in cases:
        r, carry = fc.fe_half(a)
        assert carry and a & 1 and a + P >= M
        assert r < M and 2 * r % P == a % P
    for a in (0, 1, 2, C - 2, C - 1, P - 1, P, M - 2):
        r, carry = fc.fe_half(a)
        assert 2 * r % P == a % P and carry == (a % 2 == 1 and a >= C)


@pytest.mark.parametrize("which", ["last_fold", "cond_sub"])
def test_sc_mul_cases(which):
    cases = fc.sc_mul_cases(which)
    assert len(cases) >= Q
    for a, b in cases:
        r, last, sub = fc.sc_mul(a, b)
        assert (last if which == "last_fold" else sub)
        assert r == a * b % N
        if which == "last_fold":
            assert fc.sc_mul(a, b, skip_last_fold=True)[0] != a * b % N
        else:
            assert r < NC  # only values in [n, 2^256) are subtracted


@pytest.mark.parametrize("which", ["last_fold", "cond_sub"])
def test_sc_sqr_cases(which):
    cases = fc.sc_sqr_cases(which)
    assert len(cases) >= Q
    for (a,) in cases:
        r, last, sub = fc.sc_sqr(a)
        assert (last if which == "last_fold" else sub) and r == a * a % N


def test_models_on_random_and_edge_operands():
    """The models are the mathematical operations on every operand, rare or
    not: 2,000 random tuples and every pair of boundary values."""
    rng = random.Random(9)
    vals = [(a, b) for a in fc.FE_EDGES for b in fc.FE_EDGES] + [(rng.randrange(M), rng.randrange(M))
                                                                 for _ in range(2000)]
    for a, b in vals:
        assert fc.fe_add(a, b)[0] % P == (a + b) % P
        assert fc.fe_sub(a, b)[0] % P == (a - b) % P
        assert fc.fe_mul(a, b)[0] % P == a * b % P == fc.fe_mul_ref(a, b)[0] % P
        assert fc.fe_sqr(a)[0] % P == a * a % P == fc.fe_sqr_ref(a)[0] % P
        assert fc.fe_mul_add(a, b, b)[0] % P == (a * b + b) % P
        assert fc.fe_cneg(a, 1)[0] % P == -a % P
        assert 2 * fc.fe_half(a)[0] % P == a % P
        k, s = b % 2**16, 1 + b % 31
        assert fc.fe_mul_small(a, k)[0] % P == a * k % P
        assert fc.fe_shl(a, s)[0] % P == (a << s) % P
        for ka, kb in fc.LIN2_K:
            assert fc.fe_lin2(a, ka, b, kb)[0] % P == (ka * a - kb * b) % P
        assert fc.fe_normalize(a) == (a - P if a >= P else a)
    svals = [(a, b) for a in fc.SC_EDGES for b in fc.SC_EDGES] + [(rng.randrange(N), rng.randrange(N))
                                                                 for _ in range(2000)]
    for a, b in svals:
        assert fc.sc_mul(a, b)[0] == a * b % N
        assert fc.sc_sqr(a)[0] == a * a % N
    assert fc.sc_reduce512((M - 1) * (M - 1))[0] == (M - 1) ** 2 % N  # the widest input


def test_random_operands_never_take_a_rare_branch():
    """What the issue measured: the 4,096 pairs of test_field_ops_known_answers
    (seed 1, 14 edge values paired with random ones) reach no rare branch of
    fe_add, fe_sub or fe_mul, and fe_sqr only twice: the edge values 2^256 - 1
    and 2^256 - 2 squared. By the fold's definition (lo + T C >= 2^256) both of
    those also wrap; no operand pair does, and nothing reaches a rare branch of
    the other three ops."""
    edge = [0, 1, 2, P - 1, P, P + 1, M - 1, M - 2, 2**255, C, N - 1, N, 2**224 - 1, (M - 1) ^ 2**32]
    rng = random.Random(1)
    xs = edge + [rng.randrange(M) for _ in range(4096 - len(edge))]
    ys = (edge + [rng.randrange(M) for _ in range(4096 - len(edge))])[::-1]
    hits = {"add": 0, "sub": 0, "mul": 0, "sqr": 0}
    for x, y in zip(xs, ys):
        hits["add"] += fc.fe_add(x, y)[1]
        hits["sub"] += fc.fe_sub(x, y)[1]
        hits["mul"] += fc.fe_mul(x, y)[1]
        hits["sqr"] += fc.fe_sqr(x)[1]
        assert fc.fe_sqr(x)[1] == (x in (M - 1, M - 2))
    assert hits == {"add": 0, "sub": 0, "mul": 0, "sqr": 2}


def test_layouts_place_the_rare_lanes():
    rare, wrapc = fc.add_cases(False), fc.add_cases(True)
    plain = fc.ordinary(fc.fe_add, lambda rng: (rng.randrange(M), rng.randrange(M)), 64)
    lay = fc.layouts(rare, wrapc, plain)
    assert all(len(v) % 64 == 0 for v in lay.values())
    is_rare = {k: [fc.fe_add(*c)[1] for c in v] for k, v in lay.items()}
    assert all(is_rare["all"])
    for j, lane in enumerate((0, 31, 32, 63)):
        w = is_rare["single"][64 * j:64 * j + 64]
        assert [i for i, f in enumerate(w) if f] == sorted({lane, (lane + 1) % 64})
        wraps = [fc.fe_add(*c)[2] for c in lay["single"][64 * j:64 * j + 64]]
        assert wraps[(lane + 1) % 64] and not wraps[lane]
    assert is_rare["alt"][:64] == [i % 2 == 0 for i in range(64)]
    assert is_rare["alt"][64:] == [i % 2 == 1 for i in range(64)]
