"""Directed operands for the rare carry paths of hkv_field.h / hkv_scalar.h
(test_field_cases.py, test_gpu_primitives.py). Test infrastructure.

Every fold in hkv_field.h ends in a wave-uniform "rare continuation" that a
lane takes about once in 2^32 (fe_lin2: 2^24), and each continuation has a
second-level wrap inside it. This module restates the limb algorithms with
Python integers, one model per primitive:

    model(operands...) -> (r, rare, wrap)

r is the raw (weak-form) 256-bit result the header computes, rare says whether
the lane takes the rare continuation, wrap whether it takes the second-level
wrap inside it. With skip_rare=True a model leaves the rare helper's body out
(what a build with that helper compiled out would compute): the directed
sets are the inputs on which that build is wrong.

The conditions, with C = 2^32 + 977, M = 2^256, p = M - C, NC = M - n:

  fe_add        rare: a + b >= M and ((a + b - M) mod 2^64) + C >= 2^64
                wrap: a + b - M + C >= M                    (a = b = M - 1)
  fe_sub        rare: a < b and ((a - b + M) mod 2^64) < C
                wrap: a - b + M < C, i.e. b > p + a         (a = 0, b = M - 1)
  fe_cneg(_mask), negating lanes: fe_sub's borrow test on a ^ (M - 1) with
                subtrahend C - 1; wrap for a in (p, M)
  fe_mul, fe_sqr, fe_mul_add, the _ref forms, each half of fe_mul2 / fe_sqr2 /
  fe_sqrmul: for the product t (+ e), V = (t mod M) + (t >> 256) C,
                lo = V mod M, T = V >> 256 (fe_fold_top's operands)
                rare: (lo mod 2^96) + T C >= 2^96
                wrap: lo + T C >= M
  fe_mul_small(2), fe_shl(_var): the same fe_fold_top test, T = the bits
                multiplied or shifted out
  fe_lin2       t = ka a + kb (M - 1 - b), low = t mod M, top = t >> 256,
                delta = (top - kb) C + kb
                carry arm:  delta >= 0 and (low mod 2^64) + delta >= 2^64
                borrow arm: delta < 0 and (low mod 2^64) + delta < 0
                wrap: the carry (borrow) runs through limb 7
  fe_half       carry into bit 256: a odd and a + p >= M
  sc_reduce512  last fold: c8[8] == 1 after pass 3; cond_sub: the folded
                value is >= n

Generators are deterministic (seeded), build their cases by construction and
keep those the model confirms, at most ATTEMPTS tries per case wanted; one
that cannot fill its quota raises QuotaError.
"""
from __future__ import annotations

import random
from typing import Callable, Dict, List, Optional, Sequence, Tuple

C = 2**32 + 977
M = 2**256
P = M - C
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
NC = M - N
HALF_N = N // 2
M32, M64, M96 = 2**32, 2**64, 2**96

QUOTA = 64      # cases per predicate
ATTEMPTS = 64   # tries per case wanted

# boundary values every field op meets pairwise; the scalar analogues
FE_EDGES = [0, 1, C - 1, C, C + 1, P - 1, P, P + 1, M - 1, M - C]
SC_EDGES = [0, 1, 2, HALF_N - 1, HALF_N, HALF_N + 1, HALF_N + 2, N - 2, N - 1, NC - 1, NC, NC + 1,
            C - 1, C, C + 1, P - N - 1, P - N, P - N + 1, (M - 1) % N]   # the field's boundary values, reduced mod n
# the (ka, kb) fe_lin2's callers pass (pair_double, quad_double in hkv_group.h) and the extremes
LIN2_CALLER_K = [(9, 8), (36, 27), (2, 0), (0, 8)]
LIN2_K = LIN2_CALLER_K + [(255, 255), (255, 0), (0, 255), (27, 36), (8, 9), (1, 1)]


class QuotaError(AssertionError):
    pass


# ---------------------------------------------------------------------------
# the rare continuations
# ---------------------------------------------------------------------------
def fold_carry_rare(r: int, k: int) -> Tuple[int, bool]:
    """fe_fold_carry_rare: the carry k ran past limb 1. -> (r, wrapped again)"""
    hi = (r >> 64) + k                      # limbs 2..7 += k
    k = hi >> 192
    hi &= 2**192 - 1
    lo = (r & (M64 - 1)) + k * C            # wrapped again: limbs 0..1 += k * 977, k
    k2 = lo >> 64
    hi = (hi & ~(M32 - 1)) | ((hi + k2) & (M32 - 1))   # r.v[2] += k2, no further carry
    return (hi << 64) | (lo & (M64 - 1)), bool(k)


def fold_borrow_rare(r: int, k: int) -> Tuple[int, bool]:
    """fe_fold_borrow_rare: the borrow k ran past limb 1."""
    hi = (r >> 64) - k
    k = 1 if hi < 0 else 0
    hi &= 2**192 - 1
    lo = (r & (M64 - 1)) - k * C
    k2 = 1 if lo < 0 else 0
    hi = (hi & ~(M32 - 1)) | ((hi - k2) & (M32 - 1))
    return (hi << 64) | (lo & (M64 - 1)), bool(k)


def fold_top(r: int, top: int, skip_rare: bool = False) -> Tuple[int, bool, bool]:
    """fe_fold_top + fe_fold_top_rare: r (8 limbs) + top * 2^256 -> 8 limbs."""
    assert 0 <= r < M and 0 <= top < 2**40
    lo = (r & (M96 - 1)) + top * C          # limbs 0..2 += top * C (top * 977 + (top << 32))
    c = lo >> 96
    r = (r & ~(M96 - 1)) | (lo & (M96 - 1))
    if not c or skip_rare:
        return r, bool(c), False
    hi = (r >> 96) + c                      # limbs 3..7 += c
    c = hi >> 160
    hi &= 2**160 - 1
    lo = (r & (M64 - 1)) + c * C            # wrapped: value < 2^68, limbs 0..1 += c * C
    k = lo >> 64
    l2 = (((r >> 64) & (M32 - 1)) + k) & (M32 - 1)
    return (hi << 96) | (l2 << 64) | (lo & (M64 - 1)), True, bool(c)


# ---------------------------------------------------------------------------
# models: (r, rare, wrap)
# ---------------------------------------------------------------------------
def fe_add(a: int, b: int, skip_rare: bool = False):
    s = a + b
    c, r = s >> 256, s & (M - 1)
    lo = (r & (M64 - 1)) + c * C
    k = lo >> 64
    r = (r & ~(M64 - 1)) | (lo & (M64 - 1))
    if not k or skip_rare:
        return r, bool(k), False
    r, wrap = fold_carry_rare(r, k)
    return r, True, wrap


def fe_sub(a: int, b: int, skip_rare: bool = False):
    d = a - b
    bw, r = (1 if d < 0 else 0), d & (M - 1)
    lo = (r & (M64 - 1)) - bw * C
    k = 1 if lo < 0 else 0
    r = (r & ~(M64 - 1)) | (lo & (M64 - 1))
    if not k or skip_rare:
        return r, bool(k), False
    r, wrap = fold_borrow_rare(r, k)
    return r, True, wrap


def fe_neg(a: int, skip_rare: bool = False):
    return fe_sub(0, a, skip_rare)


def fe_cneg(a: int, neg: int, skip_rare: bool = False):
    """fe_cneg and fe_cneg_mask (the same limb steps)."""
    if not neg:
        return a, False, False
    r = a ^ (M - 1)
    lo = (r & (M64 - 1)) - (C - 1)          # limb 0 -= 976, limb 1 -= 1
    k = 1 if lo < 0 else 0
    r = (r & ~(M64 - 1)) | (lo & (M64 - 1))
    if not k or skip_rare:
        return r, bool(k), False
    r, wrap = fold_borrow_rare(r, k)
    return r, True, wrap


def scan_fold(t: int) -> Tuple[int, int]:
    """The folded product scan (mul256_red_ps and kin): o + T 2^256 = L + H C."""
    v = (t & (M - 1)) + (t >> 256) * C
    return v & (M - 1), v >> 256


def fe_mul(a: int, b: int, skip_rare: bool = False):
    return fold_top(*scan_fold(a * b), skip_rare)


def fe_sqr(a: int, skip_rare: bool = False):
    return fold_top(*scan_fold(a * a), skip_rare)


def fe_mul_add(a: int, b: int, e: int, skip_rare: bool = False):
    return fold_top(*scan_fold(a * b + e), skip_rare)


def reduce512(t: int, skip_rare: bool = False):
    """fe_reduce512 as written: L + H * 977 (9 limbs), then + (H << 32)."""
    lo, h = t & (M - 1), t >> 256
    m = h * 977
    s = lo + (m & (M - 1))
    top = (m >> 256) + (s >> 256)
    s = (s & (M - 1)) + ((h & (2**224 - 1)) << 32)
    top += (h >> 224) + (s >> 256)
    return fold_top(s & (M - 1), top, skip_rare)


def fe_mul_ref(a: int, b: int, skip_rare: bool = False):
    return reduce512(a * b, skip_rare)


def fe_sqr_ref(a: int, skip_rare: bool = False):
    return reduce512(a * a, skip_rare)


def fe_mul_small(a: int, k: int, skip_rare: bool = False):
    t = a * k
    return fold_top(t & (M - 1), t >> 256, skip_rare)


def fe_shl(a: int, s: int, skip_rare: bool = False):
    """fe_shl and fe_shl_var."""
    assert 1 <= s <= 31
    t = a << s
    return fold_top(t & (M - 1), t >> 256, skip_rare)


def fe_lin2(a: int, ka: int, b: int, kb: int, skip_rare: bool = False):
    """-> (r, arm, wrap): arm is "carry", "borrow" or None."""
    t = ka * a + kb * (M - 1 - b)
    low, top = t & (M - 1), t >> 256
    delta = (top - kb) * C + kb
    s = (low & (M64 - 1)) + delta
    r = (low & ~(M64 - 1)) | (s & (M64 - 1))
    arm = "carry" if s >= M64 else ("borrow" if s < 0 else None)
    if arm is None or skip_rare:
        return r, arm, False
    r, wrap = fold_carry_rare(r, 1) if arm == "carry" else fold_borrow_rare(r, 1)
    return r, arm, wrap


def fe_half(a: int):
    """-> (r, carry): carry = the sum a + p reached bit 256."""
    t = a + (P if a & 1 else 0)
    return t >> 1, t >= M


def fe_normalize(r: int) -> int:
    t = r + C
    return t - M if t >= M else r


def sc_reduce512(t: int, skip_last_fold: bool = False):
    """sc_reduce512's three passes. -> (r, last_fold, cond_sub)"""
    a = (t & (M - 1)) + (t >> 256) * NC     # pass 1: 14 limbs
    assert a < 2**(32 * 14)
    b = (a & (M - 1)) + (a >> 256) * NC     # pass 2: 10 limbs, b[9] == 0
    assert b < 2**(32 * 9)
    h = b >> 256
    assert ((h * (NC & (2**128 - 1))) >> 128) + h < M32   # limb 4's addend is one word
    c8 = (b & (M - 1)) + h * NC             # pass 3: 9 limbs
    last = c8 >> 256
    assert last < 2
    r = (c8 & (M - 1)) + (0 if skip_last_fold else last * NC)
    assert r < M
    sub = r >= N
    return (r - N if sub else r), bool(last), sub


def sc_mul(a: int, b: int, skip_last_fold: bool = False):
    return sc_reduce512(a * b, skip_last_fold)


def sc_sqr(a: int, skip_last_fold: bool = False):
    return sc_reduce512(a * a, skip_last_fold)


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def fill(name: str, want: int, make: Callable[[random.Random], Optional[tuple]],
          pred: Callable[..., bool], seed: int) -> List[tuple]:
    rng = random.Random(seed)
    out: List[tuple] = []
    for _ in range(want * ATTEMPTS):
        if len(out) == want:
            break
        c = make(rng)
        if c is not None and pred(*c):
            out.append(c)
    if len(out) < want:
        raise QuotaError(f"{name}: {len(out)} of {want} cases in {want * ATTEMPTS} attempts")
    return out


def _is(model, rare, wrap):
    def pred(*ops):
        _, r, w = model(*ops)
        return bool(r) == rare and bool(w) == wrap
    return pred


def _hi192(rng: random.Random, ones: bool) -> int:
    """Limbs 2..7 of a non-wrapping rare value: random, with a run of all-ones
    (zero) low limbs in half the cases so the carry (borrow) travels."""
    h = rng.getrandbits(192)
    run = rng.randrange(0, 6) * 32
    low_run = (1 << run) - 1
    h = (h | low_run) if ones else (h & ~low_run)
    if ones and h == 2**192 - 1:
        h -= 1 << 191
    if not ones and h == 0:
        h = 1 << 191
    return h


def add_cases(wrap: bool, want: int = QUOTA, seed: int = 0xADD) -> List[tuple]:
    def make(rng):
        if wrap:
            v = rng.randrange(M - C, M - 1)                      # a + b - M
        else:
            v = (_hi192(rng, True) << 64) | rng.randrange(M64 - C, M64)
        a = rng.randrange(v + 1, M)
        return a, M + v - a
    fixed = [(M - 1, M - 1)] if wrap else []
    return fixed + fill("fe_add", want, make, _is(fe_add, True, wrap), seed + wrap)


def sub_cases(wrap: bool, want: int = QUOTA, seed: int = 0x50B) -> List[tuple]:
    def make(rng):
        if wrap:
            d = rng.randrange(1, C)                              # a - b + M
        else:
            d = (_hi192(rng, False) << 64) | rng.randrange(0, C)
        a = rng.randrange(0, d)
        return a, a + M - d
    fixed = [(0, M - 1)] if wrap else []
    return fixed + fill("fe_sub", want, make, _is(fe_sub, True, wrap), seed + wrap)


def cneg_cases(wrap: bool, want: int = QUOTA, seed: int = 0xC4E6) -> List[tuple]:
    """(a, 1): the negating lanes."""
    def make(rng):
        if wrap:
            return rng.randrange(P + 1, M), 1
        r = (_hi192(rng, False) << 64) | rng.randrange(0, C - 1)
        return r ^ (M - 1), 1
    fixed = [(M - 1, 1), (P + 1, 1)] if wrap else []
    return fixed + fill("fe_cneg", want, make, _is(fe_cneg, True, wrap), seed + wrap)


def fold_residue(rng: random.Random, wrap: bool) -> int:
    """The residue a product must have so that its top fold is rare."""
    if wrap:
        return rng.randrange(2**34, 2**60)
    return (rng.getrandbits(160) << 96) | rng.getrandbits(40)    # limb 2 zero, low 64 bits < 2^40


def mul_cases(wrap: bool, want: int = QUOTA, seed: int = 0x3B1, model=None) -> List[tuple]:
    model = model or fe_mul

    def make(rng):
        a = rng.randrange(1, P)
        return a, fold_residue(rng, wrap) * pow(a, -1, P) % P
    return fill("fe_mul", want, make, _is(model, True, wrap), seed + wrap)


def sqr_cases(wrap: bool, want: int = QUOTA, seed: int = 0x5C2, model=None) -> List[tuple]:
    model = model or fe_sqr

    def make(rng):
        w = fold_residue(rng, wrap) % P
        a = pow(w, (P + 1) // 4, P)
        return (a,) if a * a % P == w else None
    return fill("fe_sqr", want, make, _is(model, True, wrap), seed + wrap)


def mul_add_chain(kinds: Sequence[Optional[bool]], seed: int = 0x3ADD) -> List[tuple]:
    """fe_mul_add cases (a, b, e) in which lane i's addend is lane i + 1's a
    (the debug hook's third operand is row (i + 1) mod n of a): kinds[i] is
    None for an ordinary lane, False for rare, True for rare with the wrap.
    The last lane's addend is lane 0's a, so it is ordinary."""
    rng = random.Random(seed)
    n = len(kinds)
    a = [rng.randrange(1, P)]
    b: List[int] = []
    for i, kind in enumerate(kinds):
        if i == n - 1:
            b.append(rng.randrange(P))
            break
        for _ in range(ATTEMPTS):
            bi = rng.randrange(1, P)
            if kind is None:
                e = rng.randrange(1, M)
            else:
                # a lane's a is the previous lane's addend and may be short; its wrap then needs a
                # smaller residue (w - C < T C), so the wrap's upper bound is drawn log-uniformly
                w = rng.randrange(2**34, 2**rng.randrange(36, 61)) if kind else fold_residue(rng, False)
                e = (w - a[i] * bi) % P or 1   # a 0 addend could not be the next lane's a
            _, rare, wrap = fe_mul_add(a[i], bi, e)
            if (kind is None and not rare) or (kind is not None and rare and wrap == kind):
                break
        else:
            raise QuotaError(f"fe_mul_add: lane {i} not built in {ATTEMPTS} attempts")
        b.append(bi)
        a.append(e)
    return [(a[i], b[i], a[(i + 1) % n]) for i in range(n)]


def _top_case(rng: random.Random, wrap: bool, top: int, step: int) -> int:
    """A value top * M + r (a multiple of step, up to rounding by the caller)
    whose fold of top is rare: r's low 96 bits just below 2^96."""
    if wrap:
        return top * M + M - 1 - rng.randrange(step, top * C - step)
    r = (rng.getrandbits(160) << 96) | (M96 - 1 - rng.randrange(step, top * C - step))
    return top * M + r


def mul_small_cases(wrap: bool, want: int = QUOTA, seed: int = 0x5A11, kmax: int = 2**16) -> List[tuple]:
    ks = [k for k in (3, 2, 255, 256, 977, kmax - 1) if k < kmax]

    def make(rng):
        k = rng.choice(ks)
        top = rng.randrange(1, k) if k > 2 else 1
        a = _top_case(rng, wrap, top, k) // k
        return (a, k) if a < M else None
    return fill("fe_mul_small", want, make, _is(fe_mul_small, True, wrap), seed + wrap)


def shl_cases(wrap: bool, want: int = QUOTA, seed: int = 0x541, shifts: Sequence[int] = (1, 3, 2, 31, 16)) -> List[tuple]:
    def make(rng):
        s = rng.choice(list(shifts))
        top = rng.randrange(1, 1 << s)
        return _top_case(rng, wrap, top, 1 << s) >> s, s
    return fill("fe_shl", want, make, _is(fe_shl, True, wrap), seed + wrap)


def lin2_case(rng: random.Random, ka: int, kb: int, arm: str, wrap: bool, b_low16: Optional[int] = None):
    """One (a, ka, b, kb) candidate for the arm, or None where (ka, kb) has
    no such case. With ka > 0 the low 16 bits of b can be forced (the debug
    hook reads a lane's ka, kb from the next row's b)."""
    tops = range(kb + (1 if ka > 1 else 0), ka + kb) if arm == "carry" else range(0, kb)
    if len(tops) == 0 or (b_low16 is not None and ka == 0):
        return None
    top = rng.choice(tops)
    delta = (top - kb) * C + kb
    if abs(delta) < 4 * (ka + kb + 1):
        return None
    slack = ka + kb + 1
    if arm == "carry":
        lo = M64 - 1 - rng.randrange(slack, delta - slack)
        hi = 2**192 - 1 if wrap else _hi192(rng, True)
    else:
        lo = rng.randrange(slack, -delta - slack)
        hi = 0 if wrap else _hi192(rng, False)
    t = top * M + ((hi << 64) | lo)
    if ka > 0:
        # kb (M - 1 - b) in (t - ka M, t]
        nlo, nhi = (max(0, t - ka * M) // kb + 1, min(M - 1, t // kb)) if kb else (0, M - 1)
        if nlo > nhi:
            return None
        b = M - 1 - rng.randrange(nlo, nhi + 1)
        if b_low16 is not None:
            b = (b & ~0xFFFF) | b_low16
        a = (t - kb * (M - 1 - b)) // ka
    else:
        a = rng.randrange(M)
        b = M - 1 - t // kb
    if not (0 <= a < M and 0 <= b < M):
        return None
    return a, ka, b, kb


def lin2_cases(arm: str, wrap: bool, want: int = QUOTA, seed: int = 0x112, ks=None) -> List[tuple]:
    ks = list(ks or LIN2_K)

    def make(rng):
        ka, kb = rng.choice(ks)
        return lin2_case(rng, ka, kb, arm, wrap)

    def pred(a, ka, b, kb):
        _, got, w = fe_lin2(a, ka, b, kb)
        return got == arm and w == wrap
    return fill(f"fe_lin2 {arm}", want, make, pred, seed + 2 * (arm == "carry") + wrap)


def lin2_rows(plan: Sequence[Optional[tuple]], seed: int = 0x1122) -> List[tuple]:
    """Rows (a, ka, b, kb) for the debug hook, where lane i's ka, kb are bytes
    0 and 1 of lane i + 1's b (cyclically). plan[i] is (ka, kb, arm, wrap) for
    a rare lane or None for an ordinary one. A lane with ka = 0 has its b
    fixed by the construction, so the lane before it must be ordinary and
    takes whatever constants that b carries; every other b has its low 16
    bits forced."""
    rng = random.Random(seed)
    n = len(plan)
    consts: List[Optional[Tuple[int, int]]] = [None if p is None else (p[0], p[1]) for p in plan]
    rows: List[Optional[tuple]] = [None] * n
    for i, p in enumerate(plan):      # pass 1: the lanes whose b cannot be forced
        if p is None or p[0] != 0:
            continue
        assert plan[i - 1] is None, "a ka = 0 lane needs an ordinary lane before it"
        for _ in range(ATTEMPTS):
            c = lin2_case(rng, p[0], p[1], p[2], p[3])
            if c is not None and fe_lin2(*c)[1:] == (p[2], p[3]):
                break
        else:
            raise QuotaError(f"fe_lin2 row {i}: {p}")
        rows[i] = c
        consts[i - 1] = (c[2] & 0xFF, (c[2] >> 8) & 0xFF)
    for i in range(n):
        if consts[i] is None:
            consts[i] = rng.choice(LIN2_CALLER_K)
    for i, p in enumerate(plan):      # pass 2: low 16 bits of b = the previous lane's constants
        if rows[i] is not None:
            continue
        ka, kb = consts[i]
        low16 = consts[i - 1][0] | (consts[i - 1][1] << 8)
        for _ in range(ATTEMPTS):
            if p is None:
                c = (rng.randrange(M), ka, (rng.randrange(M) & ~0xFFFF) | low16, kb)
                if fe_lin2(*c)[1] is None:
                    break
            else:
                c = lin2_case(rng, ka, kb, p[2], p[3], b_low16=low16)
                if c is not None and fe_lin2(*c)[1:] == (p[2], p[3]):
                    break
        else:
            raise QuotaError(f"fe_lin2 row {i}: {p}")
        rows[i] = c
    for i in range(n):
        nb = rows[(i + 1) % n][2]
        assert (rows[i][1], rows[i][3]) == (nb & 0xFF, (nb >> 8) & 0xFF)
    return rows  # type: ignore[return-value]


def neg_cases(wrap: bool, want: int = QUOTA, seed: int = 0x4E6) -> List[tuple]:
    """fe_neg = fe_sub from zero: rare when (M - a) mod 2^64 < C, wrap for a in (p, M)."""
    def make(rng):
        if wrap:
            return (rng.randrange(P + 1, M),)
        return (M - ((_hi192(rng, False) << 64) | rng.randrange(0, C)),)
    return fill("fe_neg", want, make, _is(fe_neg, True, wrap), seed + wrap)


def half_cases(want: int = QUOTA, seed: int = 0x4A1F) -> List[tuple]:
    def make(rng):
        return (rng.choice([C, C + 2, M - 1, P + 2, rng.randrange(C, M)]) | 1,)
    return fill("fe_half", want, make, lambda a: fe_half(a)[1], seed)


def sc_mul_cases(which: str, want: int = QUOTA, seed: int = 0x5C) -> List[tuple]:
    """which: "last_fold" (c8[8] == 1) or "cond_sub" (sc_cond_sub_n subtracts)."""
    def make(rng):
        a = rng.randrange(1, N)
        w = NC + rng.getrandbits(64) if which == "last_fold" else rng.getrandbits(100)
        return a, w * pow(a, -1, N) % N

    def pred(a, b):
        _, last, sub = sc_mul(a, b)
        return last if which == "last_fold" else sub
    return fill(f"sc_mul {which}", want, make, pred, seed + (which == "cond_sub"))


def sc_sqr_cases(which: str, want: int = QUOTA, seed: int = 0x5C5) -> List[tuple]:
    """The same residues through a square root mod n (Tonelli-Shanks; about
    half of them have one)."""
    def make(rng):
        a = sqrt_mod_n(NC + rng.getrandbits(64) if which == "last_fold" else rng.getrandbits(100))
        return None if a is None else (a,)

    def pred(a):
        _, last, sub = sc_sqr(a)
        return last if which == "last_fold" else sub
    return fill(f"sc_sqr {which}", want, make, pred, seed + (which == "cond_sub"))


def sqrt_mod_n(w: int) -> Optional[int]:
    """Tonelli-Shanks mod the group order."""
    w %= N
    if w == 0 or pow(w, (N - 1) // 2, N) != 1:
        return None
    q, s = N - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    z = 2
    while pow(z, (N - 1) // 2, N) != N - 1:
        z += 1
    m, c, t, r = s, pow(z, q, N), pow(w, q, N), pow(w, (q + 1) // 2, N)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % N
            i += 1
        b = pow(c, 1 << (m - i - 1), N)
        m, c = i, b * b % N
        t, r = t * c % N, r * b % N
    return r


def ordinary(model, make: Callable[[random.Random], tuple], want: int, seed: int = 0x0D) -> List[tuple]:
    """Operands that do not take the model's rare branch."""
    return fill("ordinary", want, make, lambda *ops: not model(*ops)[1], seed)


# ---------------------------------------------------------------------------
# lane layouts: where the rare lanes of a directed set sit in the wave
# ---------------------------------------------------------------------------
WAVE = 64


def layouts(rare: Sequence[tuple], wrapc: Sequence[tuple], plain: Sequence[tuple]) -> Dict[str, List[tuple]]:
    """The three lane layouts of a directed set (the expected values are per
    lane, so only the layout changes):
      all      every lane of each wave rare (non-wrap waves, then wrap waves)
      single   one rare lane among ordinary lanes, at lane 0, 31, 32 and 63
               in turn, its wrap variant in the same wave one lane on (mod 64)
      alt      alternating rare and ordinary lanes (even lanes, then odd)"""
    rare, wrapc, plain = list(rare), list(wrapc), list(plain)
    assert len(rare) >= WAVE and len(wrapc) >= WAVE and len(plain) >= WAVE

    def cyc(xs, i):
        return xs[i % len(xs)]
    out = {"all": rare[:WAVE] + wrapc[:WAVE]}
    single: List[tuple] = []
    for j, lane in enumerate((0, 31, 32, 63)):
        w = [cyc(plain, 7 * j + i) for i in range(WAVE)]
        w[lane] = cyc(rare, j)
        w[(lane + 1) % WAVE] = cyc(wrapc, j)
        single += w
    out["single"] = single
    alt: List[tuple] = []
    for par in (0, 1):
        src = [(wrapc if j % 2 else rare)[j // 2] for j in range(WAVE // 2)]   # rare, wrap, rare, ...
        alt += [src[i // 2] if i % 2 == par else cyc(plain, i) for i in range(WAVE)]
    out["alt"] = alt
    return out
