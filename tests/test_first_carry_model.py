"""The fast product scans (hkv_mul_asm.h *_fc: no carry add for a column's
first product) on the CPU: the generator's bounds, the limb model that walks
its schedule (first_carry_model.py) against the existing models, the derived
rarity of the mask on random operands, and the directed rows that
test_gpu_first_carry.py runs on the device."""
import random

import numpy as np
import pytest

import field_cases as fc
import first_carry_model as m
import test_gpu_sum_scans as ss
from field_cases import M

gen = m.gen


def existing_scan(kind, ops):
    """(o, T) by the existing scan model (test_gpu_sum_scans.sum_scan: o + T 2^256 = L + H C over the
    column lists), an addend joining L; and the folded raw limbs by field_cases' models where one exists."""
    none = [[] for _ in range(15)]
    if kind == "mul256_red_ps_fc":
        lo, T = ss.sum_scan(ss.mul_cols(*ops), none)[:2]
        folded = fc.fe_mul(*ops)[0]
    elif kind == "mul256_red_add_ps_fc":
        lo, T = ss.sum_scan(ss.mul_cols(ops[0], ops[1]), none)[:2]
        v = lo + (T << 256) + ops[2]
        lo, T = v & (M - 1), v >> 256
        folded = fc.fe_mul_add(*ops)[0]
    elif kind == "sqr256_red_ps_fc":
        lo, T = ss.sum_scan(ss.sqr_cols(ops[0]), none)[:2]
        folded = fc.fe_sqr(ops[0])[0]
    elif kind == "mul256_red_sum_ps_fc":
        lo, T = ss.sum_scan(ss.mul_cols(ops[0], ops[1]), ss.mul_cols(ops[2], ops[3]))[:2]
        folded = ss.fe_mul_sum(*ops)[0]
    else:
        lo, T = ss.sum_scan(ss.sqr_cols(ops[0]), ss.mul_cols(ops[1], ops[2]))[:2]
        folded = ss.fe_sqrmul_sum(*ops)[0]
    return (lo, T), folded


def operand_sets(kind, rng, n):
    k = len(m.KINDS[kind][0])
    E = fc.FE_EDGES
    sets = [tuple(rng.getrandbits(256) for _ in range(k)) for _ in range(n)]
    sets += [tuple(rng.choice(E) for _ in range(k)) for _ in range(n // 4)]
    sets += [m.all_ones(kind), (0,) * k, (fc.P,) * k, (fc.P - 1,) * k]
    return sets


def test_generator_bounds_hold_and_counts_match():
    """Rendering the header runs the generator's interval assertions for every
    column of every scan kind (ColumnBounds: the seeds below 2^43, a check
    product's accumulator below 2^43 + 2^32, a free product's sum below 2^64).
    Restated from the dumped schedule: the classes' order, one check per column
    at most, and the carry adds dropped per scan (15; 22 for a square)."""
    sched = gen.fast_schedules()
    assert sched == m.SCHEDULES and set(sched) == set(m.KINDS)
    dropped = {}
    for kind, cols in sched.items():
        assert [k for k, _ in cols] == list(range(8, 15)) + list(range(8))
        n = 0
        for k, prods in cols:
            cls = [c for _, _, c in prods]
            rank = {"free": 0, "check": 1, "add": 2}
            assert [rank[c] for c in cls] == sorted(rank[c] for c in cls) and cls.count("check") <= 1
            assert k == 8 or "check" in cls or "add" not in cls      # only column 8 adds without a check
            small = [min(gen.op_max(x), gen.op_max(y)) == 1 for x, y, _ in prods]
            assert small == sorted(small, reverse=True) and all(c == "free" for c, s in zip(cls, small) if s)
            n += cls.count("free") + cls.count("check")
        dropped[kind] = n
    assert dropped == {"mul256_red_ps_fc": 15, "mul256_red_add_ps_fc": 15, "sqr256_red_ps_fc": 22,
                       "mul256_red_sum_ps_fc": 15, "sqrmul256_red_sum_ps_fc": 22}
    # the all-ones walk (exact, every carry kept) meets each check product below the stated bound
    for kind in m.KINDS:
        _, _, trace = m.walk(kind, m.all_ones(kind), exact=True)
        assert trace and all(a < gen.CHECK_BOUND for a, _ in trace.values())


@pytest.mark.parametrize("kind", sorted(m.KINDS))
def test_model_equals_the_existing_models(kind):
    """The walk with every carry kept (the exact forms) gives the existing
    models' (o, T) and, folded, their raw limbs; the fast walk gives the same
    whenever its mask is empty."""
    rng = random.Random(sorted(m.KINDS).index(kind))
    for ops in operand_sets(kind, rng, 200):
        (lo, T), folded = existing_scan(kind, ops)
        res, _, _ = m.walk(kind, ops, exact=True)
        assert res == (lo, T), [hex(x) for x in ops]
        assert fc.fold_top(lo, T)[0] == folded
        fast, carried, _ = m.walk(kind, ops)
        assert carried or fast == res


@pytest.mark.parametrize("kind", sorted(m.KINDS))
def test_no_first_product_carries_on_a_million_random_operands(kind):
    """A check product carries only if both limbs lie within about 2^11 of
    2^32: at most 2^-43 per product on uniform limbs, so 10^6 operand sets
    (at most 14 check products each) give none. The bulk walk is the model
    again (checked against it on the first rows)."""
    rng = np.random.default_rng(0xF1C + sorted(m.KINDS).index(kind))
    names = m.KINDS[kind][0]
    for chunk in range(4):
        ops = [rng.integers(0, 2**32, size=(8, 250_000), dtype=np.uint64) for _ in names]
        bits, o, T = m.walk_np(kind, ops)
        assert not bits.any()
        if chunk == 0:
            for i in range(20):
                py = tuple(m.unlimbs([int(x) for x in op[:, i]]) for op in ops)
                r, t = m.walk(kind, py)[0]
                assert (m.unlimbs([int(x) for x in o[:, i]]), int(T[i])) == (r, t)
    # and the bulk walk does see the carries of the directed rows
    d = m.golden(kind)
    rows = [v["ops"] for v in d.values()] + [v["below"] for v in d.values()]
    ops = [np.array([m.limbs(r[j]) for r in rows], dtype=np.uint64).T.copy() for j in range(len(names))]
    assert list(m.walk_np(kind, ops)[0]) == [True] * len(d) + [False] * len(d)


SQUARE_COLUMN_0_GAP = 3


@pytest.mark.parametrize("kind", sorted(m.KINDS))
def test_directed_rows(kind):
    """Every column with a check product that can carry has, in the recorded
    rows, operands on which exactly that column carries and a neighbour, one
    step of one limb below, on which nothing carries and the column's
    accumulator plus product is 2^64 - 1. Which columns can: every low
    column; of the high ones, whose accumulator grows with every limb, those
    that carry on all-ones operands (all but a square's 13 and 14). The one
    exception to "one below" is a square's column 0: its accumulator is
    h[0] * 977 and its product a square, and x^2 = 2^64 - 1 (mod 977) has no
    solution, so its row has the least gap there is. All ones carry in many
    columns at once; the squares' d[8] products are 0 and a_i."""
    reach = m.reachable(kind)
    checks = m.check_columns(kind)
    assert set(reach) == set(checks) - ({13, 14} if kind == "sqr256_red_ps_fc" else set())
    d = m.golden(kind)
    assert sorted(d) == sorted(reach)
    assert pow((2**64 - 1) % 977, (977 - 1) // 2, 977) == 977 - 1      # a non-residue
    for k, v in d.items():
        assert m.walk(kind, v["ops"])[1] == {k}
        res, car, tr = m.walk(kind, v["below"])
        assert not car and res == m.walk(kind, v["below"], exact=True)[0]
        square0 = k == 0 and kind in m.SQUARE_OPERANDS
        assert 2**64 - sum(tr[k]) == v["gap"] == (SQUARE_COLUMN_0_GAP if square0 else 1), (kind, k)
        la, lb = [m.limbs(x) for x in v["ops"]], [m.limbs(x) for x in v["below"]]
        diff = [(x, y) for ra, rb in zip(la, lb) for x, y in zip(ra, rb) if x != y]
        if k or kind == "mul256_red_add_ps_fc":
            assert len(diff) == 1 and diff[0][0] == diff[0][1] + 1          # one limb, one step
        else:       # column 0: h[0] one higher, through the limbs that make it
            assert 1 <= len(diff) <= 2
    if kind in m.SQUARE_OPERANDS:      # no smaller gap exists for column 0: every x = 2^32 - u whose h0 fits a limb
        gaps = [1 + (2**64 - 1 - (2**32 - u)**2) % 977 for u in range(1, 489)]
        assert min(gaps) == SQUARE_COLUMN_0_GAP
    many = m.walk(kind, m.all_ones(kind))[1]
    assert len(many) >= 10 and set(many) <= set(reach)      # a dropped carry lowers the columns after it
    if kind in m.SQUARE_OPERANDS:
        rows = m.square_bit31_rows(kind)
        assert {(r[0] >> 255) for r in rows} == {0, 1}
        for r in rows:
            fast, car, _ = m.walk(kind, r)
            assert car or fast == m.walk(kind, r, exact=True)[0]


def test_recorded_rows_are_the_builders():
    """The recorded rows are directed()'s output (rebuilt here for the plain
    product, which takes a fraction of a second)."""
    kind = "mul256_red_ps_fc"
    built = m.directed(kind)
    assert {k: (v["ops"], v["below"], v["gap"]) for k, v in built.items()} == \
        {k: (v["ops"], v["below"], v["gap"]) for k, v in m.golden(kind).items()}
