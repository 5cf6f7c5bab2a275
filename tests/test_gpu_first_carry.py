"""GPU tests (MI355X) of the product scans' fast forms (hkv_mul_asm.h *_fc:
no carry add for a column's first product, a rare mask instead) and of the
wrappers that fall back to the exact scans, in the pattern of
test_gpu_primitives.py: debug ops on rows, against the limb model that walks
the generator's schedule (first_carry_model.py).

Random operands never set the mask (2^-43 per product), so everything here
runs on the model's directed rows: per scan kind and column, operands on which
exactly that column's first full product carries, their neighbours just below
the threshold, all ones, and the squares' a[7] with and without bit 31. A
scalar read of a carry pair that came too early or from the wrong pair shows
as a wrong mask bit on these rows and nowhere else.

Rows: lane i takes (a, b) from row i and its further operands from row
(i + 1) mod n, so a tuple is laid out as two rows and every lane, the mixed
ones in between included, is checked against the model on the operands it
actually got."""
import random

import numpy as np
import pytest

import field_cases as fc
import first_carry_model as m
import secp256k1_oracle as o
from field_cases import M, N, P

pytestmark = pytest.mark.gpu

OP = dict(FE_MUL=1, FE_SQR=2, FE_MUL_ADD=22, FE_MUL_SUM=38, FE_SQRMUL_SUM=39, FC_MUL=46, FC_SQR=47, FC_MUL_ADD=48,
          FC_MUL_SUM=49, FC_SQRMUL_SUM=50, FC_MUL_MASK=51, GEJ_DOUBLE=64, GEJ_ACCUMULATE=66)

# kind -> (fast op, wrapper op, how a lane's operands come from rows i (a, b) and i + 1 (an, bn))
KIND = {
    "mul256_red_ps_fc": ("FC_MUL", "FE_MUL", lambda a, b, an, bn: (a, b)),
    "sqr256_red_ps_fc": ("FC_SQR", "FE_SQR", lambda a, b, an, bn: (a,)),
    "mul256_red_add_ps_fc": ("FC_MUL_ADD", "FE_MUL_ADD", lambda a, b, an, bn: (a, b, an)),
    "mul256_red_sum_ps_fc": ("FC_MUL_SUM", "FE_MUL_SUM", lambda a, b, an, bn: (a, b, an, bn)),
    "sqrmul256_red_sum_ps_fc": ("FC_SQRMUL_SUM", "FE_SQRMUL_SUM", lambda a, b, an, bn: (a, b, an)),
}
RAW_FIRST = {"FE_MUL_ADD", "FE_MUL_SUM", "FE_SQRMUL_SUM"}     # raw | normalised; ops 1, 2: normalised | raw


def pack(kind, ops):
    """The two rows (a, b), (an, bn) that give lane i the operand tuple."""
    filler = 0x1234567 << 96
    slots = {"mul256_red_ps_fc": "ab..", "sqr256_red_ps_fc": "a...", "mul256_red_add_ps_fc": "abc.",
             "mul256_red_sum_ps_fc": "abcd", "sqrmul256_red_sum_ps_fc": "abc."}[kind]
    v = [ops["abcd".index(ch)] if ch != "." else filler for ch in slots]
    return [(v[0], v[1]), (v[2], v[3])]


def lane_ops(kind, rows, i):
    (a, b), (an, bn) = rows[i], rows[(i + 1) % len(rows)]
    return KIND[kind][2](a, b, an, bn)


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


_ROWS = {}


def directed_rows(kind):
    """-> (rows, [(first row of the tuple, what it is, its column or None)]),
    computed once per kind."""
    if kind not in _ROWS:
        rows, what = [], []

        def put(ops, tag, col=None):
            what.append((len(rows), tag, col))
            rows.extend(pack(kind, ops))
        for col, v in m.golden(kind).items():
            put(v["ops"], "carry", col)
            put(v["below"], "below", col)
        put(m.all_ones(kind), "ones")
        for r in m.square_bit31_rows(kind) if kind in m.SQUARE_OPERANDS else []:
            put(r, "bit31")
        rng = random.Random(0xF1C0 + len(rows))
        for _ in range(8):
            put(tuple(rng.getrandbits(256) for _ in m.KINDS[kind][0]), "random")
        _ROWS[kind] = (rows, what)
    return _ROWS[kind]


@pytest.mark.parametrize("kind", sorted(KIND))
def test_fast_form_mask_and_result_on_directed_rows(dbg, kind):
    """The fast form alone: the lane's bit of the rare mask equals the model's
    in both directions, and where it is 0, r and T are the model's bit for bit."""
    rows, what = directed_rows(kind)
    model = [m.walk(kind, lane_ops(kind, rows, i)) for i in range(len(rows))]
    for g, tag, col in what:     # the rows are what they are meant to be
        car = model[g][1]
        assert {"carry": car == {col}, "below": not car, "ones": len(car) >= 10}.get(tag, True), (kind, tag, col)
    assert sum(bool(x[1]) for x in model) >= 10 and sum(not x[1] for x in model) >= 10
    out = dbg(KIND[kind][0], [r[0] for r in rows], [r[1] for r in rows])
    for i, (r, rest) in enumerate(out):
        res, car, _ = model[i]
        T, bit = rest & (2**64 - 1), (rest >> 64) & 0xFFFFFFFF
        assert bit == int(bool(car)), (kind, i, sorted(car))
        assert rest >> 96 == 0
        if not car:
            assert (r, T) == res, (kind, i)


@pytest.mark.parametrize("kind", sorted(KIND))
def test_wrappers_give_the_exact_scan_on_directed_rows(dbg, kind):
    """The wrappers (fast form, exact form on a non-zero mask) on the same
    rows: the raw weak-form limbs are the exact scan's folded, bit for bit."""
    rows, _ = directed_rows(kind)
    wop = KIND[kind][1]
    out = dbg(wop, [r[0] for r in rows], [r[1] for r in rows])
    for i, pair in enumerate(out):
        folded = fc.fold_top(*m.walk(kind, lane_ops(kind, rows, i), exact=True)[0])[0]
        raw, norm = pair if wop in RAW_FIRST else pair[::-1]
        assert raw == folded and norm == fc.fe_normalize(folded), (kind, i)


def test_whole_mask_lane_placement(dbg):
    """The wave's whole mask (op 51, the plain product's): one carrying row at
    lane 0 only, at lane 63 only, in every lane, and a last partial wave (n no
    multiple of 64) whose active lanes all carry: exactly the lanes the model
    names, no bit for an inactive lane."""
    kind = "mul256_red_ps_fc"
    d = m.golden(kind)
    carry = [v["ops"] for v in d.values()]
    quiet = [v["below"] for v in d.values()]
    assert carry and quiet and all(m.rare(kind, c) for c in carry) and not any(m.rare(kind, c) for c in quiet)
    part = 37
    rows = []
    for lane in (0, 63):
        w = [quiet[i % len(quiet)] for i in range(64)]
        w[lane] = carry[lane % len(carry)]
        rows += w
    rows += [carry[i % len(carry)] for i in range(64)]
    rows += [carry[i % len(carry)] for i in range(part)]
    n = len(rows)
    assert n % 64 == part
    out = dbg("FC_MUL_MASK", [r[0] for r in rows], [r[1] for r in rows])
    masks = [x[0] for x in out]
    assert all(x >> 64 == 0 for x in masks)
    want = [sum(int(m.rare(kind, rows[64 * w + i])) << i for i in range(min(64, n - 64 * w))) for w in range(4)]
    assert want == [1, 1 << 63, 2**64 - 1, 2**part - 1]
    for w in range(4):
        assert masks[64 * w] == want[w], (w, hex(masks[64 * w]))                 # lane 0's copy
        assert set(masks[64 * w:64 * w + 64]) == {want[w]}                        # and every active lane's


def test_group_formulas_on_directed_coordinates(dbg):
    """gej_double and gej_accumulate (the FC forms the chain launch runs) on
    points whose Z is a directed operand, against the oracle's affine
    arithmetic. gej_accumulate's first product is the square of that Z as
    given, so on the squares' carrying rows its rare mask is set and the exact
    scan is taken inside the formula: the model says on which lanes, and that
    there are lanes of both kinds in one wave. The other products of both
    formulas have computed operands (X = x Z^2, Y = y Z^3), which cannot be
    directed; they run on all ones, values at p and these Z."""
    sq = m.golden("sqr256_red_ps_fc")
    zs = [M - 1, P - 1, P + 1, M - 2]
    for v in sq.values():
        zs += [v["ops"][0], v["below"][0]]
    for v in m.golden("mul256_red_ps_fc").values():
        zs += [z for z in v["ops"] if z % P]
    zs = [z for z in zs if z % P][:96]
    fallback = [m.rare("sqr256_red_ps_fc", (z,)) for z in zs]
    assert sum(fallback[:64]) >= 10 and fallback[:64].count(False) >= 10      # in the first wave, both kinds
    assert {k for z in zs for k in m.walk("sqr256_red_ps_fc", (z,))[1]} >= set(sq)      # every column's pair
    rng = random.Random(0x66)
    k1 = [rng.randrange(1, N) for _ in zs]
    k2 = [rng.randrange(1, N) for _ in zs]
    p1, p2 = [o.point_mul(k, o.G) for k in k1], [o.point_mul(k, o.G) for k in k2]
    a_rows, b_rows = [], []
    for i, z in enumerate(zs):
        a_rows += [k1[i], z]
        b_rows += [k2[i], (rng.randrange(1, 2**253) << 3) | 1]   # take
    for op, want in (("GEJ_DOUBLE", [o.point_add(p, p) for p in p1]),
                     ("GEJ_ACCUMULATE", [o.point_add(p, q) for p, q in zip(p1, p2)])):
        out = dbg(op, a_rows, b_rows)
        got = [None if out[2 * i + 1][0] else out[2 * i] for i in range(len(zs))]
        assert got == want, op
