"""Limb model of the product scans' fast forms (hkv_mul_asm.h *_fc) and the
directed operands for their rare mask (test_first_carry_model.py,
test_gpu_first_carry.py). Test infrastructure.

The model walks the generator's own schedule (tools/gen_mul_asm.py
fast_schedules: per column and stream the products in scan order, each with
its class "free" / "check" / "add") with Python integers, exactly as the
generated code does: a 64-bit accumulator per column, the carries of the
"add" products counted in top, the carry of the "check" product (the
column's first full product) recorded and dropped, a "free" product's carry
asserted impossible. With exact=True every carry goes to top: the exact forms.

A scan kind is named as its fast form; its operands are 256-bit integers:
    mul256_red_ps_fc (a, b)          mul256_red_add_ps_fc (a, b, e)
    sqr256_red_ps_fc (a,)            mul256_red_sum_ps_fc (a, b, c, d)
    sqrmul256_red_sum_ps_fc (a, c, d)
The paired scans (*_ps2) have no fast form.
"""
import importlib.util
import json
import os
import random

W32 = 2**32 - 1
M64 = 2**64
M = 2**256

_spec = importlib.util.spec_from_file_location(
    "gen_mul_asm", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "gen_mul_asm.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
SCHEDULES = gen.fast_schedules()

# kind -> (operand names, {array name in the schedule: (operand, role)})
KINDS = {
    "mul256_red_ps_fc": (("a", "b"), {"a": ("a", "x"), "b": ("b", "x")}),
    "mul256_red_add_ps_fc": (("a", "b", "e"), {"a": ("a", "x"), "b": ("b", "x")}),
    "sqr256_red_ps_fc": (("a",), {"a": ("a", "x"), "e": ("a", "e"), "d": ("a", "d")}),
    "mul256_red_sum_ps_fc": (("a", "b", "c", "d"), {"a": ("a", "x"), "b": ("b", "x"), "c": ("c", "x"), "d": ("d", "x")}),
    "sqrmul256_red_sum_ps_fc": (("a", "c", "d"), {"a": ("a", "x"), "ea": ("a", "e"), "da": ("a", "d"),
                                                  "c": ("c", "x"), "d": ("d", "x")}),
}
SUM_KINDS = ("mul256_red_sum_ps_fc", "sqrmul256_red_sum_ps_fc")
SQUARE_OPERANDS = {"sqr256_red_ps_fc": ("a",), "sqrmul256_red_sum_ps_fc": ("a",)}
assert set(KINDS) == set(SCHEDULES)


def limbs(x):
    return [(x >> (32 * i)) & W32 for i in range(8)]


def unlimbs(v):
    return sum(x << (32 * i) for i, x in enumerate(v))


def arrays(kind, ops):
    """The limb arrays the schedule names: operands, and for a squared operand
    e[j] = a_j << 1 and d[j] = (a_j << 1) | (a_{j-1} >> 31), d[8] = a_7 >> 31."""
    names, table = KINDS[kind]
    val = {n: limbs(x) for n, x in zip(names, ops)}
    out = {}
    for arr, (src, role) in table.items():
        a = val[src]
        if role == "x":
            out[arr] = a
        elif role == "e":
            out[arr] = [(x << 1) & W32 for x in a]
        else:
            out[arr] = [0, 0] + [((a[j] << 1) | (a[j - 1] >> 31)) & W32 for j in range(2, 8)] + [a[7] >> 31]
    return out


def _ref(arr, nm):
    name, idx = nm[:-1].split("[")
    return arr[name][int(idx)]


def walk(kind, ops, exact=False):
    """-> ((r, T), {columns whose first full product carried}, {column: (the
    accumulator before the check product, the product)})"""
    sched = SCHEDULES[kind]
    arr = arrays(kind, ops)
    e = limbs(ops[2]) if kind == "mul256_red_add_ps_fc" else None
    acc = top = h78 = 0
    h, o = [], []
    carried, trace = set(), {}
    assert [k for k, _ in sched] == list(range(8, 15)) + list(range(8))
    for k, prods in sched:
        if k == 0:                       # the end of the high half
            h78 = acc
            h += [acc & W32, acc >> 32]  # h[8]: 0 in a single product, 0 or 1 in a sum
            a = h[0] * 977 + (e[0] if e else 0)
        elif k < 8:
            a = (acc >> 32) + ((top << 32) | h[k - 1]) + h[k] * 977 + (e[k] if e else 0)
        else:
            a = acc
        assert a < M64
        t = 0
        for x, y, cls in prods:
            pr = _ref(arr, x) * _ref(arr, y)
            if cls == "check":
                trace[k] = (a, pr)
            a += pr
            c, a = a >> 64, a & (M64 - 1)
            if cls == "free":
                assert c == 0, (kind, k, x, y)
            elif cls == "check" and not exact:
                if c:
                    carried.add(k)
            else:
                t += c
        top = t
        if k >= 8:
            h.append(a & W32)
            acc = (a >> 32) | (t << 32)
        else:
            o.append(a & W32)
            acc = a
    if kind in SUM_KINDS:
        T = h[8] * 977 + h78 + ((top << 32) | (acc >> 32))
    else:
        T = (acc >> 32) + (top << 32) + h[7]
    return (unlimbs(o), T), carried, trace


def rare(kind, ops):
    return bool(walk(kind, ops)[1])


def check_columns(kind):
    """The columns that have a check product."""
    return [k for k, prods in SCHEDULES[kind] if any(c == "check" for _, _, c in prods)]


def _source_limbs(kind, nm):
    """The operand limbs [(operand index, limb, value)] that make the schedule's operand nm all ones."""
    names, table = KINDS[kind]
    name, idx = nm[:-1].split("[")
    src, role = table[name]
    i, j = names.index(src), int(idx)
    if role == "d" and j < 8:
        return [(i, j, W32), (i, j - 1, None)]   # None: keep, but set bit 31
    return [(i, j, W32)]


SAFE = W32 - 2**13      # SAFE * (any limb) < 2^64 - 2^44: such a first product never carries (accumulator < 2^44)


def reachable(kind):
    """The columns whose check product can carry at all. A high column's
    accumulator is the upper part of a true sum of products, monotone in every
    limb, so all-ones operands decide it (the squares' columns 13 and 14 are
    out of reach). A low column's accumulator also holds h[j - 1] and
    h[j] * 977, low words of the high columns, which all-ones operands make
    small (h[0] = 7 there): every low column is reachable, and directed()
    proves it by construction."""
    tr = walk(kind, all_ones(kind), exact=True)[2]
    return [k for k in check_columns(kind) if k < 8 or sum(tr[k]) >= M64]


def _ops(L):
    return tuple(unlimbs(r) for r in L)


def _with(L, i, j, v):
    L2 = [list(r) for r in L]
    L2[i][j] = v
    return L2


def _flip(kind, k, L, i, j, lo, hi):
    """Bisect limb (i, j) between lo (column k does not carry) and hi (it
    does). -> the limb value v with no carry at v and a carry at v + 1, or None."""
    if lo >= hi or k in walk(kind, _ops(_with(L, i, j, lo)))[1] or k not in walk(kind, _ops(_with(L, i, j, hi)))[1]:
        return None
    while hi - lo > 1:
        mid = (hi + lo) // 2
        if k in walk(kind, _ops(_with(L, i, j, mid)))[1]:
            hi = mid
        else:
            lo = mid
    return lo


def _exact_pair(kind, k, L, i, j, v, best=None):
    """(below, carry) rows at limb (i, j) = v, v + 1 if they are exact: nothing
    carries below, with the accumulator one short of the threshold; only
    column k carries above."""
    below, above = _ops(_with(L, i, j, v)), _ops(_with(L, i, j, v + 1))
    _, car, tr = walk(kind, below)
    if car or walk(kind, above)[1] != {k}:
        return None
    gap = M64 - sum(tr[k])
    if best is not None and (best.get(k) is None or gap < best[k][2]):
        best[k] = (below, above, gap)
    return (below, above) if gap == 1 else None


def _column0(kind):
    """Column 0's accumulator is h[0] * 977 (no unit step), so the product is
    chosen with it: x y + 977 h0 = 2^64 - g for limbs x = 2^32 - u, y = 2^32 - v
    and the least gap g >= 1, and h[0] = h0 is put there by one product of
    column 8 against the limb 1 (a[1] * b[7]; in a square a[1] * d[7], d[7] = h0
    from a[7] = h0 >> 1 and bit 31 of a[6]); h0 + 1 then carries. A product of
    two free limbs reaches g = 1. A square cannot: x^2 = 2^64 - 1 (mod 977)
    has no solution (2^64 - 1 is a quadratic non-residue mod 977), so its
    row has the least g over every x whose h0 fits a limb (u < 489).
    -> (below, carry, g)"""
    names, _ = KINDS[kind]
    square = kind in SQUARE_OPERANDS
    best = None
    for u in range(1, 489):
        for v in ([u] if square else range(1, 489)):
            r = M64 - 1 - (2**32 - u) * (2**32 - v)
            if r < 0 or r // 977 >= 2**32 - 2**13:
                continue
            h0, g = r // 977, 1 + r % 977
            if best is not None and g >= best[2]:
                continue
            rows = []
            for hh in (h0, h0 + 1):
                L = [[0] * 8 for _ in names]
                L[0][0] = 2**32 - u
                L[0][1] = 1
                if square:
                    L[0][7], L[0][6] = hh >> 1, (hh & 1) << 31
                else:
                    L[1][0], L[1][7] = 2**32 - v, hh
                rows.append(_ops(L))
            _, car, tr = walk(kind, rows[0])
            if not car and M64 - sum(tr[0]) == g and walk(kind, rows[1])[1] == {0}:
                best = (rows[0], rows[1], g)
        if best and best[2] == 1:
            break
    return best


def directed(kind, templates=1500, seed=0xF1C):
    """For every reachable column k: operands on which exactly column k's
    first full product carries ("ops"), and the neighbour one limb step below
    on which nothing carries and column k's accumulator plus product is
    2^64 - 1, one below the threshold ("below"). Built, not found by luck:
    the product's own limbs are all ones, every other limb is 0 or SAFE (so
    no other first product can carry), and one limb is bisected to the point
    where column k's carry flips — first with the product at its largest
    (the high columns, whose accumulator moves in unit steps with any limb of
    the column before), else with the product's second limb lowered to just
    below the flip and another limb raised (the low columns: the unit steps
    come from a limb that reaches only lower low columns, the coarse ones
    from the product). Column 0 has no unit step and is solved (_column0);
    with an addend its limb e[0] is the unit step. Templates (which limbs are
    SAFE) are tried in a fixed seeded order until the pair is exact; the
    model confirms every row.
    -> {k: {"ops", "below", "gap"}}: gap = 2^64 - (accumulator + product) of
    "below", 1 everywhere but in a square's column 0 (_column0)."""
    names, _ = KINDS[kind]
    n_ops = len(names)
    knobs = [(i, j) for i in range(n_ops) for j in range(8)]
    out, best = {}, {}
    for k in reachable(kind):
        if k == 0 and kind != "mul256_red_add_ps_fc":
            rows = _column0(kind)
            assert rows, (kind, k)
            out[k] = dict(below=rows[0], ops=rows[1], gap=rows[2])
            continue
        rng = random.Random(seed + k + 1024 * sorted(KINDS).index(kind))
        prods = dict(SCHEDULES[kind])[k]
        x, y = next((x, y) for x, y, c in prods if c == "check")
        forced = _source_limbs(kind, x) + _source_limbs(kind, y)
        fl = {(i, j) for i, j, _ in forced}
        yi, yj = [(i, j) for i, j, v in forced if v is not None][-1]
        found = None
        free = [q for q in knobs if q not in fl]
        for t in range(templates):
            if t < 10:      # dense: every other limb SAFE or 0
                p = (1.0, 0.7, 0.5, 0.35, 0.2)[t % 5]
                L = [[SAFE if (t == 0 or rng.random() < p) else 0 for _ in range(8)] for _ in range(n_ops)]
            else:           # sparse: a few limbs 1 (a product against 1 sets a high word exactly), 2^31 (the low
                            # bit of the next doubled limb d[j + 1]: every other step of a square is even) or SAFE
                L = [[rng.choice((0, 0, 0, 0, 1, 1, 2**31, SAFE)) for _ in range(8)] for _ in range(n_ops)]
            for i, j, v in forced:
                L[i][j] = W32 if v is not None else L[i][j] | 2**31
            if kind in SQUARE_OPERANDS and k < 8 and t % 2:
                # a square's low products all have a[0]: all ones there, a[0]^2 carries in column 0 as soon as
                # h[0] * 977 reaches 2^33; a little lower it leaves h[0] free
                L[0][0] = W32 - 300
            # the product at its largest, one limb lowered to the flip
            for i, j in free:
                if L[i][j] > 1 and found is None:
                    v = _flip(kind, k, L, i, j, 0, L[i][j])
                    found = v is not None and _exact_pair(kind, k, L, i, j, v, best) or None
            if found:
                break
            # the product's second limb just below the flip (or the product as it is, if column k does not
            # carry yet), then limb after limb raised to its flip: each pass leaves a smaller gap
            if k in walk(kind, _ops(L))[1]:
                v = _flip(kind, k, L, yi, yj, 0, L[yi][yj])
                if v is None:
                    continue
                L = _with(L, yi, yj, v)
            for _ in range(2):
                for i, j in free:
                    if found is None:
                        v = _flip(kind, k, L, i, j, L[i][j], SAFE)
                        if v is not None:
                            L = _with(L, i, j, v)
                            found = _exact_pair(kind, k, L, i, j, v, best)
            if found:
                break
        if not found:       # the nearest adjacent pair met (a square's low columns: every step is doubled)
            assert best.get(k), (kind, k)
            found = best[k]
        out[k] = dict(below=found[0], ops=found[1], gap=1 if len(found) == 2 else found[2])
    return out


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "first_carry_rows.json")


def golden(kind):
    """directed(kind) as recorded in tests/golden/first_carry_rows.json (the
    builder takes about 20 s for the five kinds; the tests confirm every
    recorded row with the model, so a stale file fails them):
        python tests/first_carry_model.py       rewrites the file"""
    rows = json.load(open(GOLDEN))[kind]
    return {int(k): dict(ops=tuple(int(x, 16) for x in v["ops"]), below=tuple(int(x, 16) for x in v["below"]),
                         gap=v["gap"]) for k, v in rows.items()}


def all_ones(kind):
    return (M - 1,) * len(KINDS[kind][0])


def square_bit31_rows(kind, seed=0x5B1):
    """For the square kinds: a[7] with and without bit 31 (d[8] = 1 or 0, the
    free products against the 1-bit limb are a_i or 0), other limbs random and
    all ones."""
    rng = random.Random(seed)
    names, _ = KINDS[kind]
    rows = []
    for base in ("random", "ones"):
        for bit in (0, 1):
            ops = []
            for n in names:
                v = rng.getrandbits(256) if base == "random" else M - 1
                if n in SQUARE_OPERANDS.get(kind, ()):
                    v = (v & ~(1 << 255)) | (bit << 255)
                ops.append(v)
            rows.append(tuple(ops))
    return rows


def walk_np(kind, ops):
    """walk() for numpy: ops are uint64 arrays of shape (8, n) (limbs below
    2^32). -> (bool array: the lane's rare bit, the o limbs (8, n), T) for
    bulk random checks."""
    import numpy as np
    names, table = KINDS[kind]
    val = dict(zip(names, ops))
    u = np.uint64
    arr = {}
    for name, (src, role) in table.items():
        a = val[src]
        if role == "x":
            arr[name] = a
        elif role == "e":
            arr[name] = (a << u(1)) & u(W32)
        else:
            d = np.zeros((9,) + a.shape[1:], dtype=np.uint64)
            d[2:8] = ((a[2:8] << u(1)) | (a[1:7] >> u(31))) & u(W32)
            d[8] = a[7] >> u(31)
            arr[name] = d
    e = val.get("e") if kind == "mul256_red_add_ps_fc" else None
    n = ops[0].shape[1]
    zero = np.zeros(n, dtype=np.uint64)
    acc, top, h78 = zero, zero, None
    h, o = [], []
    rare_bits = np.zeros(n, dtype=bool)
    for k, prods in SCHEDULES[kind]:
        if k == 0:
            h78 = acc
            h += [acc & u(W32), acc >> u(32)]
            a = h[0] * u(977) + (e[0] if e is not None else u(0))
        elif k < 8:
            a = (acc >> u(32)) + ((top << u(32)) | h[k - 1]) + h[k] * u(977) + (e[k] if e is not None else u(0))
        else:
            a = acc
        t = zero.copy()
        for x, y, cls in prods:
            (xn, xi), (yn, yi) = (nm[:-1].split("[") for nm in (x, y))
            pr = arr[xn][int(xi)] * arr[yn][int(yi)]
            a = a + pr
            c = a < pr
            if cls == "free":
                assert not c.any()
            elif cls == "check":
                rare_bits |= c
            else:
                t = t + c.astype(np.uint64)
        top = t
        if k >= 8:
            h.append(a & u(W32))
            acc = (a >> u(32)) | (t << u(32))
        else:
            o.append(a & u(W32))
            acc = a
    if kind in SUM_KINDS:
        T = h[8] * u(977) + h78 + ((top << u(32)) | (acc >> u(32)))
    else:
        T = (acc >> u(32)) + (top << u(32)) + h[7]
    return rare_bits, np.stack(o), T


if __name__ == "__main__":
    out = {}
    for kind_ in sorted(KINDS):
        out[kind_] = {str(k): dict(ops=[hex(x) for x in v["ops"]], below=[hex(x) for x in v["below"]], gap=v["gap"])
                      for k, v in directed(kind_).items()}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
