"""Python restatement of csrc/hkv_joint_digits.h: the joint radix-8 digits of
a scalar k1 + k2 lambda over Z[lambda] (lambda^2 + lambda + 1 = 0).

An element a + b lambda is the pair (a, b). The six units are
(-1)^s lambda^e, e in {0, 1, 2}; on a curve point they act as
(x, y) -> (beta^e x, (-1)^s y). A digit is the minimal-norm representative of
a class of Z[lambda] / 8; the 63 non-zero classes fall into 11 orbits under
the units, one table entry each (REPS, in the table's build order).
"""
from __future__ import annotations

WINDOWS = 44          # digits per scalar pair: |k1|, |k2| < 2^129
WORDS = 11            # four 7-bit codes to a word
ZERO = 15             # the entry field of the zero digit
# one representative per orbit, each its predecessor plus a unit
REPS = [(1, 0), (2, 0), (3, 0), (4, 0), (4, 1), (3, 1), (2, 1), (3, 2), (4, 2), (4, 3), (5, 3)]


def norm(z):
    a, b = z
    return a * a - a * b + b * b


def mul_lambda(z):
    a, b = z
    return (-b, a - b)


def unit(z, e, s):
    """(-1)^s lambda^e z"""
    for _ in range(e):
        z = mul_lambda(z)
    return (-z[0], -z[1]) if s else z


def add(z, w):
    return (z[0] + w[0], z[1] + w[1])


def sub(z, w):
    return (z[0] - w[0], z[1] - w[1])


def build_steps():
    """[(e, s)]: entry j + 1 = entry j + (-1)^s lambda^e, j = 0..9."""
    steps = []
    for prev, cur in zip(REPS, REPS[1:]):
        d = sub(cur, prev)
        hit = [(e, s) for e in range(3) for s in range(2) if unit((1, 0), e, s) == d]
        assert len(hit) == 1, (prev, cur)
        steps.append(hit[0])
    return steps


def class_table():
    """{(k1 mod 8, k2 mod 8): (d1, d2, entry, e, s)}; the zero class maps to
    (0, 0, ZERO, 0, 0). Each orbit's digits are its representative times the
    units, so ties on the hexagon's boundary break the same way all round;
    4 = -4 mod 8, so that orbit takes the three unnegated ones."""
    tab = {(0, 0): (0, 0, ZERO, 0, 0)}
    for entry, rep in enumerate(REPS):
        for e in range(3):
            for s in range(2):
                if rep == (4, 0) and s:
                    continue
                d = unit(rep, e, s)
                c = (d[0] % 8, d[1] % 8)
                assert c not in tab, (rep, e, s)
                tab[c] = (d[0], d[1], entry, e, s)
    assert len(tab) == 64
    return tab


TABLE = class_table()


def code_of(row):
    _, _, entry, e, s = row
    return entry | (e << 4) | (s << 6)


def table_words():
    """The header's 64 constants, index (k1 mod 8) * 8 + (k2 mod 8):
    code | (d1 + 8) << 7 | (d2 + 8) << 11."""
    out = []
    for c1 in range(8):
        for c2 in range(8):
            row = TABLE[(c1, c2)]
            out.append(code_of(row) | ((row[0] + 8) << 7) | ((row[1] + 8) << 11))
    return out


def joint_digits(k1, k2):
    """The 44 digit rows (d1, d2, entry, e, s), lowest window first."""
    rows = []
    for _ in range(WINDOWS):
        row = TABLE[(k1 % 8, k2 % 8)]
        rows.append(row)
        k1 = (k1 - row[0]) // 8
        k2 = (k2 - row[1]) // 8
    assert (k1, k2) == (0, 0), "more than 44 digits"
    return rows


def joint_recode(k1, k2):
    """The 11 packed words of joint_digits (window w: bits 7 (w % 4) of word w // 4)."""
    words = [0] * WORDS
    for w, row in enumerate(joint_digits(k1, k2)):
        words[w // 4] |= code_of(row) << (7 * (w % 4))
    return words


def decode(words):
    """[(entry, e, s)] of 11 packed words."""
    out = []
    for w in range(WINDOWS):
        c = (words[w // 4] >> (7 * (w % 4))) & 127
        out.append((c & 15, (c >> 4) & 3, c >> 6))
    return out


def value_of(words):
    """(k1, k2) that 11 packed words stand for."""
    k = (0, 0)
    for entry, e, s in reversed(decode(words)):
        k = (8 * k[0], 8 * k[1])
        if entry != ZERO:
            k = add(k, unit(REPS[entry], e, s))
    return k


def twos160(k):
    """five little-endian 32-bit words of k in two's complement"""
    k &= (1 << 160) - 1
    return [(k >> (32 * i)) & 0xFFFFFFFF for i in range(5)]
