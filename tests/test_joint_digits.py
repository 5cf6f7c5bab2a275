"""CPU tests of the joint radix-8 digits over Z[lambda] (tests/joint_digits.py,
the restatement of csrc/hkv_joint_digits.h): the class table's structure, the
recoding's value and length, the table build's walk, the digits' action on
points (oracle/secp256k1_oracle.py), and the header itself, compiled with
tests/joint_digits.cpp under ASan and UBSan, on the golden rows the model
wrote (tests/golden/joint_digits_rows.json)."""
import json
import os
import random
import subprocess

import joint_digits as jd
import secp256k1_oracle as o
from conftest import GOLDEN, ROOT

UNITS = [(e, s) for e in range(3) for s in range(2)]
SEED = 0x4A44


def directed_pairs():
    """All of [-64, 64]^2, +-(2^128 - 1) and +-(2^129 - 1) in every sign
    combination, and k_i = +-(8^j +- 1)."""
    pairs = [(a, b) for a in range(-64, 65) for b in range(-64, 65)]
    for top in (2**128 - 1, 2**129 - 1):
        pairs += [(sa * top, sb * top) for sa in (1, -1) for sb in (1, -1)]
        pairs += [(sa * top, 0) for sa in (1, -1)] + [(0, sb * top) for sb in (1, -1)]
    edge = [s * (8**j + d) for j in range(43) for d in (1, -1) for s in (1, -1)]
    pairs += [(v, 0) for v in edge] + [(0, v) for v in edge] + [(v, w) for v, w in zip(edge, reversed(edge))]
    return pairs


def random_pairs(count, seed=SEED):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        bits = rng.choice((129, 129, 128, 127, 64, 12))
        out.append((rng.randrange(-(2**bits) + 1, 2**bits), rng.randrange(-(2**bits) + 1, 2**bits)))
    return out


def test_class_table_has_eleven_orbits_closed_under_the_units():
    tab = jd.TABLE
    assert len(tab) == 64 and tab[(0, 0)][2] == jd.ZERO
    digits = {c: row[:2] for c, row in tab.items() if c != (0, 0)}
    assert len(set(digits.values())) == 63
    orbits = {}
    for c, d in digits.items():
        orbits.setdefault(tab[c][2], set()).add(d)
    assert sorted(orbits) == list(range(11))
    assert sorted(len(v) for v in orbits.values()) == [3] + [6] * 10
    assert orbits[3] == {(4, 0), (0, 4), (-4, -4)}
    for c, d in digits.items():
        for e, s in UNITS:
            ud = jd.unit(d, e, s)
            uc = (ud[0] % 8, ud[1] % 8)
            # the unit image of a digit is the digit of the image's class (4 = -4 mod 8: up to sign there)
            if tab[c][2] == 3:
                assert digits[uc] in (ud, (-ud[0], -ud[1]))
            else:
                assert digits[uc] == ud
            assert tab[uc][2] == tab[c][2]


def test_each_digit_is_its_class_and_of_least_norm():
    for c, row in jd.TABLE.items():
        d = row[:2]
        assert (d[0] % 8, d[1] % 8) == c
        assert max(abs(d[0]), abs(d[1])) <= 5
        least = min(jd.norm((c[0] + 8 * i, c[1] + 8 * j)) for i in range(-2, 2) for j in range(-2, 2))
        assert jd.norm(d) == least
        if c != (0, 0):
            entry, e, s = row[2:]
            assert jd.unit(jd.REPS[entry], e, s) == d


def test_recoding_gives_the_pair_in_44_digits():
    for k1, k2 in directed_pairs() + random_pairs(100_000):
        words = jd.joint_recode(k1, k2)  # (asserts that nothing is left after 44 digits)
        assert all(w < 1 << 28 for w in words)
        assert jd.value_of(words) == (k1, k2), (k1, k2)


def test_build_walk_steps_are_units_and_hit_every_orbit_once():
    steps = jd.build_steps()  # (asserts that each step is one unit)
    assert len(steps) == 10 and jd.REPS[0] == (1, 0)
    assert [jd.TABLE[(a % 8, b % 8)][2:] for a, b in jd.REPS] == [(j, 0, 0) for j in range(11)]
    # the header's packed steps
    e_word = sum(e << (2 * j) for j, (e, _) in enumerate(steps))
    s_word = sum(s << j for j, (_, s) in enumerate(steps))
    assert (e_word, s_word) == ((1 << 6) | (2 << 12) | (1 << 16), (1 << 4) | (1 << 5) | (1 << 6))


def test_digit_times_point_is_the_unit_image_of_the_entry():
    """digit Q = (beta^e x, (-1)^s y) of (entry Q), for every digit."""
    for d in (1, 0xC0FFEE, o.N - 2):
        q = o.point_mul(d, o.G)
        for c, (d1, d2, entry, e, s) in jd.TABLE.items():
            if c == (0, 0):
                continue
            a, b = jd.REPS[entry]
            x, y = o.point_mul((a + b * o.LAMBDA) % o.N, q)
            img = (pow(o.BETA, e, o.P) * x % o.P, (o.P - y) % o.P if s else y)
            assert o.point_mul((d1 + d2 * o.LAMBDA) % o.N, q) == img, (c, d)


def golden_rows():
    with open(os.path.join(GOLDEN, "joint_digits_rows.json")) as f:
        return json.load(f)


def test_golden_rows_are_the_models():
    g = golden_rows()
    assert g["table"] == jd.table_words()
    assert len(g["rows"]) >= 1000
    for k1, k2, words in g["rows"]:
        assert jd.joint_recode(int(k1, 16), int(k2, 16)) == words


def test_header_under_sanitizers(tmp_path):
    """tests/joint_digits.cpp: the header's table and joint_recode on the golden rows."""
    exe = str(tmp_path / "joint_digits")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "joint_digits.cpp")], check=True)
    g = golden_rows()
    lines = [" ".join(f"{w:x}" for w in g["table"])]
    for k1, k2, words in g["rows"]:
        lines.append(" ".join([f"{v:x}" for v in jd.twos160(int(k1, 16)) + jd.twos160(int(k2, 16)) + words]))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"ok {len(g['rows'])} rows"
