"""Writes tests/golden/joint_digits_rows.json from the Python model
(tests/joint_digits.py): the 64 class constants and (k1, k2, 11 packed digit
words) rows, signed hex scalars. tests/joint_digits.cpp runs the header's
joint_recode against them; the GPU tests do not read them."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import joint_digits as jd  # noqa: E402


def main():
    rng = random.Random(0x4A445253)
    pairs = [(a, b) for a in range(-9, 10) for b in range(-9, 10)]
    for top in (2**128 - 1, 2**129 - 1):
        pairs += [(sa * top, sb * top) for sa in (1, -1) for sb in (1, -1)]
        pairs += [(top, 0), (-top, 0), (0, top), (0, -top)]
    edge = [s * (8**j + d) for j in range(43) for d in (1, -1) for s in (1, -1)]
    pairs += [(v, w) for v, w in zip(edge, reversed(edge))]
    for bits in (129, 128, 127, 96, 33, 32, 31):
        for _ in range(80):
            pairs.append((rng.randrange(-(2**bits) + 1, 2**bits), rng.randrange(-(2**bits) + 1, 2**bits)))
    rows = [[hex(k1), hex(k2), jd.joint_recode(k1, k2)] for k1, k2 in pairs]
    with open(os.path.join(HERE, "joint_digits_rows.json"), "w") as f:
        json.dump({"table": jd.table_words(), "rows": rows}, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
