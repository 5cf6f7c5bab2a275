"""Big-integer restatement of the joint table build (csrc/hkv_kernels.hip
qtable_build_joint) in its two forms: the walk by nine mixed additions
(gej_add_ge_core, Q' read back at each step and a Z carried along) and the
walk by nine co-Z additions with update (hkv_group.h gej_zaddu, Qc = Q' kept
on the running point's Z). Values are integers mod p; the formulas never use
the curve's b, so a key may lie on any curve y^2 = x^3 + b.

A build takes Q = (x, y) and returns a Walk: the z-ratios H_2..H_10, the 11
entries (X, Y) on the common scale Zg, Zg itself, and what stands in the
registers after the walk.
"""
from __future__ import annotations

import os
import random
from collections import namedtuple

import joint_digits as jd

P = 2**256 - 2**32 - 977
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
STEPS = jd.build_steps()  # entry j = entry j - 1 + (-1)^s lambda^e Q': STEPS[j - 1] = (e, s)
ENTRIES = len(jd.REPS)

Walk = namedtuple("Walk", "H entries Zg qc")


class Degenerate(Exception):
    """a step met H = 0: the device's table holds garbage"""


def lane_q(x):
    """the table launch's Q' = (x w, w^2) on y^2 = x^3 + 7 w^3, w = x^3 + 7"""
    w = (x * x * x + 7) % P
    return x * w % P, w * w % P


def double_halved(x, y, z):
    """hkv_group.h gej_double: 2 (x, y, z) scaled by 1/2"""
    a, b = x * x % P, y * y % P
    m = x * b % P
    e = 3 * a * pow(2, -1, P) % P
    x3 = (e * e - 2 * m) % P
    return x3, (e * (m - x3) - b * b) % P, y * z % P


def start(q):
    """(X, Y of 2Q, Z2, Q' = phi_Z2(Q)): the two points on one Z"""
    x2, y2, z2 = double_halved(q[0], q[1], 1)
    return x2, y2, z2, (q[0] * z2 * z2 % P, q[1] * pow(z2, 3, P) % P)


def unit_image(x, y, e, s):
    return x * pow(BETA, e, P) % P, (-y) % P if s else y


def mixed_add(x1, y1, z1, bx, by):
    """gej_add_ge_core: (x1, y1, z1) + (bx, by), the z-ratio H"""
    z2 = z1 * z1 % P
    h = (bx * z2 - x1) % P
    r = (by * z2 * z1 - y1) % P
    if h == 0:
        raise Degenerate
    hh = h * h % P
    hhh = hh * h % P
    v = x1 * hh % P
    x3 = (r * r - hhh - 2 * v) % P
    return x3, (r * (v - x3) - y1 * hhh) % P, z1 * h % P, h


def zaddu(px, py, rx, ry):
    """gej_zaddu: (X3, Y3), P on the new Z as (W1, A1), H, C"""
    h = (px - rx) % P
    if h == 0:
        raise Degenerate
    c = h * h % P
    w1, w2 = px * c % P, rx * c % P
    d = (py - ry) % P
    a1 = py * (w1 - w2) % P
    x3 = (d * d - w1 - w2) % P
    return x3, (d * (w1 - x3) - a1) % P, w1, a1, h, c


def rescale(raw, H):
    """pass 2: raw entry j (j = 0..10, on its own Z) times rho_j = prod_{k > j} H_k; rho_1"""
    out, rho = [None] * ENTRIES, 1
    out[ENTRIES - 1] = raw[ENTRIES - 1]
    for j in range(ENTRIES - 2, -1, -1):
        if j >= 1:
            rho = rho * H[j + 1] % P
        if raw[j] is not None:
            out[j] = (raw[j][0] * rho * rho % P, raw[j][1] * pow(rho, 3, P) % P)
    return out, rho


def walk_mixed(q):
    """the build by mixed additions: Zg = Z2 * Z of the last entry"""
    x, y, z2, qp = start(q)
    raw, H, z = [qp, (x, y)], {}, 1
    for j in range(2, ENTRIES):
        e, s = STEPS[j - 1]
        x, y, z, H[j] = mixed_add(x, y, z, *unit_image(qp[0], qp[1], e, s))
        raw.append((x, y))
    entries, _ = rescale(raw, H)
    return Walk(H, entries, z2 * z % P, None)


def walk_coz(q):
    """the build by co-Z additions: Qc carried, no Z; Zg = Z2 * rho_1; entry 0 = Qc"""
    x, y, z2, (xq, yq) = start(q)
    raw, H = [None, (x, y)], {}
    for j in range(2, ENTRIES):
        e, s = STEPS[j - 1]
        px, py = unit_image(xq, yq, e, s)
        x, y, w1, a1, H[j], _ = zaddu(px, py, x, y)
        xq = w1 * pow(BETA, (3 - e) % 3, P) % P  # beta^-e W1 = Xq C
        yq = (-a1) % P if s else a1
        raw.append((x, y))
    entries, rho = rescale(raw, H)
    entries[0] = (xq, yq)
    return Walk(H, entries, z2 * rho % P, (xq, yq))


def affine(entry, zg):
    zi = pow(zg, -1, P)
    return entry[0] * zi * zi % P, entry[1] * pow(zi, 3, P) % P


# ---- an independent affine group law (any b) for (a + b lambda) Q ----
def aff_add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        m = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        m = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (m * m - x1 - x2) % P
    return x3, (m * (x1 - x3) - y1) % P


def aff_mul(k, p):
    if k < 0:
        k, p = -k, (p[0], (-p[1]) % P)
    r = None
    while k:
        if k & 1:
            r = aff_add(r, p)
        p = aff_add(p, p)
        k >>= 1
    return r


def orbit_multiple(j, q):
    """(a + b lambda) Q for entry j's representative, lambda (x, y) = (beta x, y)"""
    a, b = jd.REPS[j]
    return aff_add(aff_mul(a, q), aff_mul(b, (q[0] * BETA % P, q[1])))


# ---- the key sets of the walk's tests ----
def on_curve(x):
    w = (x * x * x + 7) % P
    return w != 0 and pow(w, (P - 1) // 2, P) == 1


def edge_xs(golden_dir):
    """x just below p (all-ones upper limbs), small x, and the x of every key
    of tests/golden's special pool. On secp256k1 or on a twist: the walk does
    not ask. None meets H = 0 (x = 0 does: TWIST_X)."""
    xs = [P - 1, P - 2, P - 3, P - 2**32, 1, 2, 3]
    data = open(os.path.join(golden_dir, "special_pool.bin"), "rb").read()
    for i in range(0, len(data), 168):
        x = int.from_bytes(data[i + 98:i + 130], "big")  # msg32 | sig64 | len | prefix | x
        if 0 < x < P and x not in xs:
            xs.append(x)
    return xs


def random_xs(count, seed):
    """x of seeded random keys on secp256k1"""
    rng, xs = random.Random(seed), []
    while len(xs) < count:
        x = rng.randrange(1, P)
        if on_curve(x):
            xs.append(x)
    return xs


TWIST_X = 0  # Q' = (0, 49) has order 3 on y^2 = x^3 + 7^4 (7 is no square mod p): H_2 = 0
