"""Records with exact scalars for the chosen-scalar tests (no test in here):
the ctypes side of oracle/secp_fast.c's record builders, and the directed set
S of (family, u1, u2, pin) whose digits tests/test_chosen_scalars.py checks for
coverage and tests/test_gpu_chosen_scalars.py runs on every launch shape.

The families are built from tests/recoding.py, the restatement of the kernels'
GLV split and Booth recoding. A pattern is asked of a half; what the rounding
split really makes of the scalar is what the coverage asserts read, so a
pattern that lies outside the split's parallelogram only lands elsewhere."""
import ctypes
import random

import numpy as np

import recoding as rc
import secp256k1_oracle as o

PIN_U1, PIN_U2, PIN_BOTH = 1, 2, 3
ERRORS = {1: "bad argument", 2: "u2 = 0", 3: "r = 0", 4: "R at infinity", 5: "redraws exhausted"}

# tests/golden/make_special_pool.py's edge_u1 / edge_u2 values
EDGES = [1, 2, o.N - 1, o.N - 2, o.LAMBDA, o.N - o.LAMBDA, 2**128 - 1, 2**128, 2**128 + 1, 2**129 + 3,
         2**255, o.N // 2, (o.N + 1) // 2, 0xFFFFFFFF]


def bind(lib):
    lib.hkvo_fast_chosen_records.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                             ctypes.c_size_t, ctypes.c_void_p]
    lib.hkvo_fast_chosen_records.restype = ctypes.c_longlong
    lib.hkvo_fast_gtable_records.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int,
                                             ctypes.c_void_p]
    lib.hkvo_fast_gtable_records.restype = ctypes.c_int
    lib.hkvo_fast_gtable_records_strided.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_size_t,
                                                     ctypes.c_int, ctypes.c_void_p]
    lib.hkvo_fast_gtable_records_strided.restype = ctypes.c_int
    return lib


def be(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def chosen_rc(lib, u1, u2, d, pin, out=None):
    """The builder's raw return: 0, or (record index, error code) of its first failure."""
    n = len(pin)
    out = np.zeros(n * 168, dtype=np.uint8) if out is None else out
    rc_ = lib.hkvo_fast_chosen_records(be(u1), be(u2), be(d), bytes(pin), n, out.ctypes.data)
    return (0 if rc_ == 0 else divmod(-rc_, 8)), out


def chosen_records(lib, u1, u2, d, pin):
    """uint8[n * 168]: record i verifies with u1[i] and / or u2[i] as pin[i] says."""
    err, out = chosen_rc(lib, u1, u2, d, pin)
    assert err == 0, (err[0], ERRORS.get(err[1], err[1]))
    return out


def gtable_records(lib, t, j0, count, neg=0, step=1):
    """uint8[count * 168]: record k has u1 = j 2^off (neg: (2^20 - j) 2^off), j = j0 + k step."""
    out = np.zeros(count * 168, dtype=np.uint8)
    rc_ = lib.hkvo_fast_gtable_records_strided(t, j0, step, count, neg, out.ctypes.data) if step != 1 else \
        lib.hkvo_fast_gtable_records(t, j0, count, neg, out.ctypes.data)
    assert rc_ == 0, (t, j0, count, neg, step, ERRORS.get(-rc_, rc_))
    return out


def scalars_of(rec):
    """(u1, u2) a verifier computes from a record with low s: m / s and r / s."""
    m = int.from_bytes(bytes(rec[0:32]), "big") % o.N
    r = int.from_bytes(bytes(rec[32:64]), "big")
    s = int.from_bytes(bytes(rec[64:96]), "big")
    si = pow(s, -1, o.N)
    return m * si % o.N, r * si % o.N


def flip_msg_bit(recs, idx, seed):
    """A copy of records idx with one bit of msg32 flipped in each."""
    rng = np.random.default_rng(seed)
    out = recs.reshape(-1, 168)[idx].copy()
    bit = rng.integers(0, 256, size=len(idx))
    out[np.arange(len(idx)), bit // 8] ^= (1 << (bit % 8)).astype(np.uint8)
    return out.reshape(-1)


# --------------------------------------------------------------------------
# the table sweeps

# Window 6 holds 8 bits of a half and the Booth carry, so its tables (12, 13)
# are read up to entry 256, and entry 256 only with a carry from below: the
# halves 2^128 - 1 and 2^128 - 2 (the largest u1 >> 128 below n)
ENTRY_256 = {12: 2**128 - 1, 13: (2**128 - 2) << 128}


def with_flipped_twins(recs, seed):
    """(records, twin_of): recs followed by a copy of every 16th record with one
    bit of msg32 flipped; twin_of[i] = index of the record i copies, -1 for recs."""
    n = len(recs) // 168
    idx = np.arange(0, n, 16)
    twin_of = np.concatenate([np.full(n, -1), idx])
    return np.concatenate([recs, flip_msg_bit(recs, idx, seed)]), twin_of


def table_sweep(lib, t):
    """(records, j[n]): one valid record per entry j of table t that a scalar can read."""
    if t < 12:
        return gtable_records(lib, t, 1, rc.GTAB_ENTRIES), np.arange(1, rc.GTAB_ENTRIES + 1)
    top = chosen_records(lib, [ENTRY_256[t]], [0x5EED + t], [0xD00D + t], [PIN_U1])
    return np.concatenate([gtable_records(lib, t, 1, 255), top]), np.arange(1, 257)


def negative_sweep(lib):
    """(records, t[n], j[n]): the negative form for j in {1, 2, 2^19 - 1} and every 64th j, tables 0..11."""
    recs, ts, js = [], [], []
    for t in range(12):
        for j0, step, count in ((1, 1, 2), (64, 64, rc.GTAB_ENTRIES // 64 - 1), (rc.GTAB_ENTRIES - 1, 1, 1)):
            recs.append(gtable_records(lib, t, j0, count, neg=1, step=step))
            js.append(j0 + step * np.arange(count))
            ts.append(np.full(count, t))
    return np.concatenate(recs), np.concatenate(ts), np.concatenate(js)


# --------------------------------------------------------------------------
# the directed set S

def _nibbles(pattern, count):
    return int((pattern * count)[:count], 16)


def u2_families():
    """[(family, u2)]: the u2-pinned part of S."""
    fam = []
    # one half zero, the other a single nibble d at window w: the chain starts
    # from infinity at that window. d = 1..7 is the digit d, d = 8..15 the digit
    # d - 16 with a carry of +1 into window w + 1
    for w in range(32):
        for d in range(1, 16):
            fam.append((f"nibble_k1_w{w}", d * 16**w))
            fam.append((f"nibble_k2_w{w}", d * 16**w * o.LAMBDA % o.N))
    # the corners (+-v1 +- v2) / 2 of the split's parallelogram, each +-3: the largest halves
    for sa in (1, -1):
        for sb in (1, -1):
            k1, k2 = (sa * o.A1 + sb * o.A2) // 2, (sa * o.B1 + sb * o.B2) // 2
            for delta in range(-3, 4):
                fam.append((f"corner_{sa:+d}{sb:+d}", (rc.glv_join(k1, k2) + delta) % o.N))
            # and down the diagonal to the corner: every merged top digit on the way
            for step in range(1, 64):
                fam.append((f"diagonal_{sa:+d}{sb:+d}", rc.glv_join(k1 * step // 64, k2 * step // 64)))
    # halves of all-8 nibbles, all-F nibbles (a carry through every window) and 8 / 7 alternating
    for name, pat in (("all8", "8"), ("allF", "F"), ("alt87", "87"), ("alt78", "78")):
        for count in (32, 31, 30):
            h = _nibbles(pat, count)
            for s1 in (1, -1):
                fam.append((f"{name}_k1", rc.glv_join(s1 * h, 0)))
                fam.append((f"{name}_k2", rc.glv_join(0, s1 * h)))
                for s2 in (1, -1):
                    fam.append((f"{name}_both", rc.glv_join(s1 * h, s2 * h)))
    for e in EDGES:
        fam.append(("edge_u2", e))
        fam.append(("edge_u2_neg", o.N - e))
    return fam


def q_coverage(u2s):
    """(digits[half][window] = set of Booth digits, tops[half] = set of merged top
    digits, signs[half] = set of signs, fallback = any top digit outside 0..16)."""
    digits = [[set() for _ in range(rc.NWIN)] for _ in range(2)]
    tops, signs, fallback = [set(), set()], [set(), set()], False
    for u2 in u2s:
        m1, s1, m2, s2 = rc.glv_split(u2)
        for h, (m, s) in enumerate(((m1, s1), (m2, s2))):
            d = rc.q_digits(m)
            for w in range(rc.NWIN):
                digits[h][w].add(d[w])
            tops[h].add(rc.top_digit(d))
            fallback = fallback or not 0 <= rc.top_digit(d) <= 16
            if m:
                signs[h].add(s)
    return digits, tops, signs, fallback


def u1_families():
    """[(family, u1)]: the u1-pinned part of S."""
    fam = []
    for name, h in (("ones", 2**128 - 1), ("top_window_max", 2**128 - 2**19), ("half_msb", 2**127)):
        fam.append((f"lo_{name}", h))
        fam.append((f"lo_{name}_hi1", h + 2**128))
        if h << 128 < o.N:
            fam.append((f"hi_{name}", h << 128))
    hi_max = (o.N - 1) >> 128  # 2^128 - 2
    fam += [("hi_max", hi_max << 128), ("hi_max_lo_max", o.N - 1), ("hi_max_lo_ones", (hi_max << 128) - 1)]
    for h in range(2):
        for w in range(rc.GWIN):
            off = rc.GTAB_W * w + 128 * h
            # window values around the digit -2^19 and its carry; window 6 holds 8 bits
            vals = (2**19 - 1, 2**19, 2**19 + 1) if w < 6 else (0x7F, 0x80, 0xFF - h)
            for v in (1,) + vals:
                fam.append((f"window_h{h}_w{w}", v << off))
            if w:  # +2^19 (window 6: +2^7): the window value below it with a carry in from the window before
                v = 2**19 - 1 if w < 6 else 0x7F
                fam.append((f"carry_h{h}_w{w}", (v << rc.GTAB_W | 2**19) << (off - rc.GTAB_W)))
    for e in EDGES:
        fam.append(("edge_u1", e))
        fam.append(("edge_u1_neg", o.N - e))
    assert all(0 < u1 < o.N for _, u1 in fam)
    return fam


def directed_set():
    """(families[n], u1[n], u2[n], d[n], pin[n]) of S; unpinned scalars and keys are seeded fillers."""
    rng = random.Random(0x43484F53)
    names, u1, u2, pin = [], [], [], []
    for name, k in u2_families():
        names.append(name), u1.append(rng.randrange(1, o.N)), u2.append(k), pin.append(PIN_U2)
    for name, k in u1_families():
        names.append(name), u1.append(k), u2.append(rng.randrange(1, o.N)), pin.append(PIN_U1)
    for _ in range(256):
        names.append("random_pair"), u1.append(rng.randrange(1, o.N)), u2.append(rng.randrange(1, o.N))
        pin.append(PIN_BOTH)
    d = [rng.randrange(1, o.N) for _ in names]
    return names, u1, u2, d, pin
