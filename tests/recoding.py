"""The kernels' scalar recoding restated on Python integers (shared by
tests/test_oracle.py and the chosen-scalar tests): the GLV split of u2
(hkv_scalar.h glv_split), the Booth digits of its halves (hkv_kernels.hip
write_qdigits: radix 16, 33 windows), the merged top window of q_chain /
pair_chain, and the Booth digits of the halves of u1 against the fixed-base
tables (write_gdigits / gsum_lane: radix 2^20, 7 windows per half, table
t = 2 w + h)."""
import secp256k1_oracle as o

G1 = (2**384 * o.B2 + o.N // 2) // o.N
G2 = (2**384 * (-o.B1) + o.N // 2) // o.N

QW, NWIN = 4, 33          # hkv_layout.h: Q window bits, windows of a GLV half
GTAB_W, GWIN = 20, 7      # fixed-base radix, windows per half of u1
GTAB_ENTRIES = 1 << (GTAB_W - 1)


def glv_residues(k):
    """(k1, k2) in [0, n) with k1 + k2 lambda == k (mod n), as the rounding split leaves them."""
    c1 = (k * G1 + 2**383) >> 384
    c2 = (k * G2 + 2**383) >> 384
    k2 = (c1 * (-o.B1) + c2 * (-o.B2)) % o.N
    k1 = (k - k2 * o.LAMBDA) % o.N
    return k1, k2


def glv_split(k):
    """(|k1|, sign1, |k2|, sign2): k == sign1 |k1| + sign2 |k2| lambda (mod n)."""
    k1, k2 = glv_residues(k)
    s1 = -1 if k1 > o.N // 2 else 1
    s2 = -1 if k2 > o.N // 2 else 1
    return (o.N - k1 if s1 < 0 else k1), s1, (o.N - k2 if s2 < 0 else k2), s2


def glv_join(k1, k2):
    """The scalar of signed halves (k1, k2)."""
    return (k1 + k2 * o.LAMBDA) % o.N


def booth(k, w, nwin):
    digits = []
    for i in range(nwin):
        v = ((k << 1) >> (w * i)) & ((1 << (w + 1)) - 1)
        digits.append(((v + 1) >> 1) - ((v >> w) << w))
    return digits


def q_digits(mag):
    """The 33 radix-16 Booth digits (-8..8) of a half's magnitude (< 2^129)."""
    return booth(mag, QW, NWIN)


def top_digit(d):
    """The merged top window m = 16 d32 + d31 of a half's digits; the chains
    take it from the 8-entry table as min(m, 8) + (m - 8)+ when 0 <= m <= 16."""
    return 16 * d[32] + d[31]


def g_digits(u1):
    """Radix-2^20 Booth digits of u1's halves: ([7 of u1 mod 2^128], [7 of u1 >> 128])."""
    return booth(u1 & (2**128 - 1), GTAB_W, GWIN), booth(u1 >> 128, GTAB_W, GWIN)


def table_reads(u1):
    """{table t: signed digit} of the entries gsum_lane adds for u1 (entry |digit| of table t)."""
    lo, hi = g_digits(u1)
    reads = {}
    for w in range(GWIN):
        if lo[w]:
            reads[2 * w] = lo[w]
        if hi[w]:
            reads[2 * w + 1] = hi[w]
    return reads
