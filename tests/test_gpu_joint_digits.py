"""GPU tests of the joint radix-8 chain of the table and chain launches
(hkv_kernels.hip 2a with HKV_JOINT_DIGITS, hkv_joint_digits.h): the chain
launch's preamble (the known-answer op on chosen scalar pairs, against
tests/joint_digits.py), the 11-entry table build (the op's entries made
affine, against oracle/secp256k1_oracle.py), and verdicts at n = 131,136, the
smallest batch the suite runs through this shape: records whose split scalars
reach every class of Z[lambda] / 8 in every window 0..41, the adversarial
mutation, the chosen-scalar set, and the two-part plan. Expected verdicts are
oracle/secp_fast.c's on every record, or hkv.adversarial.mutate's labels."""
import os
import random

import numpy as np
import pytest

import chosen_scalars as cs
import joint_digits as jd
import launch_shapes
import recoding as rc
import secp256k1_oracle as o
from conftest import fast_batch, host_threads

pytestmark = pytest.mark.gpu

N = 131_136
SEED = 0x4A4F494E
OP_RECODE, OP_TABLE = 52, 53  # hkv_internal.h HKV_DBG_JOINT_RECODE, HKV_DBG_JOINT_TABLE


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def ver(torch):
    import hkv
    v = hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1))  # HKV_OPEN_NO_SELFCHECK
    assert launch_shapes.records(v, N)[0] == launch_shapes.TABLE_CHAIN
    yield v
    v.close()


@pytest.fixture(scope="module")
def lib(secpfast):
    return cs.bind(secpfast)


def debug_op(torch, ver, op, a, b):
    """uint32[n, 16] of the op on rows a, b (uint32[n, 8])."""
    n = a.shape[0]
    da = torch.from_numpy(a.view(np.int32)).cuda()
    db = torch.from_numpy(b.view(np.int32)).cuda()
    out = torch.zeros((n, 16), dtype=torch.int32, device="cuda")
    ver.debug_op(0, op, n, da.data_ptr(), db.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def limbs(v, count=8):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(count)]


def verify_bits(torch, ver, recs, mode, n=None):
    from hkv import adversarial
    n = len(recs) // 168 if n is None else n
    d = torch.from_numpy(recs if recs.flags.writeable else recs.copy()).cuda()
    words = torch.zeros((n + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    ver.verify_device(0, d.data_ptr(), n, mode, words.data_ptr())
    torch.cuda.synchronize()
    return adversarial.unpack_bits(words.cpu().numpy().view(np.uint32), n)


def filler(torch, ver, n, seed):
    """n generated records, 5 % invalid (host)."""
    d = torch.empty(n * 168, dtype=torch.uint8, device="cuda")
    ver.gen_batch_device(0, seed, 0, n, 65536, 100, 50, d.data_ptr(), 0)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def shuffled_into_filler(torch, ver, recs, seed):
    """(batch of N records, positions of recs in it): recs at seeded positions among generated filler."""
    ns = len(recs) // 168
    at = np.sort(np.random.default_rng(seed).choice(N, size=ns, replace=False))
    rows = np.empty((N, 168), dtype=np.uint8)
    rows[at] = recs.reshape(-1, 168)
    rows[np.setdiff1d(np.arange(N), at)] = filler(torch, ver, N - ns, seed).reshape(-1, 168)
    return rows.reshape(-1), at


def test_recode_op_on_chosen_pairs(torch, ver):
    """4,096 signed pairs below 2^129: small ones, the largest in every sign
    combination, 8^j +- 1, a negative zero, and random ones of several lengths."""
    rng = random.Random(SEED)
    pairs = [(a, b) for a in range(-8, 9) for b in range(-8, 9)]
    for top in (2**128 - 1, 2**129 - 1):
        pairs += [(sa * top, sb * top) for sa in (1, -1) for sb in (1, -1)]
    edge = [s * (8**j + d) for j in range(43) for d in (1, -1) for s in (1, -1)]
    pairs += [(v, w) for v, w in zip(edge, reversed(edge))] + [(v, 0) for v in edge] + [(0, v) for v in edge]
    while len(pairs) < 4096:
        bits = rng.choice((129, 128, 127, 64, 20))
        pairs.append((rng.randrange(-(2**bits) + 1, 2**bits), rng.randrange(-(2**bits) + 1, 2**bits)))
    assert len(pairs) == 4096
    a = np.array([limbs(abs(k1), 5) + [1 if k1 < 0 else 0, 0, 0] for k1, _ in pairs], dtype=np.uint32)
    b = np.array([limbs(abs(k2), 5) + [1 if k2 < 0 else 0, 0, 0] for _, k2 in pairs], dtype=np.uint32)
    zero = pairs.index((0, 0))  # with both sign flags set: a negative zero
    a[zero, 5] = b[zero, 5] = 1
    got = debug_op(torch, ver, OP_RECODE, a, b)
    exp = np.array([jd.joint_recode(k1, k2) for k1, k2 in pairs], dtype=np.uint32)
    bad = np.nonzero((got[:, :11] != exp).any(axis=1))[0]
    assert bad.size == 0, [pairs[i] for i in bad[:5]]


def test_table_op_entries_are_the_orbit_multiples(torch, ver):
    """64 keys: all 11 entries x | y equal (a + b lambda) k G."""
    rng = random.Random(SEED + 1)
    keys = [1, 2, o.N - 1] + [rng.randrange(1, o.N) for _ in range(61)]
    rows_a, rows_b, exp = [], [], []
    for k in keys:
        for j, (ra, rb) in enumerate(jd.REPS):
            x, y = o.point_mul((ra + rb * o.LAMBDA) % o.N * k % o.N, o.G)
            rows_a.append(limbs(k))
            rows_b.append([j] + [0] * 7)
            exp.append(limbs(x) + limbs(y))
    got = debug_op(torch, ver, OP_TABLE, np.array(rows_a, dtype=np.uint32), np.array(rows_b, dtype=np.uint32))
    bad = np.nonzero((got != np.array(exp, dtype=np.uint32)).any(axis=1))[0]
    assert bad.size == 0, [(hex(keys[i // 11]), i % 11) for i in bad[:5]]


def signed_halves(u2):
    m1, s1, m2, s2 = rc.glv_split(u2)
    return s1 * m1, s2 * m2


def test_every_class_in_every_window(torch, ver, lib):
    """2,048 records with seeded u2 (pinned; the key and u1 seeded fillers)
    among generated filler: on the CPU model their split scalars reach all 64
    classes in each of windows 0..41 (the classes of windows 42, 43 are
    printed); both modes, every verdict the checker's."""
    rng = random.Random(SEED + 2)
    u2 = [rng.randrange(1, o.N) for _ in range(2048)]
    seen = [set() for _ in range(jd.WINDOWS)]
    for k in u2:
        for w, row in enumerate(jd.joint_digits(*signed_halves(k))):
            seen[w].add((row[0] % 8, row[1] % 8))
    for w in range(42):
        assert len(seen[w]) == 64, (w, len(seen[w]))
    print("classes in window 42:", sorted(seen[42]), "window 43:", sorted(seen[43]))
    u1 = [rng.randrange(1, o.N) for _ in u2]
    d = [rng.randrange(1, o.N) for _ in u2]
    recs = cs.chosen_records(lib, u1, u2, d, [cs.PIN_U2] * len(u2))
    batch, at = shuffled_into_filler(torch, ver, recs, SEED + 2)
    for mode in (0, 1):
        exp = fast_batch(lib, batch, mode, threads=host_threads())
        assert exp[at].all() and 0.04 < 1 - np.delete(exp, at).mean() < 0.06
        got = verify_bits(torch, ver, batch, mode)
        mism = np.nonzero(got != exp)[0]
        assert mism.size == 0, (mode, mism[:10])


def test_adversarial_batch_both_modes(torch, ver):
    """hkv.adversarial.mutate of a valid batch (u1 = 0, zero GLV halves, ladder
    collisions, edge digits), against its labels."""
    from hkv import adversarial

    def valid(unc):
        d = torch.empty(N * 168, dtype=torch.uint8, device="cuda")
        ver.gen_records_device(0, SEED, N, 65536, unc, d.data_ptr())
        torch.cuda.synchronize()
        return d.cpu().numpy()

    adv, lab_lib, lab_hask, cls = adversarial.mutate(valid(100), seed=SEED, twin=valid(1000))
    for mode, lab in ((0, lab_lib), (1, lab_hask)):
        got = verify_bits(torch, ver, adv, mode)
        mism = np.nonzero(got != lab)[0]
        assert mism.size == 0, (mode, mism[:10], [adversarial.CLASSES[c] for c in cls[mism[:10]]])


@pytest.fixture(scope="module")
def directed_batch(torch, ver, lib):
    """The chosen-scalar set S with its flipped twins among filler: (batch, positions, accepted, names)."""
    names, u1, u2, d, pin = cs.directed_set()
    recs, twin_of = cs.with_flipped_twins(cs.chosen_records(lib, u1, u2, d, pin), SEED)
    batch, at = shuffled_into_filler(torch, ver, recs, SEED + 3)
    batch.setflags(write=False)
    return batch, at, twin_of < 0, [names[i if t < 0 else t] for i, t in enumerate(twin_of)]


@pytest.fixture(scope="module")
def directed_expected(lib, directed_batch):
    batch, at, accepted, names = directed_batch
    exp = {mode: fast_batch(lib, batch, mode, threads=host_threads()) for mode in (0, 1)}
    for e in exp.values():
        assert (e[at] == accepted).all()
    return exp


def test_chosen_scalar_set_in_filler(torch, ver, directed_batch, directed_expected):
    batch, at, accepted, names = directed_batch
    where = {int(p): name for p, name in zip(at, names)}
    for mode in (0, 1):
        got = verify_bits(torch, ver, batch, mode)
        mism = np.nonzero(got != directed_expected[mode])[0]
        assert mism.size == 0, (mode, [(int(i), where.get(int(i), "filler")) for i in mism[:10]])


def test_two_part_plan_gives_the_one_part_bitmap(torch, directed_batch, directed_expected):
    """Contexts opened with HKV_REC_PART = 0 and = half the padded batch: two
    parts on two streams, each with its own table slot; the bitmaps are equal
    bit for bit, and the checker's."""
    import ctypes

    import hkv

    def open_with_parts(part):
        old = os.environ.get("HKV_REC_PART")
        os.environ["HKV_REC_PART"] = str(part)
        try:
            return hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1))
        finally:
            if old is None:
                del os.environ["HKV_REC_PART"]
            else:
                os.environ["HKV_REC_PART"] = old

    batch = directed_batch[0]
    n_pad = (N + 255) // 256 * 256
    part = (n_pad // 2 + 511) // 512 * 512
    bits = {}
    for which, p in (("one", 0), ("two", part)):
        v = open_with_parts(p)
        try:
            a, b = ctypes.c_uint32(), ctypes.c_uint32()
            assert v.lib.hkv_debug_rec_parts(v.ctx, 0, N, ctypes.byref(a), ctypes.byref(b)) == 0
            assert (a.value, b.value) == ((n_pad, 1) if p == 0 else (part, 2))
            assert launch_shapes.records(v, N)[0] == launch_shapes.TABLE_CHAIN
            bits[which] = [verify_bits(torch, v, batch, mode) for mode in (0, 1)]
        finally:
            v.close()
    for mode in (0, 1):
        assert (bits["one"][mode] == bits["two"][mode]).all()
        assert (bits["two"][mode] == directed_expected[mode]).all()
