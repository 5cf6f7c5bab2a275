"""GPU tests with chosen scalars through the production verify path.

Tables: hkv_gtable_kernel's 14 fixed-base tables are read by gsum_lane with
the radix-2^20 Booth digits of u1 = m / s. oracle/secp_fast.c's
hkvo_fast_gtable_records builds valid records whose u1 is j 2^off exactly, so
one batch reads every entry a scalar can reach of one table, each by a
signature that is valid only if the entry is right: a wrong entry shows as
that (t, j). (A copy of every 16th record with one bit of msg32 flipped is
appended rather than put in the record's place, so that no entry is left to a
record that is rejected anyway.) A table's batch is above half the resident
grid: the table / chain launches and hkv_finish_kernel.

Recoding: the directed set S (tests/chosen_scalars.py; its digit coverage is
asserted on the CPU in tests/test_chosen_scalars.py) on the four launch
shapes (block kernel, pair kernel, mid-size instance, table / chain launches),
both modes.

Expected verdicts are the host checker's (oracle/secp_fast.c, whose w = 15
wNAF tables and 5 x 52 field share nothing with the kernels') on every
record, and by construction: built records valid, flipped twins not."""
import numpy as np
import pytest

import chosen_scalars as cs
import launch_shapes
import recoding as rc
from conftest import fast_batch, host_threads

pytestmark = pytest.mark.gpu

SEED = 0x43485343


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
def lib(secpfast):
    return cs.bind(secpfast)


def verify_bits(torch, ver, recs, mode):
    from hkv import adversarial
    n = len(recs) // 168
    d = torch.from_numpy(recs if recs.flags.writeable else recs.copy()).cuda()
    words = torch.zeros((n + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    ver.verify_device(0, d.data_ptr(), n, mode, words.data_ptr())
    torch.cuda.synchronize()
    return adversarial.unpack_bits(words.cpu().numpy().view(np.uint32), n)


def check_sweep(torch, ver, lib, recs, label):
    """recs and their flipped twins in mode 0: the checker accepts exactly the
    unflipped ones, and the GPU equals it; label(i) names record i."""
    batch, twin_of = cs.with_flipped_twins(recs, SEED)
    exp = fast_batch(lib, batch, 0, threads=host_threads())
    wrong = np.nonzero(exp != (twin_of < 0))[0]
    assert wrong.size == 0, ("checker", [label(i if twin_of[i] < 0 else twin_of[i]) for i in wrong[:10]])
    got = verify_bits(torch, ver, batch, 0)
    mism = np.nonzero(got != exp)[0]
    assert mism.size == 0, [label(i) if twin_of[i] < 0 else label(twin_of[i]) + ("flipped",) for i in mism[:10]]


@pytest.mark.parametrize("t", range(14))
def test_every_entry_of_table(torch, ver, lib, t):
    """Entries 1..2^19 of tables 0..11 (n = 524,288 + 32,768 twins: the table and
    chain launches), 1..256 of tables 12 and 13 (all a half below 2^128 can read:
    tests/test_chosen_scalars.py)."""
    recs, js = cs.table_sweep(lib, t)
    assert len(js) == (rc.GTAB_ENTRIES if t < 12 else 256)
    check_sweep(torch, ver, lib, recs, lambda i: (t, int(js[i])))


def test_negative_digits_of_every_table(torch, ver, lib):
    """u1 = (2^20 - j) 2^off: entry j negated and entry 1 of the next window."""
    recs, ts, js = cs.negative_sweep(lib)
    assert len(js) == 12 * (3 + 8191)
    check_sweep(torch, ver, lib, recs, lambda i: (int(ts[i]), -int(js[i])))


@pytest.fixture(scope="module")
def directed(lib):
    """S and its flipped twins: (records, family names, accepted[n])."""
    names, u1, u2, d, pin = cs.directed_set()
    batch, twin_of = cs.with_flipped_twins(cs.chosen_records(lib, u1, u2, d, pin), SEED)
    batch.setflags(write=False)
    return batch, [names[i if t < 0 else t] + ("" if t < 0 else "/flipped") for i, t in enumerate(twin_of)], twin_of < 0


# The shape each n takes is the library's plan (haskoin-node_amd/csrc/hkv_launch_plan.h), asked through
# hkv_debug_launch_shape: hkv_block_kernel, hkv_pair_split_kernel, the mid-size hkv_ecmult_kernel instance,
# hkv_qtable_kernel + hkv_chain_kernel.
SHAPE_OF_N = {0: launch_shapes.BLOCK, 8_192: launch_shapes.PAIR, 33_024: launch_shapes.MID,
              131_136: launch_shapes.TABLE_CHAIN}


@pytest.mark.parametrize("n", [0, 8_192, 33_024, 131_136])
def test_directed_set_on_every_launch_shape(torch, ver, lib, directed, n):
    """S alone (1,835 records with the twins: the block kernel, which cuts each
    chain into three segments, each started from infinity), and shuffled into
    generated filler (5 % invalid) to n = 8,192 (the pair kernel: one chain
    over all 33 windows, so the first nonzero digit falls in any window of it),
    n = 33,024 (the mid-size instance) and n = 131,136 (table and chain
    launches): both modes, every verdict the checker's, every record of S
    accepted and every flipped twin rejected."""
    recs, names, accepted = directed
    ns = len(names)
    assert ns <= 4_096
    assert launch_shapes.records(ver, n or ns)[0] == SHAPE_OF_N[n]  # (S alone: a block-kernel batch)
    at = np.arange(ns)
    batch = recs
    if n:
        filler = torch.empty((n - ns) * 168, dtype=torch.uint8, device="cuda")
        ver.gen_batch_device(0, SEED + n, 0, n - ns, 65536, 100, 50, filler.data_ptr(), 0)
        torch.cuda.synchronize()
        at = np.sort(np.random.default_rng(SEED + n).choice(n, size=ns, replace=False))
        rows = np.empty((n, 168), dtype=np.uint8)
        rows[at] = recs.reshape(-1, 168)
        rows[np.setdiff1d(np.arange(n), at)] = filler.cpu().numpy().reshape(-1, 168)
        batch = rows.reshape(-1)
    where = {int(p): name for p, name in zip(at, names)}
    for mode in (0, 1):
        exp = fast_batch(lib, batch, mode, threads=host_threads())
        wrong = np.nonzero(exp[at] != accepted)[0]
        assert wrong.size == 0, ("checker", mode, [names[i] for i in wrong[:10]])
        if n:
            assert 0.04 < 1 - np.delete(exp, at).mean() < 0.06
        got = verify_bits(torch, ver, batch, mode)
        mism = np.nonzero(got != exp)[0]
        assert mism.size == 0, (mode, [(int(i), where.get(int(i), "filler")) for i in mism[:10]])
        assert (got[at] == accepted).all()
