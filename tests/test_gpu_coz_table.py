"""GPU tests of the joint table build by co-Z additions (hkv_kernels.hip
qtable_build_joint, hkv_group.h gej_zaddu): the known-answer op's entries and
Zg against the big-integer model (tests/coz_walk.py) in launches of 256 rows
(one full workgroup sharing the LDS parking of four z-ratios) and 320 rows (a
partial second workgroup), on keys given by x: x just below p, small x, the
special pool's keys, random ones; and verdicts at n = 131,136, the smallest
batch of the table and chain launches, on the adversarial mix with keys of
order 3 on a twist put in (H = 0 in the walk: the table holds anything, the
verdict is reject), against oracle/secp_fast.c on every record."""
import numpy as np
import pytest

import coz_walk as cw
import launch_shapes
from conftest import GOLDEN, fast_batch, host_threads

pytestmark = pytest.mark.gpu

N = 131_136
SEED = 0x434F5A
OP_TABLE = 53  # hkv_internal.h HKV_DBG_JOINT_TABLE
J_ZG = 15      # the op's row of Zg
BY_X = 1       # b's limb 1: a is the key's x


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


def limbs(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def table_op(torch, ver, rows):
    """uint32[n, 16] of op 53 on rows [(x, j)]"""
    a = np.array([limbs(x) for x, _ in rows], dtype=np.uint32)
    b = np.array([[j, BY_X] + [0] * 6 for _, j in rows], dtype=np.uint32)
    da = torch.from_numpy(a.view(np.int32)).cuda()
    db = torch.from_numpy(b.view(np.int32)).cuda()
    out = torch.zeros((len(rows), 16), dtype=torch.int32, device="cuda")
    ver.debug_op(0, OP_TABLE, len(rows), da.data_ptr(), db.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def row_sets():
    """(256 rows, 320 rows) of (x, j): each x edge with every entry and Zg, each
    key of the pool and each random key with one j in turn."""
    edges = cw.edge_xs(GOLDEN)
    full = [(x, j) for x in edges[:7] for j in list(range(cw.ENTRIES)) + [J_ZG]]
    pool = edges[7:]
    turn = list(range(cw.ENTRIES)) + [J_ZG]
    one = [(x, turn[i % 12]) for i, x in enumerate(pool + cw.random_xs(256, SEED))]
    cut = 256 - len(full)
    assert len(pool) > cut
    return full + one[:cut], full + one[cut:cut + 320 - len(full)]


def expected(rows):
    exp, memo = [], {}
    for x, j in rows:
        if x not in memo:
            memo[x] = cw.walk_coz(cw.lane_q(x))
        w = memo[x]
        exp.append(limbs(w.Zg) + [0] * 8 if j == J_ZG else sum((limbs(c) for c in cw.affine(w.entries[j], w.Zg)), []))
    return np.array(exp, dtype=np.uint32)


@pytest.mark.parametrize("which, count", [(0, 256), (1, 320)])
def test_table_op_against_the_model(torch, ver, row_sets, which, count):
    rows = row_sets[which]
    assert len(rows) == count
    got = table_op(torch, ver, rows)
    bad = np.nonzero((got != expected(rows)).any(axis=1))[0]
    assert bad.size == 0, [(hex(rows[i][0]), rows[i][1]) for i in bad[:5]]


def test_table_op_returns_on_a_twist_key_of_order_3(torch, ver):
    """H_2 = 0: whatever the rows hold, the launch returns, and its neighbours' rows are right."""
    rows = [(cw.TWIST_X, 0), (1, 0), (cw.TWIST_X, J_ZG), (1, J_ZG)]
    got = table_op(torch, ver, rows)
    assert (got[[1, 3]] == expected([rows[1], rows[3]])).all()


@pytest.fixture(scope="module")
def mixed_batch(torch, ver):
    """(the joint-digit test's adversarial batch with twist keys put in, their positions)"""
    from hkv import adversarial

    def valid(unc):
        d = torch.empty(N * 168, dtype=torch.uint8, device="cuda")
        ver.gen_records_device(0, 0x4A4F494E, N, 65536, unc, d.data_ptr())
        torch.cuda.synchronize()
        return d.cpu().numpy()

    adv = adversarial.mutate(valid(100), seed=0x4A4F494E, twin=valid(1000))[0].copy().reshape(N, 168)
    at = np.sort(np.random.default_rng(SEED).choice(N, size=64, replace=False))
    key = np.zeros(65, dtype=np.uint8)  # the compressed key of x = 0
    for i, pos in enumerate(at):
        key[0] = 2 + (i & 1)
        adv[pos, 96] = 33
        adv[pos, 97:162] = key
    return adv.reshape(-1), at


@pytest.mark.parametrize("mode", [0, 1])
def test_verdicts_on_the_adversarial_mix_with_twist_keys(torch, ver, secpfast, mixed_batch, mode):
    from hkv import adversarial
    batch, at = mixed_batch
    exp = fast_batch(secpfast, batch, mode, threads=host_threads())
    assert not exp[at].any() and exp.any() and not np.delete(exp, at).all()
    d = torch.from_numpy(batch).cuda()
    words = torch.zeros((N + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    ver.verify_device(0, d.data_ptr(), N, mode, words.data_ptr())
    torch.cuda.synchronize()
    got = adversarial.unpack_bits(words.cpu().numpy().view(np.uint32), N)
    assert not got[at].any()
    mism = np.nonzero(got != exp)[0]
    assert mism.size == 0, (mode, mism[:10])
