"""GPU test (MI355X) of the library's grow-only device scratch (hkv_api.cpp
DevBuf): on one fresh context every host form is called small -> larger ->
small, so each staging, intermediate, aux, verdict and multisig buffer is
allocated, regrown once (the old block freed while the context stays in use)
and then reused by a call that needs less than it holds. Every answer is
compared with the form's oracle.

Sizes are the smallest that regrow everything: 64 -> 4,160 records (past the
4,096 one block kernel launch takes on 256 CUs, so the pair kernel's aux rows
grow too), 1 -> 300 headers, 1 block of 1 tx -> 3 blocks of up to 33 txs, and
2 standard inputs -> a block of about 200 that includes the multisig cases."""
import random

import numpy as np
import pytest

import header_oracle as ho
import merkle_oracle as mo
import sighash_oracle as sh
import txid_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ver():
    import torch
    import hkv
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    v = hkv.Verifier(hkv.VerifierConfig(device_ids=[0]))
    yield v
    v.close()


def test_verify_records_regrow(ver, kat):
    import hkv
    recs, man = kat
    flat = np.frombuffer(b"".join(recs), dtype=np.uint8)

    def tiled(n):
        reps = (n + len(recs) - 1) // len(recs)
        return np.tile(flat, reps)[: n * 168], reps

    for mode, key in ((hkv.HKV_LIBSECP, "libsecp"), (hkv.HKV_HASKOIN, "haskoin")):
        labels = np.array([r[key] for r in man], dtype=bool)
        for n in (64, 4160, 64):
            data, reps = tiled(n)
            got, exp = ver.verify_records(data, mode), np.tile(labels, reps)[:n]
            assert (got == exp).all(), (key, n, np.nonzero(got != exp)[0][:10])


def test_check_headers_regrow(ver):
    import hkv
    from test_headers import make_headers, REGTEST
    hdrs = make_headers(300, seed=0x52454752)
    for case in (hdrs[:1], hdrs, hdrs[:1]):
        hashes, status = hkv.check_headers(ver, case, REGTEST, prev_hash=case[0][4:36])
        eh, es = ho.check_headers(case, REGTEST, prev_hash=case[0][4:36])
        assert hashes == eh
        assert status.tolist() == es


@pytest.fixture(scope="module")
def block_shapes():
    """(small, large): one block of 1 tx; three blocks of 33, 2 and 20 txs.
    Each block is (header committing to its txids, raw txs, txids)."""
    rng = random.Random(0x5247)
    txs = tc.random_txs()[:56]
    ids = [tc.oracle_txid(t) for t in txs]

    def block(lo, hi):
        return tc.merkle_header(rng, ids[lo:hi]), txs[lo:hi], ids[lo:hi]

    return [block(0, 1)], [block(1, 34), block(34, 36), block(36, 56)]


def test_merkle_roots_regrow(ver, block_shapes):
    import hkv
    for case in (block_shapes[0], block_shapes[1], block_shapes[0]):
        roots, mut = hkv.merkle_roots(ver, [ids for _, _, ids in case])
        assert roots == [mo.merkle_root(ids)[0] for _, _, ids in case]
        assert not mut.any()


def test_tx_ids_and_check_blocks_regrow(ver, block_shapes):
    import hkv
    for case in (block_shapes[0], block_shapes[1], block_shapes[0]):
        raws = [r for _, txs, _ in case for r in txs]
        got, status = hkv.tx_ids(ver, raws)
        assert status == [hkv.HKV_TXID_OK] * len(raws)
        assert got == [i for _, _, ids in case for i in ids]
        st, roots, txids = hkv.check_blocks(ver, [(h, txs) for h, txs, _ in case])
        assert st.tolist() == [hkv.HKV_BLK_MERKLE_OK] * len(case)
        assert roots == [mo.merkle_root(ids)[0] for _, _, ids in case]
        assert txids == [ids for _, _, ids in case]


def test_verify_std_inputs_regrow(ver, coracle):
    import torch
    import hkv
    from hkv import blockgen
    from test_sighash_oracle import multisig_verdicts
    # (signed on the device, through a context of its own: the one under test stays fresh)
    with hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1)) as gen:
        btxs, bjobs = blockgen.make_block(gen, torch, n_tx=20, seed=0x52475357, n_keys=256)
        mtxs, mjobs = blockgen.make_multisig_block(gen, torch, n_tx=160, seed=0x52475358, n_keys=256,
                                                   invalid_permille=250)
    raw = btxs + mtxs
    jobs = list(bjobs) + [(t + len(btxs), i, p, v) for (t, i, p, v) in mjobs]
    random.Random(0x5247).shuffle(jobs)
    assert 180 <= len(jobs) <= 16 * 256
    want = multisig_verdicts(coracle, [sh.tx_parse(t) for t in raw], jobs, None)
    assert all(w for w, (t, _, _, _) in zip(want, jobs) if t < len(btxs))
    assert 0 < sum(not w for w in want) < 80
    # the small batch: two single-signature inputs and their two txs alone, the
    # second's prevout script with its last byte changed
    (ta, ia, pa, va), (tb, ib, pb, vb) = bjobs[0], bjobs[1]
    raw2 = [raw[ta], raw[tb]]
    two = [(0, ia, pa, va), (1, ib, pb[:-1] + bytes([pb[-1] ^ 1]), vb)]
    want2 = multisig_verdicts(coracle, [sh.tx_parse(t) for t in raw2], two, None)
    assert want2 == [True, False]
    for txs, case, exp in ((raw2, two, want2), (raw, jobs, want), (raw2, two, want2)):
        assert hkv.verify_std_inputs(ver, txs, case, None) == exp
