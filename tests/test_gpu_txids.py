"""GPU tests (MI355X) of txHash on device and the whole-block merkle check:
hkv_txid_kernel (csrc/hkv_sighash.hip) and hkv_block_verdict_kernel
(csrc/hkv_headers.hip) through the C ABI, byte-exact against the oracle
composition sha256d(tx_serialize(tx_parse(raw), with_witness=False)) that
tests/test_txids.py pins, and for witness txs also against hashlib over the
stripped serialisation of the Tx object (no parser involved).

Sizes are the smallest that reach each path: 301 lanes (64-thread groups),
16,555 lanes (past HKV_XSMALL = 16,384: 256-thread groups), stripped lengths
60..140 (every SHA-256 padding boundary up to two blocks), whole-range and
piecewise emission, and block batches on both sides of launch_merkle's
256-block route switch."""
import ctypes
import random

import numpy as np
import pytest

import merkle_oracle as mo
import sighash_oracle as sh
import txgen
import txid_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def ver(torch):
    import hkv
    v = hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1))
    yield v
    v.close()


@pytest.fixture(scope="module")
def rand_txs():
    """Case 2's 301 txs and their expected txids (computed once)."""
    txs = tc.random_txs()
    return txs, [tc.oracle_txid(t) for t in txs]


def upload(torch, arr: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def test_txid_known_answers(ver):
    import hkv
    kats = tc.kats()
    coinbases = [hkv.split_block(b) for b in tc.fixture_wire_blocks()]
    raws = [bytes.fromhex(k["raw"]) for k in kats] + [txs[0] for _, txs in coinbases]
    got, status = hkv.tx_ids(ver, raws)
    assert status == [hkv.HKV_TXID_OK] * len(raws)
    assert [g[::-1].hex() for g in got[:len(kats)]] == [k["txid"] for k in kats]
    assert got[len(kats):] == [h[36:68] for h, _ in coinbases]


def test_txid_random_vs_oracle(ver, rand_txs):
    import hkv
    txs, exp = rand_txs
    got, status = hkv.tx_ids(ver, txs)
    assert status == [0] * len(txs)
    bad = [k for k in range(len(txs)) if got[k] != exp[k]]
    assert not bad, [(k, len(txs[k]), got[k].hex(), exp[k].hex()) for k in bad[:5]]
    # the stripped form without any parser, for the witness txs
    for k in range(0, 300, 3):
        tx = sh.tx_parse(txs[k])
        assert any(len(w) for w in tx.witness)
        assert got[k] == tc.stripped_txid(tx) and got[k] != sh.sha256d(txs[k])


def test_txid_random_tiled_past_xsmall(ver, rand_txs):
    import hkv
    txs, exp = rand_txs
    got, status = hkv.tx_ids(ver, txs * 55)
    assert len(got) == 16555 and not any(status)
    bad = [k for k in range(len(got)) if got[k] != exp[k % len(txs)]]
    assert not bad, bad[:10]


def test_txid_padding_boundaries(ver):
    """Stripped lengths 60..140 cross 64, 119/120 and 127/128: where the 0x80
    byte and the length field do or do not fit the last block. The third form
    (output script length sent as FD ss 00) takes the piecewise path, with a
    piece boundary moving across the block boundary."""
    import hkv
    raws, exp = [], []
    for s in range(81):
        plain, wit = tc.padding_tx(s), tc.padding_tx(s, witness=True)
        for raw, tx in ((sh.tx_serialize(plain), plain), (sh.tx_serialize(wit), wit),
                        (tc.serialize_forms(plain, {("olen", 0): "fd"}), plain)):
            raws.append(raw)
            assert tc.oracle_txid(raw) == tc.stripped_txid(tx)
            exp.append(tc.oracle_txid(raw))
    assert len(raws) == 243 and len(set(raws)) == 243
    got, status = hkv.tx_ids(ver, raws)
    assert not any(status)
    bad = [(k // 3, k % 3) for k in range(243) if got[k] != exp[k]]
    assert not bad, bad[:10]


def test_txid_noncanonical_varints(ver):
    import hkv
    rng = random.Random(21)
    raws, exp = [], []
    for seg in (True, False):
        tx = txgen.rand_tx(rng, 2, 2, segwit=seg)
        tx.inputs[1].script = txgen.rand_script(rng, 25)
        tx.outputs[1].script = txgen.rand_script(rng, 23)
        keys = ["nin", ("slen", 1), "nout", ("olen", 1)]
        if seg:
            tx.witness = [[b"\x07" * 33, b""], [b"\x09" * 72]]
            keys += [("wcnt", 0), ("wlen", 1, 0)]   # dropped from the txid
        canon = sh.tx_serialize(tx)
        want = tc.stripped_txid(tx)
        assert tc.oracle_txid(canon) == want
        for key in keys:
            for form in ("fd", "fe", "ff"):
                nc = tc.serialize_forms(tx, {key: form})
                assert nc != canon and sh.tx_parse(nc) == tx
                assert tc.oracle_txid(nc) == want and sh.sha256d(nc) != want
                raws.append(nc)
                exp.append(want)
        raws.append(canon)
        exp.append(want)
    got, status = hkv.tx_ids(ver, raws)
    assert not any(status)
    assert got == exp


def test_txid_errors(ver):
    import hkv
    rng = random.Random(5)
    a = sh.tx_serialize(txgen.rand_tx(rng, 2, 2))
    b = sh.tx_serialize(txgen.rand_tx(rng, 1, 2, segwit=True))
    big_count = a[:4] + b"\xff\x02\x00\x00\x00\x01\x00\x00\x00" + a[5:]   # input count 2 + 2^32
    assert a[4] == 2
    raws = [a, a[:-5], b + b"\x00", a[:9], big_count, b]
    got, status = hkv.tx_ids(ver, raws)
    bad = hkv.HKV_TXID_BAD_TX
    assert status == [0, bad, bad, bad, bad, 0]
    assert got[1:5] == [bytes(32)] * 4
    assert got[0] == tc.oracle_txid(a) and got[5] == tc.oracle_txid(b)
    # an empty batch; a NULL status array
    assert hkv.tx_ids(ver, []) == ([], [])
    tb = hkv.TxBatch(raws)
    st, pool = tb.struct()
    out = np.zeros(len(raws) * 32, dtype=np.uint8)
    assert ver.lib.hkv_tx_ids(ver.ctx, ctypes.byref(st), out.ctypes.data, None) == 0
    assert out.tobytes() == b"".join(got)
    # offsets that decrease are an argument error of the host form
    tb.offsets[2] = tb.offsets[1] - 1
    assert ver.lib.hkv_tx_ids(ver.ctx, ctypes.byref(st), out.ctypes.data, None) == -1


def test_txid_device_form_on_a_side_stream(torch, ver, rand_txs):
    import hkv
    txs, _ = rand_txs
    host, host_status = hkv.tx_ids(ver, txs)
    tb = hkv.TxBatch(txs)
    d_bytes, d_off = upload(torch, tb.bytes), upload(torch, tb.offsets)
    dt = hkv.HkvTxs(d_bytes.data_ptr(), d_off.data_ptr(), len(txs), None, 0)
    out = torch.full((len(txs) * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    status = torch.full((len(txs),), 0xEE, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    hkv.tx_ids_device(ver, 0, dt, out.data_ptr(), status.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert out.cpu().numpy().tobytes() == b"".join(host)
    assert status.cpu().numpy().tolist() == host_status


# --- whole blocks ---------------------------------------------------------------

def block_cases(rand_txs):
    """[(header, [raw tx], expected status, expected root, expected txids)]."""
    import hkv
    txs, ids = rand_txs
    idof = dict(zip(txs, ids))
    rng = random.Random(77)
    OK, MUT, BAD, EMPTY = hkv.HKV_BLK_MERKLE_OK, hkv.HKV_BLK_MUTATED, hkv.HKV_BLK_BAD_TX, hkv.HKV_BLK_EMPTY
    cases = []

    def add(header, raws, status):
        t = [idof.get(r, bytes(32)) for r in raws]
        cases.append((header, list(raws), status, mo.merkle_root(t)[0], t))

    for b in tc.fixture_wire_blocks():   # the reference's own blocks
        header, raws = hkv.split_block(b)
        idof[raws[0]] = tc.oracle_txid(raws[0])
        add(header, raws, OK)
    synth, at = {}, 0
    for n in (1, 2, 3, 5, 8, 257):
        raws = txs[at:at + n]
        at += n
        synth[n] = (tc.merkle_header(rng, [idof[r] for r in raws]), raws)
        add(*synth[n], OK)
    # one change each
    h5, r5 = synth[5]
    add(h5[:40] + bytes([h5[40] ^ 0x10]) + h5[41:], r5, 0)
    h3, r3 = synth[3]
    add(h3, r3 + [r3[2]], OK | MUT)
    h8, r8 = synth[8]
    add(h8, r8, OK)
    add(h8, r8[:4] + [r8[4][:-5]] + r8[5:], BAD)
    add(h8, r8, OK)
    add(rng.randbytes(80), [], EMPTY)
    h2, r2 = synth[2]
    add(h2, r2, OK)
    return cases


def run_check(ver, cases):
    import hkv
    status, roots, txids = hkv.check_blocks(ver, [(h, raws) for h, raws, _, _, _ in cases])
    assert status.tolist() == [c[2] for c in cases]
    assert roots == [c[3] for c in cases]
    assert txids == [c[4] for c in cases]
    return status


def test_blocks_reference_and_synthetic(ver, rand_txs):
    import hkv
    cases = block_cases(rand_txs)
    assert len(cases) < 256
    status = run_check(ver, cases)
    assert (status[:15] == hkv.HKV_BLK_MERKLE_OK).all()
    for (h, _, st, root, _) in cases[:21]:
        assert root == h[36:68]
    empty = [c for c in cases if not c[1]]
    assert empty and all(c[3] == bytes(32) for c in empty)


def test_blocks_past_the_merkle_route_switch(ver, rand_txs):
    """The same set plus 300 one-tx blocks: more blocks than the MI355X has
    CUs, so launch_merkle takes one workgroup per block."""
    import hkv
    txs, ids = rand_txs
    rng = random.Random(78)
    cases = block_cases(rand_txs)
    for k in range(300):
        cases.append((tc.merkle_header(rng, [ids[k]]), [txs[k]], hkv.HKV_BLK_MERKLE_OK, ids[k], [ids[k]]))
    rng.shuffle(cases)
    run_check(ver, cases)


def test_blocks_bad_offsets_are_argument_errors(ver, rand_txs):
    import hkv
    txs, _ = rand_txs
    tb = hkv.TxBatch(txs[:6])
    st, pool = tb.struct()
    headers = np.zeros(3 * 80, dtype=np.uint8)
    status = np.zeros(3, dtype=np.uint8)

    def call(offsets, n_blocks=3):
        off = np.array(offsets, dtype=np.uint32)
        return ver.lib.hkv_check_blocks(ver.ctx, ctypes.byref(st), off.ctypes.data, n_blocks, headers.ctypes.data,
                                        None, None, status.ctypes.data)

    assert call([0, 2, 4, 6]) == 0          # (txids_out and roots_out may be NULL)
    assert call([0, 4, 2, 6]) == -1         # decreasing
    assert call([0, 2, 4, 7]) == -1         # last entry above n_tx
    assert call([1, 2, 4, 6]) == -1         # does not start at 0
    assert call([0], 0) == 0                # no block


def test_blocks_device_form_matches_host(torch, ver, rand_txs):
    import hkv
    cases = block_cases(rand_txs)
    host_status = run_check(ver, cases)
    raws = [r for c in cases for r in c[1]]
    n, nb = len(raws), len(cases)
    tb = hkv.TxBatch(raws)
    boff = np.cumsum([0] + [len(c[1]) for c in cases]).astype(np.uint32)
    d_bytes, d_off, d_boff = upload(torch, tb.bytes), upload(torch, tb.offsets), upload(torch, boff)
    d_hdr = upload(torch, np.frombuffer(b"".join(c[0] for c in cases), dtype=np.uint8))
    dt = hkv.HkvTxs(d_bytes.data_ptr(), d_off.data_ptr(), n, None, 0)
    d_txids, d_scratch = (torch.full((n * 32,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2))
    d_roots = torch.full((nb * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    d_mut, d_status = (torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    hkv.check_blocks_device(ver, 0, dt, d_boff.data_ptr(), nb, d_hdr.data_ptr(), d_txids.data_ptr(),
                            d_scratch.data_ptr(), d_roots.data_ptr(), d_mut.data_ptr(), d_status.data_ptr(),
                            s.cuda_stream)
    s.synchronize()
    assert d_status.cpu().numpy().tolist() == host_status.tolist()
    assert d_roots.cpu().numpy().tobytes() == b"".join(c[3] for c in cases)
    assert d_txids.cpu().numpy().tobytes() == b"".join(t for c in cases for t in c[4])
