"""CPU tests of the txHash / whole-block path: the oracle composition every
txid test uses as its expectation is pinned first (the mainnet genesis
coinbase and the reference's 15 fixture blocks, whose one txid is the header's
merkle field: test/Haskoin/NodeSpec.hs:185-193), then the host block walk
(hkv.split_block) and the C ABI's behaviour without a device."""
import ctypes
import random

import pytest

import sighash_oracle as sh
import txgen
import txid_cases as tc


def test_oracle_txid_genesis_coinbase():
    for k in tc.kats():
        raw = bytes.fromhex(k["raw"])
        assert tc.oracle_txid(raw)[::-1].hex() == k["txid"]
    assert len(bytes.fromhex(tc.kats()[0]["raw"])) == 204


def test_oracle_txid_reference_blocks():
    import hkv
    blocks = tc.fixture_wire_blocks()
    assert len(blocks) == 15
    for b in blocks:
        header, txs = hkv.split_block(b)
        assert len(header) == 80 and len(txs) == 1
        assert tc.oracle_txid(txs[0]) == header[36:68]


def test_oracle_txid_drops_witness_and_recanonicalises():
    """A witness tx whose input count is sent as FF 02 00..: the txid is the
    canonical tx's and not SHA-256d of the wire bytes."""
    rng = random.Random(3)
    tx = txgen.rand_tx(rng, 2, 2, segwit=True)
    raw = sh.tx_serialize(tx)
    nc = tc.serialize_forms(tx, {"nin": "ff"})
    assert nc != raw and nc[6] == 0xFF
    assert tc.oracle_txid(nc) == tc.oracle_txid(raw) == tc.stripped_txid(tx)
    assert tc.oracle_txid(nc) != sh.sha256d(nc) and tc.oracle_txid(raw) != sh.sha256d(raw)


def _synthetic_block():
    rng = random.Random(11)
    txs = [sh.tx_serialize(txgen.rand_tx(rng, nin, nout, segwit=seg))
           for nin, nout, seg in ((1, 1, False), (2, 3, True), (3, 0, False), (1, 2, False), (17, 9, False))]
    return rng.randbytes(80), txs


def test_split_block_roundtrip():
    import hkv
    header, txs = _synthetic_block()
    assert hkv.split_block(tc.wire_block(header, txs)) == (header, txs)
    assert hkv.split_block(header + b"\x00") == (header, [])
    # a tx count sent as FD 05 00 is still a count of 5
    assert hkv.split_block(header + b"\xfd\x05\x00" + b"".join(txs)) == (header, txs)


def test_split_block_rejects_malformed():
    import hkv
    header, txs = _synthetic_block()
    good = tc.wire_block(header, txs)
    for cut in (1, 4, 5, 40, len(txs[-1]), len(good) - 80, len(good) - 79):
        with pytest.raises(ValueError):
            hkv.split_block(good[:-cut])      # truncated
    with pytest.raises(ValueError):
        hkv.split_block(good + b"\x00")       # a trailing byte
    with pytest.raises(ValueError):
        hkv.split_block(header + b"\x06" + b"".join(txs))  # 6 txs announced, 5 present
    with pytest.raises(ValueError):
        hkv.split_block(header + b"\xff" + b"\xff" * 8 + b"".join(txs))


def test_calls_without_a_device_are_rejected():
    import hkv
    import hkv.lib as hl
    lib = hkv.load_library()
    for name in ("hkv_tx_ids", "hkv_tx_ids_device", "hkv_check_blocks", "hkv_check_blocks_device"):
        assert name in hl.EXPORTS
    tb = hkv.TxBatch([bytes.fromhex(tc.kats()[0]["raw"])])
    st, pool = tb.struct()
    out = (ctypes.c_uint8 * 64)()
    assert lib.hkv_tx_ids(None, ctypes.byref(st), out, out) == -1
    assert lib.hkv_tx_ids_device(None, 0, ctypes.byref(st), out, out, None) == -1
    assert lib.hkv_check_blocks(None, ctypes.byref(st), out, 1, out, out, out, out) == -1
    assert lib.hkv_check_blocks_device(None, 0, ctypes.byref(st), out, 1, out, out, out, out, out, out, None) == -1
    assert lib.hkv_version() >> 16 == 1
    assert lib.hkv_version() & 0xFFFF >= 1   # the minor half counts the additions to the ABI
