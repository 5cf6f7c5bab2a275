"""Batch transaction hashes and whole-block merkle checks — host-side mirror
of haskoin-core ``txHash :: Tx -> TxHash`` [dep, haskoin-core-1.1.0] and of the
reference's block assertion on ``getBlocks`` results
(test/Haskoin/NodeSpec.hs:185-193, blocks from src/Haskoin/Node/Peer.hs:309-344):

    b.header.merkle == buildMerkleRoot (txHash <$> b.txs)

All hashing runs in libhkv's HIP kernels: hkv_txid_kernel (csrc/hkv_sighash.hip)
streams each tx's witness-stripped re-serialisation through SHA-256d, the
merkle kernels and hkv_block_verdict_kernel (csrc/hkv_headers.hip) take the
txids from HBM.

    tx_ids(v, raw_txs) -> ([32-byte txid, digest order], [HKV_TXID_* status])
    split_block(raw)   -> (header80, [raw_tx, ...])       (host walk of one wire block)
    check_blocks(v, [(header80, [raw_tx, ...])])
        -> (status: uint8[n_blocks] of HKV_BLK_* flags, [root], [[txid]])

txHash hashes the decoded and re-serialised tx: witness data is dropped and
non-canonical varints are re-emitted canonically. A tx that does not parse
gets 32 zero bytes and HKV_TXID_BAD_TX; its block gets HKV_BLK_BAD_TX.
"""
from __future__ import annotations

import ctypes
from typing import List, Sequence, Tuple

import numpy as np

from .lib import check
from .sighash import TxBatch


def _ptr(p: int):
    return ctypes.c_void_p(p) if p else None


def tx_ids(v, raw_txs: Sequence[bytes]) -> Tuple[List[bytes], List[int]]:
    """Batch txHash on the context's first device (blocking)."""
    n = len(raw_txs)
    tb = TxBatch(raw_txs)
    st, pool = tb.struct()
    out = np.zeros(max(1, n) * 32, dtype=np.uint8)
    status = np.zeros(max(1, n), dtype=np.uint8)
    rc = v.lib.hkv_tx_ids(v.ctx, ctypes.byref(st), out.ctypes.data, status.ctypes.data)
    check(rc, "hkv_tx_ids", v.lib)
    ob = out.tobytes()
    return [ob[32 * k: 32 * k + 32] for k in range(n)], [int(x) for x in status[:n]]


def tx_ids_device(v, dev: int, d_txs, d_txids: int, d_status: int = 0, stream: int = 0) -> None:
    """Device-pointer form: d_txs is an HkvTxs of device pointers; d_txids
    (n_tx * 32 bytes, 16-aligned) and d_status (n_tx bytes, or 0) in HBM of
    ``dev``. Enqueued on ``stream``, not synchronised."""
    rc = v.lib.hkv_tx_ids_device(v.ctx, dev, ctypes.byref(d_txs), _ptr(d_txids), _ptr(d_status), _ptr(stream))
    check(rc, "hkv_tx_ids_device", v.lib)


def _varint(b: bytes, off: int) -> Tuple[int, int]:
    if off >= len(b):
        raise ValueError("truncated varint")
    t = b[off]
    if t < 0xFD:
        return t, off + 1
    w = {0xFD: 2, 0xFE: 4, 0xFF: 8}[t]
    if len(b) - off < 1 + w:
        raise ValueError("truncated varint")
    return int.from_bytes(b[off + 1: off + 1 + w], "little"), off + 1 + w


def _skip(b: bytes, off: int, n: int) -> int:
    if n > len(b) - off:
        raise ValueError("truncated block")
    return off + n


def _tx_end(b: bytes, off: int) -> int:
    """End offset of the wire tx (BIP144 form allowed) that starts at off."""
    off = _skip(b, off, 4)
    seg = b[off: off + 2] == b"\x00\x01"
    if seg:
        off += 2
    nin, off = _varint(b, off)
    for _ in range(nin):
        off = _skip(b, off, 36)
        sl, off = _varint(b, off)
        off = _skip(b, off, sl + 4)
    nout, off = _varint(b, off)
    for _ in range(nout):
        off = _skip(b, off, 8)
        sl, off = _varint(b, off)
        off = _skip(b, off, sl)
    if seg:
        for _ in range(nin):
            cnt, off = _varint(b, off)
            for _ in range(cnt):
                il, off = _varint(b, off)
                off = _skip(b, off, il)
    return _skip(b, off, 4)


def split_block(raw: bytes) -> Tuple[bytes, List[bytes]]:
    """One wire block -> (80-byte header, [raw tx]): header, varint tx count,
    txs. ValueError on a malformed block or bytes after the last tx."""
    raw = bytes(raw)
    if len(raw) < 81:
        raise ValueError("truncated block")
    n, off = _varint(raw, 80)
    txs = []
    for _ in range(n):
        end = _tx_end(raw, off)
        txs.append(raw[off:end])
        off = end
    if off != len(raw):
        raise ValueError("bytes after the block's last tx")
    return raw[:80], txs


def _block_batch(blocks: Sequence[Tuple[bytes, Sequence[bytes]]]):
    nb = len(blocks)
    offsets = np.zeros(nb + 1, dtype=np.uint32)
    txs: List[bytes] = []
    for b, (hdr, btxs) in enumerate(blocks):
        if len(hdr) != 80:
            raise ValueError("a block header is 80 bytes")
        txs.extend(btxs)
        offsets[b + 1] = len(txs)
    headers = np.frombuffer(b"".join(h for h, _ in blocks) or b"\0", dtype=np.uint8).copy()
    return TxBatch(txs), offsets, headers


def check_blocks(v, blocks: Sequence[Tuple[bytes, Sequence[bytes]]]) -> Tuple[np.ndarray, List[bytes], List[List[bytes]]]:
    """The reference's block assertion for a batch of (header80, [raw tx])
    blocks, on the context's first device (blocking): HKV_BLK_* status per
    block, the computed roots and every block's txids."""
    nb = len(blocks)
    tb, offsets, headers = _block_batch(blocks)
    n = len(tb.offsets) - 1
    st, pool = tb.struct()
    txids = np.zeros(max(1, n) * 32, dtype=np.uint8)
    roots = np.zeros(max(1, nb) * 32, dtype=np.uint8)
    status = np.zeros(max(1, nb), dtype=np.uint8)
    rc = v.lib.hkv_check_blocks(v.ctx, ctypes.byref(st), offsets.ctypes.data, nb, headers.ctypes.data,
                                txids.ctypes.data, roots.ctypes.data, status.ctypes.data)
    check(rc, "hkv_check_blocks", v.lib)
    tbytes, rbytes = txids.tobytes(), roots.tobytes()
    ids = [[tbytes[32 * k: 32 * k + 32] for k in range(int(offsets[b]), int(offsets[b + 1]))] for b in range(nb)]
    return status[:nb].copy(), [rbytes[32 * b: 32 * b + 32] for b in range(nb)], ids


def check_blocks_device(v, dev: int, d_txs, d_block_offsets: int, n_blocks: int, d_headers: int, d_txids: int,
                        d_scratch: int, d_roots: int, d_mutated: int, d_status: int, stream: int = 0) -> None:
    """Device-pointer form (the block's tx buffer is the one a
    verify_std_inputs batch already uploaded); enqueued, not synchronised."""
    rc = v.lib.hkv_check_blocks_device(v.ctx, dev, ctypes.byref(d_txs), _ptr(d_block_offsets), n_blocks,
                                       _ptr(d_headers), _ptr(d_txids), _ptr(d_scratch), _ptr(d_roots),
                                       _ptr(d_mutated), _ptr(d_status), _ptr(stream))
    check(rc, "hkv_check_blocks_device", v.lib)


__all__ = ["tx_ids", "tx_ids_device", "split_block", "check_blocks", "check_blocks_device"]
