"""Batch verifyStdTx for whole blocks — ``hkv_verify_block_txs*``: the txs of
one or more blocks in block order plus, per tx, the prevouts the caller has
(its UTXO hits). An input whose prevout is not in its tx's list is looked up
among the EARLIER txs of the batch by the device-computed txHash
(csrc/hkv_blocktx.hip: a txid table, a lookup per unmatched input, a walk to
the parent's output), so the caller parses, hashes and copies nothing. The
rule is stated in include/hkv.h.

    verify_block_txs(v, raw_txs, prevouts, forkid) -> [bool]
    verify_block_txs_detail(...) -> ([tx verdict], [[input verdict]], [[input src]])
        src: HKV_SRC_LIST, HKV_SRC_NONE, or the index of the parent tx.

The device-pointer forms need the script pool behind the tx bytes in one
buffer; ``block_layout`` builds it.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .lib import HKV_SRC_LIST, HKV_SRC_NONE, check
from .records import unpack_bits
from .sighash import TxBatch
from .stdtx import Prevout, _device_run, _forkid, _ptr, pack_prevouts


def txid_table_slots(v, n_tx: int) -> int:
    """hkv_txid_table_slots: the slot count of the txid table for n_tx txs."""
    return int(v.lib.hkv_txid_table_slots(n_tx))


def block_layout(tb: TxBatch) -> Tuple[np.ndarray, int]:
    """(buffer, pool_at): tb's tx bytes, zero padding up to a multiple of 4,
    then tb's script pool — the one address range the block entry points
    read. Call after every script has gone into tb's pool."""
    _, pool = tb.struct()
    n = int(tb.offsets[-1])
    pool_at = (n + 3) // 4 * 4
    buf = np.zeros(max(1, pool_at + tb._len), dtype=np.uint8)
    buf[:n] = tb.bytes[:n]
    buf[pool_at:pool_at + tb._len] = pool[:tb._len]
    return buf, pool_at


def debug_txid_hash_mask(v, dev: int, mask: int) -> None:
    """hkv_debug_txid_hash_mask (test hook): AND the table's slot hash with mask."""
    check(v.lib.hkv_debug_txid_hash_mask(v.ctx, dev, mask & 0xFFFFFFFF), "hkv_debug_txid_hash_mask", v.lib)


def txid_index_device(v, dev: int, d_txids: int, n_tx: int, d_table: int, n_slots: int, stream: int = 0) -> None:
    """hkv_txid_index_device: build the table over n_tx device txids."""
    check(v.lib.hkv_txid_index_device(v.ctx, dev, _ptr(d_txids), n_tx, _ptr(d_table), n_slots, _ptr(stream)),
          "hkv_txid_index_device", v.lib)


def txid_lookup_device(v, dev: int, d_txids: int, n_tx: int, d_table: int, n_slots: int, d_queries: int, n_q: int,
                       d_found: int, stream: int = 0) -> None:
    """hkv_txid_lookup_device: d_found[q] = the smallest tx index whose txid is
    query q, or 0xFFFFFFFF."""
    check(v.lib.hkv_txid_lookup_device(v.ctx, dev, _ptr(d_txids), n_tx, _ptr(d_table), n_slots, _ptr(d_queries), n_q,
                                       _ptr(d_found), _ptr(stream)), "hkv_txid_lookup_device", v.lib)


def block_tx_jobs_device(v, dev: int, d_txs, d_prev_offsets: int, d_prev_outpoints: int, d_prev_scripts: int,
                         d_prev_values: int, n_inputs: int, d_txids: int, d_table: int, n_slots: int,
                         d_input_first: int, d_jobs: int, d_input_src: int, d_status: int, stream: int = 0) -> None:
    """hkv_block_tx_jobs_device: the prevout provider alone (txids, table,
    counts, one job and one src word per input). Enqueued, not synchronised."""
    rc = v.lib.hkv_block_tx_jobs_device(v.ctx, dev, ctypes.byref(d_txs), _ptr(d_prev_offsets), _ptr(d_prev_outpoints),
                                        _ptr(d_prev_scripts), _ptr(d_prev_values), n_inputs, _ptr(d_txids),
                                        _ptr(d_table), n_slots, _ptr(d_input_first), _ptr(d_jobs), _ptr(d_input_src),
                                        _ptr(d_status), _ptr(stream))
    check(rc, "hkv_block_tx_jobs_device", v.lib)


def verify_block_txs_device(v, dev: int, d_txs, d_prev_offsets: int, d_prev_outpoints: int, d_prev_scripts: int,
                            d_prev_values: int, forkid: int, n_inputs: int, d_txids: int, d_table: int, n_slots: int,
                            d_input_first: int, d_jobs: int, d_input_src: int, d_records: int, d_input_bits: int,
                            d_tx_bits: int, d_status: int, stream: int = 0) -> None:
    """hkv_verify_block_txs_device: provider, standard-input verify and per-tx
    reduction enqueued on ``stream`` with no host wait."""
    rc = v.lib.hkv_verify_block_txs_device(v.ctx, dev, ctypes.byref(d_txs), _ptr(d_prev_offsets),
                                           _ptr(d_prev_outpoints), _ptr(d_prev_scripts), _ptr(d_prev_values), forkid,
                                           n_inputs, _ptr(d_txids), _ptr(d_table), n_slots, _ptr(d_input_first),
                                           _ptr(d_jobs), _ptr(d_input_src), _ptr(d_records), _ptr(d_input_bits),
                                           _ptr(d_tx_bits), _ptr(d_status), _ptr(stream))
    check(rc, "hkv_verify_block_txs_device", v.lib)


def _split(flat, first, n_tx):
    return [flat[int(first[t]): int(first[t + 1])] for t in range(n_tx)]


class _HostCall:
    """What the host forms of the block calls share: the batch as the C ABI
    takes it (``head``: ctx, txs, the four prevout arrays) and the output
    arrays of hkv_verify_block_txs (``outs``: tx words, input_first,
    input_src; ``cap``: the room of input_src)."""

    def __init__(self, verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]]):
        if len(prevouts) != len(txs):
            raise ValueError("one prevout list per tx")
        self.n_tx = n_tx = len(txs)
        tb = TxBatch(txs)
        packed = pack_prevouts(tb, prevouts)
        st, pool = tb.struct()
        self._keep = (tb, packed, st, pool)
        self.head = (verifier.ctx, ctypes.byref(st)) + tuple(a.ctypes.data for a in packed)
        self.words = np.zeros(max(1, (n_tx + 31) // 32), dtype=np.uint32)
        self.first = np.zeros(n_tx + 1, dtype=np.uint32)
        self.cap = int(tb.offsets[-1]) // 41 + 1   # (an input is at least 41 bytes of its tx)
        self.src = np.zeros(self.cap, dtype=np.uint32)
        self.outs = (self.words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), self.first.ctypes.data,
                     self.src.ctypes.data)

    def tx_ok(self) -> List[bool]:
        return unpack_bits(self.words, self.n_tx).tolist()

    def srcs(self) -> List[List[int]]:
        return _split(self.src.tolist(), self.first, self.n_tx)


def verify_block_txs_host(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]],
                          forkid: Optional[int] = None) -> Tuple[List[bool], List[List[int]]]:
    """hkv_verify_block_txs (the host form, first device, blocking):
    ([tx verdict], [[src of input i of tx t]])."""
    h = _HostCall(verifier, txs, prevouts)
    if h.n_tx == 0:
        return [], []
    rc = verifier.lib.hkv_verify_block_txs(*h.head, _forkid(forkid), *h.outs, h.cap)
    check(rc, "hkv_verify_block_txs", verifier.lib)
    return h.tx_ok(), h.srcs()


def verify_block_txs(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]],
                     forkid: Optional[int] = None) -> List[bool]:
    """Batch verifyStdTx over the txs of whole blocks, in block order: element
    t equals ``verifyStdTx net ctx tx_t (prevouts_t ++ the outputs of earlier
    txs of the batch that tx_t spends and prevouts_t lacks)``."""
    return verify_block_txs_host(verifier, txs, prevouts, forkid)[0]


def verify_block_txs_detail(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]],
                            forkid: Optional[int] = None, dev: int = 0
                            ) -> Tuple[List[bool], List[List[bool]], List[List[int]]]:
    """verify_block_txs with what the device form keeps readable: ([tx
    verdict], [[verdict of input i of tx t]], [[src of input i of tx t]]).
    Runs the device forms on torch-allocated buffers of the context's device
    ``dev`` (blocking): the count of hkv_std_tx_jobs_device with n_inputs = 0
    to learn the input total, then the composed call."""
    r = _device_run(verifier, txs, prevouts, forkid, dev, block=True)
    if r is None:
        return [], [], []
    n_tx = len(txs)
    return r.tx_ok, _split(r.input_ok, r.first, n_tx), _split(r.src.tolist(), r.first, n_tx)


__all__ = ["verify_block_txs", "verify_block_txs_host", "verify_block_txs_detail", "verify_block_txs_device",
           "block_tx_jobs_device", "txid_index_device", "txid_lookup_device", "txid_table_slots", "block_layout",
           "debug_txid_hash_mask", "HKV_SRC_LIST", "HKV_SRC_NONE"]
