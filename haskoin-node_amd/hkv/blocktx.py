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

from .lib import HKV_SRC_LIST, HKV_SRC_NONE, HkvTxs, check
from .records import unpack_bits
from .sighash import TxBatch
from .stdtx import Prevout, _forkid, _ptr, pack_prevouts


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


def verify_block_txs_host(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]],
                          forkid: Optional[int] = None) -> Tuple[List[bool], List[List[int]]]:
    """hkv_verify_block_txs (the host form, first device, blocking):
    ([tx verdict], [[src of input i of tx t]])."""
    if len(prevouts) != len(txs):
        raise ValueError("one prevout list per tx")
    n_tx = len(txs)
    if n_tx == 0:
        return [], []
    tb = TxBatch(txs)
    offsets, outpoints, scripts, values = pack_prevouts(tb, prevouts)
    st, pool = tb.struct()
    words = np.zeros(max(1, (n_tx + 31) // 32), dtype=np.uint32)
    first = np.zeros(n_tx + 1, dtype=np.uint32)
    cap = int(tb.offsets[-1]) // 41 + 1   # (an input is at least 41 bytes of its tx)
    src = np.zeros(cap, dtype=np.uint32)
    rc = verifier.lib.hkv_verify_block_txs(verifier.ctx, ctypes.byref(st), offsets.ctypes.data, outpoints.ctypes.data,
                                           scripts.ctypes.data, values.ctypes.data, _forkid(forkid),
                                           words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), first.ctypes.data,
                                           src.ctypes.data, cap)
    check(rc, "hkv_verify_block_txs", verifier.lib)
    return unpack_bits(words, n_tx).tolist(), _split(src.tolist(), first, n_tx)


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
    import torch
    from .stdtx import std_tx_jobs_device
    if len(prevouts) != len(txs):
        raise ValueError("one prevout list per tx")
    n_tx = len(txs)
    if n_tx == 0:
        return [], [], []
    tb = TxBatch(txs)
    offsets, outpoints, scripts, values = pack_prevouts(tb, prevouts)
    buf, pool_at = block_layout(tb)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    d_buf, d_off = up(buf), up(tb.offsets)
    d_po, d_op, d_ps, d_pv = up(offsets), up(outpoints), up(scripts), up(values)
    dt = HkvTxs(d_buf.data_ptr(), d_off.data_ptr(), n_tx, d_buf.data_ptr() + pool_at, tb._len)
    first = torch.zeros(n_tx + 1, dtype=torch.int32, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    std_tx_jobs_device(verifier, dev, dt, d_po.data_ptr(), d_op.data_ptr(), d_ps.data_ptr(), d_pv.data_ptr(), 0,
                       first.data_ptr(), 0, status.data_ptr())
    n = int(first[n_tx].item()) & 0xFFFFFFFF
    status.zero_()
    n_slots = txid_table_slots(verifier, n_tx)
    txids = torch.zeros(n_tx * 32, dtype=torch.uint8, device="cuda")
    table = torch.zeros(n_slots, dtype=torch.int32, device="cuda")
    jobs = torch.zeros(max(1, n) * 24, dtype=torch.uint8, device="cuda")
    src = torch.zeros(max(1, n), dtype=torch.int32, device="cuda")
    recs = torch.zeros(max(1, n) * 168, dtype=torch.uint8, device="cuda")
    bits = torch.zeros(max(1, (n + 63) // 64) * 2, dtype=torch.int32, device="cuda")
    tx_bits = torch.zeros((n_tx + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    verify_block_txs_device(verifier, dev, dt, d_po.data_ptr(), d_op.data_ptr(), d_ps.data_ptr(), d_pv.data_ptr(),
                            _forkid(forkid), n, txids.data_ptr(), table.data_ptr(), n_slots, first.data_ptr(),
                            jobs.data_ptr(), src.data_ptr(), recs.data_ptr(), bits.data_ptr(), tx_bits.data_ptr(),
                            status.data_ptr())
    torch.cuda.synchronize()
    st = int(status[0].item())
    if st:
        check(-5, f"hkv_verify_block_txs_device (status {st})")
    f = first.cpu().numpy().view(np.uint32)
    per_input = unpack_bits(bits.cpu().numpy().view(np.uint32), n).tolist()
    srcs = src.cpu().numpy().view(np.uint32)[:n].tolist()
    ok = unpack_bits(tx_bits.cpu().numpy().view(np.uint32), n_tx).tolist()
    return ok, _split(per_input, f, n_tx), _split(srcs, f, n_tx)


__all__ = ["verify_block_txs", "verify_block_txs_host", "verify_block_txs_detail", "verify_block_txs_device",
           "block_tx_jobs_device", "txid_index_device", "txid_lookup_device", "txid_table_slots", "block_layout",
           "debug_txid_hash_mask", "HKV_SRC_LIST", "HKV_SRC_NONE"]
