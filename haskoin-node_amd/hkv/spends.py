"""Whole-block spend checks — ``hkv_block_spends_device`` and
``hkv_verify_block_txs_spends``: behind the block call's signature verdicts,
the first spender of every outpoint of the batch (a later spender of the same
outpoint is a double spend) and each tx's value balance against ``max_money``
(csrc/hkv_spends.hip: a walk per tx, a table over the inputs' outpoints, a
lookup per input, a fold per tx), on what the block call leaves in HBM. The
rule is stated in include/hkv.h.

    check_block_txs(v, raw_txs, prevouts, forkid, max_money)
        -> ([tx verdict], [[input verdict]], [[src]], [[spender]], [(in_sum, out_sum)], [flags])
        spender: (tx, input) of the first input of the batch with that outpoint.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .blocktx import _split, block_layout, txid_table_slots, verify_block_txs_device
from .lib import (HKV_SPEND_BALANCED, HKV_SPEND_COINBASE, HKV_SPEND_FIRST, HKV_SPEND_IN_RANGE, HKV_SPEND_OK,
                  HKV_SPEND_OUT_RANGE, HKV_SPEND_RESOLVED, HkvTxs, check)
from .records import unpack_bits
from .sighash import TxBatch
from .stdtx import Prevout, _forkid, _ptr, pack_prevouts

SUM_NONE = 0xFFFFFFFFFFFFFFFF   # a sum whose RANGE flag is clear


def spend_table_slots(v, n_inputs: int) -> int:
    """hkv_spend_table_slots: the slot count of the spent-outpoint table for
    n_inputs inputs (0: more than 2^30 inputs)."""
    return int(v.lib.hkv_spend_table_slots(n_inputs))


def debug_spend_stages(v, dev: int, stages: int) -> None:
    """hkv_debug_spend_stages (measurement hook): the launches later
    block_spends_device calls run (bit 0 walk, 1 table, 2 spender, 3 fold)."""
    check(v.lib.hkv_debug_spend_stages(v.ctx, dev, stages & 0xFFFFFFFF), "hkv_debug_spend_stages", v.lib)


def block_spends_device(v, dev: int, d_txs, d_input_first: int, d_jobs: int, d_input_src: int, n_inputs: int,
                        max_money: int, d_input_off: int, d_table: int, n_slots: int, d_input_spender: int,
                        d_tx_sums: int, d_tx_flags: int, d_status: int, stream: int = 0) -> None:
    """hkv_block_spends_device: the spend stage on the arrays
    block_tx_jobs_device / verify_block_txs_device left on the same stream.
    Enqueued, not synchronised."""
    rc = v.lib.hkv_block_spends_device(v.ctx, dev, ctypes.byref(d_txs), _ptr(d_input_first), _ptr(d_jobs),
                                       _ptr(d_input_src), n_inputs, max_money, _ptr(d_input_off), _ptr(d_table),
                                       n_slots, _ptr(d_input_spender), _ptr(d_tx_sums), _ptr(d_tx_flags),
                                       _ptr(d_status), _ptr(stream))
    check(rc, "hkv_block_spends_device", v.lib)


def _pairs(spender, first, n_tx) -> List[List[Tuple[int, int]]]:
    """Flat first-spender indices -> per tx, (tx, input) of each input's first spender."""
    f = np.asarray(first, dtype=np.int64)
    flat = np.asarray(spender, dtype=np.int64)
    t_of = np.searchsorted(f[1:], flat, side="right")
    return _split([(int(t), int(g - f[t])) for g, t in zip(flat, t_of)], first, n_tx)


def verify_block_txs_spends_host(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]],
                                 forkid: Optional[int], max_money: int):
    """hkv_verify_block_txs_spends (the host form, first device, blocking):
    ([tx verdict], [[src]], [[spender as (tx, input)]], [(in_sum, out_sum)], [flags])."""
    if len(prevouts) != len(txs):
        raise ValueError("one prevout list per tx")
    n_tx = len(txs)
    if n_tx == 0:
        return [], [], [], [], []
    tb = TxBatch(txs)
    offsets, outpoints, scripts, values = pack_prevouts(tb, prevouts)
    st, pool = tb.struct()
    words = np.zeros(max(1, (n_tx + 31) // 32), dtype=np.uint32)
    first = np.zeros(n_tx + 1, dtype=np.uint32)
    cap = int(tb.offsets[-1]) // 41 + 1   # (an input is at least 41 bytes of its tx)
    src = np.zeros(cap, dtype=np.uint32)
    spender = np.zeros(cap, dtype=np.uint32)
    sums = np.zeros(2 * n_tx, dtype=np.uint64)
    flags = np.zeros(n_tx, dtype=np.uint8)
    rc = verifier.lib.hkv_verify_block_txs_spends(
        verifier.ctx, ctypes.byref(st), offsets.ctypes.data, outpoints.ctypes.data, scripts.ctypes.data,
        values.ctypes.data, _forkid(forkid), max_money, words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
        first.ctypes.data, src.ctypes.data, spender.ctypes.data, cap, sums.ctypes.data, flags.ctypes.data)
    check(rc, "hkv_verify_block_txs_spends", verifier.lib)
    n = int(first[n_tx])
    return (unpack_bits(words, n_tx).tolist(), _split(src.tolist(), first, n_tx), _pairs(spender[:n], first, n_tx),
            [(int(sums[2 * t]), int(sums[2 * t + 1])) for t in range(n_tx)], flags.tolist())


def check_block_txs(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]],
                    forkid: Optional[int], max_money: int, dev: int = 0):
    """verify_block_txs_detail with the spend stage behind it: ([tx verdict],
    [[verdict of input i of tx t]], [[src]], [[first spender of the input's
    outpoint as (tx, input)]], [(in_sum, out_sum)], [flags]). Composed from the
    device forms on torch-allocated buffers of the context's device ``dev``
    (blocking): the count of hkv_std_tx_jobs_device with n_inputs = 0 to learn
    the input total, hkv_verify_block_txs_device, then
    hkv_block_spends_device on the same (null) stream."""
    import torch
    from .stdtx import std_tx_jobs_device
    if len(prevouts) != len(txs):
        raise ValueError("one prevout list per tx")
    n_tx = len(txs)
    if n_tx == 0:
        return [], [], [], [], [], []
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
    s_slots = spend_table_slots(verifier, n)
    if s_slots == 0:
        check(-1, "hkv_spend_table_slots (more than 2^30 inputs)")
    m = max(1, n)
    txids = torch.zeros(n_tx * 32, dtype=torch.uint8, device="cuda")
    table = torch.zeros(n_slots, dtype=torch.int32, device="cuda")
    jobs = torch.zeros(m * 24, dtype=torch.uint8, device="cuda")
    src = torch.zeros(m, dtype=torch.int32, device="cuda")
    recs = torch.zeros(m * 168, dtype=torch.uint8, device="cuda")
    bits = torch.zeros(max(1, (n + 63) // 64) * 2, dtype=torch.int32, device="cuda")
    tx_bits = torch.zeros((n_tx + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    in_off = torch.zeros(m, dtype=torch.int32, device="cuda")
    s_table = torch.zeros(s_slots, dtype=torch.int32, device="cuda")
    spender = torch.zeros(m, dtype=torch.int32, device="cuda")
    sums = torch.zeros(2 * n_tx, dtype=torch.int64, device="cuda")
    flags = torch.zeros(n_tx, dtype=torch.uint8, device="cuda")
    verify_block_txs_device(verifier, dev, dt, d_po.data_ptr(), d_op.data_ptr(), d_ps.data_ptr(), d_pv.data_ptr(),
                            _forkid(forkid), n, txids.data_ptr(), table.data_ptr(), n_slots, first.data_ptr(),
                            jobs.data_ptr(), src.data_ptr(), recs.data_ptr(), bits.data_ptr(), tx_bits.data_ptr(),
                            status.data_ptr())
    block_spends_device(verifier, dev, dt, first.data_ptr(), jobs.data_ptr(), src.data_ptr(), n, max_money,
                        in_off.data_ptr(), s_table.data_ptr(), s_slots, spender.data_ptr(), sums.data_ptr(),
                        flags.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    st = int(status[0].item())
    if st:
        check(-5, f"hkv_block_spends_device (status {st})")
    f = first.cpu().numpy().view(np.uint32)
    per_input = unpack_bits(bits.cpu().numpy().view(np.uint32), n).tolist()
    srcs = src.cpu().numpy().view(np.uint32)[:n].tolist()
    ok = unpack_bits(tx_bits.cpu().numpy().view(np.uint32), n_tx).tolist()
    sm = sums.cpu().numpy().view(np.uint64)
    return (ok, _split(per_input, f, n_tx), _split(srcs, f, n_tx),
            _pairs(spender.cpu().numpy().view(np.uint32)[:n], f, n_tx),
            [(int(sm[2 * t]), int(sm[2 * t + 1])) for t in range(n_tx)], flags.cpu().numpy().tolist())


__all__ = ["spend_table_slots", "block_spends_device", "verify_block_txs_spends_host", "check_block_txs",
           "debug_spend_stages", "SUM_NONE", "HKV_SPEND_RESOLVED", "HKV_SPEND_FIRST", "HKV_SPEND_IN_RANGE",
           "HKV_SPEND_OUT_RANGE", "HKV_SPEND_BALANCED", "HKV_SPEND_COINBASE", "HKV_SPEND_OK"]
