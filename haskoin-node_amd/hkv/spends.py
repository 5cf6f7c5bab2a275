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

from .blocktx import _HostCall, _split
from .lib import (HKV_SPEND_BALANCED, HKV_SPEND_COINBASE, HKV_SPEND_FIRST, HKV_SPEND_IN_RANGE, HKV_SPEND_OK,
                  HKV_SPEND_OUT_RANGE, HKV_SPEND_RESOLVED, check)
from .stdtx import Prevout, _device_run, _forkid, _ptr

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


def _sum_pairs(sums, n_tx) -> List[Tuple[int, int]]:
    return [(int(sums[2 * t]), int(sums[2 * t + 1])) for t in range(n_tx)]


def verify_block_txs_spends_host(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]],
                                 forkid: Optional[int], max_money: int):
    """hkv_verify_block_txs_spends (the host form, first device, blocking):
    ([tx verdict], [[src]], [[spender as (tx, input)]], [(in_sum, out_sum)], [flags])."""
    h = _HostCall(verifier, txs, prevouts)
    n_tx = h.n_tx
    if n_tx == 0:
        return [], [], [], [], []
    spender = np.zeros(h.cap, dtype=np.uint32)
    sums = np.zeros(2 * n_tx, dtype=np.uint64)
    flags = np.zeros(n_tx, dtype=np.uint8)
    rc = verifier.lib.hkv_verify_block_txs_spends(*h.head, _forkid(forkid), max_money, *h.outs, spender.ctypes.data,
                                                  h.cap, sums.ctypes.data, flags.ctypes.data)
    check(rc, "hkv_verify_block_txs_spends", verifier.lib)
    n = int(h.first[n_tx])
    return h.tx_ok(), h.srcs(), _pairs(spender[:n], h.first, n_tx), _sum_pairs(sums, n_tx), flags.tolist()


def check_block_txs(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]],
                    forkid: Optional[int], max_money: int, dev: int = 0):
    """verify_block_txs_detail with the spend stage behind it: ([tx verdict],
    [[verdict of input i of tx t]], [[src]], [[first spender of the input's
    outpoint as (tx, input)]], [(in_sum, out_sum)], [flags]). Composed from the
    device forms on torch-allocated buffers of the context's device ``dev``
    (blocking): the count of hkv_std_tx_jobs_device with n_inputs = 0 to learn
    the input total, hkv_verify_block_txs_device, then
    hkv_block_spends_device on the same (null) stream."""
    r = _device_run(verifier, txs, prevouts, forkid, dev, block=True, max_money=max_money)
    if r is None:
        return [], [], [], [], [], []
    n_tx = len(txs)
    return (r.tx_ok, _split(r.input_ok, r.first, n_tx), _split(r.src.tolist(), r.first, n_tx),
            _pairs(r.spender, r.first, n_tx), _sum_pairs(r.sums, n_tx), r.flags)


__all__ = ["spend_table_slots", "block_spends_device", "verify_block_txs_spends_host", "check_block_txs",
           "debug_spend_stages", "SUM_NONE", "HKV_SPEND_RESOLVED", "HKV_SPEND_FIRST", "HKV_SPEND_IN_RANGE",
           "HKV_SPEND_OUT_RANGE", "HKV_SPEND_BALANCED", "HKV_SPEND_COINBASE", "HKV_SPEND_OK"]
