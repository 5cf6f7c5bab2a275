"""Batch verifyStdTx — whole transactions against outpoint-keyed prevout
lists, the host-side mirror of haskoin-core's

    verifyStdTx :: Network -> Ctx -> Tx -> [(ScriptOutput, Word64, OutPoint)] -> Bool

[dep, haskoin-core-1.1.0 Haskoin.Transaction.Builder]. The caller hands over
raw txs and, per tx, an unordered list of prevouts; the outpoint match
(matchTemplate), verifyStdInput per matched input and the per-tx ``all`` run
in libhkv's HIP kernels (csrc/hkv_stdtx.hip around the standard-input verify).
No host-side tx parser is involved.

    verify_std_txs(v, raw_txs, prevouts, forkid) -> [bool]
        prevouts[t] = [(outpoint36, scriptPubKey, value), ...] in list order;
        outpoint36 = the 32 hash bytes as they appear in the tx + LE32 index.

The device-pointer forms (``std_tx_jobs_device``, ``tx_verdicts_device``,
``verify_std_txs_device``) take the four prevout arrays ``pack_prevouts``
builds, uploaded by the caller.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .lib import HKV_NO_FORKID, check
from .records import unpack_bits
from .sighash import TxBatch

Prevout = Tuple[bytes, bytes, int]  # (36-byte wire outpoint, scriptPubKey, value)


def _ptr(p: int):
    return ctypes.c_void_p(p) if p else None


def _forkid(forkid: Optional[int]) -> int:
    return HKV_NO_FORKID if forkid is None else int(forkid)


def pack_prevouts(tb: TxBatch, prevouts: Sequence[Sequence[Prevout]]):
    """The four prevout arrays of include/hkv.h for a batch whose scripts go
    into tb's pool: (offsets uint32[n_tx + 1], outpoints uint8[36 E],
    scripts uint32[2 E] as (offset, length) pairs, values uint64[E])."""
    offsets = np.zeros(len(prevouts) + 1, dtype=np.uint32)
    ops: List[bytes] = []
    scripts: List[int] = []
    values: List[int] = []
    for t, entries in enumerate(prevouts):
        for (op, spk, value) in entries:
            if len(op) != 36:
                raise ValueError("an outpoint is 36 bytes: 32 hash bytes in wire order, then the LE32 index")
            ops.append(bytes(op))
            scripts.extend(tb.script(bytes(spk)))
            values.append(int(value))
        offsets[t + 1] = len(values)
    outpoints = np.frombuffer(b"".join(ops) or b"\0" * 36, dtype=np.uint8).copy()
    return (offsets, outpoints, np.array(scripts or [0, 0], dtype=np.uint32),
            np.array(values or [0], dtype=np.uint64))


def verify_std_txs(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]],
                   forkid: Optional[int] = None) -> List[bool]:
    """Batch verifyStdTx on the context's first device (blocking): element t
    equals ``verifyStdTx net ctx tx_t prevouts_t``."""
    if len(prevouts) != len(txs):
        raise ValueError("one prevout list per tx")
    tb = TxBatch(txs)
    offsets, outpoints, scripts, values = pack_prevouts(tb, prevouts)
    st, pool = tb.struct()
    words = np.zeros(max(1, (len(txs) + 31) // 32), dtype=np.uint32)
    rc = verifier.lib.hkv_verify_std_txs(verifier.ctx, ctypes.byref(st), offsets.ctypes.data, outpoints.ctypes.data,
                                         scripts.ctypes.data, values.ctypes.data, _forkid(forkid),
                                         words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    check(rc, "hkv_verify_std_txs", verifier.lib)
    return unpack_bits(words, len(txs)).tolist()


def std_tx_jobs_device(v, dev: int, d_txs, d_prev_offsets: int, d_prev_outpoints: int, d_prev_scripts: int,
                       d_prev_values: int, n_inputs: int, d_input_first: int, d_jobs: int, d_status: int,
                       stream: int = 0) -> None:
    """hkv_std_tx_jobs_device: the prevout provider alone (d_input_first:
    n_tx + 1 words; d_jobs: n_inputs jobs; d_status: a word the caller
    zeroed). Enqueued on ``stream``, not synchronised."""
    rc = v.lib.hkv_std_tx_jobs_device(v.ctx, dev, ctypes.byref(d_txs), _ptr(d_prev_offsets), _ptr(d_prev_outpoints),
                                      _ptr(d_prev_scripts), _ptr(d_prev_values), n_inputs, _ptr(d_input_first),
                                      _ptr(d_jobs), _ptr(d_status), _ptr(stream))
    check(rc, "hkv_std_tx_jobs_device", v.lib)


def tx_verdicts_device(v, dev: int, d_input_first: int, n_tx: int, d_input_bits: int, d_tx_bits: int,
                       stream: int = 0) -> None:
    """hkv_tx_verdicts_device: tx bit t = every input bit of
    [input_first[t], input_first[t+1]) is 1 and the range is not empty."""
    rc = v.lib.hkv_tx_verdicts_device(v.ctx, dev, _ptr(d_input_first), n_tx, _ptr(d_input_bits), _ptr(d_tx_bits),
                                      _ptr(stream))
    check(rc, "hkv_tx_verdicts_device", v.lib)


def verify_std_txs_device(v, dev: int, d_txs, d_prev_offsets: int, d_prev_outpoints: int, d_prev_scripts: int,
                          d_prev_values: int, forkid: int, n_inputs: int, d_input_first: int, d_jobs: int,
                          d_records: int, d_input_bits: int, d_tx_bits: int, d_status: int, stream: int = 0) -> None:
    """hkv_verify_std_txs_device: job builder, standard-input verify and
    per-tx reduction enqueued on ``stream`` with no host wait."""
    rc = v.lib.hkv_verify_std_txs_device(v.ctx, dev, ctypes.byref(d_txs), _ptr(d_prev_offsets),
                                         _ptr(d_prev_outpoints), _ptr(d_prev_scripts), _ptr(d_prev_values), forkid,
                                         n_inputs, _ptr(d_input_first), _ptr(d_jobs), _ptr(d_records),
                                         _ptr(d_input_bits), _ptr(d_tx_bits), _ptr(d_status), _ptr(stream))
    check(rc, "hkv_verify_std_txs_device", v.lib)


JOB_BYTES, REC_BYTES = 24, 168   # hkv_input_job; a verify record


def _pair_words(n_bits: int) -> int:
    """The verdict words of n_bits verdicts: the kernels write a pair per 64."""
    return (n_bits + 63) // 64 * 2


def _device_run(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]], forkid: Optional[int],
                dev: int, block: bool = False, max_money: Optional[int] = None):
    """The composed device forms on torch-allocated buffers of the context's
    device ``dev`` (blocking), behind verify_std_txs_detail, blocktx's
    verify_block_txs_detail (``block``) and spends' check_block_txs
    (``max_money``: the spend stage behind the block call on the same (null)
    stream). Uploads the batch — the std form with the pool as its own
    allocation, the block form behind the tx bytes (block_layout) —, runs
    hkv_std_tx_jobs_device once with n_inputs = 0 to learn the input total,
    sizes every buffer, runs the composed call, waits and checks the status
    word. Returns None for an empty batch, else the host arrays: n, first
    (uint32[n_tx + 1]), tx_ok and input_ok (lists of bool), and for a block
    src, with max_money spender (uint32[n]), sums (uint64[2 n_tx]), flags."""
    import torch
    from types import SimpleNamespace
    from .lib import HkvTxs
    if len(prevouts) != len(txs):
        raise ValueError("one prevout list per tx")
    n_tx = len(txs)
    if n_tx == 0:
        return None
    tb = TxBatch(txs)
    packed = pack_prevouts(tb, prevouts)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    def zeros(count, dtype=torch.int32):
        return torch.zeros(count, dtype=dtype, device="cuda")

    def host(t, dtype=np.uint32):
        return t.cpu().numpy().view(dtype)

    d_off = up(tb.offsets)
    if block:
        from .blocktx import block_layout, txid_table_slots, verify_block_txs_device
        buf, pool_at = block_layout(tb)
        d_bytes = up(buf)
        d_pool_ptr = d_bytes.data_ptr() + pool_at
    else:
        d_bytes, d_pool = up(tb.bytes), up(tb.struct()[1])
        d_pool_ptr = d_pool.data_ptr()
    dt = HkvTxs(d_bytes.data_ptr(), d_off.data_ptr(), n_tx, d_pool_ptr, tb._len)
    d_prev = [up(a) for a in packed]
    prev = [t.data_ptr() for t in d_prev]
    first, status = zeros(n_tx + 1), zeros(2)
    std_tx_jobs_device(verifier, dev, dt, *prev, 0, first.data_ptr(), 0, status.data_ptr())
    n = int(first[n_tx].item()) & 0xFFFFFFFF
    status.zero_()
    m = max(1, n)
    jobs, recs = zeros(m * JOB_BYTES, torch.uint8), zeros(m * REC_BYTES, torch.uint8)
    bits, tx_bits = zeros(max(2, _pair_words(n))), zeros(_pair_words(n_tx))
    out = SimpleNamespace(n=n)
    if not block:
        name = "hkv_verify_std_txs_device"
        verify_std_txs_device(verifier, dev, dt, *prev, _forkid(forkid), n, first.data_ptr(), jobs.data_ptr(),
                              recs.data_ptr(), bits.data_ptr(), tx_bits.data_ptr(), status.data_ptr())
    else:
        name = "hkv_verify_block_txs_device"
        n_slots = txid_table_slots(verifier, n_tx)
        txids, table, src = zeros(n_tx * 32, torch.uint8), zeros(n_slots), zeros(m)
        if max_money is not None:
            from .spends import block_spends_device, spend_table_slots
            name = "hkv_block_spends_device"
            s_slots = spend_table_slots(verifier, n)
            if s_slots == 0:
                check(-1, "hkv_spend_table_slots (more than 2^30 inputs)")
            in_off, s_table, spender = zeros(m), zeros(s_slots), zeros(m)
            sums, flags = zeros(2 * n_tx, torch.int64), zeros(n_tx, torch.uint8)
        verify_block_txs_device(verifier, dev, dt, *prev, _forkid(forkid), n, txids.data_ptr(), table.data_ptr(),
                                n_slots, first.data_ptr(), jobs.data_ptr(), src.data_ptr(), recs.data_ptr(),
                                bits.data_ptr(), tx_bits.data_ptr(), status.data_ptr())
        if max_money is not None:
            block_spends_device(verifier, dev, dt, first.data_ptr(), jobs.data_ptr(), src.data_ptr(), n, max_money,
                                in_off.data_ptr(), s_table.data_ptr(), s_slots, spender.data_ptr(), sums.data_ptr(),
                                flags.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    st = int(status[0].item())
    if st:
        check(-5, f"{name} (status {st})")
    out.first = host(first)
    out.input_ok = unpack_bits(host(bits), n).tolist()
    out.tx_ok = unpack_bits(host(tx_bits), n_tx).tolist()
    if block:
        out.src = host(src)[:n]
    if max_money is not None:
        out.spender, out.sums, out.flags = host(spender)[:n], host(sums, np.uint64), host(flags, np.uint8).tolist()
    return out


def verify_std_txs_detail(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]],
                          forkid: Optional[int] = None, dev: int = 0) -> Tuple[List[bool], List[List[bool]]]:
    """verify_std_txs with the per-input verdicts the device form keeps
    readable: ([tx verdict], [[verdict of input i of tx t]]), so a caller can
    name the failing inputs of a rejected tx (a tx that does not parse has no
    inputs to name). Runs the device forms on torch-allocated buffers of the
    context's device ``dev`` (blocking): the prevout provider once with
    n_inputs = 0 to learn the batch's input total, then the composed call."""
    r = _device_run(verifier, txs, prevouts, forkid, dev)
    if r is None:
        return [], []
    return r.tx_ok, [r.input_ok[int(r.first[t]): int(r.first[t + 1])] for t in range(len(txs))]


__all__ = ["verify_std_txs", "verify_std_txs_detail", "pack_prevouts", "std_tx_jobs_device", "tx_verdicts_device",
           "verify_std_txs_device"]
