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


def verify_std_txs_detail(verifier, txs: Sequence[bytes], prevouts: Sequence[Sequence[Prevout]],
                          forkid: Optional[int] = None, dev: int = 0) -> Tuple[List[bool], List[List[bool]]]:
    """verify_std_txs with the per-input verdicts the device form keeps
    readable: ([tx verdict], [[verdict of input i of tx t]]), so a caller can
    name the failing inputs of a rejected tx (a tx that does not parse has no
    inputs to name). Runs the device forms on torch-allocated buffers of the
    context's device ``dev`` (blocking): the prevout provider once with
    n_inputs = 0 to learn the batch's input total, then the composed call."""
    import torch
    if len(prevouts) != len(txs):
        raise ValueError("one prevout list per tx")
    n_tx = len(txs)
    if n_tx == 0:
        return [], []
    from .lib import HkvTxs
    tb = TxBatch(txs)
    offsets, outpoints, scripts, values = pack_prevouts(tb, prevouts)
    _, pool = tb.struct()

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    d_bytes, d_off, d_pool = up(tb.bytes), up(tb.offsets), up(pool)
    d_po, d_op, d_ps, d_pv = up(offsets), up(outpoints), up(scripts), up(values)
    dt = HkvTxs(d_bytes.data_ptr(), d_off.data_ptr(), n_tx, d_pool.data_ptr(), tb._len)
    first = torch.zeros(n_tx + 1, dtype=torch.int32, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    std_tx_jobs_device(verifier, dev, dt, d_po.data_ptr(), d_op.data_ptr(), d_ps.data_ptr(), d_pv.data_ptr(), 0,
                       first.data_ptr(), 0, status.data_ptr())
    n = int(first[n_tx].item()) & 0xFFFFFFFF
    status.zero_()
    jobs = torch.zeros(max(1, n) * 24, dtype=torch.uint8, device="cuda")
    recs = torch.zeros(max(1, n) * 168, dtype=torch.uint8, device="cuda")
    bits = torch.zeros(max(1, (n + 63) // 64) * 2, dtype=torch.int32, device="cuda")
    tx_bits = torch.zeros((n_tx + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    verify_std_txs_device(verifier, dev, dt, d_po.data_ptr(), d_op.data_ptr(), d_ps.data_ptr(), d_pv.data_ptr(),
                          _forkid(forkid), n, first.data_ptr(), jobs.data_ptr(), recs.data_ptr(), bits.data_ptr(),
                          tx_bits.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    st = int(status[0].item())
    if st:
        check(-5, f"hkv_verify_std_txs_device (status {st})")
    f = first.cpu().numpy().view(np.uint32)
    per_input = unpack_bits(bits.cpu().numpy().view(np.uint32), n).tolist()
    ok = unpack_bits(tx_bits.cpu().numpy().view(np.uint32), n_tx).tolist()
    return ok, [per_input[int(f[t]): int(f[t + 1])] for t in range(n_tx)]


__all__ = ["verify_std_txs", "verify_std_txs_detail", "pack_prevouts", "std_tx_jobs_device", "tx_verdicts_device",
           "verify_std_txs_device"]
