#!/usr/bin/env python3
"""What batch verifyStdTx costs beside the per-input call it wraps.

For the configs[0] block (2,000 txs x 2 P2PKH inputs) and a large mixed batch
(560,000 txs by default, ~1M inputs), on HBM-resident data:

  std_txs_device     hkv_verify_std_txs_device: counts + scan, job builder,
                     hkv_verify_std_inputs_device_status, per-tx reduction
                     (four launches more than the per-input call);
  std_inputs_device  hkv_verify_std_inputs_device on jobs built on the host,
                     by this tree's library and, with --parent-lib, by a
                     library built from the parent commit (its C ABI is bound
                     here by hand: it lacks the new symbols);
  builder_only /     the added launches on their own (hkv_std_tx_jobs_device,
  count_scan_only /  the same with n_inputs = 0: its count and scan launches
  verdicts_only      without the job launch, hkv_tx_verdicts_device);
  host_*             the host work the device form removes, as this package
                     does it in Python: walking each tx's wire bytes for its
                     outpoints, looking them up, numbering the inputs and
                     packing hkv_input_jobs (host_build_jobs_ms), and folding
                     the verdict bits per tx (host_fold_ms).

Device times are HIP-event times of k calls back to back on one stream, after
at least 100 ms of untimed calls, the variants alternating within each of
--reps rounds; the median round is reported and every round kept. One JSON
object on stdout and in --out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "haskoin-node_amd"))


def outpoints_of(raw: bytes):
    """The host walk verifyStdTx callers do today: every input's 36-byte outpoint."""
    from hkv.blocks import _varint
    off = 4
    if raw[4] == 0 and raw[5] == 1:
        off = 6
    nin, off = _varint(raw, off)
    out = []
    for _ in range(nin):
        out.append(raw[off:off + 36])
        sl, off = _varint(raw, off + 36)
        off += sl + 4
    return out


def host_build_jobs(np, txs, utxo):
    """(tx, input, script, value) per input from an outpoint-keyed map, packed
    as verify_std_inputs packs them."""
    from hkv.sighash import INPUT_JOB_DTYPE, TxBatch
    tb = TxBatch(txs)
    rows = []
    for t, raw in enumerate(txs):
        for i, op in enumerate(outpoints_of(raw)):
            spk, value = utxo[op]
            so, sl = tb.script(spk)
            rows.append((t, i, so, sl, value))
    arr = np.array(rows, dtype=INPUT_JOB_DTYPE)
    return tb, arr


def host_fold(np, bits_words, jobs_tx, n_tx):
    """Per-tx verdicts from per-input bits (what hkv/actor.py does per block)."""
    ok = np.unpackbits(bits_words.view(np.uint8), bitorder="little")[:len(jobs_tx)].astype(bool)
    bad = np.zeros(n_tx, dtype=bool)
    bad[jobs_tx[~ok]] = True
    seen = np.zeros(n_tx, dtype=bool)
    seen[jobs_tx] = True
    return seen & ~bad


class ParentLib:
    """The three calls of a parent-commit libhkv.so this tool needs."""

    def __init__(self, path):
        from hkv.lib import HkvTxs
        c, P = ctypes, ctypes.POINTER
        self.lib = lib = ctypes.CDLL(path)
        lib.hkv_open_devices.argtypes = [P(c.c_int), c.c_int, c.c_uint32, P(c.c_void_p)]
        lib.hkv_close.argtypes = [c.c_void_p]
        lib.hkv_close.restype = None
        lib.hkv_verify_std_inputs_device.argtypes = [c.c_void_p, c.c_int, P(HkvTxs), c.c_void_p, c.c_size_t, c.c_int32,
                                                     c.c_void_p, c.c_void_p, c.c_void_p]
        self.version = lib.hkv_version()
        self.ctx = c.c_void_p()
        rc = lib.hkv_open_devices((c.c_int * 1)(0), 1, 1, c.byref(self.ctx))
        if rc:
            raise RuntimeError(f"parent hkv_open_devices: {rc}")

    def verify_std_inputs_device(self, db, stream):
        rc = self.lib.hkv_verify_std_inputs_device(self.ctx, 0, ctypes.byref(db.txs), db.d_jobs.data_ptr(), db.n, -1,
                                                   db.records.data_ptr(), db.bits.data_ptr(), stream)
        if rc:
            raise RuntimeError(f"parent hkv_verify_std_inputs_device: {rc}")

    def close(self):
        self.lib.hkv_close(self.ctx)


def measure(torch, np, hkv, v, parent, txs, inputs, k, reps):
    from hkv import blockgen
    from hkv.stdtx import pack_prevouts
    # the outpoint-keyed view of the same prevouts, entry lists reversed so
    # that list order is not input order
    ops = [outpoints_of(raw) for raw in txs]
    prevouts = [[] for _ in txs]
    utxo = {}
    for (t, i, spk, value) in inputs:
        prevouts[t].append((ops[t][i], spk, value))
        utxo[ops[t][i]] = (spk, value)
    for entries in prevouts:
        entries.reverse()
    res = {"txs": len(txs), "inputs": len(inputs)}

    # -- host work the device form removes
    n_host = 3 if len(inputs) < 100000 else 1
    ts = []
    for _ in range(n_host):
        t0 = time.perf_counter()
        tb_h, arr_h = host_build_jobs(np, txs, utxo)
        ts.append(time.perf_counter() - t0)
    res["host_build_jobs_ms"] = round(sorted(ts)[len(ts) // 2] * 1e3, 3)
    t0 = time.perf_counter()
    torch.from_numpy(arr_h.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    res["host_jobs_upload_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["host_jobs_bytes"] = int(arr_h.nbytes)

    db = blockgen.DeviceBlock(torch, txs, inputs)
    # the prevout arrays share db's script pool offsets: rebuild the batch with both
    from hkv.sighash import TxBatch
    from hkv.lib import HkvTxs
    tb = TxBatch(txs)
    po, outpoints, scripts, values = pack_prevouts(tb, prevouts)
    _, pool = tb.struct()

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    keep = [up(a) for a in (tb.bytes, tb.offsets, pool, po, outpoints, scripts, values)]
    p = [t.data_ptr() for t in keep]
    dtx = HkvTxs(p[0], p[1], len(txs), p[2], tb._len)
    res["prevout_bytes"] = int(po.nbytes + outpoints.nbytes + scripts.nbytes + values.nbytes)
    n, n_tx = len(inputs), len(txs)
    first = torch.zeros(n_tx + 1, dtype=torch.int32, device="cuda")
    jobs = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
    recs = torch.zeros(n * 168, dtype=torch.uint8, device="cuda")
    bits = torch.zeros((n + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    tx_bits = torch.zeros((n_tx + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    variants = {
        "std_txs_device": lambda: hkv.verify_std_txs_device(v, 0, dtx, *p[3:], -1, n, first.data_ptr(), jobs.data_ptr(),
                                                            recs.data_ptr(), bits.data_ptr(), tx_bits.data_ptr(),
                                                            status.data_ptr(), sp),
        "std_inputs_device": lambda: v.verify_std_inputs_device(0, db.txs, db.d_jobs.data_ptr(), db.n, -1,
                                                                db.records.data_ptr(), db.bits.data_ptr(), sp),
        "builder_only": lambda: hkv.std_tx_jobs_device(v, 0, dtx, *p[3:], n, first.data_ptr(), jobs.data_ptr(),
                                                       status.data_ptr(), sp),
        "verdicts_only": lambda: hkv.tx_verdicts_device(v, 0, first.data_ptr(), n_tx, bits.data_ptr(),
                                                        tx_bits.data_ptr(), sp),
    }
    # (n_inputs = 0 and no job array: the count and scan launches alone; its own status word)
    status2 = torch.zeros(2, dtype=torch.int32, device="cuda")
    first2 = torch.zeros(n_tx + 1, dtype=torch.int32, device="cuda")
    variants["count_scan_only"] = lambda: hkv.std_tx_jobs_device(v, 0, dtx, *p[3:], 0, first2.data_ptr(), 0,
                                                                 status2.data_ptr(), sp)
    if parent is not None:
        variants["parent_std_inputs_device"] = lambda: parent.verify_std_inputs_device(db, sp)

    # results first: the two paths must agree before they are compared for speed
    variants["std_txs_device"]()
    variants["std_inputs_device"]()
    torch.cuda.synchronize()
    got_tx = np.unpackbits(tx_bits.cpu().numpy().view(np.uint8), bitorder="little")[:n_tx].astype(bool)
    jobs_tx = np.array([t for (t, _, _, _) in inputs], dtype=np.int64)
    words = db.bits.cpu().numpy().view(np.uint32)
    t0 = time.perf_counter()
    folded = host_fold(np, words, jobs_tx, n_tx)
    res["host_fold_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["status"] = int(status[0].item())
    res["tx_accepted"] = int(got_tx.sum())
    res["agrees_with_folded_per_input_verdicts"] = bool((got_tx == folded).all())
    if parent is not None:
        db.bits.zero_()
        variants["parent_std_inputs_device"]()
        torch.cuda.synchronize()
        res["parent_agrees"] = bool((db.bits.cpu().numpy().view(np.uint32) == words).all())

    for name, fn in variants.items():   # warm every shape up
        t_w = time.perf_counter()
        while True:
            for _ in range(max(k, 10)):
                fn()
            torch.cuda.synchronize()
            if time.perf_counter() - t_w > 0.1:
                break
    rounds = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(k):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            rounds[name].append(e0.elapsed_time(e1) * 1e3 / k)
    for name, xs in rounds.items():
        res[f"{name}_us"] = round(sorted(xs)[len(xs) // 2], 1)
        res[f"{name}_us_rounds"] = [round(x, 1) for x in xs]
    base = res.get("parent_std_inputs_device_us", res["std_inputs_device_us"])
    res["added_us"] = round(res["std_txs_device_us"] - base, 1)
    res["added_launches"] = 4
    res["host_removed_ms"] = round(res["host_build_jobs_ms"] + res["host_jobs_upload_ms"] + res["host_fold_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libhkv.so built from the parent commit (same box, same session)")
    ap.add_argument("--batch-txs", type=int, default=560000)
    ap.add_argument("--steps", type=int, default=20, help="calls per timed loop on the block (the batch: a tenth)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stdtx", "bench_stdtx.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stdtx needs the MI355X: nothing here is measured without it")
    import hkv
    from hkv import blockgen
    res = {"tool": "tools/bench_stdtx.py", "device": torch.cuda.get_device_name(0)}
    with hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1)) as v:
        parent = ParentLib(args.parent_lib) if args.parent_lib else None
        res["version"] = hex(v.lib.hkv_version())
        res["parent_version"] = hex(parent.version) if parent else None
        txs, inputs = blockgen.make_p2pkh_block(v, torch, n_tx=2000)
        res["block"] = measure(torch, np, hkv, v, parent, txs, inputs, args.steps, args.reps)
        if args.batch_txs > 0:
            txs, inputs = blockgen.make_block(v, torch, n_tx=args.batch_txs, seed=blockgen.SEED + args.batch_txs)
            res["batch"] = measure(torch, np, hkv, v, parent, txs, inputs, max(2, args.steps // 10), args.reps)
        if parent:
            parent.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
