#!/usr/bin/env python3
"""What the spend stage behind the block call costs.

The two batches of tools/bench_blocktx.py (its generator is imported): the
configs[0] block shape (2,000 txs x 2 P2PKH inputs) and a large batch of such
blocks (560,000 txs by default), HBM-resident, half the inputs spending
in-batch outputs, every signature valid.

  block_txs_device        hkv_verify_block_txs_device alone, by this tree's
                          library and, with --parent-lib, by a library built
                          from the parent commit (bound by hand: it lacks the
                          new symbols); the verdict words must be equal;
  block_txs_then_spends   the same followed by hkv_block_spends_device;
  spends_only             hkv_block_spends_device alone, on the arrays a block
                          call left;
  walk_only, table_only,  each of its four launches alone
  spender_only, fold_only (hkv_debug_spend_stages; table_only includes the
                          memset of the table);
  host_spends_ms          the Python the stage replaces: every tx parsed for
                          its outpoints, a dict from outpoint to its first
                          input, the output amounts and the listed input
                          amounts summed. Its FIRST and BALANCED answers must
                          equal the device's.

Device times are HIP-event times of k calls back to back on one stream, after
at least 100 ms of untimed calls, the variants alternating within each of
--reps rounds (the three block-call variants next to each other, behind an
untimed loop of block calls); the median round is reported and every round kept.
added_us = block_txs_then_spends - block_txs_device; same-session repeats of
the large batch move by about 3 % of the block call, so a
smaller difference between two columns is not a finding. One JSON object on
stdout and in --out.
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "haskoin-node_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MAX_MONEY = 2_100_000_000_000_000
STAGES = {"walk_only": 1, "table_only": 2, "spender_only": 4, "fold_only": 8}


def host_spends(txs, explicit):
    """(seconds, per-tx first flags, per-tx balanced flags): what a caller does
    today around verifyStdTx for double spends and the value balance."""
    from hkv.blocks import _varint
    t0 = time.perf_counter()
    seen = {}
    first, balanced = [], []
    g = 0
    for t, raw in enumerate(txs):
        nin, off = _varint(raw, 4)
        ok = True
        for _ in range(nin):
            op = raw[off:off + 36]
            if seen.setdefault(op, g) != g:
                ok = False
            g += 1
            sl, off = _varint(raw, off + 36)
            off += sl + 4
        nout, off = _varint(raw, off)
        out_sum = 0
        for _ in range(nout):
            out_sum += struct.unpack_from("<Q", raw, off)[0]
            sl, off = _varint(raw, off + 8)
            off += sl
        in_sum = sum(e[2] for e in explicit[t])
        first.append(ok)
        balanced.append(in_sum <= MAX_MONEY and out_sum <= MAX_MONEY and in_sum >= out_sum)
    return time.perf_counter() - t0, first, balanced


class ParentLib:
    """hkv_verify_block_txs_device of a parent-commit libhkv.so."""

    def __init__(self, path):
        from hkv.lib import HkvTxs
        c, P = ctypes, ctypes.POINTER
        self.lib = lib = ctypes.CDLL(path)
        lib.hkv_open_devices.argtypes = [P(c.c_int), c.c_int, c.c_uint32, P(c.c_void_p)]
        lib.hkv_close.argtypes = [c.c_void_p]
        lib.hkv_close.restype = None
        lib.hkv_verify_block_txs_device.argtypes = [c.c_void_p, c.c_int, P(HkvTxs)] + [c.c_void_p] * 4 + \
            [c.c_int32, c.c_size_t, c.c_void_p, c.c_void_p, c.c_size_t] + [c.c_void_p] * 8
        self.version = lib.hkv_version()
        self.ctx = c.c_void_p()
        rc = lib.hkv_open_devices((c.c_int * 1)(0), 1, 1, c.byref(self.ctx))
        if rc:
            raise RuntimeError(f"parent hkv_open_devices: {rc}")

    def verify_block_txs_device(self, dtx, prev, n, txids, table, n_slots, first, jobs, src, recs, bits, tx_bits,
                                status, stream):
        rc = self.lib.hkv_verify_block_txs_device(self.ctx, 0, ctypes.byref(dtx), *prev, -1, n, txids.data_ptr(),
                                                  table.data_ptr(), n_slots, first.data_ptr(), jobs.data_ptr(),
                                                  src.data_ptr(), recs.data_ptr(), bits.data_ptr(),
                                                  tx_bits.data_ptr(), status.data_ptr(), stream)
        if rc:
            raise RuntimeError(f"parent hkv_verify_block_txs_device: {rc}")

    def close(self):
        self.lib.hkv_close(self.ctx)


def measure(torch, np, hkv, v, parent, txs, explicit, external, n_in_batch, k, reps):
    from hkv.lib import HkvTxs
    from hkv.sighash import TxBatch
    from hkv.stdtx import pack_prevouts
    n_tx = len(txs)
    n = sum(len(e) for e in explicit)
    res = {"txs": n_tx, "inputs": n, "in_batch_inputs": n_in_batch}
    th, host_first, host_balanced = host_spends(txs, explicit)
    res["host_spends_ms"] = round(th * 1e3, 3)
    print(f"bench_spends: host leg done ({res['host_spends_ms']} ms)", file=sys.stderr, flush=True)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    tb = TxBatch(txs)
    arrays = pack_prevouts(tb, external)
    buf, pool_at = hkv.block_layout(tb)
    keep = [up(a) for a in (buf, tb.offsets) + tuple(arrays)]
    p = [t.data_ptr() for t in keep]
    dtx, prev = HkvTxs(p[0], p[1], n_tx, p[0] + pool_at, tb._len), p[2:]
    n_slots = hkv.txid_table_slots(v, n_tx)
    s_slots = hkv.spend_table_slots(v, n)
    zeros = lambda count, dtype: torch.zeros(count, dtype=dtype, device="cuda")
    first, status = zeros(n_tx + 1, torch.int32), zeros(2, torch.int32)
    jobs, src, recs = zeros(n * 24, torch.uint8), zeros(n, torch.int32), zeros(n * 168, torch.uint8)
    bits = zeros((n + 63) // 64 * 2, torch.int32)
    tx_bits, tx_bits2 = zeros((n_tx + 63) // 64 * 2, torch.int32), zeros((n_tx + 63) // 64 * 2, torch.int32)
    txids, table = zeros(n_tx * 32, torch.uint8), zeros(n_slots, torch.int32)
    in_off, s_table, spender = zeros(n, torch.int32), zeros(s_slots, torch.int32), zeros(n, torch.int32)
    sums, flags = zeros(2 * n_tx, torch.int64), zeros(n_tx, torch.uint8)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def block():
        hkv.verify_block_txs_device(v, 0, dtx, *prev, -1, n, txids.data_ptr(), table.data_ptr(), n_slots,
                                    first.data_ptr(), jobs.data_ptr(), src.data_ptr(), recs.data_ptr(), bits.data_ptr(),
                                    tx_bits.data_ptr(), status.data_ptr(), sp)

    def spends():
        hkv.block_spends_device(v, 0, dtx, first.data_ptr(), jobs.data_ptr(), src.data_ptr(), n, MAX_MONEY,
                                in_off.data_ptr(), s_table.data_ptr(), s_slots, spender.data_ptr(), sums.data_ptr(),
                                flags.data_ptr(), status.data_ptr(), sp)

    def both():
        block()
        spends()

    # name -> (call, the stage's launches it runs). The three heavy calls stand
    # next to each other, each behind a call of the same weight (an untimed
    # spacer loop of block calls opens every round): a call timed right behind
    # the light per-launch loops reads several microseconds slower.
    variants = {"block_txs_then_spends": (both, 15)}
    if parent is not None:
        variants["parent_block_txs_device"] = (lambda: parent.verify_block_txs_device(
            dtx, prev, n, txids, table, n_slots, first, jobs, src, recs, bits, tx_bits2, status, sp), 15)
    variants["block_txs_device"] = (block, 15)
    variants["spends_only"] = (spends, 15)
    for name, mask in STAGES.items():
        variants[name] = (spends, mask)

    # results first: the paths must agree before they are compared for speed
    both()
    torch.cuda.synchronize()
    w1 = tx_bits.cpu().numpy()
    f = flags.cpu().numpy()
    res["status"] = int(status[0].item())
    res["tx_accepted"] = int(np.unpackbits(w1.view(np.uint8), bitorder="little")[:n_tx].sum())
    res["tx_spend_ok"] = int(((f & 0x1F) == 0x1F).sum())
    res["tx_first"] = int(((f & 0x02) != 0).sum())
    res["tx_balanced"] = int(((f & 0x10) != 0).sum())
    res["spender_is_self"] = bool((spender.cpu().numpy() == np.arange(n, dtype=np.int32)).all())
    res["host_equals_device"] = bool(((f & 0x02) != 0).tolist() == host_first and
                                     ((f & 0x10) != 0).tolist() == host_balanced)
    if parent is not None:
        variants["parent_block_txs_device"][0]()
        torch.cuda.synchronize()
        res["parent_agrees"] = bool((tx_bits2.cpu().numpy() == w1).all())

    def run(name, count):
        fn, mask = variants[name]
        hkv.debug_spend_stages(v, 0, mask)
        for _ in range(count):
            fn()

    for name in variants:   # warm every shape up
        t_w = time.perf_counter()
        while True:
            run(name, max(k, 10))
            torch.cuda.synchronize()
            if time.perf_counter() - t_w > 0.1:
                break
    rounds = {name: [] for name in variants}
    print("bench_spends: warmed up", file=sys.stderr, flush=True)
    for _ in range(reps):
        for _ in range(k):
            block()
        for name in variants:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            hkv.debug_spend_stages(v, 0, variants[name][1])
            e0.record(stream)
            run(name, k)
            e1.record(stream)
            torch.cuda.synchronize()
            rounds[name].append(e0.elapsed_time(e1) * 1e3 / k)
    hkv.debug_spend_stages(v, 0, 15)
    for name, xs in rounds.items():
        res[f"{name}_us"] = round(sorted(xs)[len(xs) // 2], 1)
        res[f"{name}_us_rounds"] = [round(x, 1) for x in xs]
    res["added_us"] = round(res["block_txs_then_spends_us"] - res["block_txs_device_us"], 1)
    if parent is not None:
        xs = res["parent_block_txs_device_us_rounds"]
        res["parent_spread_us"] = round(max(xs) - min(xs), 1)
        res["block_txs_minus_parent_us"] = round(res["block_txs_device_us"] - res["parent_block_txs_device_us"], 1)
        res["added_over_parent_us"] = round(res["block_txs_then_spends_us"] - res["parent_block_txs_device_us"], 1)
    # the full call once more, so the arrays hold a whole stage's results when the leg ends
    both()
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libhkv.so built from the parent commit (same box, same session)")
    ap.add_argument("--batch-txs", type=int, default=560000)
    ap.add_argument("--steps", type=int, default=20, help="calls per timed loop on the block (the batch: a tenth)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spends", "bench_spends.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_spends needs the MI355X: nothing here is measured without it")
    import hkv
    from bench_blocktx import make_chained
    res = {"tool": "tools/bench_spends.py", "device": torch.cuda.get_device_name(0)}
    with hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1)) as v:
        parent = ParentLib(args.parent_lib) if args.parent_lib else None
        res["version"] = hex(v.lib.hkv_version())
        res["parent_version"] = hex(parent.version) if parent else None
        res["block"] = measure(torch, np, hkv, v, parent, *make_chained(v, torch, np, 2000, 41), args.steps, args.reps)
        if args.batch_txs > 0:
            res["batch"] = measure(torch, np, hkv, v, parent, *make_chained(v, torch, np, args.batch_txs, 42),
                                   max(2, args.steps // 10), args.reps)
        if parent:
            parent.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
