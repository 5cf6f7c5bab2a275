#!/usr/bin/env python3
"""What resolving in-batch prevouts on the device costs.

Two legs on HBM-resident data: the configs[0] block shape (2,000 txs x 2 P2PKH
inputs) and a large batch of such blocks (560,000 txs as 280 blocks by
default). In every block the first half of the txs spend external prevouts and
pay to known keys, the second half spend exactly those outputs, so half the
inputs of the batch spend in-batch outputs and every signature is valid (the
parents are signed and final before the children are built and signed).

  block_txs_device   hkv_verify_block_txs_device: the caller lists only the
                     external prevouts; txids, table, count, scan, block jobs,
                     verify, per-tx reduction;
  std_txs_device     hkv_verify_std_txs_device on the same batch with every
                     prevout supplied explicitly, by this tree's library and,
                     with --parent-lib, by a library built from the parent
                     commit (bound by hand: it lacks the new symbols);
  provider_only      hkv_block_tx_jobs_device (txids, table, count, scan, jobs);
  index_only         hkv_txid_index_device on finished txids (memset + inserts);
  txids_only         hkv_tx_ids_device;
  host_*             the host work the block call removes, as this package
                     would do it in Python: hashlib txids of every tx
                     (host_txids_ms), a dict from txid to index, and per
                     in-batch input a walk to the parent's output and a list
                     entry for it (host_resolve_ms).

Device times are HIP-event times of k calls back to back on one stream, after
at least 100 ms of untimed calls, the variants alternating within each of
--reps rounds; the median round is reported and every round kept. One JSON
object on stdout and in --out.
"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "haskoin-node_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HALF = 1000  # txs per half block


def sha256d(b: bytes) -> bytes:
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


def make_chained(v, torch, np, n_tx: int, seed: int):
    """(txs, explicit prevouts, external prevouts, in-batch inputs): blocks of
    2 * HALF txs, each 2 P2PKH inputs and 2 P2PKH outputs; the second half of a
    block spends the outputs of its first half."""
    from hkv import blockgen as bg
    from hkv.lib import HKV_SIGHASH_LEGACY
    from hkv.sighash import tx_sig_hash_batch
    rng = random.Random(seed)
    n_keys = 4096
    priv = torch.zeros(n_keys * 32, dtype=torch.uint8, device="cuda")
    pub = torch.zeros(n_keys * 33, dtype=torch.uint8, device="cuda")
    h160 = torch.zeros(n_keys * 20, dtype=torch.uint8, device="cuda")
    v.gen_keys_device(0, seed, n_keys, priv.data_ptr(), pub.data_ptr(), h160.data_ptr())
    torch.cuda.synchronize()
    pubs, hs = pub.cpu().numpy().tobytes(), h160.cpu().numpy().tobytes()
    spk_of = lambda k: bg.p2pkh(hs[20 * k:20 * k + 20])

    def sign_layer(skeletons, tag):
        """skeletons: (version, [(outpoint, key, value)], outs, lock) -> signed raw txs."""
        raw0, jobs, key_idx = [], [], []
        for t, (ver, spends, outs, lock) in enumerate(skeletons):
            raw0.append(bg.serialize(ver, [(op, b"", 0xFFFFFFFF) for (op, _, _) in spends], outs, [], lock))
            for j, (_, k, value) in enumerate(spends):
                jobs.append((t, j, spk_of(k), value, 1, HKV_SIGHASH_LEGACY))
                key_idx.append(k)
        msgs, status = tx_sig_hash_batch(v, raw0, jobs)
        assert not any(status)
        d_msg = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()).cuda()
        d_idx = torch.tensor(key_idx, dtype=torch.int32, device="cuda")
        d_sig = torch.zeros(len(jobs) * 64, dtype=torch.uint8, device="cuda")
        v.gen_sign_device(0, seed ^ tag, len(jobs), priv.data_ptr(), d_idx.data_ptr(), d_msg.data_ptr(), 32,
                          d_sig.data_ptr())
        torch.cuda.synchronize()
        sigs = d_sig.cpu().numpy().tobytes()
        out, q = [], 0
        for (ver, spends, outs, lock) in skeletons:
            ins = []
            for (op, k, _) in spends:
                sig = bg.der(sigs[64 * q:64 * q + 32], sigs[64 * q + 32:64 * q + 64]) + b"\x01"
                ins.append((op, bg.push(sig) + bg.push(pubs[33 * k:33 * k + 33]), 0xFFFFFFFF))
                q += 1
            out.append(bg.serialize(ver, ins, outs, [], lock))
        return out

    n_half = n_tx // 2
    parents = []
    for _ in range(n_half):
        spends = [(rng.randbytes(32) + struct.pack("<I", rng.randrange(4)), rng.randrange(n_keys),
                   rng.randrange(1000, 2**45)) for _ in range(2)]
        outs = [(rng.randrange(546, 2**40), rng.randrange(n_keys)) for _ in range(2)]
        parents.append((rng.choice([1, 2]), spends, outs, rng.randrange(800000)))
    raw_p = sign_layer([(ver, sp, [(val, spk_of(k)) for (val, k) in outs], lock) for (ver, sp, outs, lock) in parents], 1)
    children = []
    for u, (_, _, outs, _) in enumerate(parents):
        h = sha256d(raw_p[u])   # (no witness, canonical varints: txHash is the hash of the wire bytes)
        spends = [(h + struct.pack("<I", k), outs[k][1], outs[k][0]) for k in range(2)]
        couts = [(rng.randrange(546, 2**40), bg.p2pkh(rng.randbytes(20))) for _ in range(2)]
        children.append((rng.choice([1, 2]), spends, couts, rng.randrange(800000)))
    raw_c = sign_layer(children, 2)
    print(f"bench_blocktx: {n_tx} txs signed", file=sys.stderr, flush=True)
    txs, explicit, external, n_in_batch = [], [], [], 0
    for b0 in range(0, n_half, HALF):
        for u in range(b0, min(b0 + HALF, n_half)):
            txs.append(raw_p[u])
            entries = [(op, spk_of(k), value) for (op, k, value) in parents[u][1]]
            explicit.append(entries)
            external.append(entries)
        for u in range(b0, min(b0 + HALF, n_half)):
            txs.append(raw_c[u])
            explicit.append([(op, spk_of(k), value) for (op, k, value) in children[u][1]])
            external.append([])
            n_in_batch += 2
    return txs, explicit, external, n_in_batch


def host_resolve(txs, external):
    """What a caller of hkv_verify_std_txs does for in-batch spends today:
    (seconds for the txids, seconds for the map, the walk and the entries)."""
    from hkv.blocks import _varint
    t0 = time.perf_counter()
    ids = [sha256d(raw) for raw in txs]
    t1 = time.perf_counter()
    index = {}
    for u, h in enumerate(ids):
        index.setdefault(h, u)
    out = []
    for t, raw in enumerate(txs):
        entries = list(external[t])
        have = {e[0] for e in entries}
        nin, off = _varint(raw, 4)
        for _ in range(nin):
            op = raw[off:off + 36]
            sl, off = _varint(raw, off + 36)
            off += sl + 4
            if op in have:
                continue
            p = index.get(op[:32])
            if p is None or p >= t:
                continue
            par = txs[p]
            n, o = _varint(par, 4)
            for _ in range(n):
                sl, o = _varint(par, o + 36)
                o += sl + 4
            nout, o = _varint(par, o)
            k = struct.unpack("<I", op[32:])[0]
            if k >= nout:
                continue
            for _ in range(k):
                sl, o = _varint(par, o + 8)
                o += sl
            value = struct.unpack("<Q", par[o:o + 8])[0]
            sl, o = _varint(par, o + 8)
            entries.append((op, par[o:o + sl], value))
        out.append(entries)
    return t1 - t0, time.perf_counter() - t1, out


def measure(torch, np, hkv, v, parent, txs, explicit, external, n_in_batch, k, reps):
    from hkv.lib import HkvTxs
    from hkv.sighash import TxBatch
    from hkv.stdtx import pack_prevouts
    n_tx = len(txs)
    n = sum(len(e) for e in explicit)
    res = {"txs": n_tx, "inputs": n, "in_batch_inputs": n_in_batch}
    th, tr, resolved = host_resolve(txs, external)
    res["host_txids_ms"] = round(th * 1e3, 3)
    res["host_resolve_ms"] = round(tr * 1e3, 3)
    res["host_resolution_equals_explicit"] = resolved == explicit
    print(f"bench_blocktx: host legs done ({res['host_txids_ms']} + {res['host_resolve_ms']} ms)", file=sys.stderr,
          flush=True)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    def batch(prevouts):
        tb = TxBatch(txs)
        arrays = pack_prevouts(tb, prevouts)
        buf, pool_at = hkv.block_layout(tb)
        keep = [up(a) for a in (buf, tb.offsets) + tuple(arrays)]
        p = [t.data_ptr() for t in keep]
        return keep, HkvTxs(p[0], p[1], n_tx, p[0] + pool_at, tb._len), p[2:]

    keep_e, dtx_e, prev_e = batch(explicit)
    keep_x, dtx_x, prev_x = batch(external)
    n_slots = hkv.txid_table_slots(v, n_tx)
    first = torch.zeros(n_tx + 1, dtype=torch.int32, device="cuda")
    jobs = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
    src = torch.zeros(n, dtype=torch.int32, device="cuda")
    recs = torch.zeros(n * 168, dtype=torch.uint8, device="cuda")
    bits = torch.zeros((n + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    tx_bits = torch.zeros((n_tx + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    tx_bits2 = torch.zeros((n_tx + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    txids = torch.zeros(n_tx * 32, dtype=torch.uint8, device="cuda")
    table = torch.zeros(n_slots, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    variants = {
        "block_txs_device": lambda: hkv.verify_block_txs_device(
            v, 0, dtx_x, *prev_x, -1, n, txids.data_ptr(), table.data_ptr(), n_slots, first.data_ptr(), jobs.data_ptr(),
            src.data_ptr(), recs.data_ptr(), bits.data_ptr(), tx_bits.data_ptr(), status.data_ptr(), sp),
    }
    # (the two libraries' explicit calls next to each other, each behind a call of the same weight)
    if parent is not None:
        variants["parent_std_txs_device"] = lambda: parent.verify_std_txs_device(
            dtx_e, prev_e, n, first, jobs, recs, bits, tx_bits2, status, sp)
    variants.update({
        "std_txs_device": lambda: hkv.verify_std_txs_device(
            v, 0, dtx_e, *prev_e, -1, n, first.data_ptr(), jobs.data_ptr(), recs.data_ptr(), bits.data_ptr(),
            tx_bits2.data_ptr(), status.data_ptr(), sp),
        "provider_only": lambda: hkv.block_tx_jobs_device(
            v, 0, dtx_x, *prev_x, n, txids.data_ptr(), table.data_ptr(), n_slots, first.data_ptr(), jobs.data_ptr(),
            src.data_ptr(), status.data_ptr(), sp),
        "index_only": lambda: hkv.txid_index_device(v, 0, txids.data_ptr(), n_tx, table.data_ptr(), n_slots, sp),
        "txids_only": lambda: hkv.tx_ids_device(v, 0, dtx_x, txids.data_ptr(), 0, sp),
    })

    # results first: the paths must agree before they are compared for speed
    variants["block_txs_device"]()
    variants["std_txs_device"]()
    torch.cuda.synchronize()
    w1, w2 = tx_bits.cpu().numpy(), tx_bits2.cpu().numpy()
    res["status"] = int(status[0].item())
    res["tx_accepted"] = int(np.unpackbits(w1.view(np.uint8), bitorder="little")[:n_tx].sum())
    res["block_call_equals_explicit_call"] = bool((w1 == w2).all())
    res["in_batch_src_words"] = int((src.cpu().numpy().view(np.uint32) < 0xFFFFFFFE).sum())
    if parent is not None:
        tx_bits2.zero_()
        variants["parent_std_txs_device"]()
        torch.cuda.synchronize()
        res["parent_agrees"] = bool((tx_bits2.cpu().numpy() == w1).all())

    for name, fn in variants.items():   # warm every shape up
        t_w = time.perf_counter()
        while True:
            for _ in range(max(k, 10)):
                fn()
            torch.cuda.synchronize()
            if time.perf_counter() - t_w > 0.1:
                break
    rounds = {name: [] for name in variants}
    print("bench_blocktx: warmed up", file=sys.stderr, flush=True)
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
    res["added_us"] = round(res["block_txs_device_us"] - res["std_txs_device_us"], 1)
    if parent is not None:
        xs = res["parent_std_txs_device_us_rounds"]
        res["parent_spread_us"] = round(max(xs) - min(xs), 1)
        res["std_txs_minus_parent_us"] = round(res["std_txs_device_us"] - res["parent_std_txs_device_us"], 1)
    return res


class ParentLib:
    """hkv_verify_std_txs_device of a parent-commit libhkv.so."""

    def __init__(self, path):
        from hkv.lib import HkvTxs
        c, P = ctypes, ctypes.POINTER
        self.lib = lib = ctypes.CDLL(path)
        lib.hkv_open_devices.argtypes = [P(c.c_int), c.c_int, c.c_uint32, P(c.c_void_p)]
        lib.hkv_close.argtypes = [c.c_void_p]
        lib.hkv_close.restype = None
        lib.hkv_verify_std_txs_device.argtypes = [c.c_void_p, c.c_int, P(HkvTxs)] + [c.c_void_p] * 4 + \
            [c.c_int32, c.c_size_t] + [c.c_void_p] * 7
        self.version = lib.hkv_version()
        self.ctx = c.c_void_p()
        rc = lib.hkv_open_devices((c.c_int * 1)(0), 1, 1, c.byref(self.ctx))
        if rc:
            raise RuntimeError(f"parent hkv_open_devices: {rc}")

    def verify_std_txs_device(self, dtx, prev, n, first, jobs, recs, bits, tx_bits, status, stream):
        rc = self.lib.hkv_verify_std_txs_device(self.ctx, 0, ctypes.byref(dtx), *prev, -1, n, first.data_ptr(),
                                                jobs.data_ptr(), recs.data_ptr(), bits.data_ptr(), tx_bits.data_ptr(),
                                                status.data_ptr(), stream)
        if rc:
            raise RuntimeError(f"parent hkv_verify_std_txs_device: {rc}")

    def close(self):
        self.lib.hkv_close(self.ctx)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libhkv.so built from the parent commit (same box, same session)")
    ap.add_argument("--batch-txs", type=int, default=560000)
    ap.add_argument("--steps", type=int, default=20, help="calls per timed loop on the block (the batch: a tenth)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocktx", "bench_blocktx.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_blocktx needs the MI355X: nothing here is measured without it")
    import hkv
    res = {"tool": "tools/bench_blocktx.py", "device": torch.cuda.get_device_name(0)}
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
