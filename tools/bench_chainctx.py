#!/usr/bin/env python3
"""What the chain-context stage behind the header checks costs.

Two batches of synthetic headers (tests/chainctx_model.py random_chain: chosen
version, time and bits on mainnet's constants, a few percent wrong on each
rule; nothing is mined, the stage does not look at proof of work), HBM-resident:
one 2,000-header message and 1,048,576 headers.

  check_headers_device         hkv_check_headers_device alone, by this tree's
                               library and, with --parent-lib, by a library
                               built from the parent commit (bound by hand: it
                               lacks the new symbols); hashes and status bytes
                               must be equal;
  connect_headers_device       the same followed by the stage and the first_bad
                               reduction (hkv_connect_headers_device);
  chain_context_only           hkv_chain_context_device alone, on the hashes a
                               header call left;
  facts_only, scan_only,       each of its three launches alone
  verdict_only                 (hkv_debug_chain_stages);
  headers_armed,               the first_bad word set to 0xFFFFFFFF by a fill on
  headers_armed_first_bad      the stream, then the header kernel; and the same
                               followed by the reduction
                               (hkv_connect_headers_device with the stage's
                               three launches left out). The fill stands for the
                               scan launch's arming of the word, so the
                               reduction meets a word above every index, as in
                               a full call; first_bad_us is the difference.
                               Nothing here is mined, so every header fails and
                               every workgroup has a candidate: the reduction's
                               worst case;
  host_model_ms                the Python the stage replaces: the model's walk
                               over the same headers (a sort of 11 times per
                               header, the big-integer retarget and work
                               divisions, a running sum). Its outputs must equal
                               the device's on every header.

Device times are HIP-event times of k calls back to back on one stream, after
at least 100 ms of untimed calls, the variants alternating within each of
--reps rounds (the parent library's header call right before this tree's, behind
an untimed loop of header calls); the median round is reported and every round
kept. A difference between this tree's and the parent's header call counts only
if it exceeds the spread of the parent's own rounds. One JSON object on stdout
and in --out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("haskoin-node_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, d))

STAGES = {"facts_only": 1, "scan_only": 2, "verdict_only": 4}
BASE = 1500000000


class ParentLib:
    """hkv_check_headers_device of a parent-commit libhkv.so."""

    def __init__(self, path):
        c, P = ctypes, ctypes.POINTER
        self.lib = lib = ctypes.CDLL(path)
        lib.hkv_open_devices.argtypes = [P(c.c_int), c.c_int, c.c_uint32, P(c.c_void_p)]
        lib.hkv_close.argtypes = [c.c_void_p]
        lib.hkv_close.restype = None
        lib.hkv_check_headers_device.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_size_t] + [c.c_void_p] * 5
        self.version = lib.hkv_version()
        self.has_new_symbols = hasattr(lib, "hkv_connect_headers_device")
        self.ctx = c.c_void_p()
        rc = lib.hkv_open_devices((c.c_int * 1)(0), 1, 1, c.byref(self.ctx))
        if rc:
            raise RuntimeError(f"parent hkv_open_devices: {rc}")

    def check_headers_device(self, d_h, n, lim, hashes, status, stream):
        rc = self.lib.hkv_check_headers_device(self.ctx, 0, d_h.data_ptr(), n, lim.data_ptr(), None,
                                               hashes.data_ptr(), status.data_ptr(), stream)
        if rc:
            raise RuntimeError(f"parent hkv_check_headers_device: {rc}")

    def close(self):
        self.lib.hkv_close(self.ctx)


def measure(torch, np, hkv, v, parent, n, seed, k, reps):
    import chainctx_model as cm
    from hkv.chain import ChainParams, ChainTip, work_ints
    p = cm.params()
    tp = cm.tip(2016 * 300 + 1000, [BASE - 600 * (10 - j) for j in range(11)], 0x1b0404cb, BASE - 600 * 1000,
                0x1b0404cb, 1 << 70)
    now = BASE + n * 1000 + 10000
    facts = cm.random_chain(seed, n, tp, p, now)
    raw = np.frombuffer(b"".join(cm.make_header(*f) for f in facts), dtype=np.uint8).copy()
    t0 = time.perf_counter()
    want = cm.connect(facts, tp, p, now)
    res = {"headers": n, "host_model_ms": round((time.perf_counter() - t0) * 1e3, 3)}
    print(f"bench_chainctx: host leg done ({res['host_model_ms']} ms)", file=sys.stderr, flush=True)

    hp = ChainParams(pow_limit=p.pow_limit, bip34_height=p.bip34_height, bip66_height=p.bip66_height,
                     bip65_height=p.bip65_height)
    ctx = hkv.chain_ctx(ChainTip(tp.height, tp.times, tp.bits, tp.period_first_time, tp.period_real_bits, tp.work),
                        hp, now)
    zeros = lambda count, dtype: torch.zeros(count, dtype=dtype, device="cuda")
    d_h = torch.from_numpy(raw).cuda()
    lim = torch.from_numpy(np.frombuffer(p.pow_limit.to_bytes(32, "little"), dtype=np.uint8).copy()).cuda()
    hashes, hashes2 = zeros(n * 32, torch.uint8), zeros(n * 32, torch.uint8)
    hst, hst2 = zeros(n, torch.uint8), zeros(n, torch.uint8)
    mtp, bits, work, st = zeros(n, torch.int32), zeros(n, torch.int32), zeros(n * 32, torch.uint8), zeros(n, torch.uint8)
    scratch = zeros(hkv.chain_scratch_words(v, n), torch.int32)
    fb = zeros(1, torch.int32)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def headers():
        hkv.check_headers_device(v, 0, d_h.data_ptr(), n, lim.data_ptr(), None, hashes.data_ptr(), hst.data_ptr(), sp)

    def stage():
        hkv.chain_context_device(v, 0, d_h.data_ptr(), n, hashes.data_ptr(), ctx, None, None, 0, mtp.data_ptr(),
                                 bits.data_ptr(), work.data_ptr(), st.data_ptr(), scratch.data_ptr(), sp)

    def connect():
        hkv.connect_headers_device(v, 0, d_h.data_ptr(), n, lim.data_ptr(), None, ctx, None, None, 0,
                                   hashes.data_ptr(), hst.data_ptr(), mtp.data_ptr(), bits.data_ptr(), work.data_ptr(),
                                   st.data_ptr(), scratch.data_ptr(), fb.data_ptr(), sp)

    # name -> (call, the stage's launches it runs): the heavy calls next to each
    # other, the parent's header call right before this tree's
    variants = {"connect_headers_device": (connect, 15)}
    if parent is not None:
        variants["parent_check_headers_device"] = (lambda: parent.check_headers_device(d_h, n, lim, hashes2, hst2, sp), 15)
    variants["check_headers_device"] = (headers, 15)
    variants["chain_context_only"] = (stage, 15)
    for name, mask in STAGES.items():
        variants[name] = (stage, mask)

    def arm():
        with torch.cuda.stream(stream):
            fb.fill_(-1)

    def armed_headers():
        arm()
        headers()

    def armed_first_bad():
        arm()
        connect()

    variants["headers_armed"] = (armed_headers, 15)
    variants["headers_armed_first_bad"] = (armed_first_bad, 8)

    # results first: the paths must agree before they are compared for speed
    connect()
    torch.cuda.synchronize()
    got = (mtp.cpu().numpy().view(np.uint32).tolist(), bits.cpu().numpy().view(np.uint32).tolist(),
           work_ints(work.cpu().numpy()), st.cpu().numpy().tolist())
    res["device_equals_model"] = all(g == w for g, w in zip(got, want))
    res["chain_all_ok"] = int(sum(f == 31 for f in got[3]))
    res["first_bad"] = int(fb.cpu().numpy().view(np.uint32)[0])
    if parent is not None:
        variants["parent_check_headers_device"][0]()
        torch.cuda.synchronize()
        res["parent_agrees"] = bool((hashes2 == hashes).all().item() and (hst2 == hst).all().item())

    def run(name, count):
        fn, mask = variants[name]
        hkv.debug_chain_stages(v, 0, mask)
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
    print("bench_chainctx: warmed up", file=sys.stderr, flush=True)
    for _ in range(reps):
        for _ in range(k):
            headers()
        for name in variants:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            hkv.debug_chain_stages(v, 0, variants[name][1])
            e0.record(stream)
            run(name, k)
            e1.record(stream)
            torch.cuda.synchronize()
            rounds[name].append(e0.elapsed_time(e1) * 1e3 / k)
    hkv.debug_chain_stages(v, 0, 15)
    for name, xs in rounds.items():
        res[f"{name}_us"] = round(sorted(xs)[len(xs) // 2], 1)
        res[f"{name}_us_rounds"] = [round(x, 1) for x in xs]
    res["added_us"] = round(res["connect_headers_device_us"] - res["check_headers_device_us"], 1)
    res["first_bad_us"] = round(res["headers_armed_first_bad_us"] - res["headers_armed_us"], 1)
    if parent is not None:
        xs = res["parent_check_headers_device_us_rounds"]
        res["parent_spread_us"] = round(max(xs) - min(xs), 1)
        res["check_headers_minus_parent_us"] = round(res["check_headers_device_us"] - res["parent_check_headers_device_us"], 1)
    connect()   # leave a whole call's results behind
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libhkv.so built from the parent commit (same box, same session)")
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=50, help="calls per timed loop on the message (the batch: a fifth)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chainctx", "bench_chainctx.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_chainctx needs the MI355X: nothing here is measured without it")
    import hkv
    res = {"tool": "tools/bench_chainctx.py", "device": torch.cuda.get_device_name(0)}
    with hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1)) as v:
        parent = ParentLib(args.parent_lib) if args.parent_lib else None
        res["version"] = hex(v.lib.hkv_version())
        res["parent_version"] = hex(parent.version) if parent else None
        res["parent_has_new_symbols"] = parent.has_new_symbols if parent else None
        res["message"] = measure(torch, np, hkv, v, parent, 2000, 41, args.steps, args.reps)
        if args.batch > 0:
            res["batch"] = measure(torch, np, hkv, v, parent, args.batch, 42, max(2, args.steps // 5), args.reps)
        if parent:
            parent.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
