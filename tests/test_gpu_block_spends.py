"""GPU tests (MI355X) of hkv_block_spends_device and
hkv_verify_block_txs_spends: the first spender of every outpoint against a
dict, the walk's offsets and output sums, every output on the chained batch
against tests/spends_model.py, the replayed-tx block that hkv_verify_block_txs
accepts, the count mismatch, and the host form's shared outputs against
hkv_verify_block_txs word for word."""
import ctypes
import random
import struct
from collections import Counter

import numpy as np
import pytest

import blocktx_model as bm
import sighash_oracle as sh
import spends_model as sm

pytestmark = pytest.mark.gpu

GUARD = 0xA5
NONE = 0xFFFFFFFF
MONEY = sm.MAX_MONEY
WG = 256


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def ver(torch):
    import hkv
    v = hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1))
    yield v
    v.close()


class masked:
    """The slot hashes ANDed with mask inside the block, the default after it."""

    def __init__(self, ver, mask):
        self.ver, self.mask = ver, mask

    def __enter__(self):
        import hkv
        hkv.debug_txid_hash_mask(self.ver, 0, self.mask)

    def __exit__(self, *exc):
        import hkv
        hkv.debug_txid_hash_mask(self.ver, 0, 0xFFFFFFFF)


def upload(torch, arr: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def guarded(torch, n_bytes: int):
    """n_bytes of device memory with 256 guard bytes behind them, all GUARD."""
    return torch.full((n_bytes + 256,), GUARD, dtype=torch.uint8, device="cuda")


def split_guard(t, n_bytes: int):
    a = t.cpu().numpy()
    return a[:n_bytes], bool((a[n_bytes:] == GUARD).all())


class DeviceBlock:
    """A batch laid out for the block entry points (tx bytes, then the pool, in
    one buffer) with its prevout arrays, in HBM."""

    def __init__(self, torch, raw_txs, prevouts):
        import hkv
        from hkv.sighash import TxBatch
        from hkv.stdtx import pack_prevouts
        self.tb = TxBatch(raw_txs)
        arrays = pack_prevouts(self.tb, prevouts)
        buf, self.pool_at = hkv.block_layout(self.tb)
        self.n_tx = len(raw_txs)
        self.keep = [upload(torch, a) for a in (buf, self.tb.offsets) + tuple(arrays)]
        p = [t.data_ptr() for t in self.keep]
        self.txs = hkv.HkvTxs(p[0], p[1], self.n_tx, p[0] + self.pool_at, self.tb._len)
        self.prev = p[2:]
        self.n_slots = int(hkv.load_library().hkv_txid_table_slots(self.n_tx))


class Out:
    pass


def run_stage(torch, ver, b: DeviceBlock, n_inputs: int, max_money: int = MONEY, rezero: bool = False) -> Out:
    """hkv_block_tx_jobs_device, then hkv_block_spends_device on the same
    (null) stream with n_inputs as the caller's total, every array it writes
    guarded. rezero: the status word is cleared between the two, so a set bit
    is the stage's own."""
    import hkv
    first = torch.full((b.n_tx + 1,), -1, dtype=torch.int32, device="cuda")
    txids = torch.zeros(b.n_tx * 32, dtype=torch.uint8, device="cuda")
    table = torch.zeros(b.n_slots, dtype=torch.int32, device="cuda")
    jobs = guarded(torch, n_inputs * 24)
    src = guarded(torch, n_inputs * 4)
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    hkv.block_tx_jobs_device(ver, 0, b.txs, *b.prev, n_inputs, txids.data_ptr(), table.data_ptr(), b.n_slots,
                             first.data_ptr(), jobs.data_ptr(), src.data_ptr(), status.data_ptr())
    if rezero:
        torch.cuda.synchronize()
        status.zero_()
    s_slots = hkv.spend_table_slots(ver, n_inputs)
    in_off = guarded(torch, n_inputs * 4)
    s_table = guarded(torch, s_slots * 4)
    spender = guarded(torch, n_inputs * 4)
    sums = guarded(torch, b.n_tx * 16)
    flags = guarded(torch, b.n_tx)
    hkv.block_spends_device(ver, 0, b.txs, first.data_ptr(), jobs.data_ptr(), src.data_ptr(), n_inputs, max_money,
                            in_off.data_ptr(), s_table.data_ptr(), s_slots, spender.data_ptr(), sums.data_ptr(),
                            flags.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    o = Out()
    intact = []
    for name, t, nb, dt in (("jobs", jobs, n_inputs * 24, np.uint8), ("src", src, n_inputs * 4, np.uint32),
                            ("off", in_off, n_inputs * 4, np.uint32), ("table", s_table, s_slots * 4, np.uint32),
                            ("spender", spender, n_inputs * 4, np.uint32), ("sums", sums, b.n_tx * 16, np.uint64),
                            ("flags", flags, b.n_tx, np.uint8)):
        a, ok = split_guard(t, nb)
        setattr(o, name, a.view(dt))
        intact.append(ok)
    o.intact = all(intact)
    o.first = first.cpu().numpy().view(np.uint32)
    o.status = int(status[0].item())
    o.sums = [(int(o.sums[2 * t]), int(o.sums[2 * t + 1])) for t in range(b.n_tx)]
    return o


def assert_equals_model(o: Out, s: sm.Spends):
    n = s.first[-1]
    assert o.intact and o.status == 0 and o.first.tolist() == s.first
    assert o.off.tolist() == s.off
    bad = [g for g in range(n) if int(o.spender[g]) != s.spender[g]]
    assert not bad, [(g, int(o.spender[g]), s.spender[g]) for g in bad[:10]]
    assert o.sums == s.sums, [(t, o.sums[t], s.sums[t]) for t in range(len(s.sums)) if o.sums[t] != s.sums[t]][:10]
    assert o.flags.tolist() == s.flags, [(t, int(o.flags[t]), s.flags[t]) for t in range(len(s.flags))
                                         if int(o.flags[t]) != s.flags[t]][:10]
    # the table holds exactly the first spender of every distinct outpoint but the null one
    held = sorted(int(x) for x in o.table if x != NONE)
    assert held == sorted({s.spender[g] for g in range(n) if s.outpoint[g] != sm.NULL_OUTPOINT})


# --- the spender against a dict ---------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 5000])
def test_spender_vs_dict(torch, ver, n):
    """n inputs on a pool of n / 5 outpoints (one below, at and one above the
    workgroup size, several workgroups), at hash masks 0xFFFFFFFF and 0xF, and
    0 (one probe chain, quadratic) up to 1,024 inputs."""
    raws, prevouts = sm.outpoint_batch(100 + n, n)
    s = sm.Spends(raws, prevouts, MONEY)
    assert s.first[-1] == n
    if n >= 255:
        seen = Counter(s.outpoint)
        h = next(op for op in seen if op[32:] == struct.pack("<I", 1) and op[:32] + struct.pack("<I", 2) in seen)
        # equal hash with another index; equal index, the last hash byte flipped; equal first 8 bytes and
        # index with other bytes behind them (one hash value); a triple; a duplicate inside one tx; null
        # outpoints in three txs
        assert h[:31] + bytes([h[31] ^ 1]) + h[32:] in seen
        assert any(op[:8] == h[:8] and op[32:] == h[32:] and op[8:31] != h[8:31] for op in seen)
        assert max(seen.values()) >= 3
        per_tx = [s.outpoint[s.first[t]:s.first[t + 1]] for t in range(len(raws))]
        assert any(len(set(p)) < len(p) for p in per_tx)
        assert sum(sm.NULL_OUTPOINT in p for p in per_tx) >= 3
        assert any(s.spender[g] != g for g in range(n)) and len(raws) > WG / 4
    b = DeviceBlock(torch, raws, prevouts)
    outs = []
    for mask in (0xFFFFFFFF, 0xF) + ((0,) if n <= 1024 else ()):
        with masked(ver, mask):
            o = run_stage(torch, ver, b, n)
        assert_equals_model(o, s)
        outs.append((o.spender.tolist(), o.flags.tolist()))
    assert all(x == outs[0] for x in outs)


def test_one_outpoint_in_512_inputs_of_six_workgroups(torch, ver):
    """512 of 1,290 inputs, spread over six workgroups, carry one outpoint:
    every one reports the smallest index (the atomicMin race), and the table
    holds that outpoint once."""
    rng = random.Random(512)
    x = rng.randbytes(36)
    ops, carried = [], 0
    for g in range(5 * WG + 10):
        if g >= 7 and g % 5 in (1, 3) and carried < 512:
            ops.append(x)
            carried += 1
        else:
            ops.append(rng.randbytes(36))
    assert carried == 512 and ops.index(x) == 8 and max(g for g, o in enumerate(ops) if o == x) > 4 * WG
    raws = [sh.tx_serialize(bm._tx(rng, ops[k:k + 2])) for k in range(0, len(ops), 2)]
    prevouts = [[] for _ in raws]
    s = sm.Spends(raws, prevouts, MONEY)
    assert [s.spender[g] for g, o in enumerate(ops) if o == x] == [8] * 512
    b = DeviceBlock(torch, raws, prevouts)
    for mask in (0xFFFFFFFF, 0xF):
        with masked(ver, mask):
            o = run_stage(torch, ver, b, len(ops))
        assert_equals_model(o, s)
        assert sum(int(v) == 8 for v in o.table) == 1
        # the tx of inputs 8 and 9 is first; every other tx with a carrier is not
        first = [bool(f & sm.FIRST) for f in o.flags.tolist()]
        assert first == [all(ops[g] != x or g == 8 for g in (2 * t, 2 * t + 1)) for t in range(len(raws))]


# --- the walk -------------------------------------------------------------------------------

def test_walk_offsets_and_output_sums(torch, ver):
    """A tx of 300 inputs and 300 outputs, a BIP144 tx, a non-canonical
    input-count varint, 0xFD-length scripts, a tx that does not parse between
    parsing ones: the offsets and the output sums are the model's."""
    raws, prevouts = sm.walk_batch()
    s = sm.Spends(raws, prevouts, MONEY)
    assert s.first[1] == 300 and s.first[5] == s.first[4] and s.first[-1] == 300 + 2 + 1 + 2 + 3
    assert all(s.flags[t] & sm.OUT_RANGE for t in (1, 2, 3, 5)) and s.flags[4] == 0
    b = DeviceBlock(torch, raws, prevouts)
    o = run_stage(torch, ver, b, s.first[-1])
    assert_equals_model(o, s)
    blob = b"".join(raws)
    assert all(blob[int(a):int(a) + 36] == op for a, op in zip(o.off, s.outpoint))
    # the 300 amounts below 2^50 exceed max_money together; with a bound above them the sum is exact
    total = sum(v for (_, _, v) in bm.output_refs(raws[0]))
    assert total > MONEY and s.sums[0][1] == sm.SUM_NONE and not s.flags[0] & sm.OUT_RANGE
    wide = sm.Spends(raws, prevouts, 2**62)
    assert wide.sums[0][1] == total and wide.flags[0] & sm.OUT_RANGE
    assert_equals_model(run_stage(torch, ver, b, s.first[-1], max_money=2**62), wide)


def test_directed_amounts_on_device(torch, ver):
    raws, prevouts, want = sm.directed_amounts()
    s = sm.Spends(raws, prevouts, MONEY)
    o = run_stage(torch, ver, DeviceBlock(torch, raws, prevouts), s.first[-1])
    assert_equals_model(o, s)
    for name, (t, flags, sums) in want.items():
        assert (int(o.flags[t]), o.sums[t]) == (flags, sums), name


# --- parity on the chained batch ----------------------------------------------------------------

@pytest.fixture(scope="module")
def chain():
    c = bm.chained_batch(7, 200)
    return c, sm.Spends(c.raw, c.prevouts, MONEY)


@pytest.mark.parametrize("mask", [0xFFFFFFFF, 0], ids=["hashed", "one_chain"])
def test_chained_batch_vs_model(torch, ver, chain, mask):
    c, s = chain
    assert s.first[-1] == 465
    b = DeviceBlock(torch, c.raw, c.prevouts)
    with masked(ver, mask):
        o = run_stage(torch, ver, b, s.first[-1])
    assert_equals_model(o, s)
    assert o.src.tolist() == s.src


def test_host_form_and_check_block_txs_equal_the_model_and_each_other(ver, chain):
    import hkv
    c, s = chain
    n_tx = len(c.raw)
    split = lambda flat: [flat[s.first[t]:s.first[t + 1]] for t in range(n_tx)]
    ok_h, src_h, spender_h, sums_h, flags_h = hkv.verify_block_txs_spends_host(ver, c.raw, c.prevouts, None, MONEY)
    ok_d, per_input, src_d, spender_d, sums_d, flags_d = hkv.check_block_txs(ver, c.raw, c.prevouts, None, MONEY)
    assert (ok_h, src_h, spender_h, sums_h, flags_h) == (ok_d, src_d, spender_d, sums_d, flags_d)
    assert src_h == split(s.src) and spender_h == s.pairs() and sums_h == s.sums and flags_h == s.flags
    assert ok_d == [bool(p) and all(p) for p in per_input]
    with masked(ver, 0):
        assert hkv.check_block_txs(ver, c.raw, c.prevouts, None, MONEY) == (ok_d, per_input, src_d, spender_d, sums_d,
                                                                             flags_d)


# --- the hole, closed -------------------------------------------------------------------------

def test_replayed_tx_verifies_and_loses_first(ver):
    """A block in which a tx is repeated: hkv_verify_block_txs gives the copy
    verdict 1 (the copy spends the same outputs again, every signature still
    verifies); the spend stage clears HKV_SPEND_FIRST on exactly that tx and
    names the original's inputs as the first spenders."""
    import hkv
    c = bm.SignedChain(9300, None, n=48, coinbase=True)
    s0 = sm.Spends(c.raw, c.prevouts, MONEY)
    ok, _, _, spender, _, flags = hkv.check_block_txs(ver, c.raw, c.prevouts, None, MONEY)
    assert all(ok[1:]) and not ok[0]
    assert all(f & sm.FIRST for f in flags) and [t for t, f in enumerate(flags) if f & sm.COINBASE] == [0]
    assert flags == s0.flags and spender == s0.pairs()
    u = next(t for t in range(1, len(c.raw)) if len(c.spends[t]) >= 2)
    raws, prevouts = c.raw + [c.raw[u]], c.prevouts + [c.prevouts[u]]
    copy = len(raws) - 1
    today = hkv.verify_block_txs(ver, raws, prevouts, None)
    assert today[copy] and today[1:] == [True] * copy
    s = sm.Spends(raws, prevouts, MONEY)
    earlier = set()
    lacking = []
    for t in range(len(raws)):
        ops = s.outpoint[s.first[t]:s.first[t + 1]]
        if any(op in earlier or ops.index(op) != i for i, op in enumerate(ops) if op != sm.NULL_OUTPOINT):
            lacking.append(t)
        earlier.update(ops)
    assert lacking == [copy]
    ok, _, _, spender, sums, flags = hkv.check_block_txs(ver, raws, prevouts, None, MONEY)
    assert ok == today
    assert [t for t, f in enumerate(flags) if not f & sm.FIRST] == [copy]
    assert spender[copy] == [(u, i) for i in range(len(c.spends[u]))]
    assert all(spender[t] == [(t, i) for i in range(len(spender[t]))] for t in range(copy))
    assert flags == s.flags and sums == s.sums and flags[copy] & ~sm.FIRST == flags[u] & ~sm.FIRST
    host = hkv.verify_block_txs_spends_host(ver, raws, prevouts, None, MONEY)
    assert host[0] == today and host[2] == spender and host[4] == flags


# --- count mismatch ---------------------------------------------------------------------------

@pytest.mark.parametrize("rezero", [False, True], ids=["provider_set_it", "stage_sets_it"])
@pytest.mark.parametrize("delta", [-1, 1], ids=["one_too_few", "one_too_many"])
def test_count_mismatch(torch, ver, chain, delta, rezero):
    """n_inputs one too small and one too large: the status bit (the
    provider's, or with the word cleared in between the stage's own), all
    flags and sums 0, the guard words behind every per-input array untouched,
    no HIP error."""
    from hkv.lib import HKV_STATUS_INPUT_COUNT
    c, s = chain
    n = s.first[-1]
    b = DeviceBlock(torch, c.raw, c.prevouts)
    o = run_stage(torch, ver, b, n + delta, rezero=rezero)
    assert o.status == HKV_STATUS_INPUT_COUNT and o.intact and o.first.tolist() == s.first
    assert not o.flags.any() and o.sums == [(0, 0)] * len(c.raw)
    m = min(n, n + delta)
    assert o.off[:m].tolist() == s.off[:m] and o.spender[:m].tolist() == s.spender[:m]
    if delta > 0:
        assert int(o.spender[n]) == NONE      # a slot past the device's total
    # the device still answers, and a call with the right total is the model's
    assert_equals_model(run_stage(torch, ver, b, n), s)


# --- the host form ---------------------------------------------------------------------------

def test_host_form_shares_hkv_verify_block_txs_outputs_word_for_word(ver):
    from hkv.sighash import TxBatch
    from hkv.stdtx import pack_prevouts
    c = bm.SignedChain(9300, None, n=48, coinbase=True)
    n_tx = len(c.raw)
    tb = TxBatch(c.raw)
    offsets, outpoints, scripts, values = pack_prevouts(tb, c.prevouts)
    st, pool = tb.struct()
    cap = int(tb.offsets[-1]) // 41 + 1
    P = ctypes.POINTER(ctypes.c_uint32)

    def arrays():
        return (np.zeros((n_tx + 31) // 32, dtype=np.uint32), np.zeros(n_tx + 1, dtype=np.uint32),
                np.full(cap, 0x5A5A5A5A, dtype=np.uint32))

    w0, f0, s0 = arrays()
    rc = ver.lib.hkv_verify_block_txs(ver.ctx, ctypes.byref(st), offsets.ctypes.data, outpoints.ctypes.data,
                                      scripts.ctypes.data, values.ctypes.data, -1, w0.ctypes.data_as(P),
                                      f0.ctypes.data, s0.ctypes.data, cap)
    assert rc == 0
    w1, f1, s1 = arrays()
    spender = np.full(cap, 0x5A5A5A5A, dtype=np.uint32)
    sums = np.zeros(2 * n_tx, dtype=np.uint64)
    flags = np.zeros(n_tx, dtype=np.uint8)
    rc = ver.lib.hkv_verify_block_txs_spends(ver.ctx, ctypes.byref(st), offsets.ctypes.data, outpoints.ctypes.data,
                                             scripts.ctypes.data, values.ctypes.data, -1, MONEY, w1.ctypes.data_as(P),
                                             f1.ctypes.data, s1.ctypes.data, spender.ctypes.data, cap,
                                             sums.ctypes.data, flags.ctypes.data)
    assert rc == 0
    assert (w0 == w1).all() and (f0 == f1).all() and (s0 == s1).all()
    n = int(f0[n_tx])
    assert w0[0] & 2 and (spender[n:] == 0x5A5A5A5A).all() and spender[:n].tolist() == list(range(n))
    # the optional outputs left out; a capacity below the input total
    w2, _, _ = arrays()
    rc = ver.lib.hkv_verify_block_txs_spends(ver.ctx, ctypes.byref(st), offsets.ctypes.data, outpoints.ctypes.data,
                                             scripts.ctypes.data, values.ctypes.data, -1, MONEY, w2.ctypes.data_as(P),
                                             None, None, None, 0, None, flags.ctypes.data)
    assert rc == 0 and (w2 == w0).all()
    rc = ver.lib.hkv_verify_block_txs_spends(ver.ctx, ctypes.byref(st), offsets.ctypes.data, outpoints.ctypes.data,
                                             scripts.ctypes.data, values.ctypes.data, -1, MONEY, w2.ctypes.data_as(P),
                                             None, None, spender.ctypes.data, n - 1, None, flags.ctypes.data)
    assert rc == -1


def test_bad_arguments_on_a_live_context(torch, ver, chain):
    import hkv
    c, s = chain
    b = DeviceBlock(torch, c.raw, c.prevouts)
    n = s.first[-1]
    z = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = z.data_ptr()
    slots = hkv.spend_table_slots(ver, n)
    assert slots == 1024

    def call(n_inputs=n, money=MONEY, n_slots=slots, sums=p, txs=b.txs):
        hkv.block_spends_device(ver, 0, txs, p, p, p, n_inputs, money, p, p, n_slots, p, sums, p, p)

    for kw in (dict(money=2**63), dict(n_slots=slots - 1), dict(n_slots=slots // 2), dict(n_slots=slots + 64),
               dict(n_slots=2**32), dict(sums=p + 4), dict(n_inputs=0xFFFFFF01), dict(sums=0)):
        with pytest.raises(hkv.HkvError) as e:
            call(**kw)
        assert e.value.rc == -1, kw
    # no tx: HKV_OK with nothing launched, whatever the other pointers
    empty = hkv.HkvTxs(b.txs.bytes, b.txs.offsets, 0, b.txs.scripts, 0)
    hkv.block_spends_device(ver, 0, empty, 0, 0, 0, 0, MONEY, 0, 0, 64, 0, 0, 0, 0)
    torch.cuda.synchronize()
