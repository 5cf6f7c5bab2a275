"""GPU tests (MI355X) of hkv_verify_block_txs*: the txid table and its lookup
alone, the block job builder alone, and the composed call end to end, each
against tests/blocktx_model.py (the in-batch prevout rule restated on
stdtx_model's matchTemplate and the oracle's tx codec; verifyStdInput by the
oracle with the C restatement's ECDSA), and against hkv_verify_std_txs* with
every in-batch prevout supplied explicitly."""
import random
import struct

import numpy as np
import pytest

import blocktx_model as bm
import sighash_oracle as sh
import stdtx_model as model

pytestmark = pytest.mark.gpu

JOB = np.dtype([("tx", "<u4"), ("input", "<u4"), ("script_off", "<u4"), ("script_len", "<u4"), ("value", "<u8")])
GUARD = 0xA5
NONE = 0xFFFFFFFF


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
    """The txid table's slot hash ANDed with mask inside the block, the default after it."""

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


# --- the index and the lookup alone ---------------------------------------------------

def txid_case(n_tx: int):
    """n_tx txids with duplicates and all-zero entries; queries: every txid,
    near misses (the last byte or the first word flipped, as
    stdtx_model.outpoint_pool does), strangers and zero; the expected index."""
    rng = random.Random(7000 + n_tx)
    ids = []
    for t in range(n_tx):
        u = rng.random()
        if t and u < 0.15:
            ids.append(b"\0" * 32)
        elif t and u < 0.45:
            ids.append(rng.choice(ids))
        else:
            ids.append(rng.randbytes(32))
    index = {}
    for t, h in enumerate(ids):
        if any(h):
            index.setdefault(h, t)
    queries = list(ids) + [b"\0" * 32]
    for h in [x for x in ids if any(x)][:40]:
        queries += [h[:31] + bytes([h[31] ^ 1]), bytes([h[0] ^ 0x80]) + h[1:], rng.randbytes(32)]
    return ids, queries, [index.get(q, NONE) for q in queries]


@pytest.mark.parametrize("n_tx", [1, 63, 64, 65, 257])
def test_txid_index_and_lookup_vs_dict(torch, ver, n_tx):
    import hkv
    ids, queries, want = txid_case(n_tx)
    assert n_tx == 1 or (any(not any(h) for h in ids) and len(set(ids)) < n_tx)
    n_slots = hkv.txid_table_slots(ver, n_tx)
    assert n_slots >= 2 * n_tx and n_slots >= 64 and n_slots & (n_slots - 1) == 0
    d_ids = upload(torch, np.frombuffer(b"".join(ids), dtype=np.uint8))
    # the queries at an odd address: they are read at any alignment
    d_q = upload(torch, np.frombuffer(b"\0" + b"".join(queries), dtype=np.uint8))
    outs = []
    for mask in (0xFFFFFFFF, 0):
        table = guarded(torch, n_slots * 4)
        found = guarded(torch, len(queries) * 4)
        with masked(ver, mask):
            hkv.txid_index_device(ver, 0, d_ids.data_ptr(), n_tx, table.data_ptr(), n_slots)
            hkv.txid_lookup_device(ver, 0, d_ids.data_ptr(), n_tx, table.data_ptr(), n_slots, d_q.data_ptr() + 1,
                                   len(queries), found.data_ptr())
            torch.cuda.synchronize()
        slots, slots_intact = split_guard(table, n_slots * 4)
        got, found_intact = split_guard(found, len(queries) * 4)
        assert slots_intact and found_intact
        got = got.view(np.uint32).tolist()
        assert got == want, [(q, g, w) for q, (g, w) in enumerate(zip(got, want)) if g != w][:10]
        # the table holds exactly the smallest index of every distinct non-zero txid
        held = sorted(int(s) for s in slots.view(np.uint32) if s != NONE)
        assert held == sorted({h: t for t, h in reversed(list(enumerate(ids))) if any(h)}.values())
        outs.append(got)
    assert outs[0] == outs[1]


# --- the provider alone ----------------------------------------------------------------

class DeviceBlock:
    """A batch laid out for the block entry points (tx bytes, then the pool, in
    one buffer) with its prevout arrays, in HBM."""

    def __init__(self, torch, raw_txs, prevouts, patch=None):
        import hkv
        from hkv.sighash import TxBatch
        from hkv.stdtx import pack_prevouts
        self.tb = TxBatch(raw_txs)
        po, outpoints, scripts, values = pack_prevouts(self.tb, prevouts)
        if patch is not None:
            patch(self.tb, po, scripts)
        buf, self.pool_at = hkv.block_layout(self.tb)
        self.n_tx = len(raw_txs)
        self.keep = [upload(torch, a) for a in (buf, self.tb.offsets, po, outpoints, scripts, values)]
        p = [t.data_ptr() for t in self.keep]
        self.txs = hkv.HkvTxs(p[0], p[1], self.n_tx, p[0] + self.pool_at, self.tb._len)
        self.prev = p[2:]
        self.n_slots = int(hkv.load_library().hkv_txid_table_slots(self.n_tx))


def run_provider(torch, ver, b: DeviceBlock, n_inputs: int):
    """hkv_block_tx_jobs_device with n_inputs as the caller's total: (txids,
    input_first, jobs, src, status, every guard intact)."""
    import hkv
    first = torch.full((b.n_tx + 1,), -1, dtype=torch.int32, device="cuda")
    txids = guarded(torch, b.n_tx * 32)
    table = guarded(torch, b.n_slots * 4)
    jobs = guarded(torch, n_inputs * 24)
    src = guarded(torch, n_inputs * 4)
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    hkv.block_tx_jobs_device(ver, 0, b.txs, *b.prev, n_inputs, txids.data_ptr(), table.data_ptr(), b.n_slots,
                             first.data_ptr(), jobs.data_ptr(), src.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    ids, ok1 = split_guard(txids, b.n_tx * 32)
    _, ok2 = split_guard(table, b.n_slots * 4)
    jb, ok3 = split_guard(jobs, n_inputs * 24)
    sr, ok4 = split_guard(src, n_inputs * 4)
    return (ids.tobytes(), first.cpu().numpy().view(np.uint32), jb.view(JOB), sr.view(np.uint32),
            int(status[0].item()), ok1 and ok2 and ok3 and ok4)


class ProviderCase:
    """bm.chained_batch plus two txs whose list entry overruns the pool (by one
    byte; and an offset past the pool's end), with the expected arrays."""

    def __init__(self, torch):
        c = bm.chained_batch(20262, n_fill=250)
        rng = c.rng
        overrun = []
        for name in ("overrun_length", "overrun_offset"):
            op = rng.randbytes(36)
            t = c.add(sh.tx_serialize(bm._tx(rng, [op])), [bm._entry(rng, op)])
            c.name(name, t, 0)
            overrun.append(t)
        self.chain = c

        def patch(tb, po, scripts):
            e = int(po[overrun[0]])
            scripts[2 * e + 1] = tb._len - int(scripts[2 * e]) + 1
            e = int(po[overrun[1]])
            scripts[2 * e], scripts[2 * e + 1] = tb._len + 1, 0

        self.b = DeviceBlock(torch, c.raw, c.prevouts, patch)
        self.first, rows = bm.resolve(c.raw, c.prevouts)
        self.rows = rows
        tb, at = self.b.tb, self.b.pool_at
        self.jobs = np.zeros(len(rows), dtype=JOB)
        self.src = np.zeros(len(rows), dtype=np.uint32)
        for g, (t, i, src, ref, spk, value) in enumerate(rows):
            self.src[g] = src
            if src == bm.SRC_LIST:
                off, ln = tb.script(spk)
                self.jobs[g] = (t, i, 0, 0, value) if t in overrun else (t, i, at + off, ln, value)
            elif src == bm.SRC_NONE:
                self.jobs[g] = (t, i, 0, 0, 0)
            else:
                self.jobs[g] = (t, i, int(tb.offsets[src]) + ref[1], ref[2], value)
        self.at = {(r[0], r[1]): g for g, r in enumerate(rows)}


@pytest.fixture(scope="module")
def provider_case(torch):
    return ProviderCase(torch)


def test_provider_case_holds_every_variant(provider_case):
    pc = provider_case
    src = lambda name: int(pc.src[pc.at[pc.chain.named[name]]])
    job = lambda name: pc.jobs[pc.at[pc.chain.named[name]]]
    earlier = ("plain_parent", "zero_length_parent_script", "bip144_parent", "noncanonical_parent_txhash",
               "fd_form_parent", "duplicate_parents_between", "duplicate_parents_after", "shared_outpoint_batch")
    nothing = ("index_equals_count", "index_past_count", "index_ffffffff", "bip144_wire_hash",
               "noncanonical_parent_wire_hash", "forward_reference", "unparsable_parent", "coinbase_form")
    listed = ("list_precedence", "shared_outpoint_list", "overrun_length", "overrun_offset")
    assert set(earlier + nothing + listed) == set(pc.chain.named)
    assert all(src(n) < pc.chain.named[n][0] for n in earlier)
    assert all(src(n) == bm.SRC_NONE and job(n)["script_len"] == 0 for n in nothing)
    assert all(src(n) == bm.SRC_LIST for n in listed)
    assert job("zero_length_parent_script")["script_len"] == 0 and job("zero_length_parent_script")["script_off"] > 0
    assert job("overrun_length")["script_len"] == 0 and job("overrun_offset")["script_off"] == 0
    assert job("list_precedence")["script_off"] >= pc.b.pool_at > job("plain_parent")["script_off"]
    assert len(pc.chain.raw) > 250


@pytest.mark.parametrize("mask", [0xFFFFFFFF, 0], ids=["hashed", "one_chain"])
def test_provider_vs_model(torch, ver, provider_case, mask):
    pc = provider_case
    n = int(pc.first[-1])
    with masked(ver, mask):
        ids, first, jobs, src, status, intact = run_provider(torch, ver, pc.b, n)
    assert intact and status == 0
    assert ids == b"".join(bm.tx_ids(pc.chain.raw))
    assert first.tolist() == pc.first
    bad = np.nonzero((jobs != pc.jobs) | (src != pc.src))[0]
    assert bad.size == 0, [(int(g), pc.rows[g][:3], jobs[g], int(src[g]), pc.jobs[g], int(pc.src[g])) for g in bad[:5]]


def test_provider_count_mismatch(torch, ver, provider_case):
    """n_inputs one too few and one too many: HKV_STATUS_INPUT_COUNT, the jobs
    and src words that fit, a never-verifying job and HKV_SRC_NONE in the
    surplus slot, nothing written past n_inputs either way."""
    from hkv.lib import HKV_STATUS_INPUT_COUNT
    pc = provider_case
    n = int(pc.first[-1])
    _, first, jobs, src, status, intact = run_provider(torch, ver, pc.b, n - 1)
    assert status == HKV_STATUS_INPUT_COUNT and intact and first.tolist() == pc.first
    assert (jobs == pc.jobs[:n - 1]).all() and (src == pc.src[:n - 1]).all()
    _, first, jobs, src, status, intact = run_provider(torch, ver, pc.b, n + 1)
    assert status == HKV_STATUS_INPUT_COUNT and intact and first.tolist() == pc.first
    assert (jobs[:n] == pc.jobs).all() and (src[:n] == pc.src).all()
    assert jobs[n].tolist() == (0xFFFFFFFF, 0, 0, 0, 0) and int(src[n]) == NONE


def test_pool_in_front_of_the_tx_bytes_is_rejected(torch, ver, provider_case):
    import hkv
    b = provider_case.b
    txs = hkv.HkvTxs(b.txs.bytes + 64, b.txs.offsets, b.n_tx, b.txs.bytes, 32)
    z = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(hkv.HkvError) as e:
        hkv.block_tx_jobs_device(ver, 0, txs, *b.prev, 0, z.data_ptr(), z.data_ptr(), b.n_slots, z.data_ptr(), 0, 0,
                                 z.data_ptr())
    assert e.value.rc == -1
    with pytest.raises(hkv.HkvError) as e:   # a table smaller than the sizing rule's
        hkv.block_tx_jobs_device(ver, 0, b.txs, *b.prev, 0, z.data_ptr(), z.data_ptr(), b.n_slots // 2, z.data_ptr(),
                                 0, 0, z.data_ptr())
    assert e.value.rc == -1


# --- the composed call end to end ----------------------------------------------------------

class World:
    """bm.SignedChain and its damaged copies, with the oracle's verifyStdInput behind a memo."""

    def __init__(self, coracle, forkid):
        self.forkid = forkid
        self.chain = c = bm.SignedChain(9100 + (forkid or 0), forkid, n=48)
        ok = model.oracle_input_ok(coracle, forkid)
        memo = {}

        def input_ok_of(raw):
            def f(tx, i, spk, val):
                key = (raw, i, spk, val)
                if key not in memo:
                    memo[key] = bool(ok(tx, i, spk, val))
                return memo[key]
            return f
        self.input_ok_of = input_ok_of
        self.batches = {"good": (c.raw, c.prevouts)}
        # a flipped byte in a parent's output script: its txid changes, its children's inputs find nothing
        p = max(range(len(c.raw)), key=lambda t: len(c.children_of(t)))
        self.parent, self.children = p, c.children_of(p)
        ref = bm.output_refs(c.raw[p])[0]
        raw = bytearray(c.raw[p])
        raw[ref[0] + 3] ^= 1
        self.batches["parent_script"] = (c.raw[:p] + [bytes(raw)] + c.raw[p + 1:], c.prevouts)
        # a wrong amount under BIP143 (a listed witness prevout: the amount is signed)
        t = next(t for t in range(len(c.raw)) if any(len(e[1]) == 22 for e in c.prevouts[t]))
        k = next(k for k, e in enumerate(c.prevouts[t]) if len(e[1]) == 22)
        prevouts = [list(x) for x in c.prevouts]
        e = prevouts[t][k]
        prevouts[t][k] = (e[0], e[1], e[2] + 1)
        self.amount_tx = t
        self.batches["amount"] = (c.raw, prevouts)
        # a child moved in front of its parent
        child = self.children[0]
        order = list(range(len(c.raw)))
        order[p], order[child] = order[child], order[p]
        self.moved_to = p
        self.batches["moved"] = ([c.raw[t] for t in order], [c.prevouts[t] for t in order])

    def expect(self, name):
        raws, prevouts = self.batches[name]
        return bm.verify_block_txs(raws, prevouts, self.input_ok_of)


_WORLDS = {}


@pytest.fixture(scope="module", params=[None, 0], ids=["btc", "forkid0"])
def world(request, coracle):
    if request.param not in _WORLDS:
        _WORLDS[request.param] = World(coracle, request.param)
    return _WORLDS[request.param]


def test_signed_chain_spends_every_kind_in_the_batch(world):
    c = world.chain
    in_batch = [k for s in c.spends for (k, parent) in s if parent is not None]
    assert set(in_batch) == set(bm.KINDS) and len(in_batch) > 30
    assert sum(1 for s in c.spends for (_, parent) in s if parent is None) > 20
    assert len(world.children) >= 2


@pytest.mark.parametrize("name", ["good", "parent_script", "amount", "moved"])
def test_block_txs_vs_model_host_and_device_forms(ver, world, name):
    import hkv
    raws, prevouts = world.batches[name]
    want = world.expect(name)
    first, rows = bm.resolve(raws, prevouts)
    want_src = [[r[2] for r in rows[first[t]:first[t + 1]]] for t in range(len(raws))]
    got, src = hkv.verify_block_txs_host(ver, raws, prevouts, world.forkid)
    assert got == want, [(t, got[t], want[t]) for t in range(len(want)) if got[t] != want[t]]
    assert src == want_src
    ok, per_input, dsrc = hkv.verify_block_txs_detail(ver, raws, prevouts, world.forkid)
    assert ok == want and dsrc == want_src
    assert ok == [bool(p) and all(p) for p in per_input]
    with masked(ver, 0):
        assert hkv.verify_block_txs(ver, raws, prevouts, world.forkid) == want
        assert hkv.verify_block_txs_detail(ver, raws, prevouts, world.forkid) == (ok, per_input, dsrc)
    # the differential: every in-batch prevout supplied explicitly, through hkv_verify_std_txs
    assert hkv.verify_std_txs(ver, raws, bm.augmented(raws, prevouts), world.forkid) == got
    if name == "good":
        assert all(want)
    elif name == "parent_script":
        bad = sorted(t for t in range(len(want)) if not want[t])
        assert bad == sorted([world.parent] + world.children)
        assert all(NONE in want_src[t] for t in world.children)
    elif name == "amount":
        assert [t for t in range(len(want)) if not want[t]] == [world.amount_tx]
    else:
        assert not want[world.moved_to] and NONE in want_src[world.moved_to] and sum(want) >= len(want) - 3


def test_random_script_batch_equals_verify_std_txs_on_augmented_lists(ver, provider_case):
    """The provider's batch (random scripts: every verdict is false but for no
    reason the two calls could differ in) through both calls."""
    import hkv
    c = provider_case.chain
    got = hkv.verify_block_txs(ver, c.raw, c.prevouts, None)
    assert got == hkv.verify_std_txs(ver, c.raw, bm.augmented(c.raw, c.prevouts), None)
    assert not any(got)


def run_composed(torch, ver, b, forkid, n_inputs, block: bool):
    """The composed device call of either kind on batch b: (tx words, input
    words, input_first, status)."""
    import hkv
    first = torch.zeros(b.n_tx + 1, dtype=torch.int32, device="cuda")
    jobs = torch.zeros(max(1, n_inputs) * 24, dtype=torch.uint8, device="cuda")
    recs = torch.zeros(max(1, n_inputs) * 168, dtype=torch.uint8, device="cuda")
    bits = torch.zeros((n_inputs + 63) // 64 * 2 + 2, dtype=torch.int32, device="cuda")
    tx_bits = torch.full(((b.n_tx + 63) // 64 * 2,), -1, dtype=torch.int32, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    fk = -1 if forkid is None else forkid
    if block:
        txids = torch.zeros(b.n_tx * 32, dtype=torch.uint8, device="cuda")
        table = torch.zeros(b.n_slots, dtype=torch.int32, device="cuda")
        src = torch.zeros(max(1, n_inputs), dtype=torch.int32, device="cuda")
        hkv.verify_block_txs_device(ver, 0, b.txs, *b.prev, fk, n_inputs, txids.data_ptr(), table.data_ptr(),
                                    b.n_slots, first.data_ptr(), jobs.data_ptr(), src.data_ptr(), recs.data_ptr(),
                                    bits.data_ptr(), tx_bits.data_ptr(), status.data_ptr())
    else:
        hkv.verify_std_txs_device(ver, 0, b.txs, *b.prev, fk, n_inputs, first.data_ptr(), jobs.data_ptr(),
                                  recs.data_ptr(), bits.data_ptr(), tx_bits.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    n_words = (min(n_inputs, int(first[b.n_tx].item())) + 31) // 32
    return (tx_bits.cpu().numpy().tobytes(), bits.cpu().numpy()[:n_words].tobytes(), first.cpu().numpy().tobytes(),
            int(status[0].item()))


def test_all_empty_lists_and_no_pool(torch, ver, world):
    """A batch without a single list entry, so without a script pool: the txs
    whose inputs all spend earlier outputs of the chain verify, the others
    find nothing. The device form takes a zero-length pool at the end of the
    tx bytes (the pointer is its only bound on them) and refuses a null one."""
    import hkv
    raws = world.chain.raw
    empty = [[] for _ in raws]
    want = bm.verify_block_txs(raws, empty, world.input_ok_of)
    in_batch_only = [all(parent is not None for _, parent in s) for s in world.chain.spends]
    assert want == in_batch_only and sum(want) >= 8 and not all(want)
    b = DeviceBlock(torch, raws, empty)
    assert b.tb._len == 0 and b.txs.scripts_len == 0
    n = bm.resolve(raws, empty)[0][-1]
    fk = -1 if world.forkid is None else world.forkid
    ends = int(b.tb.offsets[-1])
    for pool in (b.txs.bytes + ends, b.txs.bytes + b.pool_at):
        b.txs = hkv.HkvTxs(b.txs.bytes, b.txs.offsets, b.n_tx, pool, 0)
        words = run_composed(torch, ver, b, world.forkid, n, True)
        got = np.unpackbits(np.frombuffer(words[0], dtype=np.uint8), bitorder="little")[:len(raws)].astype(bool)
        assert got.tolist() == want and words[3] == 0
    assert hkv.verify_block_txs(ver, raws, empty, world.forkid) == want
    assert hkv.verify_block_txs_detail(ver, raws, empty, world.forkid)[0] == want
    # no pool pointer at all: nothing bounds the tx bytes, HKV_E_ARG from both device forms
    null = hkv.HkvTxs(b.txs.bytes, b.txs.offsets, b.n_tx, None, 0)
    z = torch.zeros(max(1 << 16, n * 168), dtype=torch.uint8, device="cuda")
    with pytest.raises(hkv.HkvError) as e:
        hkv.block_tx_jobs_device(ver, 0, null, *b.prev, n, z.data_ptr(), z.data_ptr(), b.n_slots, z.data_ptr(),
                                 z.data_ptr(), z.data_ptr(), z.data_ptr())
    assert e.value.rc == -1
    with pytest.raises(hkv.HkvError) as e:
        hkv.verify_block_txs_device(ver, 0, null, *b.prev, fk, n, z.data_ptr(), z.data_ptr(), b.n_slots, z.data_ptr(),
                                    z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                                    z.data_ptr())
    assert e.value.rc == -1


def test_no_in_batch_spends_is_verify_std_txs_bit_for_bit(torch, ver, world):
    """With every prevout in the lists the block call is hkv_verify_std_txs*:
    the same tx words, input words, prefix sums and status, also for a batch
    that sets HKV_STATUS_INPUT_COUNT."""
    from hkv.lib import HKV_STATUS_INPUT_COUNT
    raws, prevouts = world.batches["amount"]
    aug = bm.augmented(raws, prevouts)
    first, rows = bm.resolve(raws, aug)
    assert all(r[2] == bm.SRC_LIST for r in rows)
    b = DeviceBlock(torch, raws, aug)
    n = first[-1]
    for n_inputs in (n, n - 1, n + 1):
        block = run_composed(torch, ver, b, world.forkid, n_inputs, True)
        std = run_composed(torch, ver, b, world.forkid, n_inputs, False)
        assert block == std
        assert block[3] == (0 if n_inputs == n else HKV_STATUS_INPUT_COUNT)
        tx = np.unpackbits(np.frombuffer(block[0], dtype=np.uint8), bitorder="little")[:len(raws)]
        if n_inputs == n:
            assert tx.sum() == len(raws) - 1 and not tx[world.amount_tx]
        else:
            assert not tx.any()


# --- the host forms' prevout arrays need not start at entry 0 -----------------------------------

def _one_input_spend(rng, outpoint, kind, who, value, out_spk):
    """A signed tx with one input of ``kind`` on ``outpoint`` and one output."""
    tx = sh.Tx(2, [sh.TxIn(outpoint[:32], struct.unpack("<I", outpoint[32:])[0], b"", 0xFFFFFFFF)],
               [sh.TxOut(value - 1000, out_spk)], [[]], 0)
    bm._sign_input(rng, tx, 0, kind, who, value, None)
    return sh.tx_serialize(tx)


def test_host_forms_with_prevout_lists_that_start_past_entry_0(ver, coracle):
    """hkv_verify_std_txs, hkv_verify_block_txs and hkv_verify_block_txs_spends
    with prev_offsets[0] = 3: three entries no list names stand in front of
    the lists' own, one of them the very prevout tx 1 lacks. Only the entries
    the offsets name are staged, the offsets rebased: every output equals
    that of the call whose arrays start at entry 0, and the verdicts are the
    models'."""
    import ctypes
    import secp256k1_oracle as o
    import spends_model as sm
    import txgen
    from hkv.sighash import TxBatch
    from hkv.stdtx import pack_prevouts
    rng = random.Random(20303)
    ka, kb, kc, kd = (txgen.Key(rng.randrange(1, o.N)) for _ in range(4))
    ext = [rng.randbytes(32) + struct.pack("<I", k) for k in range(3)]
    value = 5 * 10**8
    # 0: a P2PKH spend, its prevout listed; it pays kb, whom tx 3 spends in the batch
    # 1: a P2PKH spend with an empty list (its prevout is nowhere in the batch)
    # 2: a P2WPKH spend (the amount is signed) whose listed prevout is one satoshi off
    # 3: the child of tx 0, its prevout not listed
    raws = [_one_input_spend(rng, ext[0], "p2pkh", ka, value, bm._spk("p2pkh", kb)),
            _one_input_spend(rng, ext[1], "p2pkh", kc, value, bm._spk("p2pkh", kd)),
            _one_input_spend(rng, ext[2], "p2wpkh", kd, value, bm._spk("p2pkh", ka))]
    raws.append(_one_input_spend(rng, bm.tx_hash(raws[0]) + struct.pack("<I", 0), "p2pkh", kb, value - 1000,
                                 bm._spk("p2wpkh", kc)))
    lacking = (ext[1], bm._spk("p2pkh", kc), value)
    prevouts = [[(ext[0], bm._spk("p2pkh", ka), value)], [], [(ext[2], bm._spk("p2wpkh", kd), value + 1)], []]
    ok = model.oracle_input_ok(coracle, None)
    # (txs 1 and 2 are signed well: the entry tx 1 lacks, and tx 2's at the right value, verify them)
    assert model.verify_std_tx(raws[1], [lacking], ok)
    assert model.verify_std_tx(raws[2], [(ext[2], prevouts[2][0][1], value)], ok)
    want_std = [model.verify_std_tx(r, p, ok) for r, p in zip(raws, prevouts)]
    want_block = bm.verify_block_txs(raws, prevouts, lambda raw: ok)
    assert want_std == [True, False, False, False] and want_block == [True, False, False, True]

    n_tx = len(raws)
    tb = TxBatch(raws)
    offsets, outpoints, scripts, values = pack_prevouts(tb, prevouts)
    front = [(rng.randbytes(36), rng.randbytes(25), 7), lacking, (ext[0], rng.randbytes(22), value)]
    f_scripts = np.array([w for e in front for w in tb.script(e[1])], dtype=np.uint32)
    st, pool = tb.struct()    # (after every script has gone into the pool)
    assert offsets.tolist() == [0, 1, 1, 2, 2]
    shifted = ((offsets + 3).astype(np.uint32),
               np.concatenate([np.frombuffer(b"".join(e[0] for e in front), dtype=np.uint8), outpoints]),
               np.concatenate([f_scripts, scripts]),
               np.concatenate([np.array([e[2] for e in front], dtype=np.uint64), values]))
    assert shifted[0][0] == 3 and len(shifted[1]) == 5 * 36 and len(shifted[2]) == 10 and len(shifted[3]) == 5
    cap = int(tb.offsets[-1]) // 41 + 1
    P = ctypes.POINTER(ctypes.c_uint32)

    def run(prev):
        head = (ver.ctx, ctypes.byref(st)) + tuple(a.ctypes.data for a in prev)
        out = {}

        def arrays():
            return (np.zeros(1, dtype=np.uint32), np.full(n_tx + 1, 0x5A5A5A5A, dtype=np.uint32),
                    np.full(cap, 0x5A5A5A5A, dtype=np.uint32))

        w, _, _ = arrays()
        assert ver.lib.hkv_verify_std_txs(*head, -1, w.ctypes.data_as(P)) == 0
        out["std"] = w.tolist()
        w, first, src = arrays()
        assert ver.lib.hkv_verify_block_txs(*head, -1, w.ctypes.data_as(P), first.ctypes.data, src.ctypes.data, cap) == 0
        out["block"] = (w.tolist(), first.tolist(), src.tolist())
        w, first, src = arrays()
        spender = np.full(cap, 0x5A5A5A5A, dtype=np.uint32)
        sums = np.full(2 * n_tx, 0x5A5A5A5A, dtype=np.uint64)
        flags = np.full(n_tx, 0x5A, dtype=np.uint8)
        assert ver.lib.hkv_verify_block_txs_spends(*head, -1, sm.MAX_MONEY, w.ctypes.data_as(P), first.ctypes.data,
                                                   src.ctypes.data, spender.ctypes.data, cap, sums.ctypes.data,
                                                   flags.ctypes.data) == 0
        out["spends"] = (w.tolist(), first.tolist(), src.tolist(), spender.tolist(), sums.tolist(), flags.tolist())
        return out

    at0, at3 = run((offsets, outpoints, scripts, values)), run(shifted)
    assert at3 == at0
    bits = lambda word: [bool(word >> t & 1) for t in range(n_tx)]
    assert bits(at0["std"][0]) == want_std
    assert bits(at0["block"][0][0]) == want_block and bits(at0["spends"][0][0]) == want_block
    assert at0["block"][1] == [0, 1, 2, 3, 4] and at0["block"][2][:4] == [bm.SRC_LIST, bm.SRC_NONE, bm.SRC_LIST, 0]
    assert at0["spends"][:3] == at0["block"]
    s = sm.Spends(raws, prevouts, sm.MAX_MONEY)
    assert at0["spends"][3][:4] == s.spender and at0["spends"][5] == s.flags
    assert [tuple(at0["spends"][4][2 * t:2 * t + 2]) for t in range(n_tx)] == s.sums
