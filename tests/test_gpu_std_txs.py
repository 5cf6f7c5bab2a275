"""GPU tests (MI355X) of batch verifyStdTx: the job builder alone, the per-tx
reduction alone, and the composed call end to end, each against
tests/stdtx_model.py (matchTemplate / verifyStdTx restated on the oracle's tx
codec, verifyStdInput by the oracle with the C restatement's ECDSA)."""
import random
import struct
import time

import numpy as np
import pytest

import secp256k1_oracle as o
import sighash_oracle as sh
import stdtx_model as model
import txgen

pytestmark = pytest.mark.gpu

JOB = np.dtype([("tx", "<u4"), ("input", "<u4"), ("script_off", "<u4"), ("script_len", "<u4"), ("value", "<u8")])
GUARD = 0xA5


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


def upload(torch, arr: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()


def download(t, dtype):
    return t.cpu().numpy().view(dtype)


class DeviceBatch:
    """A tx batch and its prevout arrays in HBM (the arrays of include/hkv.h)."""

    def __init__(self, torch, tx_bytes, tx_offsets, pool, po, outpoints, scripts, values):
        import hkv
        self.n_tx = len(tx_offsets) - 1
        arrays = (tx_bytes, tx_offsets, pool, po, outpoints, scripts, values)
        self.keep = [upload(torch, a if a.size else np.zeros(8, dtype=np.uint8)) for a in arrays]   # (no null pointers)
        p = [t.data_ptr() for t in self.keep]
        self.txs = hkv.HkvTxs(p[0], p[1], self.n_tx, p[2], len(pool))
        self.prev = p[3:]

    @classmethod
    def of(cls, torch, raw_txs, prevouts):
        from hkv.sighash import TxBatch
        from hkv.stdtx import pack_prevouts
        tb = TxBatch(raw_txs)
        po, outpoints, scripts, values = pack_prevouts(tb, prevouts)
        _, pool = tb.struct()
        b = cls(torch, tb.bytes, tb.offsets, pool[:max(1, tb._len)], po, outpoints, scripts, values)
        b.tb = tb
        return b


def run_builder(torch, ver, b: DeviceBatch, n_inputs: int):
    """hkv_std_tx_jobs_device with n_inputs as the caller's total:
    (input_first, the n_inputs jobs, status, guard bytes after d_jobs intact)."""
    import hkv
    first = torch.full((b.n_tx + 1,), -1, dtype=torch.int32, device="cuda")
    jobs = torch.full((n_inputs * 24 + 256,), GUARD, dtype=torch.uint8, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    hkv.std_tx_jobs_device(ver, 0, b.txs, *b.prev, n_inputs, first.data_ptr(), jobs.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    jb = jobs.cpu().numpy()
    return (download(first, np.uint32), jb[:n_inputs * 24].view(JOB), int(status[0].item()),
            bool((jb[n_inputs * 24:] == GUARD).all()))


# --- the job builder alone -------------------------------------------------------

class Variants:
    """64 distinct (tx, entry list) pairs of 0-3 inputs — plain, BIP144 form,
    without inputs, and not parsing — with the model's answer for each, so
    batches of any size are assembled (and expected) by numpy gathers."""

    def __init__(self):
        from hkv.sighash import TxBatch
        rng = random.Random(4107)
        pool = TxBatch([])
        self.raw, self.cnt, self.jobs, self.po, self.ps, self.pv = [], [], [], [], [], []
        kinds = ["plain"] * 5 + ["segwit"] * 2 + ["empty", "truncated", "trailing"]
        for k in range(64):
            kind = kinds[k % len(kinds)]
            ops = model.outpoint_pool(rng)
            tx = model.dup_tx(rng, 0 if kind == "empty" else rng.randrange(1, 4), ops)
            if kind == "empty":
                tx.outputs = [sh.TxOut(5, b"\x51"), sh.TxOut(6, b"")]   # (an output count of 1 would read as the BIP144 flag)
            if kind == "segwit":
                tx.witness = [[rng.randbytes(rng.choice([1, 33, 72]))] for _ in tx.inputs]
            raw = sh.tx_serialize(tx)
            if kind == "truncated":
                raw = raw[:-1]
            elif kind == "trailing":
                raw = raw + b"\x00"
            entries = model.entry_list(rng, tx, ops) if tx.inputs else [(rng.randbytes(36), b"\x51", 7)]
            first, mj = model.model_jobs([raw], [entries])
            assert first[1] == (len(tx.inputs) if kind in ("plain", "segwit") else 0), kind
            ja = np.zeros(len(mj), dtype=JOB)
            for g, (_, i, spk, val) in enumerate(mj):
                so, sl = pool.script(spk) if spk is not None else (0, 0)
                ja[g] = (0, i, so, sl, val)
            self.raw.append(raw)
            self.cnt.append(len(mj))
            self.jobs.append(ja)
            self.po.append(np.frombuffer(b"".join(e[0] for e in entries), dtype=np.uint8))
            self.ps.append(np.array([x for e in entries for x in pool.script(e[1])], dtype=np.uint32))
            self.pv.append(np.array([e[2] for e in entries], dtype=np.uint64))
        self.pool = pool.struct()[1][:pool._len].copy()
        self.cnt = np.array(self.cnt)
        assert {0, 1, 2, 3} <= set(self.cnt.tolist())

    def batch(self, torch, ids):
        """(DeviceBatch, expected input_first, expected jobs) of txs ids[0..]."""
        raws = [self.raw[k] for k in ids]
        tx_off = np.zeros(len(ids) + 1, dtype=np.uint32)
        tx_off[1:] = np.cumsum([len(r) for r in raws])
        po = np.zeros(len(ids) + 1, dtype=np.uint32)
        po[1:] = np.cumsum([len(self.pv[k]) for k in ids])
        first = np.zeros(len(ids) + 1, dtype=np.uint32)
        first[1:] = np.cumsum(self.cnt[ids])
        jobs = np.concatenate([self.jobs[k] for k in ids])
        jobs["tx"] = np.repeat(np.arange(len(ids), dtype=np.uint32), self.cnt[ids])
        b = DeviceBatch(torch, np.frombuffer(b"".join(raws), dtype=np.uint8), tx_off, self.pool,
                        po, np.concatenate([self.po[k] for k in ids]), np.concatenate([self.ps[k] for k in ids]),
                        np.concatenate([self.pv[k] for k in ids]))
        return b, first, jobs


@pytest.fixture(scope="module")
def variants():
    return Variants()


# 65,537 is one more than two levels of 256-wide blocks cover. The scan here is
# shaped differently — 8 counts per lane, 64 lanes per wave, 16 waves per tile
# of 8,192, tiles in sequence — so one more than each of its levels covers is
# added: 9, 513, 8,193 (and 65,537 runs nine tiles).
@pytest.mark.parametrize("n_tx", [1, 8, 9, 63, 64, 65, 255, 256, 257, 512, 513, 8192, 8193, 65537])
def test_job_builder_vs_model(torch, ver, variants, n_tx):
    rng = np.random.default_rng(n_tx)
    ids = rng.integers(0, 64, size=n_tx)
    if n_tx == 1:
        ids[:] = 0   # (a plain tx with inputs)
    b, first, jobs = variants.batch(torch, ids)
    n = int(first[-1])
    got_first, got_jobs, status, intact = run_builder(torch, ver, b, n)
    assert (got_first == first).all(), np.nonzero(got_first != first)[0][:10]
    assert status == 0 and intact
    bad = np.nonzero(got_jobs != jobs)[0]
    assert bad.size == 0, [(int(g), got_jobs[g], jobs[g]) for g in bad[:5]]


@pytest.mark.parametrize("nin", [300, 2500])
def test_job_builder_one_large_tx(torch, ver, nin):
    """One tx of many inputs between two small ones: half its inputs on three
    outpoints (ranks up to nin / 6 and beyond), half on outpoints of their own."""
    rng = random.Random(nin)
    ops = model.outpoint_pool(rng)
    tx = model.dup_tx(rng, nin, ops + [rng.randbytes(36) for _ in range(nin // 2)], script_lens=(0, 1, 25, 253))
    small = model.dup_tx(rng, 2, ops)
    raws = [sh.tx_serialize(small), sh.tx_serialize(tx), sh.tx_serialize(small)]
    prevouts = [model.entry_list(rng, small, ops), model.entry_list(rng, tx, ops), []]
    del prevouts[1][::7]   # (some inputs find no entry, whatever entry_list drew)
    first, mj = model.model_jobs(raws, prevouts)
    assert first == [0, 2, 2 + nin, 4 + nin]
    b = DeviceBatch.of(torch, raws, prevouts)
    got_first, got_jobs, status, intact = run_builder(torch, ver, b, len(mj))
    assert got_first.tolist() == first and status == 0 and intact
    want = np.zeros(len(mj), dtype=JOB)
    for g, (t, i, spk, val) in enumerate(mj):
        want[g] = (t, i) + (b.tb.script(spk) if spk is not None else (0, 0)) + (val,)
    bad = np.nonzero(got_jobs != want)[0]
    assert bad.size == 0, [(int(g), got_jobs[g], want[g]) for g in bad[:5]]
    assert sum(1 for j in mj if j[2] is None) > 0 and sum(1 for j in mj if j[2] is not None) > nin // 2


def test_job_builder_count_mismatch(torch, ver, variants):
    """n_inputs one too few and one too many: HKV_STATUS_INPUT_COUNT, the jobs
    that fit, a never-verifying job in the surplus slot, and nothing written
    past n_inputs jobs either way."""
    from hkv.lib import HKV_STATUS_INPUT_COUNT
    ids = np.random.default_rng(5).integers(0, 64, size=300)
    ids[-1] = 0   # (the last tx has inputs)
    b, first, jobs = variants.batch(torch, ids)
    n = int(first[-1])
    got_first, got_jobs, status, intact = run_builder(torch, ver, b, n - 1)
    assert status == HKV_STATUS_INPUT_COUNT and intact
    assert (got_first == first).all() and (got_jobs == jobs[:n - 1]).all()
    got_first, got_jobs, status, intact = run_builder(torch, ver, b, n + 1)
    assert status == HKV_STATUS_INPUT_COUNT and intact
    assert (got_first == first).all() and (got_jobs[:n] == jobs).all()
    assert got_jobs[n].tolist() == (0xFFFFFFFF, 0, 0, 0, 0)
    got_first, got_jobs, status, intact = run_builder(torch, ver, b, n)
    assert status == 0 and intact and (got_jobs == jobs).all()


# --- the reduction alone -----------------------------------------------------------

def reduction_case(rng, n_tx):
    """Input ranges of every shape against the 32-bit words (empty, inside a
    word, from and to mid-word, over more than 64 bits) with bit patterns:
    all ones, all ones but the first / the last / a bit next to a word
    boundary, and random."""
    counts = rng.choice([0, 0, 1, 2, 5, 31, 32, 33, 63, 64, 65, 100, 200], size=n_tx)
    first = np.zeros(n_tx + 1, dtype=np.uint32)
    first[1:] = np.cumsum(counts)
    bits = np.ones(int(first[-1]) + 64, dtype=np.uint8)
    for t in range(n_tx):
        b, e = int(first[t]), int(first[t + 1])
        if e == b:
            continue
        pat = rng.integers(0, 6)
        if pat == 1:
            bits[b] = 0
        elif pat == 2:
            bits[e - 1] = 0
        elif pat == 3:      # the last bit of a word, or the first of the next, where the range has one
            edge = [g for g in range(b, e) if g % 32 in (0, 31)]
            if edge:
                bits[edge[rng.integers(0, len(edge))]] = 0
        elif pat == 4:
            bits[b:e] = rng.integers(0, 2, size=e - b)
        elif pat == 5 and e - b > 2:
            bits[rng.integers(b + 1, e - 1)] = 0
    bits[int(first[-1]):] = rng.integers(0, 2, size=64)   # (beyond the last input: never read into a verdict)
    want = np.array([first[t + 1] > first[t] and bits[first[t]:first[t + 1]].all() for t in range(n_tx)])
    return first, bits, want


@pytest.mark.parametrize("n_tx", [1, 63, 64, 65, 127, 128, 129, 1000])
def test_tx_verdicts_vs_numpy(torch, ver, n_tx):
    import hkv
    rng = np.random.default_rng(900 + n_tx)
    first, bits, want = reduction_case(rng, n_tx)
    words = np.packbits(bits, bitorder="little")
    words = np.concatenate([words, np.zeros(-len(words) % 8, dtype=np.uint8)]).view(np.uint32)
    n_words = (n_tx + 63) // 64 * 2
    out = torch.full((n_words + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_first, d_bits = upload(torch, first), upload(torch, words)
    hkv.tx_verdicts_device(ver, 0, d_first.data_ptr(), n_tx, d_bits.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    w = download(out, np.uint32)
    assert (w[n_words:] == 0x5A5A5A5A).all()                   # exactly ceil(n_tx/64)*2 words are written
    exp = np.zeros(n_words * 32, dtype=np.uint8)
    exp[:n_tx] = want
    assert (w[:n_words] == np.packbits(exp, bitorder="little").view(np.uint32)).all(), \
        np.nonzero(np.unpackbits(w[:n_words].view(np.uint8), bitorder="little")[:n_tx] != want)[0][:10]
    if n_tx >= 63:
        assert want.any() and not want.all()


# --- end to end ----------------------------------------------------------------------

class World:
    """A signed block (txgen.std_block: ~300 txs of every single-key template)
    plus txgen.multisig_cases, one prevout entry per signed input, and the
    oracle's verifyStdInput behind a memo."""

    def __init__(self, coracle, forkid):
        self.forkid = forkid
        rng = random.Random(8800 + (forkid or 0))
        keys = [txgen.Key(rng.randrange(1, o.N), compressed=(k % 4 != 0)) for k in range(24)]
        btxs, bjobs = txgen.std_block(rng, 300, keys, forkid=forkid, p2wpkh_share=0.3, p2pk_share=0.2, p2sh_share=0.2)
        mtxs, mjobs, self.names = txgen.multisig_cases(rng, keys, forkid)
        self.n_block = len(btxs)
        self.txs = btxs + mtxs
        self.raw = [sh.tx_serialize(t) for t in self.txs]
        self.jobs = bjobs + [(t + len(btxs), i, p, v) for (t, i, p, v) in mjobs]
        self.prevouts = [[] for _ in self.raw]
        for (t, i, spk, val) in self.jobs:
            self.prevouts[t].append((self.txs[t].inputs[i].outpoint(), spk, val))
        for p in self.prevouts:
            rng.shuffle(p)
        self.rng = rng
        self._ok = model.oracle_input_ok(coracle, forkid)
        self._memo = {}

    def input_ok(self, raw):
        def f(tx, i, spk, val):
            key = (raw, i, spk, val)
            if key not in self._memo:
                self._memo[key] = bool(self._ok(tx, i, spk, val))
            return self._memo[key]
        return f

    def expect(self, raws, prevouts):
        return [model.verify_std_tx(r, p, self.input_ok(r)) for r, p in zip(raws, prevouts)]


_WORLDS = {}


def get_world(coracle, forkid):
    if forkid not in _WORLDS:
        _WORLDS[forkid] = World(coracle, forkid)
    return _WORLDS[forkid]


@pytest.fixture(scope="module", params=[None, 0], ids=["btc", "forkid0"])
def world(request, coracle):
    return get_world(coracle, request.param)


def test_std_txs_shuffled_lists_vs_model(ver, world):
    """Every tx of the signed block verifies from its shuffled list; the
    multisig cases (valid and adversarial, some with an input nobody signed)
    follow the model."""
    import hkv
    want = world.expect(world.raw, world.prevouts)
    got = hkv.verify_std_txs(ver, world.raw, world.prevouts, world.forkid)
    bad = [(t, got[t], want[t]) for t in range(len(want)) if got[t] != want[t]]
    assert not bad, bad[:10]
    assert all(got[:world.n_block])
    ms = got[world.n_block:]
    assert sum(ms) > 20 and len(ms) - sum(ms) > 400
    assert {nm.split("-")[0] for nm in world.names} == {"bare", "p2sh", "p2wsh", "p2sh_p2wsh"}


def test_std_txs_mutations_reject_exactly_their_txs(ver, world):
    """One entry removed, one value changed (a BIP143 input: the amount is
    signed), one script swapped, one signature byte flipped: exactly those four
    txs of the block turn false."""
    import hkv
    rng = random.Random(61)
    raws, prevouts = list(world.raw), [list(p) for p in world.prevouts]
    seg = [t for t in range(world.n_block) if any(len(e[1]) in (22, 23) for e in prevouts[t])]
    picks = rng.sample([t for t in range(world.n_block) if t not in seg[:1]], 3)
    t_removed, t_script, t_sig = picks
    t_value = seg[0]
    prevouts[t_removed].pop(rng.randrange(len(prevouts[t_removed])))
    k = next(k for k, e in enumerate(prevouts[t_value]) if len(e[1]) in (22, 23))
    e = prevouts[t_value][k]
    prevouts[t_value][k] = (e[0], e[1], e[2] + 1)
    e = prevouts[t_script][0]
    other = next(x[1] for p in world.prevouts for x in p if x[1] != e[1] and len(x[1]) == len(e[1]))
    prevouts[t_script][0] = (e[0], other, e[2])
    tx = sh.tx_parse(raws[t_sig])
    if tx.witness and tx.witness[0]:
        w = tx.witness[0][0]
        tx.witness[0][0] = w[:8] + bytes([w[8] ^ 1]) + w[9:]
    else:
        s = tx.inputs[0].script
        tx.inputs[0].script = s[:9] + bytes([s[9] ^ 1]) + s[10:]
    raws[t_sig] = sh.tx_serialize(tx)
    want = world.expect(raws, prevouts)
    got = hkv.verify_std_txs(ver, raws, prevouts, world.forkid)
    assert got == want
    assert sorted(t for t in range(world.n_block) if not got[t]) == sorted([t_removed, t_value, t_script, t_sig])


def _dup_outpoint_tx(rng, k0, k1):
    """Two validly signed P2PKH inputs on ONE outpoint, input 0 for k0's
    script and input 1 for k1's."""
    outpoint, value = rng.randbytes(32), 90000
    ins = [sh.TxIn(outpoint, 1, b"", 0xFFFFFFFF) for _ in range(2)]
    tx = sh.Tx(2, ins, [sh.TxOut(1000, sh.p2pkh_script(rng.randbytes(20)))], [], 0)
    for j, k in enumerate((k0, k1)):
        m = sh.sighash_legacy(tx, sh.p2pkh_script(k.h160), value, j, 0x01, None)
        r, s = txgen.sign(m, k.d, rng.randrange(1, o.N))
        tx.inputs[j].script = txgen.push(sh.der_encode(r, s) + b"\x01") + txgen.push(k.pub)
    return sh.tx_serialize(tx), ins[0].outpoint(), value


def test_std_txs_duplicate_outpoint(ver, coracle):
    import hkv
    rng = random.Random(77)
    ka, kb = txgen.Key(rng.randrange(1, o.N)), txgen.Key(rng.randrange(1, o.N))
    A, B = sh.p2pkh_script(ka.h160), sh.p2pkh_script(kb.h160)
    raw_aa, op_aa, v = _dup_outpoint_tx(rng, ka, ka)
    raw_ab, op_ab, _ = _dup_outpoint_tx(rng, ka, kb)
    raws = [raw_aa, raw_aa, raw_ab, raw_ab]
    prevouts = [[(op_aa, A, v)],                      # one entry for the outpoint
                [(op_aa, A, v), (op_aa, A, v)],      # two equal entries
                [(op_ab, A, v), (op_ab, B, v)],      # (A, B), inputs signed for (A, B)
                [(op_ab, B, v), (op_ab, A, v)]]      # (B, A), inputs signed for (A, B)
    ok = model.oracle_input_ok(coracle, None)
    assert [model.verify_std_tx(r, p, ok) for r, p in zip(raws, prevouts)] == [False, True, True, False]
    assert hkv.verify_std_txs(ver, raws, prevouts, None) == [False, True, True, False]


def _unmatched_as_empty(jobs):
    return [(t, i, spk if spk is not None else b"", val) for (t, i, spk, val) in jobs]


def test_device_form_input_bits_equal_verify_std_inputs_on_model_jobs(ver, world):
    """The composed device call leaves input_first and the per-input bits
    readable: they equal the model's prefix sums and verify_std_inputs on the
    model's jobs (an unmatched input: an empty script), with one list cut so
    that some inputs are unmatched; its tx bits equal the host form's."""
    import hkv
    prevouts = [list(p) for p in world.prevouts]
    cut = [t for t in range(world.n_block) if len(prevouts[t]) >= 2][:5]
    for t in cut:
        prevouts[t].pop(0)
    first, mj = model.model_jobs(world.raw, prevouts)
    ok, per_input = hkv.verify_std_txs_detail(ver, world.raw, prevouts, world.forkid)
    assert [len(p) for p in per_input] == [first[t + 1] - first[t] for t in range(len(world.raw))]
    flat = [v for p in per_input for v in p]
    assert flat == hkv.verify_std_inputs(ver, world.raw, _unmatched_as_empty(mj), world.forkid)
    assert ok == hkv.verify_std_txs(ver, world.raw, prevouts, world.forkid)
    assert ok == [bool(p) and all(p) for p in per_input]
    assert not any(ok[t] for t in cut)


def test_device_form_count_mismatch_zeroes_every_tx_bit(torch, ver, world):
    import hkv
    from hkv.lib import HKV_STATUS_INPUT_COUNT
    raws, prevouts = world.raw[:70], world.prevouts[:70]
    b = DeviceBatch.of(torch, raws, prevouts)
    n = model.model_jobs(raws, prevouts)[0][-1]
    for n_inputs in (n - 1, n + 1, n):
        first = torch.zeros(b.n_tx + 1, dtype=torch.int32, device="cuda")
        jobs = torch.full((n_inputs * 24 + 256,), GUARD, dtype=torch.uint8, device="cuda")
        recs = torch.zeros(n_inputs * 168, dtype=torch.uint8, device="cuda")
        bits = torch.zeros((n_inputs + 63) // 64 * 2, dtype=torch.int32, device="cuda")
        tx_bits = torch.full(((b.n_tx + 63) // 64 * 2,), -1, dtype=torch.int32, device="cuda")
        status = torch.zeros(2, dtype=torch.int32, device="cuda")
        hkv.verify_std_txs_device(ver, 0, b.txs, *b.prev, -1 if world.forkid is None else world.forkid, n_inputs,
                                  first.data_ptr(), jobs.data_ptr(), recs.data_ptr(), bits.data_ptr(),
                                  tx_bits.data_ptr(), status.data_ptr())
        torch.cuda.synchronize()
        assert bool((jobs.cpu().numpy()[n_inputs * 24:] == GUARD).all())
        w = download(tx_bits, np.uint32)
        if n_inputs == n:
            assert int(status[0].item()) == 0
            assert np.unpackbits(w.view(np.uint8), bitorder="little")[:70].all()
        else:
            assert int(status[0].item()) == HKV_STATUS_INPUT_COUNT
            assert not w.any()


def test_std_txs_device_returns_before_the_stream_runs(torch, ver, coracle):
    """hkv_verify_std_txs_device only enqueues: with its stream gated behind
    ~20 full-grid verifies on another stream it returns long before the gate
    opens, and once it has run the tx verdicts equal the model's."""
    import hkv
    world = get_world(coracle, None)
    want = world.expect(world.raw, world.prevouts)
    b = DeviceBatch.of(torch, world.raw, world.prevouts)
    n = model.model_jobs(world.raw, world.prevouts)[0][-1]
    first = torch.zeros(b.n_tx + 1, dtype=torch.int32, device="cuda")
    jobs = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
    recs = torch.zeros(n * 168, dtype=torch.uint8, device="cuda")
    bits = torch.zeros((n + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    tx_bits = torch.zeros((b.n_tx + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    n_big = 1 << 20
    big = torch.empty(n_big * 168, dtype=torch.uint8, device="cuda")
    bbits = torch.zeros(n_big // 32 + 2, dtype=torch.int32, device="cuda")
    ver.gen_records_device(0, 77, n_big, 4096, 100, big.data_ptr())
    gate, s = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        ver.verify_device(0, big.data_ptr(), n_big, 0, bbits.data_ptr(), gate.cuda_stream)
    ev = torch.cuda.Event()
    ev.record(gate)
    s.wait_event(ev)
    t1 = time.perf_counter()
    hkv.verify_std_txs_device(ver, 0, b.txs, *b.prev, -1, n, first.data_ptr(), jobs.data_ptr(), recs.data_ptr(),
                              bits.data_ptr(), tx_bits.data_ptr(), status.data_ptr(), s.cuda_stream)
    t_call = time.perf_counter() - t1
    torch.cuda.synchronize()
    t_gate = time.perf_counter() - t0
    assert t_gate > 0.1, t_gate
    assert t_call < 0.25 * t_gate, (t_call, t_gate)
    assert int(status[0].item()) == 0
    got = np.unpackbits(download(tx_bits, np.uint8), bitorder="little")[:b.n_tx].astype(bool).tolist()
    assert got == want


def test_actor_verify_std_tx_names_the_failing_inputs(ver, coracle):
    """The actor's verify_std_tx on the real library: a tx of the block with
    its shuffled list verifies; with one entry removed it is rejected and the
    event names exactly the input that lost its prevout."""
    from hkv.actor import TxRejected, TxVerified, VerifyActor, VerifyActorConfig
    world = get_world(coracle, None)
    t = next(t for t in range(world.n_block) if len(world.prevouts[t]) >= 2)
    tx = world.txs[t]
    gone = world.prevouts[t][0]
    lost = next(i for i, ti in enumerate(tx.inputs) if ti.outpoint() == gone[0])
    out = []
    with VerifyActor(ver, out.append, VerifyActorConfig(forkid=None)) as a:
        a.verify_std_tx("whole", world.raw[t], world.prevouts[t])
        a.verify_std_tx("cut", world.raw[t], world.prevouts[t][1:])
        a.verify_std_tx("garbage", world.raw[t][:-1], world.prevouts[t])
    assert out == [TxVerified("whole"), TxRejected("cut", (lost,)), TxRejected("garbage", ())]
