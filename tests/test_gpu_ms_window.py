"""The multisig tail's record windows: the candidate and
key-check records of a chunk run in rounds through windows capped at
~512 MiB instead of buffers sized by the 16-of-16 bound (3.35 GB per
131,072-input chunk). Verdicts must equal the oracle's whatever the window
(forced small with hkv_debug_ms_window, so that records straddle rounds),
a 131,072-input all-multisig chunk must equal the oracle, and a chunk holds
at most the budget whether it has multisig inputs or not. Data source:
blocks from getBlocks, /root/reference/src/Haskoin/Node/Peer.hs:309-324."""
import ctypes
import random

import pytest

import secp256k1_oracle as o
import sighash_oracle as sh
from conftest import host_threads, oracle_batch

pytestmark = pytest.mark.gpu

BUDGET = 512 << 20


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


def _window(ver, cand, keys):
    assert ver.lib.hkv_debug_ms_window(ver.ctx, 0, cand, keys) == 0


def _scratch(ver):
    b = ctypes.c_size_t()
    assert ver.lib.hkv_debug_ms_scratch(ver.ctx, 0, ctypes.byref(b)) == 0
    return b.value


def batched_oracle(coracle, raw_txs, jobs, forkid=None):
    """The oracle's verifyStdInput over every job (oracle/sighash_oracle.py
    verify_std_input: countMulSig over candidate verdicts), with ONE C-oracle
    call for every candidate record of the batch: a first pass collects the
    records (placeholder verdicts), a second replays each walk on the real
    ones. Key parses are memoised (keys repeat from a pool)."""
    parsed = [sh.tx_parse(t) for t in raw_txs]
    memo = {}

    def key_ok(k):
        if k not in memo:
            memo[k] = o.pubkey_parse(k) is not None
        return memo[k]

    recs, spans = [], []

    def collect(rs):
        spans.append((len(recs), len(rs)))
        recs.extend(rs)
        return [True] * len(rs)

    for (t, i, p, v) in jobs:
        n0 = len(spans)
        sh.verify_std_input(parsed[t], i, p, v, forkid, collect, key_ok)
        if len(spans) == n0:
            spans.append((len(recs), 0))
    flat = oracle_batch(coracle, b"".join(recs), 1, threads=host_threads()).tolist() if recs else []
    out = []
    for k, (t, i, p, v) in enumerate(jobs):
        a, n = spans[k]
        out.append(sh.verify_std_input(parsed[t], i, p, v, forkid, lambda rs: flat[a:a + n], key_ok))
    return out


@pytest.mark.parametrize("cand,keys", [(64, 64), (4096, 256), (0, 0)])
def test_forced_windows_equal_oracle(torch, ver, coracle, cand, keys):
    """Every multisig case of tests/txgen.py (all wraps and variants) beside
    signed single-signature txs, through the block kernel and the host form,
    with windows of 64 / 4,096 candidate records (tens of rounds) and the
    default: verdicts equal the oracle's each time."""
    import hkv
    from test_gpu_sighash import _device_verify_std, _ms_block
    rng = random.Random(0x57 + cand)
    raw, jobs, labels = _ms_block(rng, None)
    want = batched_oracle(coracle, raw, jobs)
    _window(ver, cand, keys)
    try:
        got = _device_verify_std(torch, ver, raw, jobs, None)
        bad = [(labels[k], got[k], want[k]) for k in range(len(jobs)) if got[k] != want[k]]
        assert not bad, bad[:10]
        assert hkv.verify_std_inputs(ver, raw, jobs) == want
    finally:
        _window(ver, 0, 0)
    assert sum(g for g, lb in zip(want, labels) if lb != "single") > 40
    assert ver.device_fault(0) == 0


# ---------------------------------------------------------------------------
# Dense inputs (up to 16-of-16: the bound the verdict words are sized by) in
# forced windows, on a fresh context each — so the candidate verdict words
# hold exactly ms_cbits_words(n) words and a group past a round's records
# would store outside them — with the device's own view of the launch
# (hkv_debug_ms_tail_counts) checked against the case's numbers: the scan's
# totals, whose residues are the premise of each case, and the number of work
# items the tail completed, restated here from the per-round record counts
# (csrc/hkv_tail_plan.h holds the kernel's form; tests/tail_plan.cpp walks it
# exhaustively on the CPU, these cases included).
# ---------------------------------------------------------------------------
WIN_CAND_DEFAULT, WIN_KEYS_DEFAULT = 2752512, 442368  # include/hkv.h (hkv_debug_ms_window)
DECODABLE = ("wrong_key", "swap")  # damage that leaves every signature in place and decodable


def _cands(m, n):
    """Candidate records of an m-of-n input with m decodable signatures:
    signature j is compared with keys j .. n-1."""
    return m * n - m * (m - 1) // 2


def _tail_items(n, n_cand, n_keys, win_cand, win_keys):
    """Work items of a tail launch apart from the fused path's hash chunks:
    per round ceil(n / 256) emit chunks, a group per 32 candidate records and
    a chunk per 256 key-check records of the round's windows (nothing for an
    empty window); then ceil(n / 256) resolve chunks."""
    def cdiv(a, b):
        return -(-a // b)
    wc = cdiv(min(136 * n, win_cand or WIN_CAND_DEFAULT), 64) * 64
    wk = cdiv(min(16 * n, win_keys or WIN_KEYS_DEFAULT), 64) * 64
    rounds = max(cdiv(n_cand, wc), cdiv(n_keys, wk))
    n2 = cdiv(n, 256)
    verify = 0
    for r in range(rounds):
        c_r = min(max(n_cand - r * wc, 0), wc)
        k_r = min(max(n_keys - r * wk, 0), wk)
        verify += cdiv(c_r, 32) + cdiv(k_r, 256)
    return rounds * n2 + verify + n2


def _tail_counts(v):
    out = (ctypes.c_uint64 * 3)()
    assert v.lib.hkv_debug_ms_tail_counts(v.ctx, 0, out) == 0
    return out[0] & 0xFFFFFFFF, out[0] >> 32, out[1], out[2]


def _concat(blocks):
    txs, inputs = [], []
    for (bt, bi) in blocks:
        o1 = len(txs)
        txs += bt
        inputs += [(t + o1, i, p, v) for (t, i, p, v) in bi]
    return txs, inputs


def _intended(txs, inputs):
    """(candidate records, key-check records) of the batch by the oracle's
    decode of each multisig input (signatures dropped by the generator's
    damage change the count)."""
    parsed = [sh.tx_parse(t) for t in txs]
    c = k = 0
    for (t, i, p, v) in inputs:
        ms = sh.std_multisig(parsed[t], i, p, v, None)
        if ms is not None:
            c += len(ms.candidates())
            k += len(ms.keys)
    return c, k


def _dense_case(torch, coracle, txs, inputs, windows, n_cand, n_keys):
    """One case on a fresh context: the device form with a status word, then
    the host form; verdicts against the oracle; after each call the scan's
    totals and the completed work items."""
    import hkv
    from test_gpu_sighash import _device_verify_std
    want = batched_oracle(coracle, txs, inputs)
    assert any(want) and not all(want)
    n = len(inputs)
    items = _tail_items(n, n_cand, n_keys, *windows)
    hash_chunks = -(-3 * len(txs) // 256)  # the fused path's BIP143 per-tx hash chunks
    with hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1)) as v:
        _window(v, *windows)
        try:
            got, st = _device_verify_std(torch, v, txs, inputs, None, status=True)
            c, k, claimed, done = _tail_counts(v)
            print(f"device form: n={n} n_cand={c} n_keys={k} claimed={claimed} done={done} items={items}")
            assert (c, k) == (n_cand, n_keys)
            assert done - items in (0, hash_chunks), (done, items, hash_chunks)
            assert st == 0
            bad = [(j, got[j], want[j]) for j in range(n) if got[j] != want[j]]
            assert not bad, bad[:10]
            assert hkv.verify_std_inputs(v, txs, inputs) == want
            c, k, claimed, done = _tail_counts(v)
            print(f"host form: n={n} n_cand={c} n_keys={k} claimed={claimed} done={done} items={items}")
            assert (c, k) == (n_cand, n_keys)
            assert done - items in (0, hash_chunks), (done, items, hash_chunks)
        finally:
            _window(v, 0, 0)
        assert v.device_fault(0) == 0


def test_dense_key_only_rounds(torch, ver, coracle):
    """64 x 1-of-16 in windows of (4096, 64): 1,024 candidates in one round,
    1,024 key checks in 16 — rounds 1..15 hold no candidate record, so they
    have no candidate group (a group there would store verdict words up to
    bit 62,463 of the 8,704 allocated, and re-verify round 0's window)."""
    from hkv import blockgen
    txs, inputs = blockgen.make_multisig_block(ver, torch, n_tx=64, seed=0x484B5650, n_keys=256, shapes=((1, 16),),
                                               damage_kinds=DECODABLE)
    _dense_case(torch, coracle, txs, inputs, (4096, 64), 64 * _cands(1, 16), 64 * 16)


def test_dense_candidate_only_rounds(torch, ver, coracle):
    """32 x 16-of-16 in windows of (64, 4096): 4,352 = 68 x 64 candidates in
    68 rounds, 512 key checks in one — no key chunk after round 0, and every
    signature's 16 .. 1 candidates straddle rounds."""
    from hkv import blockgen
    txs, inputs = blockgen.make_multisig_block(ver, torch, n_tx=32, seed=0x484B5651, n_keys=256, shapes=((16, 16),),
                                               damage_kinds=DECODABLE)
    assert 32 * _cands(16, 16) == 4352 == 68 * 64
    _dense_case(torch, coracle, txs, inputs, (64, 4096), 4352, 512)


def test_dense_ragged_last_round(torch, ver, coracle):
    """31 x 16-of-16 in windows of (1024, 64): 4,216 candidates — the last
    candidate round holds 120 records, 4 groups, the last with 24 valid
    slots; a full round's 32 groups would put the first stray verdict word
    exactly at the end of the 4,224 bits allocated."""
    from hkv import blockgen
    txs, inputs = blockgen.make_multisig_block(ver, torch, n_tx=31, seed=0x484B5652, n_keys=256, shapes=((16, 16),),
                                               damage_kinds=DECODABLE)
    assert 31 * 136 == 4216 == 4 * 1024 + 120 and (31 * 136 + 63) // 64 * 64 == 4224
    _dense_case(torch, coracle, txs, inputs, (1024, 64), 4216, 31 * 16)


@pytest.mark.parametrize("j", [1, 15, 16])
def test_dense_residues(torch, ver, coracle, j):
    """30 x 16-of-16 and j x 1-of-1 in windows of (1024, 1024): 4,081 / 4,095
    / 4,096 candidates — a last group of 17 / 31 / 32 valid slots, and the
    exact multiple of the window."""
    from hkv import blockgen
    a = blockgen.make_multisig_block(ver, torch, n_tx=30, seed=0x484B5653, n_keys=256, shapes=((16, 16),),
                                     invalid_permille=200, damage_kinds=DECODABLE)
    b = blockgen.make_multisig_block(ver, torch, n_tx=j, seed=0x484B5654 + j, n_keys=256, shapes=((1, 1),),
                                     invalid_permille=0)
    txs, inputs = _concat([a, b])
    assert 30 * 136 + j in (4081, 4095, 4096)
    _dense_case(torch, coracle, txs, inputs, (1024, 1024), 30 * 136 + j, 30 * 16 + j)


def _dense_mix(ver, torch, seed):
    """96 inputs: 20 each of 15-of-16, 16-of-16, 8-of-16 and 1-of-16 (8 %
    damaged: a wrong key, two signatures swapped, or one dropped), and 16 of
    16-of-16 each with one signature by a wrong key."""
    from hkv import blockgen
    blocks = [blockgen.make_multisig_block(ver, torch, n_tx=20, seed=seed + q, n_keys=256, shapes=(shape,))
              for q, shape in enumerate(((15, 16), (16, 16), (8, 16), (1, 16)))]
    blocks.append(blockgen.make_multisig_block(ver, torch, n_tx=16, seed=seed + 4, n_keys=256, shapes=((16, 16),),
                                               invalid_permille=1000, damage_kinds=("wrong_key",)))
    return _concat(blocks)


@pytest.mark.parametrize("windows", [(4096, 64), (0, 0)])
def test_dense_mix(torch, ver, coracle, windows):
    """The dense mix in windows of (4096, 64) — 3 candidate rounds beside 24
    key rounds — and at the default windows, one round, where the per-round
    plan changes nothing."""
    txs, inputs = _dense_mix(ver, torch, 0x484B5668)
    n_cand, n_keys = _intended(txs, inputs)
    full = 20 * (_cands(15, 16) + _cands(16, 16) + _cands(8, 16) + _cands(1, 16)) + 16 * _cands(16, 16)
    assert full == 9916 and (n_cand, n_keys) == (9914, 96 * 16)  # (one 15-of-16 input lost a signature: 133)
    _dense_case(torch, coracle, txs, inputs, windows, n_cand, n_keys)


def test_dense_mix_past_the_block_kernel(torch, ver, coracle):
    """The dense mix shuffled among the ~5,400 single-signature inputs of a
    3,000-tx block (> 4,096 inputs: the pair kernel and the separate scan
    kernel, whose offsets place the dense record ranges) in windows of
    (1024, 64)."""
    from hkv import blockgen
    singles = blockgen.make_block(ver, torch, n_tx=3000, seed=0x484B5670)
    txs, inputs = _concat([_dense_mix(ver, torch, 0x484B5668), singles])
    assert len(inputs) > 4096 + 96
    random.Random(0x484B5671).shuffle(inputs)
    n_cand, n_keys = _intended(txs, inputs)
    assert (n_cand, n_keys) == (9914, 96 * 16)
    _dense_case(torch, coracle, txs, inputs, (1024, 64), n_cand, n_keys)


@pytest.mark.timeout(900)
def test_full_chunk_all_multisig_equals_oracle(torch, ver, coracle):
    """131,072 multisig inputs (one chunk: 1-of-1 .. 3-of-3, every wrap, 8 %
    damaged), device-signed: verdicts equal the oracle's at the default
    windows and with windows forced to 65,536 candidate / 16,384 key records
    (several rounds); the record windows stay within the ~512 MiB budget."""
    import hkv
    from hkv import blockgen
    txs, inputs = blockgen.make_multisig_block(ver, torch, n_tx=131072)
    assert len(inputs) == 131072
    want = batched_oracle(coracle, txs, inputs)
    assert 0.85 * len(want) < sum(want) < 0.97 * len(want)
    got = hkv.verify_std_inputs(ver, txs, inputs)
    assert got == want
    assert _scratch(ver) <= BUDGET
    _window(ver, 65536, 16384)
    try:
        assert hkv.verify_std_inputs(ver, txs, inputs) == want
    finally:
        _window(ver, 0, 0)
    assert ver.device_fault(0) == 0


def test_multisig_free_chunk_within_budget(torch):
    """A fresh context given a 75,000-tx single-signature batch (> one
    131,072-input chunk) holds at most the budget of multisig records (the
    16-of-16 bound would be 3.35 GB)."""
    import hkv
    from hkv import blockgen
    with hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1)) as v:
        txs, inputs = blockgen.make_block(v, torch, n_tx=75000, seed=0x484B5644)
        assert len(inputs) > 131072
        assert all(hkv.verify_std_inputs(v, txs, inputs))
        b = ctypes.c_size_t()
        assert v.lib.hkv_debug_ms_scratch(v.ctx, 0, ctypes.byref(b)) == 0
        assert 0 < b.value <= BUDGET


@pytest.mark.timeout(900)
def test_two_chunks_with_multisig_on_both_sides(torch, ver, coracle):
    """A batch past one 131,072-input chunk with multisig inputs in both
    chunks (6,000 multisig inputs, 126,000 single-signature inputs, 6,000
    more multisig inputs: the chunk boundary falls among the single-signature
    inputs, so each chunk holds multisig inputs and the second chunk's jobs
    start mid-batch): each chunk runs its own scan, windows and tail; verdicts
    of the host form and of the device form with a status word equal the
    oracle's, with no fault."""
    import hkv
    from hkv import blockgen
    from test_gpu_sighash import _device_verify_std
    mt1, mi1 = blockgen.make_multisig_block(ver, torch, n_tx=6000, seed=0x484B5647)
    st_, si = blockgen.make_block(ver, torch, n_tx=76000, seed=0x484B5648, inputs_per_tx=(1, 2, 2, 2))
    mt2, mi2 = blockgen.make_multisig_block(ver, torch, n_tx=6000, seed=0x484B5649)
    txs = mt1 + st_ + mt2
    o1, o2 = len(mt1), len(mt1) + len(st_)
    si = si[:126000]
    inputs = list(mi1) + [(t + o1, i, p, v) for (t, i, p, v) in si] + [(t + o2, i, p, v) for (t, i, p, v) in mi2]
    assert len(si) == 126000 and len(inputs) == 138000 and len(mi1) + len(si) > 131072 > len(mi1)
    want = batched_oracle(coracle, txs, inputs)
    assert 0 < sum(not w for w in want) < 2000
    assert hkv.verify_std_inputs(ver, txs, inputs) == want
    got, st = _device_verify_std(torch, ver, txs, inputs, None, status=True)
    assert st == 0 and got == want
    assert ver.device_fault(0) == 0


@pytest.mark.timeout(1200)
def test_past_one_grid_full_grid_chunks(torch, ver, coracle):
    """A batch past one resident grid (262,144 inputs) runs in chunks of up
    to 2^20 inputs through the full-grid instance (extraction, then the record
    verify at 4 waves per SIMD) instead of half-grid chunks: ~290,000 inputs,
    multisig inputs at both ends, in one chunk through the host form and the
    device form with a status word; and with HKV_STD_CHUNK=196608 (a fresh
    context) as a full-grid chunk of 196,608 inputs followed by a half-grid
    one — every verdict equal to the oracle's, no fault."""
    import os
    import hkv
    from hkv import blockgen
    from test_gpu_sighash import _device_verify_std
    mt1, mi1 = blockgen.make_multisig_block(ver, torch, n_tx=3000, seed=0x484B564A)
    st_, si = blockgen.make_block(ver, torch, n_tx=163000, seed=0x484B564B, inputs_per_tx=(1, 2, 2, 2))
    mt2, mi2 = blockgen.make_multisig_block(ver, torch, n_tx=3000, seed=0x484B564C)
    txs = mt1 + st_ + mt2
    o1, o2 = len(mt1), len(mt1) + len(st_)
    inputs = list(mi1) + [(t + o1, i, p, v) for (t, i, p, v) in si] + [(t + o2, i, p, v) for (t, i, p, v) in mi2]
    assert len(inputs) > 262144 + 20000
    want = batched_oracle(coracle, txs, inputs)
    assert 0 < sum(not w for w in want) < 1000
    assert hkv.verify_std_inputs(ver, txs, inputs) == want
    got, st = _device_verify_std(torch, ver, txs, inputs, None, status=True)
    assert st == 0 and got == want
    assert ver.device_fault(0) == 0
    os.environ["HKV_STD_CHUNK"] = "196608"
    try:
        with hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1)) as v2:
            got, st = _device_verify_std(torch, v2, txs, inputs, None, status=True)
            assert st == 0 and got == want
            assert v2.device_fault(0) == 0
    finally:
        del os.environ["HKV_STD_CHUNK"]
