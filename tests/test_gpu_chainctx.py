"""The header chain-context stage on the GPU (hkv_connect_headers,
hkv_connect_headers_device, hkv_chain_context_device) against the Python model
of the rule (tests/chainctx_model.py), bit for bit: mtp, the expected bits, the
256-bit chain work, the flag byte, and n_ok against the model's first_bad over
the oracle's header status (oracle/header_oracle.py).

Headers are synthetic 80-byte records with chosen version, time and bits; the
stage does not look at proof of work. Only the first_bad tests need headers
that pass isValidPOW: those take a nonce against the regtest limit (two tries
on average)."""
import hashlib
import json
import os

import numpy as np
import pytest

import chainctx_model as cm
import header_oracle as ho
from conftest import GOLDEN
from test_headers import fixture_headers

pytestmark = pytest.mark.gpu

TILE = 256            # CHAIN_TILE of csrc/hkv_chainctx.h: headers per workgroup, and lanes of the one scan workgroup
BASE = 1500000000
REGTEST_GENESIS_TIME = 1296688602


@pytest.fixture(scope="module")
def verifier():
    import torch
    import hkv
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    v = hkv.Verifier(hkv.VerifierConfig(device_ids=[0]))
    yield v
    v.close()


def to_params(p):
    from hkv.chain import ChainParams
    return ChainParams(pow_limit=p.pow_limit, bip34_height=p.bip34_height, bip66_height=p.bip66_height,
                       bip65_height=p.bip65_height, flags=p.flags, interval=p.interval,
                       target_timespan=p.target_timespan, min_diff_spacing=p.min_diff_spacing)


def to_tip(tp):
    from hkv.chain import ChainTip
    return ChainTip(tp.height, tuple(tp.times), tp.bits, tp.period_first_time, tp.period_real_bits, tp.work)


def stage_on_device(v, facts, tp, p, now, checkpoints=(), hashes=None):
    """hkv_chain_context_device alone on torch buffers: (mtp, want, work, flags) as lists.
    hashes: n 32-byte strings the checkpoints are compared with, or None (d_hashes = NULL)."""
    import torch
    import hkv
    from hkv.chain import pack_checkpoints, work_ints
    n = len(facts)
    raw = np.frombuffer(b"".join(cm.make_header(*f) for f in facts), dtype=np.uint8)
    d_h = torch.from_numpy(raw.copy()).cuda()
    d_hash = None if hashes is None else torch.from_numpy(np.frombuffer(b"".join(hashes), dtype=np.uint8).copy()).cuda()
    cph, cpx = pack_checkpoints(checkpoints)
    d_cph = torch.from_numpy(cph.view(np.int32).copy()).cuda() if len(cph) else None
    d_cpx = torch.from_numpy(cpx).cuda() if len(cph) else None
    mtp = torch.zeros(n, dtype=torch.int32, device="cuda")
    bits = torch.zeros(n, dtype=torch.int32, device="cuda")
    work = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(hkv.chain_scratch_words(v, n), dtype=torch.int32, device="cuda")
    hkv.chain_context_device(v, 0, d_h.data_ptr(), n, None if d_hash is None else d_hash.data_ptr(),
                             hkv.chain_ctx(to_tip(tp), to_params(p), now),
                             None if d_cph is None else d_cph.data_ptr(), None if d_cpx is None else d_cpx.data_ptr(),
                             len(cph), mtp.data_ptr(), bits.data_ptr(), work.data_ptr(), st.data_ptr(),
                             scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (mtp.cpu().numpy().view(np.uint32).tolist(), bits.cpu().numpy().view(np.uint32).tolist(),
            work_ints(work.cpu().numpy()), st.cpu().numpy().tolist())


def connect_on_device(v, headers, tp, p, now, checkpoints=(), prev_hash=None):
    """hkv_connect_headers_device on torch buffers -> (hashes, hdr_status, mtp, want, work, flags, first_bad)."""
    import torch
    import hkv
    from hkv.chain import pack_checkpoints, work_ints
    n = len(headers)
    d_h = torch.from_numpy(np.frombuffer(b"".join(headers), dtype=np.uint8).copy()).cuda()
    lim = torch.from_numpy(np.frombuffer(p.pow_limit.to_bytes(32, "little"), dtype=np.uint8).copy()).cuda()
    prev = None if prev_hash is None else torch.from_numpy(np.frombuffer(prev_hash, dtype=np.uint8).copy()).cuda()
    cph, cpx = pack_checkpoints(checkpoints)
    d_cph = torch.from_numpy(cph.view(np.int32).copy()).cuda() if len(cph) else None
    d_cpx = torch.from_numpy(cpx).cuda() if len(cph) else None
    hashes = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    hst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mtp = torch.zeros(n, dtype=torch.int32, device="cuda")
    bits = torch.zeros(n, dtype=torch.int32, device="cuda")
    work = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(hkv.chain_scratch_words(v, n), dtype=torch.int32, device="cuda")
    fb = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    hkv.connect_headers_device(v, 0, d_h.data_ptr(), n, lim.data_ptr(), None if prev is None else prev.data_ptr(),
                               hkv.chain_ctx(to_tip(tp), to_params(p), now),
                               None if d_cph is None else d_cph.data_ptr(),
                               None if d_cpx is None else d_cpx.data_ptr(), len(cph), hashes.data_ptr(),
                               hst.data_ptr(), mtp.data_ptr(), bits.data_ptr(), work.data_ptr(), st.data_ptr(),
                               scratch.data_ptr(), fb.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    hb = hashes.cpu().numpy().tobytes()
    return ([hb[32 * i:32 * i + 32] for i in range(n)], hst.cpu().numpy().tolist(),
            mtp.cpu().numpy().view(np.uint32).tolist(), bits.cpu().numpy().view(np.uint32).tolist(),
            work_ints(work.cpu().numpy()), st.cpu().numpy().tolist(), int(fb.cpu().numpy().view(np.uint32)[0]))


def first_diff(got, want):
    return next(((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w), None)


def assert_stage(got, want, what=""):
    for name, g, w in zip(("mtp", "want", "work", "flags"), got, want):
        assert len(g) == len(w) and first_diff(g, w) is None, (what, name, first_diff(g, w))


def check_both_forms(v, headers, tp, p, now, checkpoints=(), prev_hash=None, what=""):
    """The host form and the device form against the model and the header oracle; -> the model's n_ok."""
    import hkv
    facts = [cm.fields(h) for h in headers]
    e_hash, e_hst = ho.check_headers(list(headers), p.pow_limit, prev_hash)
    want = cm.connect(facts, tp, p, now, checkpoints, e_hash)
    n_ok = cm.first_bad(want[3], e_hst)
    r = hkv.connect_headers(v, headers, to_tip(tp), to_params(p), checkpoints, now, prev_hash)
    assert r.hashes == e_hash and r.hdr_status.tolist() == e_hst, what
    assert_stage((r.mtp.tolist(), r.bits.tolist(), r.work, r.chain_status.tolist()), want, what + " host form")
    assert r.n_ok == n_ok, what
    d = connect_on_device(v, headers, tp, p, now, checkpoints, prev_hash)
    assert d[0] == e_hash and d[1] == e_hst, what
    assert_stage(d[2:6], want, what + " device form")
    assert d[6] == n_ok, what
    return n_ok


# ---------------------------------------------------------------- the fixture chain

def test_fixture_chain_connects(verifier):
    """The reference's 15 bchRegTest headers on the regtest genesis: all 15
    connect, every flag set, work[i] = 2 (i + 2)."""
    import hkv
    from hkv.chain import ChainTip
    hdrs = fixture_headers()
    genesis = cm.make_header(1, REGTEST_GENESIS_TIME, 0x207fffff, bytes(32),
                             bytes.fromhex("4a5e1e4baab89f3a32518a88c31bc87f618f76673e2cc77ab2127b7afdeda33b")[::-1], 2)
    # the constant is pinned: the genesis header built from it is header 1's parent
    assert ho.header_hash(genesis) == hdrs[0][4:36]
    p = hkv.CHAIN_PARAMS["btcRegTest"]
    tip = ChainTip.genesis(p, genesis)
    assert (tip.height, tip.times, tip.work, tip.period_real_bits) == (0, (REGTEST_GENESIS_TIME,), 2, 0x207fffff)
    now = max(cm.fields(h)[1] for h in hdrs) + 1
    r = hkv.connect_headers(verifier, hdrs, tip, p, (), now, prev_hash=ho.header_hash(genesis))
    assert r.n_ok == 15
    assert r.work == [2 * (i + 2) for i in range(15)]
    assert r.chain_status.tolist() == [hkv.HKV_CHN_ALL] * 15
    assert all(s & 3 == 3 for s in r.hdr_status.tolist())
    fx = json.load(open(os.path.join(GOLDEN, "ref_fixtures.json")))["hashes"]
    assert r.hashes[14][::-1].hex() == fx["best_h15"]
    mp = cm.params(pow_limit=p.pow_limit, bip34_height=p.bip34_height, bip66_height=p.bip66_height,
                   bip65_height=p.bip65_height, flags=p.flags)
    mt = cm.tip(0, tip.times, tip.bits, tip.period_first_time, tip.period_real_bits, 2)
    assert check_both_forms(verifier, hdrs, mt, mp, now, (), ho.header_hash(genesis), "fixture") == 15
    # the next message's context
    nxt = tip.advance(hdrs, r, 15)
    assert (nxt.height, nxt.work, len(nxt.times), nxt.bits) == (15, 32, 11, 0x207fffff)


# ---------------------------------------------------------------- retarget vectors

@pytest.mark.parametrize("first,last,old,new", cm.VECTORS)
def test_published_retarget_vectors(verifier, first, last, old, new):
    """Bitcoin's four published vectors, with the period's first block in the
    context and as a 2,017-header batch that holds the period."""
    p, tp, facts = cm.boundary_case(first, last, old)
    got = stage_on_device(verifier, facts, tp, p, last + 10000)
    assert got[1] == [new] and got[3] == [cm.ALL]
    check_both_forms(verifier, [cm.make_header(*f) for f in facts], tp, p, last + 10000, what="context")
    step = (last - first) // 2015
    times = [first + step * j for j in range(2015)] + [last]
    batch = [(4, t, old) for t in times] + [(4, last + 600, new)]
    tp = cm.tip(2016 * 9 - 1, [first - 600], old, first - 1209600, old, 1)
    got = stage_on_device(verifier, batch, tp, p, last + 10000)
    assert got[1][2016] == new and got[3][2016] == cm.ALL
    check_both_forms(verifier, [cm.make_header(*f) for f in batch], tp, p, last + 10000, what="batch")


# ---------------------------------------------------------------- scan and halo edges

SIZES = [1, 2, 10, 11, 12, 13, 255, 256, 257, 1023, 1024, 1025, 2000, 2016, 2017, 4033, 8191, 8193, 65537, 300000]
PLACEMENTS = ("at_0", "at_1", "at_last", "twice")


def edge_batch(n, n_prev, placement, min_difficulty):
    """A random batch of n headers whose period boundary falls where `placement`
    says. The interval is 2016 where two boundaries fit in n headers that way,
    else the largest that does (at least 2), the timespan scaled with it.

    A batch of 2 to 254 headers is too short for the few percent of random
    faults to clear every flag, so its first two headers are directed and
    complementary: header 0 is in the future and of a version its height
    forbids, with the bits the rule wants and its checkpoint's hash; header 1
    lies at or below the median, with other bits than wanted and another hash
    than its checkpoint's. The random headers follow them. A batch of one
    header is directed too: every flag set, or (where `min_difficulty` is
    asked for, with `now` set before the context's times) every flag cleared."""
    interval = 2016
    if placement == "twice":
        interval = min(2016, max(2, (n - 1) // 2))
    p = cm.params(interval=interval, target_timespan=interval * 600, bip34_height=100, bip66_height=200,
                  bip65_height=300, flags=cm.MIN_DIFFICULTY if min_difficulty else 0)
    at = {"at_0": 0, "at_1": 1, "at_last": n - 1, "twice": min(1, n - 1)}[placement]
    h0 = interval * (50 + at // interval) - at          # header `at` stands on a period start; h0 stays positive
    times = [BASE - 600 * (n_prev - 1 - j) for j in range(n_prev)]
    tp = cm.tip(h0 - 1, times, 0x1c05a3f4, BASE - 600 * ((h0 - 1) % interval) - 5, 0x1c05a3f4, (1 << 255) - 3)
    now = BASE + n * 1000 + 10000
    head = []
    if 2 <= n < 255:
        head.append((1, now + 100000, cm.want_next(head, tp, p, now + 100000)))
        head.append((0x20000000, 1, cm.want_next(head, tp, p, 1) ^ 1))
    if n == 1 and min_difficulty:
        now = BASE - 100000
        head.append((1, BASE - 50000, cm.want_next(head, tp, p, BASE - 50000) ^ 1))
    elif n == 1:
        head.append((0x20000000, BASE + 600, cm.want_next(head, tp, p, BASE + 600)))
    facts = cm.random_chain(n * 131 + n_prev * 7 + PLACEMENTS.index(placement), n, tp, p, now,
                            wrong=0.03 if n >= 1023 else 0.06 if n >= 255 else 0.2, head=head)
    rng = np.random.default_rng(n + n_prev)
    hashes = [rng.bytes(32) for _ in range(n)]
    picks = sorted(set(int(x) for x in rng.integers(0, n, size=min(n, 6))) | set(range(len(head))))
    wrong_at_0 = n == 1 and min_difficulty
    cps = [(h0 + i, bytes(32) if i == 1 or (i > 1 and k % 2) or (i == 0 and wrong_at_0) else hashes[i])
           for k, i in enumerate(picks)]
    cps = [(5, bytes(32))] + cps + [(h0 + n + 3, hashes[0])]
    return p, tp, facts, now, cps, hashes


def flag_states(flags):
    """(the flags set somewhere, the flags cleared somewhere) of a batch."""
    b_set = b_clear = 0
    for f in flags:
        b_set |= f
        b_clear |= ~f & cm.ALL
    return b_set, b_clear


def placement_fits(n, placement):
    """A boundary at index 1 needs two headers, two boundaries need five (the interval is at least 2)."""
    return not (placement == "at_1" and n < 2) and not (placement == "twice" and n < 5)


EDGE_CASES = [(n, k, pl) for n in SIZES for k in (1, 5, 11) for pl in PLACEMENTS if placement_fits(n, pl)]


def edge_case(n, n_prev, placement):
    return edge_batch(n, n_prev, placement, min_difficulty=(n + (1, 5, 11).index(n_prev) + PLACEMENTS.index(placement)) % 2 == 1)


@pytest.mark.parametrize("n,n_prev,placement", EDGE_CASES)
def test_scan_and_halo_edges(verifier, n, n_prev, placement):
    """Every listed size (around the tile of 256, the retarget period and the
    11-header halo, and 300,000: 1,172 tiles, more than the 256 lanes of the
    one scan workgroup, so its loop over rounds carries both operators) with
    every n_prev_times of {1, 5, 11} and every boundary placement that fits the
    size: the whole cross product, one batch per case.

    Each of the five flags is both set and cleared in every batch of two
    headers or more. A batch of one header cannot hold both states of a flag:
    test_one_header_batches_reach_both_states (tests/test_chainctx_model.py, a
    check of this generator that needs no GPU) takes those together."""
    assert 300000 > TILE * TILE
    p, tp, facts, now, cps, hashes = edge_case(n, n_prev, placement)
    want = cm.connect(facts, tp, p, now, cps, hashes)
    if n >= 2:
        assert flag_states(want[3]) == (cm.ALL, cm.ALL), flag_states(want[3])
    boundaries = [i for i in range(n) if (tp.height + 1 + i) % p.interval == 0]
    assert len(boundaries) >= (2 if placement == "twice" else 1)
    assert {"at_0": 0, "at_1": 1, "at_last": n - 1, "twice": 1}[placement] in boundaries
    got = stage_on_device(verifier, facts, tp, p, now, cps, hashes)
    assert_stage(got, want, "n=%d n_prev=%d %s" % (n, n_prev, placement))


@pytest.mark.parametrize("n", [1, 12, 257, 2017])
def test_edges_through_the_composed_forms(verifier, n):
    """The same random batches as real headers through hkv_connect_headers and
    hkv_connect_headers_device (the hashes are then the headers' own)."""
    p, tp, facts, now, _, _ = edge_batch(n, 5, "at_1" if n > 1 else "at_0", min_difficulty=n % 2 == 1)
    headers = [cm.make_header(*f, nonce=i) for i, f in enumerate(facts)]
    hs = [ho.header_hash(h) for h in headers]
    cps = [(tp.height + 1, hs[0]), (tp.height + n, bytes(32))]
    check_both_forms(verifier, headers, tp, p, now, cps if n > 1 else cps[:1], what="n=%d" % n)


# ---------------------------------------------------------------- directed operands

def test_directed_operands(verifier):
    """The CPU case file's operands through the device: the vectors, both
    clamps, a negative span, a result above the limit, an overflowing parent,
    every compact shape's work, the eight-limb carry chains, the median
    windows with ties, the version thresholds, the minimum-difficulty runs."""
    cases = cm.directed_cases()
    assert len(cases) > 50
    for name, p, tp, facts, now, cps, hs in cases:
        want = cm.connect(facts, tp, p, now, cps, hs)
        got = stage_on_device(verifier, facts, tp, p, now, cps, hs)
        assert_stage(got, want, name)
    for name in ("work_carry_all_limbs", "above_limit_nine_limbs", "md_run_ends_in_context", "future_64_bit"):
        _, p, tp, facts, now, _, _ = next(c for c in cases if c[0] == name)
        check_both_forms(verifier, [cm.make_header(*f) for f in facts], tp, p, now, what=name)


def test_minimum_difficulty_run_longer_than_a_tile(verifier):
    """700 headers: a run at the limit that starts in the context, 290 headers
    long, then one of 319 that crosses a period start: real(P) comes through
    the tile scan's carry-in for whole tiles."""
    pm, tp, facts, now = cm.long_min_difficulty_run()
    want = cm.connect(facts, tp, pm, now)
    assert all(f & cm.BITS_OK for f in want[3]) and want[1][290] == 0x1c05a3f4 and want[1][289] == 0x1d00ffff
    assert_stage(stage_on_device(verifier, facts, tp, pm, now), want)
    # the same with every gap too short: every header then wants real(P), tiles away
    short = [(v, facts[0][1] + 600 * i, b) for i, (v, _, b) in enumerate(facts)]
    want = cm.connect(short, tp, pm, now)
    assert want[1][289] == 0x1c05a3f4 and want[1][600] != 0x1d00ffff
    assert_stage(stage_on_device(verifier, short, tp, pm, now), want)


def test_work_carries_across_tiles(verifier):
    """1,000 headers of work 2^255 on a parent work of 2^256 - 1: every sum
    wraps, inside the tiles and through the tile scan."""
    p = cm.params(pow_limit=(1 << 255) - 1, flags=cm.NO_RETARGET)
    tp = cm.tip(99, [BASE], 0x01010000, BASE, 0x01010000, cm.M256)
    facts = [(4, BASE + 600 * (i + 1), 0x01010000) for i in range(1000)]
    want = cm.connect(facts, tp, p, BASE + 10**6)
    assert want[2][0] == (1 << 255) - 1 and want[2][1] == cm.M256 and want[2][999] == cm.M256
    assert_stage(stage_on_device(verifier, facts, tp, p, BASE + 10**6), want)


# ---------------------------------------------------------------- checkpoints

@pytest.mark.parametrize("count", [0, 1, 64])
def test_checkpoints(verifier, count):
    import hkv
    n = 600
    p = cm.params()
    tp = cm.tip(9999, [BASE], 0x1c05a3f4, BASE - 5000, 0x1c05a3f4, 1)
    facts = [(4, BASE + 600 * (i + 1), 0x1c05a3f4) for i in range(n)]
    hashes = [cm.fake_hash(i, 7) for i in range(n)]
    # heights below the batch, inside it (every other one with the wrong hash), above it
    inside = [10000 + (i * 37) % n for i in range(max(0, count - 4))] if count > 1 else ([10255] if count else [])
    cps = sorted(set([(h, hashes[h - 10000] if k % 2 == 0 else cm.fake_hash(k, 8)) for k, h in enumerate(inside)] +
                     ([(3, bytes(32)), (9999, hashes[0]), (10600, hashes[1]), (2**32 - 1, hashes[2])] if count > 1 else [])))
    assert len(cps) == count
    want = cm.connect(facts, tp, p, BASE + 10**6, cps, hashes)
    bad = [i for i, f in enumerate(want[3]) if not f & cm.CHECKPOINT_OK]
    assert len(bad) == (30 if count == 64 else 0)
    assert_stage(stage_on_device(verifier, facts, tp, p, BASE + 10**6, cps, hashes), want)
    if count == 0:
        # no checkpoints: d_hashes may be NULL
        assert_stage(stage_on_device(verifier, facts, tp, p, BASE + 10**6, (), None), want)
    else:
        with pytest.raises(hkv.HkvError) as e:
            stage_on_device(verifier, facts, tp, p, BASE + 10**6, cps, None)
        assert e.value.rc == -1


# ---------------------------------------------------------------- first_bad

def mined_chain(n, tp, p, now, seed, break_link_at=None, bad_version_at=None):
    """n linked regtest headers that pass isValidPOW (a nonce per header), with
    a broken prev link or a version the height forbids where asked."""
    rng = np.random.default_rng(seed)
    prev = hashlib.sha256(b"tip%d" % seed).digest()
    tip_hash, out, t = prev, [], tp.times[-1]
    for i in range(n):
        t += 600
        version = 2 if i == bad_version_at else 4
        link = rng.bytes(32) if i == break_link_at else prev
        merkle, nonce = rng.bytes(32), 0
        while True:
            h = cm.make_header(version, t, 0x207fffff, link, merkle, nonce)
            if ho.pow_flags(h, p.pow_limit) & ho.POW_OK:
                break
            nonce += 1
        out.append(h)
        prev = ho.header_hash(h)
    return out, tip_hash


@pytest.mark.parametrize("link_at,version_at", [(300, None), (None, 300), (257, 400), (500, 255), (None, None), (0, None),
                                                (None, 599)])
def test_first_bad(verifier, link_at, version_at):
    """n_ok is the index of the first header that fails hkv_check_headers (a
    broken link), the chain rule (a version below 3 above the BIP66 height), or
    either; 600 when none does."""
    p = cm.params(pow_limit=(1 << 255) - 1, flags=cm.NO_RETARGET | cm.MIN_DIFFICULTY, bip34_height=10**8,
                  bip66_height=1251, bip65_height=1351)
    tp = cm.tip(1999, [BASE], 0x207fffff, BASE, 0x207fffff, 4000)
    headers, tip_hash = mined_chain(600, tp, p, BASE + 10**6, 1, link_at, version_at)
    n_ok = check_both_forms(verifier, headers, tp, p, BASE + 10**6, (), tip_hash, "first_bad")
    assert n_ok == min(x for x in (link_at, version_at, 600) if x is not None)


def test_first_bad_in_a_later_step_of_its_chunk(verifier):
    """70,000 linked regtest headers that pass isValidPOW: 274 tiles, more than
    the reduction's 256 workgroups, so each covers a chunk of 512 headers in two
    steps. The first failing header stands in a second step (51,500 = 100 * 512
    + 300); a later one stands in the first step of its chunk (60,000)."""
    n = 70000
    p = cm.params(pow_limit=(1 << 255) - 1, flags=cm.NO_RETARGET | cm.MIN_DIFFICULTY, bip34_height=10**8,
                  bip66_height=1251, bip65_height=1351)
    tp = cm.tip(1999, [BASE], 0x207fffff, BASE, 0x207fffff, 4000)
    target = 0x7fffff << 232
    prev = tip_hash = hashlib.sha256(b"long").digest()
    headers = []
    tail = (0x207fffff).to_bytes(4, "little")
    for i in range(n):
        head = (2 if i in (51500, 60000) else 4).to_bytes(4, "little") + prev + bytes(32) + \
            (BASE + 600 * (i + 1)).to_bytes(4, "little") + tail
        nonce = 0
        while True:
            h = head + nonce.to_bytes(4, "little")
            d = hashlib.sha256(hashlib.sha256(h).digest()).digest()
            if int.from_bytes(d, "little") <= target:
                break
            nonce += 1
        headers.append(h)
        prev = d
    now = BASE + 600 * n + 100
    e_hash, e_hst = ho.check_headers(headers, p.pow_limit, tip_hash)
    assert all(s == ho.POW_OK | ho.LINK_OK for s in e_hst)
    want = cm.connect([cm.fields(h) for h in headers], tp, p, now, (), e_hash)
    assert cm.first_bad(want[3], e_hst) == 51500 and want[3][60000] != cm.ALL
    d = connect_on_device(verifier, headers, tp, p, now, (), tip_hash)
    assert d[1] == e_hst
    assert_stage(d[2:6], want)
    assert d[6] == 51500
    # and with nothing failing (a network whose heights allow version 2): every chunk is read to its end
    p2 = cm.params(pow_limit=(1 << 255) - 1, flags=cm.NO_RETARGET | cm.MIN_DIFFICULTY, bip34_height=10**8,
                   bip66_height=10**8, bip65_height=10**8)
    d = connect_on_device(verifier, headers, tp, p2, now, (), tip_hash)
    assert d[6] == n and d[5] == [cm.ALL] * n


def test_argument_errors(verifier):
    import ctypes
    import hkv
    from hkv.chain import ChainParams, ChainTip
    p = hkv.CHAIN_PARAMS["btc"]
    tip = ChainTip(100, (BASE,), 0x1d00ffff, BASE, 0x1d00ffff, 5)
    hdrs = [cm.make_header(4, BASE + 600 * (i + 1), 0x1d00ffff) for i in range(3)]

    def rc_of(tip=tip, p=p, cps=(), headers=hdrs, mutate=None):
        raw = np.frombuffer(b"".join(headers), dtype=np.uint8).copy() if headers else np.zeros(1, dtype=np.uint8)
        n = len(headers)
        c = hkv.chain_ctx(tip, p, BASE + 10**6)
        if mutate:
            mutate(c)
        cph, cpx = hkv.chain.pack_checkpoints(cps)
        out = [np.zeros(max(1, n) * k, dtype=np.uint8) for k in (32, 1, 4, 4, 32, 1)]
        ok = ctypes.c_size_t(99)
        rc = verifier.lib.hkv_connect_headers(verifier.ctx, raw.ctypes.data, n, None, ctypes.byref(c),
                                              cph.ctypes.data if len(cph) else None,
                                              cpx.ctypes.data if len(cph) else None, len(cph),
                                              *[o.ctypes.data for o in out], ctypes.byref(ok))
        return rc, ok.value

    assert rc_of() == (0, 0)                       # (nothing mined: header 0 fails isValidPOW)
    assert rc_of(headers=[]) == (0, 0)             # n = 0 succeeds with n_ok = 0
    assert rc_of(mutate=lambda c: setattr(c, "height0", 0))[0] == -1
    assert rc_of(mutate=lambda c: setattr(c, "n_prev_times", 0))[0] == -1
    assert rc_of(mutate=lambda c: setattr(c, "n_prev_times", 12))[0] == -1
    assert rc_of(mutate=lambda c: setattr(c, "interval", 0))[0] == -1
    assert rc_of(mutate=lambda c: setattr(c, "target_timespan", 3))[0] == -1
    assert rc_of(mutate=lambda c: setattr(c, "target_timespan", 4))[0] == 0
    assert rc_of(cps=[(7, bytes(32)), (5, bytes(32))])[0] == -1
    assert rc_of(cps=[(5, bytes(32)), (5, bytes(32))])[0] == -1
    assert rc_of(cps=[(5, bytes(32)), (7, bytes(32))])[0] == 0
    assert rc_of(mutate=lambda c: setattr(c, "height0", 2**32 - 2))[0] == -1   # height0 + n passes 2^32 - 1
    # the device forms on the live context: the same context checks (height0 = 0, a timespan below 4)
    facts = [cm.fields(h) for h in hdrs]
    mp = cm.params()
    for bad_tip, bad_p in ((cm.tip(-1, [BASE], 0x1d00ffff, BASE, 0x1d00ffff, 5), mp),
                           (cm.tip(100, [BASE], 0x1d00ffff, BASE, 0x1d00ffff, 5), cm.params(target_timespan=3))):
        with pytest.raises(hkv.HkvError) as e:
            stage_on_device(verifier, facts, bad_tip, bad_p, BASE + 10**6)
        assert e.value.rc == -1
        with pytest.raises(hkv.HkvError) as e:
            connect_on_device(verifier, hdrs, bad_tip, bad_p, BASE + 10**6)
        assert e.value.rc == -1
    assert stage_on_device(verifier, facts, cm.tip(100, [BASE], 0x1d00ffff, BASE, 0x1d00ffff, 5), mp, BASE + 10**6)[3] == \
        cm.connect(facts, cm.tip(100, [BASE], 0x1d00ffff, BASE, 0x1d00ffff, 5), mp, BASE + 10**6)[3]


# ---------------------------------------------------------------- threading on device

def test_threading_messages_on_device(verifier):
    """10,000 headers as one call and as five calls of 2,000 threaded through
    ChainTip.advance: equal outputs, and the model's."""
    import hkv
    from hkv.chain import ChainTip
    p = cm.params(interval=144, target_timespan=144 * 600, bip34_height=100, bip66_height=3000, bip65_height=7000,
                  flags=cm.MIN_DIFFICULTY)
    tp = cm.tip(1000, (BASE - 1200, BASE - 600, BASE), 0x1c05a3f4, BASE - 70000, 0x1c05a3f4, (1 << 70) + 5)
    now = BASE + 10000 * 1000
    facts = cm.random_chain(77, 10000, tp, p, now)
    headers = [cm.make_header(*f) for f in facts]
    hp, tip = to_params(p), to_tip(tp)
    whole = hkv.connect_headers(verifier, headers, tip, hp, (), now)
    want = cm.connect(facts, tp, p, now)
    assert_stage((whole.mtp.tolist(), whole.bits.tolist(), whole.work, whole.chain_status.tolist()), want)
    got = ([], [], [], [])
    for k in range(0, 10000, 2000):
        r = hkv.connect_headers(verifier, headers[k:k + 2000], tip, hp, (), now)
        for a, b in zip(got, (r.mtp.tolist(), r.bits.tolist(), r.work, r.chain_status.tolist())):
            a.extend(b)
        tip = tip.advance(headers[k:k + 2000], r, 2000)
    assert_stage(got, want, "threaded")
    assert (tip.height, tip.work) == (11000, want[2][-1])
