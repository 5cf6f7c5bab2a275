"""CPU tests of the header chain-context stage below the GPU: the Python model
of the rule (tests/chainctx_model.py) on Bitcoin's published retarget vectors
and known headerWork values; ChainTip.advance threading 2,000-header messages;
the rule's header (haskoin-node_amd/csrc/hkv_chainctx.h) as a stand-alone host
program under AddressSanitizer and UndefinedBehaviorSanitizer against the
model's case files; and the new entry points' bad-argument returns, which need
no device."""
import ctypes
import os
import subprocess

import pytest

import chainctx_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("first,last,old,new", cm.VECTORS)
def test_published_retarget_vectors(first, last, old, new):
    """Bitcoin's pow_tests vectors (get_next_work, pow_limit, lower and upper
    limit of the actual time span). The expected bits are the published ones."""
    p = cm.params()
    assert cm.retarget(p, old, last, first) == (new, False)
    # through the whole rule: one header on a boundary, the period's first block in the context
    p, tp, facts = cm.boundary_case(first, last, old)
    mtp, want, work, flags = cm.connect(facts, tp, p, last + 10000)
    assert want == [new] and flags == [cm.ALL] and mtp == [last]
    # as a 2,017-header batch that holds the period: header 0 is its first block
    step = (last - first) // 2015
    times = [first + step * j for j in range(2015)] + [last]
    batch = [(4, t, old) for t in times] + [(4, last + 600, new)]
    tp = cm.tip(2016 * 9 - 1, [first - 600], old, first - 1209600, old, 1)
    # (header 0 stands on a boundary itself: whatever it wants, the last header's want is the vector's)
    _, want, _, flags = cm.connect(batch, tp, p, last + 10000)
    assert want[2016] == new and flags[2016] == cm.ALL


def test_header_work_known_values():
    assert cm.header_work(0x1d00ffff) == 0x100010001
    assert cm.header_work(0x207fffff) == 2
    assert cm.header_work(0x01010000) == 1 << 255
    for bits in (0x01810000, 0x04923456, 0x22000100, 0x21010000, 0x23000001, 0xff123456, 0, 0x00123456, 0x03000000):
        assert cm.header_work(bits) == 0, hex(bits)


def test_readings_are_listed_in_the_design():
    """Every reading taken without haskoin-core's source is named in the model's
    docstring and in DESIGN.md (as tests/test_std_readings.py does for templates)."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in cm.READINGS:
        assert name in cm.__doc__ and name in design, name


def test_directed_cases_say_what_they_claim():
    cases = {c[0]: c for c in cm.directed_cases()}

    def run(name):
        _, p, tp, facts, now, cps, hs = cases[name]
        return cm.connect(facts, tp, p, now, cps, hs)

    T = 1209600
    assert run("clamp_low")[1][0] == run("clamp_low_edge")[1][0] == cm.encode_compact((0x05a3f4 << 200) // 4)
    assert run("negative_span")[1][0] == run("clamp_low")[1][0]
    assert run("clamp_high")[1][0] == run("clamp_high_edge")[1][0] == cm.encode_compact((0x05a3f4 << 200) * 4)
    assert run("above_limit")[1][0] == 0x1d00ffff and run("above_limit_nine_limbs")[1][0] == 0x207fffff
    assert 1 << 256 <= (0x7fffff << 232) * 4 * T < 1 << 288          # that product has nine limbs
    _, want, _, flags = run("overflow_parent")
    assert want[0] == 0 and not flags[0] & cm.BITS_OK
    assert all(f & cm.BITS_OK for f in run("clamp_low")[3][:1]) and not run("clamp_low")[3][1] & cm.BITS_OK
    assert run("zero_parent")[1][0] == 0 and run("zero_parent")[3][0] & cm.BITS_OK
    # the sums wrap through all eight limbs
    w = run("work_carry_all_limbs")[2]
    assert w[0] == 1 and w[1] == (1 << 255) + 1 and w[3] == 3
    w = run("work_carry_top")[2]
    assert w[1] == 9 and w[0] == (1 << 255) + 9
    # median windows: c = n_prev + i elements, ties included
    for n_prev in range(1, 12):
        _, p, tp, facts, now, _, _ = cases["mtp_window_%d" % n_prev]
        mtp = cm.connect(facts, tp, p, now)[0]
        times = list(tp.times) + [f[1] for f in facts]
        for i in range(len(facts)):
            win = sorted(times[max(0, n_prev + i - 11):n_prev + i])
            assert mtp[i] == win[len(win) // 2]
    # versions: (version, first height at which it fails)
    for v, bad_from in ((1, 1000), (2, 1003), (3, 1006), (4, None), (0x20000000, None), (0x80000000, 1000)):
        for h0 in (999, 1002, 1005):
            fl = run("version_%x_at_%d" % (v, h0))[3]
            assert [bool(f & cm.VERSION_OK) for f in fl] == [bad_from is None or h0 + j < bad_from for j in range(3)]
    assert [f & cm.BITS_OK for f in run("md_run_ends_at_non_limit")[3]] == [4] * 5
    assert [f & cm.BITS_OK for f in run("md_run_ends_in_context")[3]] == [4] * 4
    assert run("md_run_ends_at_period_start")[1][5] == 0x1d00ffff    # the period start's own bits, though the limit's
    assert [f & cm.BITS_OK for f in run("md_gap_exact")[3]] == [4, 0, 4, 4]
    assert [bool(f & cm.CHECKPOINT_OK) for f in run("checkpoints")[3]] == [True, True, True, False, True, True, True, True]
    assert [bool(f & cm.NOT_FUTURE) for f in run("future")[3]] == [True, True, False, False]
    assert all(f & cm.NOT_FUTURE for f in run("future_64_bit")[3])


def test_threading_messages_through_chain_tip():
    """10,000 headers at interval 144 as one batch and as five messages of
    2,000 threaded through ChainTip.advance: every output is equal."""
    import hkv
    from hkv.chain import ChainParams, ChainTip, ConnectResult
    base = 1500000000
    for flags in (0, cm.MIN_DIFFICULTY):
        p = ChainParams(pow_limit=(1 << 224) - 1, bip34_height=100, bip66_height=3000, bip65_height=7000, flags=flags,
                        interval=144, target_timespan=144 * 600)
        tip0 = ChainTip(height=1000, times=(base - 1200, base - 600, base), bits=0x1c05a3f4,
                        period_first_time=base - 70000, period_real_bits=0x1c05a3f4, work=(1 << 70) + 5)
        now = base + 10000 * 700
        facts = cm.random_chain(21 + flags, 10000, tip0, p, now)
        headers = [cm.make_header(*f) for f in facts]
        whole = cm.connect(facts, tip0, p, now)
        assert {f & flag for f in whole[3] for flag in (1, 2, 4, 8)} == {0, 1, 2, 4, 8}
        tip, got = tip0, ([], [], [], [])
        for k in range(0, 10000, 2000):
            part = cm.connect(facts[k:k + 2000], tip, p, now)
            for a, b in zip(got, part):
                a.extend(b)
            r = ConnectResult([], None, None, None, None, part[2], 2000, p)
            nxt = tip.advance(headers[k:k + 2000], r, 2000)
            m = cm.advance(tip, facts[k:k + 2000], part[2], 2000, p)
            assert (nxt.height, nxt.times, nxt.bits, nxt.period_first_time, nxt.period_real_bits, nxt.work) == \
                (m.height, m.times, m.bits, m.period_first_time, m.period_real_bits, m.work)
            tip = nxt
        assert tuple(got) == tuple(whole)
    assert hkv.CHAIN_PARAMS["btc"].limit_bits == 0x1d00ffff and hkv.CHAIN_PARAMS["btcRegTest"].limit_bits == 0x207fffff
    assert hkv.chain.header_work(0x1d00ffff) == cm.header_work(0x1d00ffff)


def test_package_compact_helpers_equal_the_model():
    """hkv.chain's own encode_compact and header_work (ChainParams.limit_bits,
    ChainTip.genesis) against the model's and the oracle's on every compact
    shape of the work cases and on the targets they decode to."""
    import random
    from hkv import chain
    for bits in cm.WORK_COMPACTS + [cm.VECTORS[k][j] for k in range(4) for j in (2, 3)]:
        assert chain.header_work(bits) == cm.header_work(bits), hex(bits)
        value, neg, over = cm.decode_compact(bits)
        if not over:
            assert chain.encode_compact(value) == cm.encode_compact(value), hex(bits)
    rng = random.Random(5)
    for _ in range(2000):
        bits = rng.getrandbits(32)
        assert chain.header_work(bits) == cm.header_work(bits), hex(bits)
        x = rng.getrandbits(rng.randrange(0, 257))
        assert chain.encode_compact(x) == cm.encode_compact(x), hex(x)
    for x in (0, 1, 0x7f, 0x80, 0x7fff, 0x8000, 0x7fffff, 0x800000, (1 << 224) - 1, (1 << 255) - 1, (1 << 256) - 1):
        assert chain.encode_compact(x) == cm.encode_compact(x), hex(x)


def test_one_header_batches_reach_both_states():
    """A check of the GPU test's generator, on the model alone: the batches of
    one header that tests/test_gpu_chainctx.py test_scan_and_halo_edges draws,
    taken together, set and clear each of the five flags. One header cannot
    hold both states of a flag, so this is the form the property takes at
    n = 1; the device's answers on those batches are compared there."""
    import test_gpu_chainctx as g
    seen_set = seen_clear = 0
    ones = [c for c in g.EDGE_CASES if c[0] == 1]
    assert len(ones) == 6
    for n, n_prev, placement in ones:
        p, tp, facts, now, cps, hashes = g.edge_case(n, n_prev, placement)
        b_set, b_clear = g.flag_states(cm.connect(facts, tp, p, now, cps, hashes)[3])
        seen_set, seen_clear = seen_set | b_set, seen_clear | b_clear
    assert (seen_set, seen_clear) == (cm.ALL, cm.ALL)


def _host_program(tmp_path):
    exe = str(tmp_path / "chainctx_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "chainctx_host.cpp")], check=True)
    return exe


def test_rule_header_vs_model_under_asan_ubsan(tmp_path):
    """hkv_chainctx.h compiled for the host with the sanitizers: mtp, want,
    work and flags equal the model's on every directed case, on the long
    minimum-difficulty run and on random chains of both flag sets; the median
    network sorts all 2^11 zero-one inputs."""
    exe = _host_program(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["network", "ok"], r.stdout + r.stderr
    cases = [(c[0], c[1], c[2], c[3], c[4], c[5], c[6]) for c in cm.directed_cases()]
    pm, tp, facts, now = cm.long_min_difficulty_run()
    cases.append(("long_min_difficulty", pm, tp, facts, now, (), None))
    base = 1500000000
    for seed, flags in ((1, 0), (2, cm.MIN_DIFFICULTY), (3, cm.NO_RETARGET)):
        p = cm.params(interval=144, target_timespan=144 * 600, flags=flags, bip34_height=100, bip66_height=1500,
                      bip65_height=2500)
        tp = cm.tip(1000 + seed, [base - 600, base], 0x1c05a3f4, base - 70000, 0x1c05a3f4, 1 << 200)
        cases.append(("random%d" % seed, p, tp, cm.random_chain(seed, 3000, tp, p, base + 3000 * 700), base + 3000 * 700,
                      (), None))
    assert len(cases) > 50
    paths = []
    for name, p, tp, facts, now, cps, hs in cases:
        path = tmp_path / (name + ".txt")
        path.write_text(cm.emit_case(p, tp, facts, now, cps, hs))
        paths.append((str(path), len(facts)))
    r = subprocess.run([exe] + [p for p, _ in paths], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [w for _, n in paths for w in ("ok", str(n))]


def test_scratch_size_and_bad_arguments_without_device():
    import hkv
    from hkv.lib import HkvChainCtx
    lib = hkv.load_library()
    for n in (0, 1, 256, 257, 2000, 1 << 20):
        assert lib.hkv_chain_scratch_words(n) == 3 * n + 20 * ((n + 255) // 256)
    c = HkvChainCtx()
    ok = ctypes.c_size_t()
    w = ctypes.c_uint32()
    # a NULL context, whatever else is passed
    assert lib.hkv_chain_context_device(None, 0, None, 0, None, ctypes.byref(c), None, None, 0, None, None, None, None,
                                        None, None) == -1
    assert lib.hkv_connect_headers_device(None, 0, None, 0, None, None, ctypes.byref(c), None, None, 0, None, None,
                                          None, None, None, None, None, ctypes.byref(w), None) == -1
    assert lib.hkv_connect_headers(None, None, 0, None, ctypes.byref(c), None, None, 0, None, None, None, None, None,
                                   None, ctypes.byref(ok)) == -1
    assert lib.hkv_debug_chain_stages(None, 0, 15) == -1
    assert (hkv.HKV_CHN_TIME_OK, hkv.HKV_CHN_NOT_FUTURE, hkv.HKV_CHN_BITS_OK, hkv.HKV_CHN_VERSION_OK,
            hkv.HKV_CHN_CHECKPOINT_OK, hkv.HKV_CHN_ALL) == (1, 2, 4, 8, 16, 31)
    assert (hkv.HKV_CHAIN_NO_RETARGET, hkv.HKV_CHAIN_MIN_DIFFICULTY) == (1, 2)
