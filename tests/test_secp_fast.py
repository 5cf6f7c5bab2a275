"""The libsecp256k1-class CPU stand-in (oracle/secp_fast.c, bench.py's
cpu_baseline fast leg) against the port (oracle/hkv_oracle.c) and the
fixtures (CPU only):

- every golden KAT class and the special pool (r + n branch, edge scalars,
  u1 = 0, msg >= n, sum = infinity, ladder collisions), both modes, equal to
  the manifest labels;
- every adversarial class of hkv.adversarial (configs[3]) and generated
  configs[4]-style batches (5-30% invalid), equal to the port and the labels;
- its s^-1 (variable-time safegcd) against pow(s, -1, n) on edge and random
  scalars, and its GLV split: k1 + k2 lambda == k (mod n), |k1|, |k2| < 2^129;
- it is the faster checker: >= 2x the port's single-thread rate here, under
  the parallel test load (3.4x on the GPU box's host, profiles/r04a_bench.log);
- its record builders (hkvo_fast_chosen_records, hkvo_fast_gtable_records, the
  input of tests/test_gpu_chosen_scalars.py): m / s and r / s of every record,
  recomputed on Python integers, are the requested scalars (or the documented
  sign pair); the port, the Python oracle and OpenSSL accept the records; the
  error returns; and one stand-alone run under ASan + UBSan
  (tests/secp_fast_builders.c)."""
import ctypes
import json
import multiprocessing
import os
import random
import subprocess
import time

import numpy as np
import pytest

import chosen_scalars as cs
import recoding as rc
import secp256k1_oracle as o
from conftest import GOLDEN, ROOT, c_gen_batch, fast_batch, host_threads, openssl_batch, oracle_batch
from hkv import adversarial

@pytest.fixture(scope="module")
def fast(secpfast):
    lib = secpfast
    lib.hkvo_fast_sc_inverse.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.hkvo_fast_glv_split.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p]
    return lib


@pytest.mark.parametrize("mode,key", [(0, "libsecp"), (1, "haskoin")])
def test_golden_kats_and_special_pool(fast, mode, key):
    man = json.load(open(os.path.join(GOLDEN, "kat_manifest.json")))
    data = open(os.path.join(GOLDEN, "kat_records.bin"), "rb").read()
    got = fast_batch(fast, data, mode)
    exp = np.array([r[key] for r in man["records"]])
    bad = [man["records"][i]["class"] for i in np.nonzero(got != exp)[0]]
    assert not bad, bad
    sp = json.load(open(os.path.join(GOLDEN, "special_pool.json")))
    data = open(os.path.join(GOLDEN, "special_pool.bin"), "rb").read()
    got = fast_batch(fast, data, mode)
    exp = np.array([r[key] for r in sp["records"]])
    bad = sorted({sp["records"][i]["class"] for i in np.nonzero(got != exp)[0]})
    assert not bad, bad


def test_every_adversarial_class(fast, coracle):
    rng = random.Random(11)
    recs = []
    for i in range(64):
        q = o.point_mul(rng.randrange(1, o.N), o.G)
        m, r, s = o.keyless_tuple(rng.randrange(1, o.N), rng.randrange(1, o.N), q)
        if s > o.N // 2:
            s = o.N - s
        recs.append(o.make_record(m, r.to_bytes(32, "big") + s.to_bytes(32, "big"), o.pubkey_serialize(q, i % 5 != 0)))
    base = np.frombuffer(b"".join(recs), dtype=np.uint8)
    adv, lib_lab, hask_lab, cls = adversarial.mutate(np.tile(base, 30), seed=17, invalid_frac=0.7, special_frac=0.2)
    for mode, lab in ((0, lib_lab), (1, hask_lab)):
        got = fast_batch(fast, adv, mode)
        assert (got == oracle_batch(coracle, adv.tobytes(), mode)).all()
        bad = sorted({adversarial.CLASSES[c] for c in cls[got != lab]})
        assert not bad, (mode, bad)


@pytest.mark.parametrize("seed,inv", [(0x484B5635, 50), (0x1234, 300)])
def test_generated_batches_equal_port(fast, coracle, seed, inv):
    recs, lab, _ = c_gen_batch(coracle, seed, 4096, 2000, 64, 100, inv)
    for mode in (0, 1):
        got = fast_batch(fast, recs, mode)
        assert (got == oracle_batch(coracle, recs.tobytes(), mode)).all()
        assert (got == lab).all()


def test_scalar_inverse(fast):
    rng = random.Random(5)
    vals = [1, 2, 3, o.N - 1, o.N - 2, o.N // 2, 2**128, 2**255 % o.N, (1 << 62) - 1, 1 << 62, 1 << 124]
    vals += [rng.randrange(1, o.N) for _ in range(3000)]
    out = ctypes.create_string_buffer(32)
    for v in vals:
        fast.hkvo_fast_sc_inverse(v.to_bytes(32, "big"), out)
        assert int.from_bytes(out.raw, "big") == pow(v, -1, o.N), hex(v)


def test_glv_split(fast):
    lam = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
    rng = random.Random(6)
    vals = [0, 1, o.N - 1, lam, o.N - lam, (o.N - 1) // 2] + [rng.randrange(o.N) for _ in range(3000)]
    m1 = (ctypes.c_uint64 * 3)()
    m2 = (ctypes.c_uint64 * 3)()
    s1, s2 = ctypes.c_int(), ctypes.c_int()
    for k in vals:
        fast.hkvo_fast_glv_split(k.to_bytes(32, "big"), m1, ctypes.byref(s1), m2, ctypes.byref(s2))
        a = m1[0] | m1[1] << 64 | m1[2] << 128
        b = m2[0] | m2[1] << 64 | m2[2] << 128
        assert a < 2**129 and b < 2**129
        assert (s1.value * a + s2.value * b * lam - k) % o.N == 0


def test_faster_than_port(fast, coracle):
    """The point of the stand-in: of the reference library's class (GLV,
    w = 15 G tables, safegcd), well above the port's rate on one thread (best
    of three runs of each)."""
    recs, _, _ = c_gen_batch(coracle, 0x484B5632, 0, 1200, 64, 100, 0)

    def rate(fn):
        out = np.zeros(1200, dtype=np.uint8)
        best = 0.0
        for _ in range(3):
            t0 = time.perf_counter()
            fn(recs.ctypes.data_as(ctypes.c_void_p), 1200, 0, out.ctypes.data_as(ctypes.c_void_p), 1)
            best = max(best, 1200 / (time.perf_counter() - t0))
        assert out.all()
        return best

    assert rate(fast.hkvo_fast_verify_batch) >= 2 * rate(coracle.hkvo_verify_batch)


def test_cpu_baseline_reports_both_whole_host_extrapolations(coracle, monkeypatch):
    """bench.py's CPU leg on a small sample (short points): the SMT-core
    point (1 thread on one CPU, then 2 threads on it and a sibling; the
    sibling pair is forced to two CPUs of this container's mask, which has no
    SMT) feeds whole_host.smt_extrapolated_value, and north_star_ratio quotes
    the stricter SMT ratio first and decides target_met_whole_host by it."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    aff = sorted(os.sched_getaffinity(0))
    if len(aff) < 2:
        pytest.skip("needs two CPUs")
    monkeypatch.setattr(bench, "smt_pair", lambda: (aff[0], aff[1]))
    monkeypatch.setattr(bench, "physical_cores", lambda info: 128)
    recs, _, _ = c_gen_batch(coracle, 0x484B5632, 0, 200, 64, 100, 0)
    cpu = bench.cpu_baseline([("s", recs, 1, None)], [1, 2], min_s=0.05)
    wh = cpu["whole_host"]
    smt = wh["smt_core"]
    assert smt["cpus"] == [aff[0], aff[1]] and smt["core_rate_smt"] > 0 and smt["core_rate_1t"] > 0
    assert wh["smt_extrapolated_value"] == round(smt["core_rate_smt"] * 128, 1)
    assert "UPPER bound" in cpu["kind_note"]
    assert os.sched_getaffinity(0) == set(aff)  # restored
    r = bench.north_star_ratio(1e8, cpu)
    assert list(r)[0] == "whole_host_smt_extrapolated"
    assert r["whole_host_smt_extrapolated"] == round(1e8 / wh["smt_extrapolated_value"], 1)
    assert r["target_met_whole_host"] == (r["whole_host_smt_extrapolated"] >= 50.0)


def test_bench_checker_leg_counts_mismatches(coracle, secpfast):
    """bench.py's mismatches_vs_checker leg: every record of the slice through
    secp_fast, compared bit for bit with the slice of the gathered bitmap —
    0 on the construction labels of a configs[4]-style slice, and a flipped
    verdict is counted."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    recs, lab, _ = c_gen_batch(coracle, 0x484B5635, 777_000, 2000, 65536, 100, 50)
    r = bench.checker_leg(recs, lab, 0)
    assert r["checked"] == 2000 and r["mismatches"] == 0 and r["checker"] == "oracle/secp_fast.c"
    bad = lab.copy()
    bad[[3, 1999]] ^= True
    assert bench.checker_leg(recs, bad, 0)["mismatches"] == 2


# --- the record builders with exact scalars ---------------------------------
@pytest.fixture(scope="module")
def builders(secpfast):
    return cs.bind(secpfast)


@pytest.fixture(scope="module")
def chosen(builders):
    """The directed set S (tests/chosen_scalars.py): (names, u1, u2, pin, records)."""
    names, u1, u2, d, pin = cs.directed_set()
    recs = cs.chosen_records(builders, u1, u2, d, pin)
    recs.setflags(write=False)
    return names, u1, u2, pin, recs


def table_runs():
    """(t, j0, step, count, neg) of short sweeps at both ends of every table, and of the negative form."""
    runs = []
    for t in range(14):
        last = rc.GTAB_ENTRIES if t < 12 else 255  # (entry 256 of window 6 is not a j 2^off: test_chosen_scalars.py)
        runs += [(t, 1, 1, 24, 0), (t, last - 23, 1, 24, 0)]
        if t < 12:
            runs.append((t, 1, (rc.GTAB_ENTRIES - 2) // 15, 16, 1))  # j = 1 .. 2^19 - 1
    return runs


@pytest.fixture(scope="module")
def swept(builders):
    """[(run, records)] of table_runs()."""
    return [(run, cs.gtable_records(builders, run[0], run[1], run[3], neg=run[4], step=run[2])) for run in table_runs()]


def low_s(rec):
    return 0 < int.from_bytes(bytes(rec[64:96]), "big") <= o.HALF_N


def test_chosen_records_compute_the_requested_scalars(chosen):
    """A pinned scalar comes out of m / s or r / s exactly, with s low (so both
    modes compute it). Pinning u1 alone may negate u2 (with the key); pinning
    u2 alone leaves u1 to the builder."""
    names, u1, u2, pin, recs = chosen
    assert len(names) > 1500 and {cs.PIN_U1, cs.PIN_U2, cs.PIN_BOTH} == set(pin)
    negated = 0
    for i, rec in enumerate(recs.reshape(-1, 168)):
        assert low_s(rec), names[i]
        a, b = cs.scalars_of(rec)
        if pin[i] == cs.PIN_U2:
            assert b == u2[i], names[i]
        elif pin[i] == cs.PIN_U1:
            assert a == u1[i] and b in (u2[i], o.N - u2[i]), names[i]
            negated += b != u2[i]
        else:
            assert (a, b) == (u1[i], u2[i]), names[i]
        assert rec[96] == (33 if i % 2 == 0 else 65)
    assert negated > 10  # the sign pair is exercised


def test_gtable_records_compute_the_requested_scalars(swept):
    """u1 = j 2^off (or (2^20 - j) 2^off) exactly, so the restated G digits read
    entry j of table t (and entry 1 of the next window's table in the negative
    form and at j = 2^19); u2 is one value per call, up to the sign that goes
    with the key."""
    for (t, j0, step, count, neg), recs in swept:
        off = rc.GTAB_W * (t // 2) + 128 * (t % 2)
        u2s = set()
        for k, rec in enumerate(recs.reshape(-1, 168)):
            j = j0 + k * step
            assert low_s(rec)
            a, b = cs.scalars_of(rec)
            u2s.add(min(b, o.N - b))
            assert a == ((2**20 - j) if neg else j) << off, (t, j, neg)
            reads = rc.table_reads(a)
            if neg:
                assert reads == {t: -j, t + 2: 1}, (t, j, reads)
            elif j == rc.GTAB_ENTRIES:
                assert reads == {t: -j, t + 2: 1}, (t, j, reads)
            else:
                assert reads == {t: j}, (t, j, reads)
        assert len(u2s) == 1, (t, j0, neg)


def _python_verdicts(rec):
    return o.verify_record(rec, o.HKV_LIBSECP), o.verify_record(rec, o.HKV_HASKOIN)


def test_builder_records_accepted_by_every_checker(builders, coracle, openssl, chosen, swept):
    """Every record of S and of the table runs is valid for hkv_oracle.c, for the
    Python oracle and for the stand-in itself, in both modes; OpenSSL accepts
    4,096 (all of those and a stretch from the middle of a table)."""
    recs = np.concatenate([chosen[4]] + [r for _, r in swept])
    n = len(recs) // 168
    assert 2000 < n < 4096
    for mode in (0, 1):
        assert fast_batch(builders, recs, mode).all()
        got = oracle_batch(coracle, recs.tobytes(), mode)
        assert got.all(), np.nonzero(~got)[0][:10]
    rows = [bytes(r) for r in recs.reshape(-1, 168)]
    with multiprocessing.get_context("fork").Pool(host_threads()) as pool:
        got = np.array(pool.map(_python_verdicts, rows, chunksize=16))
    assert got.all(), np.nonzero(~got.all(axis=1))[0][:10]
    sample = np.concatenate([recs, cs.gtable_records(builders, 9, 2**18, 4096 - n)])
    for mode in (0, 1):
        got = openssl_batch(openssl, sample.tobytes(), mode)
        assert len(got) == 4096 and got.all(), np.nonzero(~got)[0][:10]


def test_builder_error_returns(builders):
    """Nothing is skipped silently: the first record that cannot be built is
    named with its reason, and a table range outside 1..2^19, a u1 >= n or a
    negative form without a next window is refused."""
    u1, u2, d, pin = [5, 6, 7, 1], [9, 0, 3, 1], [2, 2, 2, o.N - 1], [cs.PIN_U1, cs.PIN_U2, cs.PIN_BOTH, cs.PIN_BOTH]
    assert cs.chosen_rc(builders, u1[:1], u2[:1], d[:1], pin[:1])[0] == 0
    assert cs.chosen_rc(builders, u1, u2, d, pin)[0] == (1, 2)            # u2 = 0
    u2[1] = 4
    assert cs.chosen_rc(builders, u1, u2, d, pin)[0] == (3, 4)            # u1 + u2 d = 0: R at infinity
    assert cs.chosen_rc(builders, u1[:3], u2[:3], [2, 0, 2], pin[:3])[0] == (1, 1)        # d = 0
    assert cs.chosen_rc(builders, u1[:3], u2[:3], d[:3], [1, 2, 4])[0] == (2, 1)          # unknown pin
    assert cs.chosen_rc(builders, [o.N, 1], [1, 1], [1, 1], [1, 1])[0] == (0, 1)          # u1 >= n
    out = np.zeros(2 * 168, dtype=np.uint8)
    for args in ((14, 1, 1, 0), (-1, 1, 1, 0), (0, 0, 1, 0), (0, 2**19, 2, 0), (13, 256, 1, 0), (12, 1, 1, 1)):
        assert builders.hkvo_fast_gtable_records(*args, out.ctypes.data) == -1, args
    assert not out.any()


def test_builders_under_asan_ubsan(tmp_path):
    """tests/secp_fast_builders.c: both builders in a program of their own under
    AddressSanitizer and UndefinedBehaviorSanitizer (any report aborts it)."""
    exe = str(tmp_path / "secp_fast_builders")
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "secp_fast_builders.c"), "-lpthread"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 5000
