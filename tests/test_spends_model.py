"""CPU tests of hkv_block_spends_device below the GPU: the Python model of the
spend rule (tests/spends_model.py) on the chained batch the GPU parity test
runs and on directed amounts; the rule's header
(haskoin-node_amd/csrc/hkv_spends.h: sizing, hash, insert, lookup, walk, fold)
as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer against the model; the sizing rule through the C
ABI; and the new entry points' bad-argument returns, which need no device."""
import ctypes
import os
import subprocess

import pytest

import blocktx_model as bm
import spends_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chain():
    return bm.chained_batch(7, 200)


@pytest.fixture(scope="module")
def spends(chain):
    return sm.Spends(chain.raw, chain.prevouts, sm.MAX_MONEY)


def test_chained_batch_leaves_every_branch(chain, spends):
    """The batch of the GPU parity test: 465 inputs, 102 of them not the first
    spender of their outpoint, one null outpoint, 13 txs without inputs, and
    each of the five flags of HKV_SPEND_OK both set and clear."""
    s = spends
    n = s.first[-1]
    assert n == 465 and len(s.off) == len(s.spender) == len(s.src) == len(s.value) == n
    assert sum(s.spender[g] != g for g in range(n)) == 102
    assert sum(op == sm.NULL_OUTPOINT for op in s.outpoint) == 1
    no_inputs = [t for t in range(len(chain.raw)) if s.first[t + 1] == s.first[t]]
    assert len(no_inputs) == 13 and all(s.flags[t] == 0 and s.sums[t] == (0, 0) for t in no_inputs)
    judged = [f for t, f in enumerate(s.flags) if s.first[t + 1] > s.first[t]]
    for flag in (sm.RESOLVED, sm.FIRST, sm.IN_RANGE, sm.OUT_RANGE, sm.BALANCED):
        assert any(f & flag for f in judged) and any(not f & flag for f in judged), hex(flag)
    # the named coinbase-form input stands in a tx of three inputs: no COINBASE flag
    t, i = chain.named["coinbase_form"]
    assert s.spender[s.first[t] + i] == s.first[t] + i and not s.flags[t] & sm.COINBASE
    # spender is the dict's answer: the smallest index with those 36 bytes
    for g in range(n):
        same = [u for u in range(n) if s.outpoint[u] == s.outpoint[g]]
        assert s.spender[g] == (g if s.outpoint[g] == sm.NULL_OUTPOINT else same[0])
    # offsets point at the outpoints in the concatenated tx bytes
    blob = b"".join(chain.raw)
    assert all(blob[s.off[g]:s.off[g] + 36] == s.outpoint[g] for g in range(n))


def test_directed_amounts():
    raws, prevouts, want = sm.directed_amounts()
    s = sm.Spends(raws, prevouts, sm.MAX_MONEY)
    for name, (t, flags, sums) in want.items():
        assert (s.flags[t], s.sums[t]) == (flags, sums), name
    assert s.sums[want["out_sum_is_max"][0]][1] == sm.MAX_MONEY
    assert s.flags[want["in_equals_out"][0]] & sm.BALANCED and not s.flags[want["in_is_out_minus_1"][0]] & sm.BALANCED
    assert s.flags[want["no_outputs"][0]] == sm.OK
    # a lone null outpoint is the coinbase form; it resolves nowhere
    cb = bm.SignedChain(9300, None, n=2, coinbase=True)
    c = sm.Spends(cb.raw, cb.prevouts, sm.MAX_MONEY)
    assert c.flags[0] & sm.COINBASE and not c.flags[0] & sm.RESOLVED and not any(f & sm.COINBASE for f in c.flags[1:])


def _host_program(tmp_path):
    exe = str(tmp_path / "spends_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "spends_host.cpp")], check=True)
    return exe


def test_rule_header_vs_model_under_asan_ubsan(tmp_path, chain):
    """hkv_spends.h compiled for the host with the sanitizers: offsets,
    spender, sums and flags equal the model's at hash masks 0xFFFFFFFF, 0xF
    and 0, on the chained batch, the directed amounts, the walk's batch and a
    batch of 1,000 inputs on a pool of 200 outpoints."""
    exe = _host_program(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    batches = {"chain": (chain.raw, chain.prevouts), "amounts": sm.directed_amounts()[:2], "walk": sm.walk_batch(),
               "pool": sm.outpoint_batch(5, 1000), "one": sm.outpoint_batch(6, 1)}
    for name, (raws, prevouts) in batches.items():
        blob, inputs = sm.emit_cases(raws, prevouts, sm.MAX_MONEY)
        path = tmp_path / f"{name}.bin"
        path.write_bytes(blob)
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, name + ": " + r.stdout + r.stderr
        assert r.stdout.split() == ["ok", str(inputs), str(len(raws))], r.stdout
    assert sm.emit_cases(*batches["chain"], sm.MAX_MONEY)[1] == 465


@pytest.mark.parametrize("n", [0, 1, 32, 33, 2**20, 2**30, 2**30 + 1])
def test_sizing_rule_through_the_abi(n):
    import hkv
    lib = hkv.load_library()
    s = lib.hkv_spend_table_slots(n)
    if n > 2**30:
        assert s == 0                              # the table would exceed 2^31 slots
        return
    assert s >= 64 and s >= 2 * n and s & (s - 1) == 0 and s <= 2**31
    assert s == 64 or s // 2 < 2 * n               # the smallest such power of two


def test_bad_arguments_rejected_without_device():
    import hkv
    lib = hkv.load_library()
    assert lib.hkv_version() == (1 << 16) | 4
    w = ctypes.c_uint32()
    f = ctypes.c_uint8()
    money = sm.MAX_MONEY
    # a NULL context, whatever else is passed
    assert lib.hkv_block_spends_device(None, 0, None, None, None, None, 0, money, None, None, 64, None, None, None,
                                       None, None) == -1
    assert lib.hkv_verify_block_txs_spends(None, None, None, None, None, None, -1, money, ctypes.byref(w), None, None,
                                           None, 0, None, ctypes.byref(f)) == -1
    assert lib.hkv_debug_spend_stages(None, 0, 15) == -1
    # max_money = 2^63, a slot count that is no power of two, one below the sizing rule's
    assert lib.hkv_block_spends_device(None, 0, None, None, None, None, 0, 2**63, None, None, 64, None, None, None,
                                       None, None) == -1
    assert lib.hkv_block_spends_device(None, 0, None, None, None, None, 0, money, None, None, 96, None, None, None,
                                       None, None) == -1
    assert lib.hkv_block_spends_device(None, 0, None, None, None, None, 100, money, None, None, 128, None, None,
                                       None, None, None) == -1
    assert lib.hkv_verify_block_txs_spends(None, None, None, None, None, None, -1, 2**63, ctypes.byref(w), None, None,
                                           None, 0, None, ctypes.byref(f)) == -1
    assert lib.hkv_verify_block_txs_spends(None, None, None, None, None, None, -1, money, ctypes.byref(w), None, None,
                                           None, 0, None, None) == -1
    assert (hkv.HKV_SPEND_RESOLVED, hkv.HKV_SPEND_FIRST, hkv.HKV_SPEND_IN_RANGE, hkv.HKV_SPEND_OUT_RANGE,
            hkv.HKV_SPEND_BALANCED, hkv.HKV_SPEND_COINBASE, hkv.HKV_SPEND_OK) == (1, 2, 4, 8, 16, 32, 31)
