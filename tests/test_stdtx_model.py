"""CPU tests of batch verifyStdTx below the GPU: the Python model
(tests/stdtx_model.py, matchTemplate / verifyStdTx restated on the oracle's tx
codec) on each consequence of the contract with hand-built lists; the matching
rule the job-builder kernel compiles (haskoin-node_amd/csrc/hkv_stdtx.h) as a
stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer
against the model on more than 10,000 inputs; and the new entry points'
bad-argument returns, which need no device."""
import ctypes
import os
import random
import struct
import subprocess

import pytest

import sighash_oracle as sh
import stdtx_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def op(tag: int, index: int = 0) -> bytes:
    return bytes([tag]) * 32 + struct.pack("<I", index)


def tx_of(outpoints) -> bytes:
    ins = [sh.TxIn(o[:32], struct.unpack("<I", o[32:])[0], b"", 0xFFFFFFFF) for o in outpoints]
    return sh.tx_serialize(sh.Tx(1, ins, [sh.TxOut(1, b"\x51")], [], 0))


def by_script(want):
    """verifyStdInput stand-in: input i verifies iff it was handed script want[i]."""
    return lambda tx, i, spk, value: spk == want[i]


def test_match_template_is_first_match_consumed():
    f = lambda a, b: a[0] == b
    assert model.match_template([("x", 1), ("y", 2), ("x", 3)], ["x", "x", "x", "y"], f) == \
        [("x", 1), ("x", 3), None, ("y", 2)]
    assert model.match_template([], ["x"], f) == [None]
    assert model.match_template([("x", 1)], [], f) == []


def test_rank_among_equal_outpoints():
    """Consequence 1: with d earlier inputs on the same outpoint, input i takes
    the (d + 1)-th entry with that outpoint in list order."""
    A, B = op(1), op(2)
    raw = tx_of([A, B, A, A, B])
    entries = [(B, b"b0", 0), (A, b"a0", 1), (op(9), b"zz", 2), (A, b"a1", 3), (B, b"b1", 4), (A, b"a2", 5)]
    assert model.matched_entries(raw, entries) == [1, 0, 3, 5, 4]
    assert model.verify_std_tx(raw, entries, by_script([b"a0", b"b0", b"a1", b"a2", b"b1"]))
    # the same entries with two A's swapped: inputs 0 and 2 get each other's script
    swapped = [entries[0], entries[3], entries[2], entries[1]] + entries[4:]
    assert model.matched_entries(raw, swapped) == [1, 0, 3, 5, 4]
    assert not model.verify_std_tx(raw, swapped, by_script([b"a0", b"b0", b"a1", b"a2", b"b1"]))
    # near-equal outpoints are different outpoints
    assert model.matched_entries(tx_of([op(1, 1)]), [(op(1, 0), b"", 0), (op(1, 1), b"", 0)]) == [1]


def test_unmatched_input_and_extra_entries():
    """Consequences 2 and 3."""
    A, B = op(1), op(2)
    raw = tx_of([A, B])
    yes = lambda *a: True
    assert model.matched_entries(raw, [(A, b"", 0)]) == [0, None]
    assert not model.verify_std_tx(raw, [(A, b"", 0)], yes)
    assert not model.verify_std_tx(tx_of([A, A]), [(A, b"", 0)], yes)          # one entry, two inputs on it
    extra = [(op(7), b"", 0), (B, b"", 0), (A, b"", 0), (A, b"", 0), (op(8), b"", 0)]
    assert model.matched_entries(raw, extra) == [2, 1]
    assert model.verify_std_tx(raw, extra, yes)


def test_empty_list_no_inputs_and_parse_failure():
    """Consequences 4, 5 and 6: all false, whatever verifyStdInput says."""
    yes = lambda *a: True
    raw = tx_of([op(1)])
    assert not model.verify_std_tx(raw, [], yes)
    empty = sh.tx_serialize(sh.Tx(1, [], [sh.TxOut(1, b"\x51"), sh.TxOut(2, b"")], [], 0))
    assert sh.tx_parse(empty).inputs == []
    assert not model.verify_std_tx(empty, [(op(1), b"", 0)], yes)
    for bad in (raw[:-1], raw + b"\0", raw[:20], b""):
        assert model.parse_or_none(bad) is None
        assert model.matched_entries(bad, [(op(1), b"", 0)]) == []
        assert not model.verify_std_tx(bad, [(op(1), b"", 0)], yes)
    assert model.verify_std_tx(raw, [(op(1), b"", 0)], yes)
    assert model.model_jobs([raw, raw[:-1], empty, tx_of([op(1), op(2)])],
                            [[(op(1), b"s", 5)], [(op(1), b"s", 5)], [], [(op(2), b"t", 6)]]) == \
        ([0, 1, 1, 1, 3], [(0, 0, b"s", 5), (3, 0, None, 0), (3, 1, b"t", 6)])


def test_matching_rule_header_vs_model_under_asan_ubsan(tmp_path):
    """hkv_stdtx.h match_prevout, compiled for the host with the sanitizers,
    gives every input of >= 10,000 (random txs of 1-40 inputs on a pool of 3
    outpoints, lists shuffled, truncated, padded with strangers and with
    surplus entries) the entry the model's matchTemplate gives it."""
    exe = str(tmp_path / "stdtx_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "stdtx_host.cpp")], check=True)
    blob, total = model.emit_match_cases(random.Random(20260), 10000)
    assert total >= 10000
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(total)], r.stdout
    # the cases do contain what the rule is about
    n_cases = struct.unpack_from("<I", blob)[0]
    assert n_cases > 300 and blob.count(struct.pack("<I", model.NONE)) > 500


def test_bad_arguments_rejected_without_device():
    import hkv
    lib = hkv.load_library()
    assert lib.hkv_version() >> 16 == 1 and lib.hkv_version() & 0xFFFF >= 2   # (the minor half counts ABI additions)
    w = ctypes.c_uint32()
    assert lib.hkv_std_tx_jobs_device(None, 0, None, None, None, None, None, 0, None, None, None, None) == -1
    assert lib.hkv_tx_verdicts_device(None, 0, None, 1, None, None, None) == -1
    assert lib.hkv_verify_std_txs_device(None, 0, None, None, None, None, None, -1, 0, None, None, None, None, None,
                                         None, None) == -1
    assert lib.hkv_verify_std_txs(None, None, None, None, None, None, -1, ctypes.byref(w)) == -1
