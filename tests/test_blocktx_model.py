"""CPU tests of hkv_verify_block_txs* below the GPU: the Python model of the
in-batch prevout rule (tests/blocktx_model.py) on each named variant of the
chained-batch generator; the rule's header (haskoin-node_amd/csrc/hkv_blocktx.h:
sizing, hash, probe, insert, lookup, output walk) as a stand-alone host program
under AddressSanitizer and UndefinedBehaviorSanitizer against the model; the
sizing rule through the C ABI; and the new entry points' bad-argument returns,
which need no device."""
import ctypes
import os
import subprocess

import pytest

import blocktx_model as bm
import sighash_oracle as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chain():
    return bm.chained_batch(20261, n_fill=200)


@pytest.fixture(scope="module")
def resolved(chain):
    first, rows = bm.resolve(chain.raw, chain.prevouts)
    return first, {(t, i): row for row in rows for (t, i) in [row[:2]]}


def test_every_variant_is_in_the_batch_and_resolves_as_the_rule_says(chain, resolved):
    first, at = resolved
    src = lambda name: at[chain.named[name]][2]
    for name in ("plain_parent", "zero_length_parent_script", "bip144_parent", "noncanonical_parent_txhash",
                 "fd_form_parent", "duplicate_parents_between", "duplicate_parents_after", "shared_outpoint_batch"):
        assert src(name) < chain.named[name][0], name           # an earlier tx of the batch
    for name in ("index_equals_count", "index_past_count", "index_ffffffff", "bip144_wire_hash",
                 "noncanonical_parent_wire_hash", "forward_reference", "unparsable_parent", "coinbase_form"):
        assert src(name) == bm.SRC_NONE, name
    for name in ("list_precedence", "shared_outpoint_list"):
        assert src(name) == bm.SRC_LIST, name
    assert src("duplicate_parents_between") == src("duplicate_parents_after") == chain.dup_first
    assert at[chain.named["zero_length_parent_script"]][4] == b""
    # the fd-form parent's output 2 lies behind two inputs and two outputs with 3-byte lengths
    row = at[chain.named["fd_form_parent"]]
    p, (k, off, ln) = row[2], row[3]
    assert k == 2 and ln == 25 and off > 253 + 300 + 300 + 253 and chain.raw[p][off:off + ln] == row[4]
    assert len(chain.raw) > 200 and first[-1] > 400
    kinds = [r[2] for r in at.values()]
    assert sum(k == bm.SRC_LIST for k in kinds) > 50 and sum(k == bm.SRC_NONE for k in kinds) > 50
    assert sum(k < bm.SRC_LIST for k in kinds) > 100


def test_augmented_lists_hold_one_more_entry_per_in_batch_input(chain):
    """P' of the differential test: the lists plus what the model resolved in
    the batch; on P' nothing is left to resolve there but what the lists
    already lacked, and the inputs' scripts and amounts are the same."""
    _, rows = bm.resolve(chain.raw, chain.prevouts)
    aug = bm.augmented(chain.raw, chain.prevouts)
    assert sum(len(a) - len(p) for a, p in zip(aug, chain.prevouts)) == sum(r[2] < bm.SRC_LIST for r in rows)
    _, again = bm.resolve(chain.raw, aug)
    assert [(r[2] == bm.SRC_NONE, r[4], r[5]) for r in again] == [(r[2] == bm.SRC_NONE, r[4], r[5]) for r in rows]
    assert all(r[2] in (bm.SRC_LIST, bm.SRC_NONE) for r in again)


def test_output_refs_follow_the_wire_bytes():
    raw = bm.chained_batch(3, n_fill=0).raw
    for r in raw:
        tx = bm.model.parse_or_none(r)
        if tx is None:
            continue
        refs = bm.output_refs(r)
        assert [(r[o:o + n], v) for (o, n, v) in refs] == [(to.script, to.value) for to in tx.outputs]


def test_rule_header_vs_model_under_asan_ubsan(tmp_path, chain):
    """hkv_blocktx.h compiled for the host with the sanitizers: the table built
    sequentially, every lookup and every input's in-batch resolution equal the
    model's, at hash masks 0xFFFFFFFF, 0x3 and 0."""
    exe = str(tmp_path / "blocktx_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "blocktx_host.cpp")], check=True)
    blob, inputs = bm.emit_cases(chain)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.split()
    assert out[:2] == ["ok", str(inputs)] and int(out[2]) > len(chain.raw), r.stdout
    assert inputs > 400


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 2**20])
def test_sizing_rule_through_the_abi(n):
    import hkv
    lib = hkv.load_library()
    s = lib.hkv_txid_table_slots(n)
    assert s >= 64 and s >= 2 * n and s & (s - 1) == 0
    assert s == 64 or s // 2 < 2 * n           # the smallest such power of two
    assert lib.hkv_txid_table_slots(0xFFFFFF00) == 0


def test_bad_arguments_rejected_without_device():
    import hkv
    lib = hkv.load_library()
    assert lib.hkv_version() >> 16 == 1 and lib.hkv_version() & 0xFFFF >= 3
    w = ctypes.c_uint32()
    assert lib.hkv_txid_index_device(None, 0, None, 0, None, 64, None) == -1
    assert lib.hkv_txid_lookup_device(None, 0, None, 0, None, 64, None, 0, None, None) == -1
    assert lib.hkv_block_tx_jobs_device(None, 0, None, None, None, None, None, 0, None, None, 64, None, None, None,
                                        None, None) == -1
    assert lib.hkv_verify_block_txs_device(None, 0, None, None, None, None, None, -1, 0, None, None, 64, None, None,
                                           None, None, None, None, None, None) == -1
    assert lib.hkv_verify_block_txs(None, None, None, None, None, None, -1, ctypes.byref(w), None, None, 0) == -1
    assert lib.hkv_debug_txid_hash_mask(None, 0, 0) == -1
    assert hkv.HKV_SRC_NONE == 0xFFFFFFFF and hkv.HKV_SRC_LIST == 0xFFFFFFFE
