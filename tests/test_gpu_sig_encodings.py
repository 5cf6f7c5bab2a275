"""GPU tests (MI355X): the signature-encoding case table
(tests/sig_encodings.py: every DER, hashtype and push-form branch, about
2,500 inputs per network) through every site that instantiates the parsers:

  records   hkv_std_input_kernel (hkv_std_inputs_device): each single-signature
            case's 168-byte record, all zero for a reject, exact r / s bytes
            for an accept
  alone     <= 4,096 inputs: the block kernel (LDS tx view, key_only parses on
            the chain waves, the fused multisig scan)
  pair      shuffled into a 2,600-tx block: the pair kernel and the separate
            scan kernel
  overlap   shuffled into a 20,000-tx block (> 32,768 inputs): the lane-prologue
            parse of the ecmult launch, the record parse and the multisig scan
            on the hash stream

In the three verify shapes the host and the device entry points run; the
single-signature records equal the oracle's, the verdicts equal the C oracle's
on the oracle's records (multisig: the oracle's countMulSig walk), every case
built to verify (each value-preserving variant's canonical twin among them)
is true and every case whose decode must fail is false, so a site that
accepts a lax encoding fails by the case's name. Batches above one resident
grid parse through the same hkv_std_input_kernel as the records shape and are
not repeated here."""
import functools
import random

import pytest

import launch_shapes
import sighash_oracle as sh
import sig_encodings as se
from conftest import oracle_batch
from test_gpu_sighash import _device_verify_std, _ms_oracle, device_std_records
from test_gpu_sighash import torch, ver  # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu

FORKIDS = [None, 0]
ZERO_REC = b"\x00" * 168


@functools.lru_cache(maxsize=None)
def _table(forkid):
    """(cases, raw txs, jobs, the oracle's records): built once per network."""
    table = se.cases(forkid)
    txs, jobs = se.batch(table)
    exp = [sh.std_input_record(t, i, p, v, forkid) for t, (_, i, p, v) in zip(txs, jobs)]
    for c, rec in zip(table, exp):    # the oracle's record is all zero exactly for a reject (and for multisig)
        assert (rec != ZERO_REC) == (c.kind == "single" and c.expectation == "accept"), c.name
    return table, [sh.tx_serialize(t) for t in txs], jobs, exp


_WANT = {}


def _want(coracle, forkid):
    """The oracle's verdict per case, computed once per network: the C oracle
    on the oracle's records; multisig by the countMulSig walk."""
    if forkid not in _WANT:
        table, raw, jobs, exp = _table(forkid)
        want = oracle_batch(coracle, b"".join(exp), 1).tolist()
        ms = [k for k, c in enumerate(table) if c.kind == "multisig"]
        ms_want = _ms_oracle(coracle, [raw[k] for k in ms], [(q,) + jobs[k][1:] for q, k in enumerate(ms)], forkid)
        for k, w in zip(ms, ms_want):
            want[k] = w
        bad = [c.name for c, w in zip(table, want) if c.verifies is not None and w != c.verifies]
        assert not bad, bad[:10]
        _WANT[forkid] = want
    return _WANT[forkid]


def _check(label, table, exp, want, got, recs):
    """got / recs in table order (recs: 168-byte slices, or None)."""
    if recs is not None:
        bad = [c.name for c, e, r in zip(table, exp, recs) if c.kind == "single" and r != e]
        assert not bad, (label, "records", bad[:10])
    bad = [(c.name, g, w) for c, g, w in zip(table, got, want) if g != w]
    assert not bad, (label, "verdicts", bad[:10])
    by = {c.name: k for k, c in enumerate(table)}
    bad = [c.name for c, g in zip(table, got) if c.expectation == "reject" and g]
    assert not bad, (label, "lax encoding accepted", bad[:10])
    bad = [c.name for c, g in zip(table, got) if c.verifies is True and not g]
    assert not bad, (label, "canonical form rejected", bad[:10])
    bad = [c.name for c in table if c.twin and not got[by[c.twin]]]
    assert not bad, (label, "canonical twin rejected", bad[:10])


def _slices(recs, n):
    return [recs[k * 168:(k + 1) * 168] for k in range(n)]


@pytest.mark.parametrize("forkid", FORKIDS)
def test_records_kernel(torch, ver, forkid):  # noqa: F811
    table, raw, jobs, exp = _table(forkid)
    idx = [k for k, c in enumerate(table) if c.kind == "single"]
    recs = _slices(device_std_records(torch, ver, raw, [jobs[k] for k in idx], forkid), len(idx))
    bad = [table[k].name for k, r in zip(idx, recs) if r != exp[k]]
    assert not bad, bad[:10]
    assert sum(r != ZERO_REC for r in recs) == sum(table[k].expectation == "accept" for k in idx) > 250


@pytest.mark.parametrize("forkid", FORKIDS)
def test_alone_block_kernel(torch, ver, coracle, forkid):  # noqa: F811
    import hkv
    table, raw, jobs, exp = _table(forkid)
    assert len(jobs) <= 16 * 256
    assert launch_shapes.std_inputs(ver, len(jobs))[:2] == (
        launch_shapes.BLOCK, launch_shapes.SCAN_IN_KERNEL | launch_shapes.ROWS_IN_KERNEL)
    want = _want(coracle, forkid)
    _check("host", table, exp, want, hkv.verify_std_inputs(ver, raw, jobs, forkid), None)
    got, recs = _device_verify_std(torch, ver, raw, jobs, forkid, records=True)
    _check("device", table, exp, want, got, _slices(recs, len(jobs)))


@pytest.mark.parametrize("forkid", FORKIDS)
@pytest.mark.parametrize("n_fill", [2600, 20000])
def test_shuffled_into_block(torch, ver, coracle, n_fill, forkid):  # noqa: F811
    """2,600-tx filler: the pair kernel with the scan kernel; 20,000-tx
    filler: the overlapped mid-size form."""
    import hkv
    from hkv import blockgen
    table, raw, jobs, exp = _table(forkid)
    want = _want(coracle, forkid)
    btxs, bjobs = blockgen.make_block(ver, torch, n_tx=n_fill, seed=blockgen.SEED + 99 + n_fill)
    all_raw = btxs + raw
    all_jobs = list(bjobs) + [(t + len(btxs), i, p, v) for (t, i, p, v) in jobs]
    order = list(range(len(all_jobs)))
    random.Random(0x5348 + n_fill).shuffle(order)
    jobs_sh = [all_jobs[k] for k in order]
    # one chunk of the shape meant (the library's plan: hkv_launch_plan.h)
    want_shape = ((launch_shapes.MID, launch_shapes.OVERLAP) if n_fill >= 20000 else (launch_shapes.PAIR, 0))
    assert launch_shapes.std_inputs(ver, len(jobs_sh)) == want_shape + (len(jobs_sh), 1)
    where = {k - len(bjobs): pos for pos, k in enumerate(order) if k >= len(bjobs)}
    fill = [pos for pos, k in enumerate(order) if k < len(bjobs)]

    got, recs = _device_verify_std(torch, ver, all_raw, jobs_sh, forkid, records=True)
    recs = _slices(recs, len(jobs_sh))
    _check("device", table, exp, want, [got[where[k]] for k in range(len(table))],
           [recs[where[k]] for k in range(len(table))])
    # the filler: verdicts equal the C oracle's on the records the call wrote
    fill_want = oracle_batch(coracle, b"".join(recs[pos] for pos in fill), 1).tolist()
    assert [got[pos] for pos in fill] == fill_want
    if forkid is None:
        assert all(fill_want)
    host = hkv.verify_std_inputs(ver, all_raw, jobs_sh, forkid)
    _check("host", table, exp, want, [host[where[k]] for k in range(len(table))], None)
    assert host == got
