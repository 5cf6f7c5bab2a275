"""GPU tests of the record pipeline (hkv_api.cpp enqueue_table_chain: a table /
chain batch cut into parts that run table, chain, finish, rare and verdict
launches over their own windows, two at a time on two streams in two slots of
the Q scratch; hkv_launch_plan.h RecPlan::part_len).

The batch is the smallest that takes the table and chain launches on this
device (found through hkv_debug_launch_shape: n = 131,073 on an MI355X, which
pads to 131,328): generated filler with 5 % invalid, every record of the golden
KAT set, and the records of tests/golden/special_pool.bin — the finish kernel's
rare lanes (A at infinity, A = +-B, the sum at infinity) and the r + n
candidate — at the last and first index of every part of the shortest length,
two indices either side of it, and densely on both sides of the boundaries of
the two- and three-part plans and at both ends of the batch. Contexts opened
with the env hook HKV_REC_PART run it in two parts, in three with a short last
part, and in parts of the shortest aligned length (each slot reused over a
hundred times); in both modes the bitmap must equal the bitmap with parts off,
bit for bit, and the verdicts of oracle/secp_fast.c on every record. The
reference verdicts are computed once per mode and shared."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, fast_batch, host_threads

pytestmark = pytest.mark.gpu

SEED = 0x50495045
WG, ALIGN = 256, 512  # hkv_layout.h WG, hkv_launch_plan.h PART_ALIGN


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


def open_with_parts(part):
    """A context whose geometry took HKV_REC_PART=part at open."""
    import hkv
    old = os.environ.get("HKV_REC_PART")
    os.environ["HKV_REC_PART"] = str(part)
    try:
        return hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1))  # HKV_OPEN_NO_SELFCHECK
    finally:
        if old is None:
            del os.environ["HKV_REC_PART"]
        else:
            os.environ["HKV_REC_PART"] = old


def launch_shape(v, n):
    out = (ctypes.c_uint32 * 4)()
    assert v.lib.hkv_debug_launch_shape(v.ctx, 0, 0, n, out) == 0
    return list(out)


def rec_parts(v, n):
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert v.lib.hkv_debug_rec_parts(v.ctx, 0, n, ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


@pytest.fixture(scope="module")
def off(torch):
    v = open_with_parts(0)
    yield v
    v.close()


@pytest.fixture(scope="module")
def n_min(off):
    """The smallest record batch of shape 4 (table and chain launches)."""
    lo, hi = 1, 1 << 22
    assert launch_shape(off, hi)[0] == 4
    while lo < hi:
        mid = (lo + hi) // 2
        if launch_shape(off, mid)[0] == 4:
            hi = mid
        else:
            lo = mid + 1
    assert launch_shape(off, lo)[0] == 4 and launch_shape(off, lo - 1)[0] == 3
    return lo


def pad(n):
    return (n + WG - 1) // WG * WG


@pytest.fixture(scope="module")
def lengths(n_min):
    """Part lengths for two parts, three with a short last one, and the shortest."""
    n_pad = pad(n_min)
    two = (n_pad // 2 + ALIGN - 1) // ALIGN * ALIGN
    three = (n_pad - 1) // 2 // ALIGN * ALIGN
    assert two < n_pad <= 2 * two and 2 * three < n_pad <= 3 * three and n_pad - 2 * three < three
    return {"two": two, "three": three, "shortest": ALIGN}


@pytest.fixture(scope="module")
def batch(torch, off, n_min, lengths):
    """The records (host, read-only): filler, the KATs, the special pool at the part edges."""
    from hkv import adversarial
    n, n_pad = n_min, pad(n_min)
    d = torch.empty(n * 168, dtype=torch.uint8, device="cuda")
    off.gen_batch_device(0, SEED, 0, n, 65536, 100, 50, d.data_ptr(), 0)
    torch.cuda.synchronize()
    recs = d.cpu().numpy().reshape(-1, 168).copy()
    pool = adversarial.load_pool()[0]
    k = pool.shape[0]
    kat = np.fromfile(os.path.join(GOLDEN, "kat_records.bin"), dtype=np.uint8).reshape(-1, 168)
    assert ALIGN + 2 + len(kat) <= 2 * ALIGN - 2
    recs[ALIGN + 2:ALIGN + 2 + len(kat)] = kat
    # every boundary of the shortest parts: a pool record at the part's last
    # index and the next part's first, the pair swapped two indices out
    for m, b in enumerate(range(ALIGN, n_pad, ALIGN)):
        for i, j in ((b - 1, 2 * m), (b, 2 * m + 1), (b - 2, 2 * m + 1), (b + 1, 2 * m)):
            if i < n:
                recs[i] = pool[j % k]
    # the boundaries of the two- and three-part plans and the head of the batch, half the pool on each side (the
    # batch ends at the three-part plan's last boundary: its last record is that part's first index)
    h = k // 2
    marks = [lengths["three"], 2 * lengths["three"], lengths["two"], h]
    assert all(abs(a - b) >= 2 * h for a in marks for b in marks if a != b) and 2 * h <= ALIGN - 2
    assert 0 < n - 2 * lengths["three"] <= h
    for m, b in enumerate(marks):
        for i in range(h):
            if b + i < n:
                recs[b + i] = pool[(2 * i + m) % k]
            recs[b - 1 - i] = pool[(2 * i + m + 1) % k]
    flat = recs.reshape(-1)
    flat.setflags(write=False)
    return flat


@pytest.fixture(scope="module")
def expected(secpfast, batch):
    """oracle/secp_fast.c on every record, per mode (computed once)."""
    exp = {mode: fast_batch(secpfast, batch, mode, threads=host_threads()) for mode in (0, 1)}
    for e in exp.values():
        assert 0.03 < 1 - e.mean() < 0.08
        e.setflags(write=False)
    return exp


def verify_words(torch, v, d, n, mode):
    """Enqueue one verify on the null stream into verdict words of its own; the caller synchronizes."""
    words = torch.zeros((n + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    v.verify_device(0, d.data_ptr(), n, mode, words.data_ptr(), 0)
    return words


def bits_of(words, n):
    from hkv import adversarial
    return adversarial.unpack_bits(words.cpu().numpy().view(np.uint32), n)


@pytest.fixture(scope="module")
def off_bits(torch, off, batch, n_min, expected):
    """The bitmap with parts off, per mode: one part, the oracle's verdicts."""
    assert rec_parts(off, n_min) == (pad(n_min), 1)
    d = torch.from_numpy(batch.copy()).cuda()
    out = {}
    for mode in (0, 1):
        w = verify_words(torch, off, d, n_min, mode)
        torch.cuda.synchronize()
        out[mode] = bits_of(w, n_min)
        mism = np.nonzero(out[mode] != expected[mode])[0]
        assert mism.size == 0, (mode, mism[:10])
    return out


@pytest.fixture(scope="module")
def piped(torch, lengths):
    """Contexts by part setting, opened on first use and closed at the end."""
    made = {}

    def get(which):
        if which not in made:
            made[which] = open_with_parts(lengths[which])
        return made[which]

    yield get
    for v in made.values():
        v.close()


@pytest.mark.parametrize("which", ["two", "three", "shortest"])
def test_parts_give_the_bitmap_of_the_whole_batch(torch, piped, which, lengths, batch, n_min, expected, off_bits):
    v, n, n_pad = piped(which), n_min, pad(n_min)
    part = lengths[which]
    n_parts = (n_pad + part - 1) // part
    assert n_parts == {"two": 2, "three": 3}.get(which, n_parts) and (which != "shortest" or n_parts > 200)
    assert launch_shape(v, n) == [4, 0, n_pad, 1]  # (the shape hook does not see the parts)
    assert rec_parts(v, n) == (part, n_parts)
    if which == "three":
        assert 0 < n_pad - 2 * part < part
    d = torch.from_numpy(batch.copy()).cuda()
    for mode in (0, 1):
        w = verify_words(torch, v, d, n, mode)
        torch.cuda.synchronize()
        got = bits_of(w, n)
        mism = np.nonzero(got != expected[mode])[0]
        assert mism.size == 0, (which, mode, mism[:10])
        assert (got == off_bits[mode]).all()


def test_calls_on_three_streams_each_get_their_own_verdicts(torch, piped, batch, n_min, expected):
    """Two calls back to back on two caller streams and a third on the null
    stream, each over its own batch (the same records in another order), all on
    one context: the calls share the scratch, the pipe stream and its events,
    so each bitmap is right only if every call is ordered after all of the
    call before it through the join. Then the host path on the same context
    (the context's own verdict words)."""
    v, n = piped("three"), n_min
    recs = batch.reshape(-1, 168)
    orders = [np.arange(n), np.arange(n)[::-1], np.roll(np.arange(n), 777)]
    ds = [torch.from_numpy(np.ascontiguousarray(recs[o]).reshape(-1)).cuda() for o in orders]
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), None]
    for mode in (0, 1):
        ws = [torch.zeros((n + 63) // 64 * 2, dtype=torch.int32, device="cuda") for _ in ds]
        torch.cuda.synchronize()  # (the caller streams do not wait for the stream that filled the words)
        for d, w, s in zip(ds, ws, streams):
            v.verify_device(0, d.data_ptr(), n, mode, w.data_ptr(), s.cuda_stream if s is not None else 0)
        torch.cuda.synchronize()
        for o, w in zip(orders, ws):
            mism = np.nonzero(bits_of(w, n) != expected[mode][o])[0]
            assert mism.size == 0, (mode, mism[:10])
    got = v.verify_records(recs, 1)
    assert (got == expected[1]).all()


def test_batch_one_short_of_its_padding(torch, piped, lengths, batch, n_min, expected):
    """n = n_pad - 1: the last part's last lane is padding, and the last
    verdict word is short. The records past n_min repeat the batch's first."""
    n_pad = pad(n_min)
    n = n_pad - 1
    recs = batch.reshape(-1, 168)
    idx = np.concatenate([np.arange(n_min), np.arange(n - n_min)])
    d = torch.from_numpy(np.ascontiguousarray(recs[idx]).reshape(-1)).cuda()
    for which in ("two", "shortest"):
        v = piped(which)
        assert rec_parts(v, n) == (lengths[which], (n_pad + lengths[which] - 1) // lengths[which])
        for mode in (0, 1):
            # (guard words behind the (n + 31) / 32 the call may write)
            words = torch.full(((n + 63) // 64 * 2 + 8,), -1, dtype=torch.int32, device="cuda")
            v.verify_device(0, d.data_ptr(), n, mode, words.data_ptr(), 0)
            torch.cuda.synchronize()
            host = words.cpu().numpy().view(np.uint32)
            assert (host[(n + 31) // 32:] == 0xFFFFFFFF).all()
            from hkv import adversarial
            got = adversarial.unpack_bits(host, n)
            mism = np.nonzero(got != expected[mode][idx])[0]
            assert mism.size == 0, (which, mode, mism[:10])
