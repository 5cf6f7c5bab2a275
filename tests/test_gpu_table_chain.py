"""GPU tests of the table / chain launches (hkv_kernels.hip 2a: batches above
half the resident grid, per-signature tables, chunks). The batch is 64
records over half the grid (131,072 on an MI355X), n = 131,136, which pads to
one workgroup more than the mid-size path takes. Every
verdict is compared with the libsecp256k1-class host checker
(oracle/secp_fast.c) on every record, or with hkv.adversarial.mutate's
labels."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import secp256k1_oracle as o
from conftest import ROOT, fast_batch, host_threads

pytestmark = pytest.mark.gpu

N = 131_136
SEED = 0x50414952


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def ver(torch):
    import hkv
    v = hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1))  # HKV_OPEN_NO_SELFCHECK
    yield v
    v.close()


def gen_batch(torch, ver, n, seed=SEED):
    """n generated records, 5 % invalid, on the device."""
    d = torch.empty(n * 168, dtype=torch.uint8, device="cuda")
    ver.gen_batch_device(0, seed, 0, n, 65536, 100, 50, d.data_ptr(), 0)
    torch.cuda.synchronize()
    return d


def gen_valid(torch, ver, unc):
    """N valid records (hkv.adversarial.mutate's input; unc = 1000: the same
    records with 65-byte keys, mutate's y source)."""
    d = torch.empty(N * 168, dtype=torch.uint8, device="cuda")
    ver.gen_records_device(0, SEED, N, 65536, unc, d.data_ptr())
    torch.cuda.synchronize()
    return d.cpu().numpy()


def verify_bits(torch, ver, d, n, mode):
    from hkv import adversarial
    words = torch.zeros((n + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    ver.verify_device(0, d.data_ptr(), n, mode, words.data_ptr())
    torch.cuda.synchronize()
    return adversarial.unpack_bits(words.cpu().numpy().view(np.uint32), n)


@pytest.fixture(scope="module")
def batch(torch, ver):
    """The generated batch (host copy, never modified)."""
    host = gen_batch(torch, ver, N).cpu().numpy()
    host.setflags(write=False)
    return host


def test_generated_batch_both_modes(torch, ver, secpfast, batch):
    d = torch.from_numpy(batch.copy()).cuda()
    for mode in (0, 1):
        exp = fast_batch(secpfast, batch, mode, threads=host_threads())
        assert 0.04 < 1 - exp.mean() < 0.06
        got = verify_bits(torch, ver, d, N, mode)
        mism = np.nonzero(got != exp)[0]
        assert mism.size == 0, (mode, mism[:10])


def test_adversarial_batch_both_modes(torch, ver):
    """u1 = 0, zero GLV halves, ladder collisions and edge digits: windows
    with zero digits and the accumulate's H = 0 path."""
    from hkv import adversarial
    adv, lab_lib, lab_hask, cls = adversarial.mutate(gen_valid(torch, ver, 100), seed=SEED,
                                                     twin=gen_valid(torch, ver, 1000))
    d = torch.from_numpy(adv).cuda()
    for mode, lab in ((0, lab_lib), (1, lab_hask)):
        got = verify_bits(torch, ver, d, N, mode)
        mism = np.nonzero(got != lab)[0]
        assert mism.size == 0, (mode, mism[:10], [adversarial.CLASSES[c] for c in cls[mism[:10]]])


def q_scratch(v):
    """(bytes of Q-table scratch, chunk in signatures) of the context's device 0."""
    b, c = ctypes.c_size_t(), ctypes.c_size_t()
    assert v.lib.hkv_debug_q_scratch(v.ctx, 0, ctypes.byref(b), ctypes.byref(c)) == 0
    return b.value, c.value


def twist_xs(count):
    """x = 1, 2, 3, ... with x^3 + 7 a non-residue mod p, in order."""
    xs, x = [], 0
    while len(xs) < count:
        x += 1
        if pow((x * x * x + 7) % o.P, (o.P - 1) // 2, o.P) == o.P - 1:
            xs.append(x)
    return xs


def test_twist_keys_of_small_order(torch, ver, secpfast, batch):
    """Each record independently, with probability 1/4, gets a compressed key
    on a twist (x^3 + 7 a non-residue), where Q' may have small order: half of
    them x = 0 (order 3: table entries repeat, T[a] = +-lambda T[b] within a
    window), the others x = 1, 2, 3, ... over the non-residues in order.
    Every such record is rejected and every other verdict equals the
    checker's."""
    recs = batch.copy().reshape(-1, 168)
    rng = np.random.default_rng(SEED)
    hit = np.nonzero(rng.random(N) < 0.25)[0]
    zero = hit[rng.random(hit.size) < 0.5]
    other = np.setdiff1d(hit, zero)
    key = np.zeros((hit.size, 72), dtype=np.uint8)  # pklen | pubkey[65] | pad[6]
    key[:, 0], key[:, 1] = 33, 2
    recs[hit, 96:] = key
    for i, x in zip(other, twist_xs(other.size)):
        recs[i, 98:130] = np.frombuffer(int(x).to_bytes(32, "big"), dtype=np.uint8)
    assert zero.size > 10000 and other.size > 10000
    flat = recs.reshape(-1)
    d = torch.from_numpy(flat).cuda()
    for mode in (0, 1):
        exp = fast_batch(secpfast, flat, mode, threads=host_threads())
        assert not exp[hit].any()
        got = verify_bits(torch, ver, d, N, mode)
        assert not got[hit].any()
        mism = np.nonzero(got != exp)[0]
        assert mism.size == 0, (mode, mism[:10])


CHILD = """
import ctypes
import json
import sys
import numpy as np
import torch
sys.path[:0] = [{pkg!r}]
import hkv
n, seed, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
with hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1)) as v:
    b, c = ctypes.c_size_t(), ctypes.c_size_t()
    assert v.lib.hkv_debug_q_scratch(v.ctx, 0, ctypes.byref(b), ctypes.byref(c)) == 0
    before = b.value
    d = torch.empty(n * 168, dtype=torch.uint8, device="cuda")
    v.gen_batch_device(0, seed, 0, n, 65536, 100, 50, d.data_ptr(), 0)
    words = torch.zeros((n + 63) // 64 * 2, dtype=torch.int32, device="cuda")
    v.verify_device(0, d.data_ptr(), n, 0, words.data_ptr())
    torch.cuda.synchronize()
    np.save(out, words.cpu().numpy().view(np.uint32))
    assert v.lib.hkv_debug_q_scratch(v.ctx, 0, ctypes.byref(b), ctypes.byref(c)) == 0
    json.dump({{"chunk": c.value, "before": before, "after": b.value}}, open(out + ".json", "w"))
"""


def test_three_chunks_ragged_last(torch, ver, secpfast):
    """A context opened in a fresh process with HKV_REC_CHUNK=98304 verifies
    n = 262,208 in three chunks (98,304 + 98,304 + 65,792 lanes): no
    mismatch against the checker, and the bitmap of the default chunk. The
    child reports the chunk its context took and its Q-table scratch: a chunk
    under the resident grid needs no more than the grid's tables, where the
    default chunk grows the scratch to 800 B per padded signature."""
    from hkv import adversarial
    n = 262_208
    d = gen_batch(torch, ver, n, seed=SEED + 1)
    exp = fast_batch(secpfast, d.cpu().numpy(), 0, threads=host_threads())
    one = verify_bits(torch, ver, d, n, 0)
    assert (one == exp).all(), np.nonzero(one != exp)[0][:10]
    grown, chunk = q_scratch(ver)
    assert chunk == 1 << 20 and grown == 262_400 * 800
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "bits.npy")
        env = dict(os.environ, HKV_REC_CHUNK="98304")
        code = CHILD.format(pkg=os.path.join(ROOT, "haskoin-node_amd"))
        subprocess.run([sys.executable, "-c", code, str(n), str(SEED + 1), out], check=True, env=env, timeout=120)
        got = adversarial.unpack_bits(np.load(out), n)
        child = json.load(open(out + ".json"))
    assert child["chunk"] == 98304
    assert child["before"] == child["after"] == 262_144 * 768 < grown
    mism = np.nonzero(got != exp)[0]
    assert mism.size == 0, mism[:10]
    assert (got == one).all()
