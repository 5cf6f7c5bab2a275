"""CPU checks of the signature-encoding case table (tests/sig_encodings.py):
the oracle agrees with the table's hand-written accept / reject column, the
strict decode accepts exactly the canonical encodings (an oracle-independent
property, also over 200,000 seeded byte mutations), the table runs every line
of the oracle's DER, hashtype and push readers (the device functions mirror
them line for line, so it reaches every device branch), and every signature
the value-preserving variants re-encode verifies in canonical form under two
independent ECDSA checkers."""
import collections
import dis
import random
import sys

import pytest

import secp256k1_oracle as o
import sighash_oracle as sh
import sig_encodings as se
import txgen
from conftest import openssl_batch, oracle_batch

FORKIDS = [None, 0]
# the column's totals: (cases, decode accepts) per network
TOTALS = {None: (2517, 474), 0: (2517, 526)}


def _decodes(c, forkid):
    _, i, prev, value = c.job
    if c.kind == "single":
        return sh.std_input(c.tx, i, prev, value, forkid).ok
    return sh.std_multisig(c.tx, i, prev, value, forkid) is not None


@pytest.mark.parametrize("forkid", FORKIDS)
def test_oracle_matches_expectation_column(forkid):
    """Every case, none skipped: the oracle's decode equals the column."""
    table = se.cases(forkid)
    got = [_decodes(c, forkid) for c in table]
    bad = [(c.name, c.expectation) for c, g in zip(table, got) if g != (c.expectation == "accept")]
    assert not bad, bad[:10]
    col = collections.Counter(c.expectation for c in table)
    assert (sum(got), len(got) - sum(got)) == (col["accept"], col["reject"])
    assert (len(table), col["accept"]) == TOTALS[forkid]
    assert set(col) == {"accept", "reject"}


@pytest.mark.parametrize("forkid", FORKIDS)
def test_table_shape(forkid):
    """The size bound and the sets each carrier holds."""
    table = se.cases(forkid)
    assert len(table) <= se.MAX_CASES == 4096
    by = {c.name: c for c in table}
    assert len(by) == len(table)
    named = {c.name.split("/")[1] for c in table if c.name.startswith("p2pk33/")}
    assert len(named) == 46 and {"canon_r33", "canon_r32", "canon_r31", "canon_r21", "canon_s32", "canon_s31",
                                 "empty_sig", "only_hashtype", "r_drop_00"} <= named
    slots = list(se.SINGLE_TEMPLATES) + [f"ms:{w}@{p}" for w in se.MS_WRAPS for p in ("item0", "item1", "past_n")]
    for slot in slots:
        assert named <= {c.name.split("/")[1] for c in table if c.name.startswith(slot + "/")}, slot
    for t in se.FULL_CARRIERS:
        mine = [c.name.split("/")[1] for c in table if c.name.startswith(t + "/")]
        n_blob = len(by[t + "/canon_r33"].blobs[0])
        assert sum(v.startswith("prefix_") for v in mine) == n_blob      # every proper prefix
        assert sum(v.startswith("hashtype_") for v in mine) == 256
        assert sum(v.startswith("r_2p") for v in mine) == 32
    for slot in ("ms:bare@item0", "ms:p2wsh@item0"):
        assert sum(c.name.startswith(slot + "/hashtype_") for c in table) == 256
    assert sum(c.name.startswith("push:") and "/forms_" in c.name for c in table) == 104
    # the lengths the canonical shapes are named for
    for slot in slots:
        pos = {"item0": 0, "item1": 1, "past_n": 3}.get(slot.split("@")[-1], 0)
        for nm, r_len, s_len in (("canon_r33", 33, None), ("canon_r32", 32, None), ("canon_r31", 31, None),
                                 ("canon_r21", 21, None), ("canon_s32", None, 32), ("canon_s31", None, 31)):
            blob = by[f"{slot}/{nm}"].blobs[pos if pos < 3 else 2]
            r, s = sh.sig_parse_der(blob[:-1])
            assert blob[:-1] == sh.der_encode(r, s)
            assert r_len is None or blob[3] == r_len
            assert s_len is None or blob[5 + blob[3]] == s_len
    # a VP variant's twin is a case that accepts and verifies
    twins = {c.twin for c in table if c.twin}
    assert twins and all(by[t].expectation == "accept" and by[t].verifies is True for t in twins)
    assert all(c.expectation == "reject" for c in table if c.twin)
    assert se.NONCES["r21"] == (o.N + 1) // 2
    assert se._nonce("r21")[1] == 0x3B78CE563F89A0ED9414F5AA28AD0D96D6795F9C63


def _canonical_pair(b: bytes):
    """(r, s) iff b is 30 L 02 lr R 02 ls S with 1 <= r < n, 1 <= s <= n/2 and
    b is der_encode(r, s): plain slicing, no part of the oracle's DER reader."""
    if len(b) < 8 or b[0] != 0x30 or b[1] != len(b) - 2 or b[2] != 2:
        return None
    lr = b[3]
    if 6 + lr > len(b) or b[4 + lr] != 2 or 6 + lr + b[5 + lr] != len(b):
        return None
    r, s = int.from_bytes(b[4:4 + lr], "big"), int.from_bytes(b[6 + lr:], "big")
    if not (1 <= r < o.N and 1 <= s <= o.N // 2):
        return None
    return (r, s) if sh.der_encode(r, s) == b else None


def test_strict_decode_accepts_exactly_canonical_table():
    n_blobs = n_ok = 0
    for forkid in FORKIDS:
        for c in se.cases(forkid):
            for blob in c.blobs:
                n_blobs += 1
                got = sh.decode_strict_sig(blob[:-1])
                assert got == _canonical_pair(blob[:-1]), (c.name, blob.hex())
                n_ok += got is not None
    assert n_blobs > 4000 and 0 < n_ok < n_blobs


def test_strict_decode_accepts_exactly_canonical_mutations():
    """200,000 seeded mutations (replace / insert / delete up to three
    bytes) of canonical encodings: accepted iff canonical."""
    rng = random.Random(0x44455253)
    bases = []
    for _ in range(64):
        r = rng.choice([rng.randrange(1, o.N), rng.randrange(1, 1 << rng.randrange(1, 256))])
        s = rng.choice([rng.randrange(1, o.N // 2 + 1), rng.randrange(1, 1 << rng.randrange(1, 255))])
        bases.append(sh.der_encode(r, s))
    accepted = 0
    for _ in range(200000):
        b = bytearray(rng.choice(bases))
        for _ in range(rng.randrange(1, 4)):
            pos = rng.randrange(len(b))
            kind = rng.randrange(4)
            if kind == 0:
                b.insert(pos, rng.choice([0, 0xFF, 0x80, 2, rng.randrange(256)]))
            elif kind == 1 and len(b) > 1:
                del b[pos]
            else:
                b[pos] = rng.choice([b[pos] ^ (1 << rng.randrange(8)), rng.randrange(256)])
        b = bytes(b)
        got = sh.decode_strict_sig(b)
        assert got == _canonical_pair(b), b.hex()
        accepted += got is not None
    assert 20000 < accepted < 180000     # both sides of the property are exercised


COVERED = ("_der_len", "_der_int", "sig_parse_der", "decode_strict_sig", "decode_tx_sig", "_push_items")


def test_table_runs_every_line_of_the_oracle_readers():
    codes = {getattr(sh, f).__code__: f for f in COVERED}
    want = {(f, ln) for code, f in codes.items() for _, ln in dis.findlinestarts(code) if ln is not None}
    seen = set()

    def local(frame, event, arg):
        seen.add((codes[frame.f_code], frame.f_lineno))
        return local

    def tracer(frame, event, arg):
        if frame.f_code in codes:
            seen.add((codes[frame.f_code], frame.f_lineno))
            return local
        return None

    old = sys.gettrace()
    sys.settrace(tracer)
    try:
        for forkid in FORKIDS:
            for c in se.cases(forkid):
                _decodes(c, forkid)
    finally:
        sys.settrace(old)
    assert len(want) > 80
    missing = sorted(want - seen)
    assert not missing, missing


@pytest.mark.parametrize("forkid", FORKIDS)
def test_valid_bases_and_fixed_verdicts(coracle, openssl, forkid):
    """Every canonical twin (and every case built to verify) verifies under
    the C oracle and under OpenSSL; every reject is false; the multisig
    cases built to verify do so under the oracle's countMulSig walk."""
    from test_sighash_oracle import multisig_verdicts
    table = se.cases(forkid)
    singles = [c for c in table if c.kind == "single"]
    recs = b"".join(sh.std_input_record(c.tx, c.job[1], c.job[2], c.job[3], forkid) for c in singles)
    for name, got in (("C oracle", oracle_batch(coracle, recs, 1)), ("OpenSSL", openssl_batch(openssl, recs, 1))):
        bad = [c.name for c, g in zip(singles, got) if c.verifies is not None and bool(g) != c.verifies]
        assert not bad, (name, bad[:10])
    multi = [c for c in table if c.kind == "multisig"]
    got = multisig_verdicts(coracle, [c.tx for c in multi], [(k,) + c.job[1:] for k, c in enumerate(multi)], forkid)
    bad = [c.name for c, g in zip(multi, got) if c.verifies is not None and g != c.verifies]
    assert not bad, bad[:10]
    assert sum(c.verifies is True for c in table) > 350 and sum(c.verifies is None for c in table) < 120


def test_push_default_is_unchanged():
    """txgen.push without a form: byte-identical to the minimal push it
    always made, lengths 0..600; the forms carry the same data."""
    def minimal(data):
        n = len(data)
        if n <= 75:
            return bytes([n]) + data
        if n <= 255:
            return b"\x4c" + bytes([n]) + data
        return b"\x4d" + n.to_bytes(2, "little") + data
    for n in range(601):
        data = bytes((7 * k + n) & 0xFF for k in range(n))
        assert txgen.push(data) == txgen.push(data, None) == minimal(data)
        forms = ["4d", "4e"] + (["4c"] if n <= 255 else [])
        for f in forms:
            enc = txgen.push(data, f)
            assert sh._push_items(enc) == [data] and enc[0] == int(f, 16)
            assert len(enc) == len(data) + {"4c": 2, "4d": 3, "4e": 5}[f]
