"""A Python restatement of haskoin-core's matchTemplate / verifyStdTx
[dep, haskoin-core-1.1.0 Haskoin.Transaction.Builder], built on the oracle's
tx codec and verifyStdInput (oracle/sighash_oracle.py), plus the generators
the verifyStdTx tests share (test infrastructure, never the product).

    verifyStdTx net ctx tx xs =
        not (null tx.inputs) && all go (zip (matchTemplate xs tx.inputs f) [0..])
      where f (_,_,o) txin = o == txin.outpoint
            go (Just (so,val,_), i) = verifyStdInput net ctx tx i so val
            go _                    = False
    matchTemplate as (b:bs) f = case break (`f` b) as of
        (l, r:rs) -> Just r  : matchTemplate (l ++ rs) bs f     -- first match, consumed
        _         -> Nothing : matchTemplate as bs f

A prevout entry is (outpoint36, scriptPubKey, value), outpoint36 being the 32
hash bytes as they appear in the tx followed by the LE32 index.
"""
from __future__ import annotations

import random
import struct
from typing import Callable, List, Optional, Sequence, Tuple

import sighash_oracle as sh

Entry = Tuple[bytes, bytes, int]
NONE = 0xFFFFFFFF


def match_template(entries: Sequence, inputs: Sequence, f: Callable) -> List[Optional[object]]:
    """matchTemplate, list for list: the first element of ``entries`` (in list
    order, not yet consumed) that ``f`` pairs with each input, or None."""
    left = list(entries)
    out = []
    for b in inputs:
        at = next((k for k, a in enumerate(left) if f(a, b)), None)   # break (`f` b) as
        if at is None:
            out.append(None)
        else:
            out.append(left[at])
            left = left[:at] + left[at + 1:]                            # l ++ rs
    return out


def parse_or_none(raw: bytes) -> Optional[sh.Tx]:
    try:
        return sh.tx_parse(raw)
    except (ValueError, IndexError):
        return None


def matched_entries(raw: bytes, entries: Sequence[Entry]) -> List[Optional[int]]:
    """Per input of the tx, the index in ``entries`` matchTemplate gives it
    (None: no entry left); [] for a tx that does not parse."""
    tx = parse_or_none(raw)
    if tx is None:
        return []
    tagged = list(enumerate(entries))
    got = match_template(tagged, tx.inputs, lambda a, txin: a[1][0] == txin.outpoint())
    return [None if g is None else g[0] for g in got]


def verify_std_tx(raw: bytes, entries: Sequence[Entry], input_ok: Callable[[sh.Tx, int, bytes, int], bool]) -> bool:
    """verifyStdTx; input_ok(tx, i, scriptPubKey, value) is verifyStdInput."""
    tx = parse_or_none(raw)
    if tx is None or not tx.inputs:
        return False
    m = matched_entries(raw, entries)
    return all(e is not None and input_ok(tx, i, entries[e][1], entries[e][2]) for i, e in enumerate(m))


def oracle_input_ok(coracle, forkid):
    """verifyStdInput by the oracle: ECDSA by the C restatement (HASKOIN mode)."""
    import secp256k1_oracle as o
    from conftest import oracle_batch
    return lambda tx, i, spk, value: sh.verify_std_input(
        tx, i, spk, value, forkid, lambda recs: oracle_batch(coracle, b"".join(recs), 1),
        lambda k: o.pubkey_parse(k) is not None)


def model_jobs(raw_txs: Sequence[bytes], prevouts: Sequence[Sequence[Entry]]):
    """What the device job builder must write: (input_first[n_tx + 1], jobs)
    with jobs = [(tx, input, scriptPubKey or None when unmatched, value)] in
    tx-major, input-minor order."""
    first, jobs = [0], []
    for t, raw in enumerate(raw_txs):
        for i, e in enumerate(matched_entries(raw, prevouts[t])):
            jobs.append((t, i, None, 0) if e is None else (t, i, prevouts[t][e][1], prevouts[t][e][2]))
        first.append(len(jobs))
    return first, jobs


# --- generators -----------------------------------------------------------------

def outpoint_pool(rng: random.Random, n: int = 3) -> List[bytes]:
    """n outpoints that differ as little as two outpoints can: the same hash
    with another index, the same index with the hash's last byte or first word
    changed — so a comparison that skips a part pairs the wrong ones."""
    h = rng.randbytes(32)
    idx = rng.randrange(4)
    pool = [h + struct.pack("<I", idx), h + struct.pack("<I", idx + 1),
            h[:31] + bytes([h[31] ^ 1]) + struct.pack("<I", idx), bytes([h[0] ^ 0x80]) + h[1:] + struct.pack("<I", idx),
            rng.randbytes(36)]
    rng.shuffle(pool)
    return pool[:n]


def dup_tx(rng: random.Random, nin: int, pool: Sequence[bytes], script_lens=(0, 1, 25, 107, 252, 253, 300)) -> sh.Tx:
    """A tx of nin inputs whose outpoints are drawn from pool (duplicates are
    common), with scriptSig lengths on both sides of the varint forms."""
    ins = []
    for _ in range(nin):
        op = rng.choice(pool)
        ins.append(sh.TxIn(op[:32], struct.unpack("<I", op[32:])[0], rng.randbytes(rng.choice(script_lens)),
                           rng.randrange(2**32)))
    outs = [sh.TxOut(rng.randrange(2**40), rng.randbytes(rng.choice([0, 22, 25]))) for _ in range(rng.randrange(1, 3))]
    return sh.Tx(rng.choice([1, 2]), ins, outs, [], rng.randrange(2**32))


def entry_list(rng: random.Random, tx: sh.Tx, pool: Sequence[bytes]) -> List[Entry]:
    """An entry per input (distinct scripts and values, so the chosen entry
    shows), shuffled, then truncated or padded with strangers and with
    surplus entries on the tx's own outpoints."""
    entries = [(ti.outpoint(), b"\x51" + struct.pack("<I", k), rng.randrange(2**50)) for k, ti in enumerate(tx.inputs)]
    rng.shuffle(entries)
    u = rng.random()
    if u < 0.3:
        entries = entries[:rng.randrange(len(entries) + 1)]
    for _ in range(rng.choice([0, 0, 1, 3])):
        entries.insert(rng.randrange(len(entries) + 1), (rng.randbytes(36), b"\x52", rng.randrange(2**50)))
    for _ in range(rng.choice([0, 0, 2])):
        entries.insert(rng.randrange(len(entries) + 1), (rng.choice(pool), b"\x53" + rng.randbytes(2), rng.randrange(2**50)))
    return entries


def inputs_start(raw: bytes) -> int:
    """Offset of the first input of a wire tx that parses."""
    off = 6 if raw[4] == 0 and raw[5] == 1 else 4
    return sh.get_varint(raw, off)[1]


def emit_match_cases(rng: random.Random, min_inputs: int) -> Tuple[bytes, int]:
    """Cases for tests/stdtx_host.cpp, as one little-endian blob:
    u32 n_cases, then per case u32 tx_len | tx | u32 ins | u32 nin |
    u32 n_entries | entries (36 bytes each) | nin x u32 expected entry
    (0xFFFFFFFF: none). Returns (blob, inputs in total)."""
    cases, total = [], 0
    while total < min_inputs:
        pool = outpoint_pool(rng)
        tx = dup_tx(rng, rng.randrange(1, 41), pool)
        raw = sh.tx_serialize(tx)
        entries = entry_list(rng, tx, pool)
        want = matched_entries(raw, entries)
        assert len(want) == len(tx.inputs)
        cases.append(struct.pack("<I", len(raw)) + raw + struct.pack("<III", inputs_start(raw), len(want), len(entries)) +
                     b"".join(e[0] for e in entries) +
                     struct.pack(f"<{len(want)}I", *[NONE if w is None else w for w in want]))
        total += len(want)
    return struct.pack("<I", len(cases)) + b"".join(cases), total
