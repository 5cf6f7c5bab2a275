"""A Python restatement of the in-batch prevout rule of hkv_verify_block_txs*
(include/hkv.h), on tests/stdtx_model.py's matchTemplate and the oracle's tx
codec, plus the generator of chained batches the block-tx tests share (test
infrastructure, never the product).

For input i of a tx t that parses, whose outpoint is (h, k) as wire bytes:
  1. the list first: tx t's own prevout list by matchTemplate
     (stdtx_model.matched_entries); a hit gives the entry, src = SRC_LIST;
  2. otherwise the batch: p = the smallest u such that tx u parses and
     txHash(tx u) == h, txHash = sha256d(tx_serialize(tx, with_witness=False));
     the input resolves only if p exists, p < t and k < len(tx p's outputs),
     and takes output k of tx p; src = p;
  3. otherwise nothing: src = SRC_NONE.
"""
from __future__ import annotations

import random
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import sighash_oracle as sh
import stdtx_model as model

SRC_NONE, SRC_LIST = 0xFFFFFFFF, 0xFFFFFFFE
Entry = model.Entry


def tx_hash(raw: bytes) -> Optional[bytes]:
    """haskoin-core txHash in digest order, None for a tx that does not parse."""
    tx = model.parse_or_none(raw)
    return None if tx is None else sh.sha256d(sh.tx_serialize(tx, with_witness=False))


def tx_ids(raw_txs: Sequence[bytes]) -> List[bytes]:
    """What hkv_tx_ids writes: 32 zero bytes for a tx that does not parse."""
    return [tx_hash(r) or b"\0" * 32 for r in raw_txs]


def first_index(raw_txs: Sequence[bytes]) -> Dict[bytes, int]:
    """txid -> the smallest index of a parsing tx with it."""
    out: Dict[bytes, int] = {}
    for u, r in enumerate(raw_txs):
        h = tx_hash(r)
        if h is not None and h not in out:
            out[h] = u
    return out


def output_refs(raw: bytes) -> List[Tuple[int, int, int]]:
    """(script offset within raw, script length, value) of each output of a
    wire tx that parses, by a walk of the wire bytes (non-canonical varints
    keep their width)."""
    off = model.inputs_start(raw)
    for _ in sh.tx_parse(raw).inputs:
        sl, off = sh.get_varint(raw, off + 36)
        off += sl + 4
    nout, off = sh.get_varint(raw, off)
    refs = []
    for _ in range(nout):
        value = int.from_bytes(raw[off:off + 8], "little")
        sl, off = sh.get_varint(raw, off + 8)
        refs.append((off, sl, value))
        off += sl
    return refs


def in_batch(raw_txs: Sequence[bytes], index: Dict[bytes, int], t: int, outpoint: bytes):
    """Step 2 alone: (p, k, script offset within tx p, script length, value) or None."""
    p = index.get(outpoint[:32])
    k = struct.unpack("<I", outpoint[32:])[0]
    if p is None or p >= t:
        return None
    refs = output_refs(raw_txs[p])
    if k >= len(refs):
        return None
    return (p, k) + refs[k]


def resolve(raw_txs: Sequence[bytes], prevouts: Sequence[Sequence[Entry]]):
    """What the block job builder must write: (input_first[n_tx + 1], rows) in
    tx-major, input-minor order, a row being
      (t, i, SRC_LIST, entry index, scriptPubKey, value)              step 1
      (t, i, p, (k, offset within tx p, length), scriptPubKey, value)  step 2
      (t, i, SRC_NONE, None, None, 0)                                  step 3."""
    index = first_index(raw_txs)
    first, rows = [0], []
    for t, raw in enumerate(raw_txs):
        tx = model.parse_or_none(raw)
        for i, e in enumerate(model.matched_entries(raw, prevouts[t])):
            if e is not None:
                rows.append((t, i, SRC_LIST, e, prevouts[t][e][1], prevouts[t][e][2]))
                continue
            hit = in_batch(raw_txs, index, t, tx.inputs[i].outpoint())
            if hit is None:
                rows.append((t, i, SRC_NONE, None, None, 0))
            else:
                p, k, off, ln, value = hit
                rows.append((t, i, p, (k, off, ln), raw_txs[p][off:off + ln], value))
        first.append(len(rows))
    return first, rows


def augmented(raw_txs: Sequence[bytes], prevouts: Sequence[Sequence[Entry]]) -> List[List[Entry]]:
    """P': every tx's list with the in-batch prevouts the model resolved
    appended, so that verifyStdTx on (B, P') is the block call on (B, P)."""
    out = [list(p) for p in prevouts]
    _, rows = resolve(raw_txs, prevouts)
    txs = [model.parse_or_none(r) for r in raw_txs]
    for (t, i, src, _, spk, value) in rows:
        if src not in (SRC_LIST, SRC_NONE):
            out[t].append((txs[t].inputs[i].outpoint(), spk, value))
    return out


def verify_block_txs(raw_txs: Sequence[bytes], prevouts: Sequence[Sequence[Entry]], input_ok_of) -> List[bool]:
    """The block call's tx verdicts; input_ok_of(raw) gives verifyStdInput for
    the inputs of that tx (stdtx_model.verify_std_tx's input_ok)."""
    aug = augmented(raw_txs, prevouts)
    return [model.verify_std_tx(r, p, input_ok_of(r)) for r, p in zip(raw_txs, aug)]


# --- the generator of chained batches ------------------------------------------------

def _tx(rng: random.Random, outpoints: Sequence[bytes], out_lens=(25, 22), witness: bool = False,
        sig_lens=(0, 1, 25, 107)) -> sh.Tx:
    ins = [sh.TxIn(o[:32], struct.unpack("<I", o[32:])[0], rng.randbytes(rng.choice(sig_lens)), rng.randrange(2**32))
           for o in outpoints]
    outs = [sh.TxOut(rng.randrange(1, 2**50), rng.randbytes(n)) for n in out_lens]
    wit = [[rng.randbytes(rng.choice([1, 33, 72]))] for _ in ins] if witness else []
    return sh.Tx(rng.choice([1, 2]), ins, outs, wit, rng.randrange(2**32))


def _op(h: bytes, k: int) -> bytes:
    return h + struct.pack("<I", k & 0xFFFFFFFF)


def _entry(rng: random.Random, outpoint: bytes) -> Entry:
    return (outpoint, b"\x51" + rng.randbytes(rng.choice([3, 24])), rng.randrange(2**50))


class Chain:
    """A batch under construction: raw txs in order, their lists, and the named
    inputs (variant -> (tx, input)) a test asserts the model's answer for."""

    def __init__(self, rng: random.Random):
        self.rng = rng
        self.raw: List[bytes] = []
        self.prevouts: List[List[Entry]] = []
        self.named: Dict[str, Tuple[int, int]] = {}
        self.spendable: List[bytes] = []   # outpoints of parsing txs already in the batch

    def add(self, raw: bytes, entries: Sequence[Entry] = ()) -> int:
        self.raw.append(raw)
        self.prevouts.append(list(entries))
        h = tx_hash(raw)
        if h is not None:
            self.spendable += [_op(h, k) for k in range(len(sh.tx_parse(raw).outputs))]
        return len(self.raw) - 1

    def name(self, variant: str, t: int, i: int) -> None:
        self.named[variant] = (t, i)


def chained_batch(seed: int, n_fill: int = 200) -> Chain:
    """Every variant of the rule once, by name, then n_fill random txs that
    spend earlier outputs of the batch, listed outpoints and strangers."""
    rng = random.Random(seed)
    c = Chain(rng)
    ext = lambda: rng.randbytes(36)

    # a plain parent; its child spends outputs 0 and 2 and the zero-length script of output 1
    plain = sh.tx_serialize(_tx(rng, [ext()], out_lens=(25, 0, 22)))
    hp = tx_hash(plain)
    c.add(plain)
    t = c.add(sh.tx_serialize(_tx(rng, [_op(hp, 0), _op(hp, 2), _op(hp, 1)])))
    c.name("plain_parent", t, 0)
    c.name("zero_length_parent_script", t, 2)
    # output index equal to the count, one past it, 0xFFFFFFFF
    t = c.add(sh.tx_serialize(_tx(rng, [_op(hp, 3), _op(hp, 4), _op(hp, 0xFFFFFFFF), _op(hp, 2)])))
    c.name("index_equals_count", t, 0)
    c.name("index_past_count", t, 1)
    c.name("index_ffffffff", t, 2)
    # a BIP144 parent: named by the hash of its stripped form
    seg = _tx(rng, [ext(), ext()], witness=True)
    raw_seg = sh.tx_serialize(seg)
    assert raw_seg[4:6] == b"\x00\x01" and tx_hash(raw_seg) != sh.sha256d(raw_seg)
    c.add(raw_seg)
    t = c.add(sh.tx_serialize(_tx(rng, [_op(tx_hash(raw_seg), 1), _op(sh.sha256d(raw_seg), 1)], witness=True)))
    c.name("bip144_parent", t, 0)
    c.name("bip144_wire_hash", t, 1)
    # a parent with a non-canonical input count (fd 01 00): txHash re-serialises it
    canon = sh.tx_serialize(_tx(rng, [ext()], out_lens=(25, 25)))
    wide = canon[:4] + b"\xfd\x01\x00" + canon[5:]
    assert tx_hash(wide) == sh.sha256d(canon) != sh.sha256d(wide)
    c.add(wide)
    t = c.add(sh.tx_serialize(_tx(rng, [_op(tx_hash(wide), 1), _op(sh.sha256d(wide), 1)])))
    c.name("noncanonical_parent_txhash", t, 0)
    c.name("noncanonical_parent_wire_hash", t, 1)
    # a parent with 0xFD-form scriptSig and output script lengths
    big = sh.tx_serialize(_tx(rng, [ext(), ext()], out_lens=(300, 253, 25), sig_lens=(253, 300)))
    c.add(big)
    t = c.add(sh.tx_serialize(_tx(rng, [_op(tx_hash(big), 2), _op(tx_hash(big), 1)])))
    c.name("fd_form_parent", t, 0)
    # a forward reference: the child stands in front of its parent
    later = sh.tx_serialize(_tx(rng, [ext()]))
    t = c.add(sh.tx_serialize(_tx(rng, [_op(tx_hash(later), 0)])))
    c.add(later)
    c.name("forward_reference", t, 0)
    # a parent that does not parse (its last byte cut), named by the hash it would have had
    whole = sh.tx_serialize(_tx(rng, [ext()]))
    c.add(whole[:-1])
    t = c.add(sh.tx_serialize(_tx(rng, [_op(tx_hash(whole), 0), _op(b"\0" * 32, 0xFFFFFFFF), _op(b"\0" * 32, 0)])))
    c.name("unparsable_parent", t, 0)
    c.name("coinbase_form", t, 1)
    # duplicate parents: a child between and one after them both take the first
    dup = sh.tx_serialize(_tx(rng, [ext()]))
    a = c.add(dup)
    t = c.add(sh.tx_serialize(_tx(rng, [_op(tx_hash(dup), 1)])))
    c.name("duplicate_parents_between", t, 0)
    c.add(dup)
    t = c.add(sh.tx_serialize(_tx(rng, [_op(tx_hash(dup), 0)])))
    c.name("duplicate_parents_after", t, 0)
    c.dup_first = a
    # a list entry takes precedence over the in-batch parent
    op = _op(hp, 0)
    t = c.add(sh.tx_serialize(_tx(rng, [op])), [_entry(rng, ext()), _entry(rng, op)])
    c.name("list_precedence", t, 0)
    # two inputs on one in-batch outpoint, one list entry: the first takes the entry, the second the batch
    t = c.add(sh.tx_serialize(_tx(rng, [ext(), op, op])), [_entry(rng, op)])
    c.name("shared_outpoint_list", t, 1)
    c.name("shared_outpoint_batch", t, 2)
    # fill: 1-4 inputs each on an earlier output (sometimes listed too), a listed outpoint or a stranger
    for _ in range(n_fill):
        ops, entries = [], []
        for _ in range(rng.randrange(1, 5)):
            u = rng.random()
            o = rng.choice(c.spendable) if u < 0.6 else ext()
            ops.append(o)
            if u < 0.1 or 0.6 <= u < 0.85:
                entries.append(_entry(rng, o))
        rng.shuffle(entries)
        kind = rng.random()
        raw = sh.tx_serialize(_tx(rng, ops, out_lens=tuple(rng.choice([0, 22, 25, 34]) for _ in range(rng.randrange(1, 4))),
                                  witness=kind < 0.3))
        if kind > 0.95:
            raw = raw[:-1]
        c.add(raw, entries)
    return c


def emit_cases(c: Chain, n_near: int = 64) -> Tuple[bytes, int]:
    """The batch for tests/blocktx_host.cpp as one little-endian blob:
      u32 n_tx | (n_tx + 1) x u32 tx offsets | the tx bytes | n_tx x 32 txid bytes |
      n_tx x u32 input count (0: the tx does not parse) |
      per input, tx-major: u32 src | u32 script offset in the batch | u32 script length | u64 value
        (step 2 alone, whatever the tx's list holds; SRC_NONE rows are all zero behind src) |
      u32 n_q | n_q x (32 query bytes | u32 the smallest index, or 0xFFFFFFFF).
    Returns (blob, inputs)."""
    rng = random.Random(len(c.raw))
    index = first_index(c.raw)
    ids = tx_ids(c.raw)
    offs = [0]
    for r in c.raw:
        offs.append(offs[-1] + len(r))
    counts, rows = [], []
    for t, raw in enumerate(c.raw):
        tx = model.parse_or_none(raw)
        counts.append(0 if tx is None else len(tx.inputs))
        for ti in (tx.inputs if tx else []):
            hit = in_batch(c.raw, index, t, ti.outpoint())
            if hit is None:
                rows.append(struct.pack("<IIIQ", SRC_NONE, 0, 0, 0))
            else:
                p, _, off, ln, value = hit
                rows.append(struct.pack("<IIIQ", p, offs[p] + off, ln, value))
    queries = [(h, index.get(h, SRC_NONE) if any(h) else SRC_NONE) for h in ids]
    for _ in range(n_near):
        h = rng.choice([x for x in ids if any(x)])
        for q in (h[:31] + bytes([h[31] ^ 1]), bytes([h[0] ^ 0x80]) + h[1:], rng.randbytes(32)):
            queries.append((q, index.get(q, SRC_NONE)))
    blob = (struct.pack("<I", len(c.raw)) + struct.pack(f"<{len(offs)}I", *offs) + b"".join(c.raw) + b"".join(ids) +
            struct.pack(f"<{len(counts)}I", *counts) + b"".join(rows) + struct.pack("<I", len(queries)) +
            b"".join(q + struct.pack("<I", want) for q, want in queries))
    return blob, len(rows)


# --- a signed chain ------------------------------------------------------------------

KINDS = ("p2pkh", "p2wpkh", "p2sh_p2wpkh", "p2sh_ms")


def _spk(kind: str, who) -> bytes:
    import txgen
    if kind == "p2pkh":
        return sh.p2pkh_script(who.h160)
    if kind == "p2wpkh":
        return sh.p2wpkh_script(who.h160)
    if kind == "p2sh_p2wpkh":
        return txgen.p2sh_script(sh.p2wpkh_script(who.h160))
    return txgen.p2sh_script(txgen.multisig_script(2, [k.pub for k in who]))


def _sign_input(rng: random.Random, tx: sh.Tx, j: int, kind: str, who, value: int, forkid: Optional[int]) -> None:
    import secp256k1_oracle as o
    import txgen
    shb = 0x41 if forkid is not None else 0x01

    def sig(msg, key):
        r, s = txgen.sign(msg, key.d, rng.randrange(1, o.N))
        return sh.der_encode(r, s) + bytes([shb])

    if kind == "p2pkh":
        m = sh.sighash_legacy(tx, sh.p2pkh_script(who.h160), value, j, shb, forkid)
        tx.inputs[j].script = txgen.push(sig(m, who)) + txgen.push(who.pub)
    elif kind in ("p2wpkh", "p2sh_p2wpkh"):
        m = sh.sighash_forkid(tx, sh.p2pkh_script(who.h160), value, j, shb, forkid)
        tx.witness[j] = [sig(m, who), who.pub]
        if kind == "p2sh_p2wpkh":
            tx.inputs[j].script = txgen.push(sh.p2wpkh_script(who.h160))
    else:
        redeem = txgen.multisig_script(2, [k.pub for k in who])
        m = sh.sighash_legacy(tx, redeem, value, j, shb, forkid)
        tx.inputs[j].script = b"\x00" + txgen.push(sig(m, who[0])) + txgen.push(sig(m, who[2])) + txgen.push(redeem)


class SignedChain:
    """n txs built in order, so parents are final before children sign: each
    spends 1-3 prevouts, a mix of earlier outputs of the chain (not listed:
    the batch must find them) and external prevouts (listed), and pays 2-3
    outputs of the four kinds. spends[t][i] = (kind, parent tx or None)."""

    def __init__(self, seed: int, forkid: Optional[int], n: int = 48, coinbase: bool = False):
        import secp256k1_oracle as o
        import txgen
        rng = random.Random(seed)
        self.forkid = forkid
        keys = [txgen.Key(rng.randrange(1, o.N), compressed=(k % 3 != 0)) for k in range(8)]
        ckeys = [k for k in keys if len(k.pub) == 33]   # (witness programs take compressed keys)
        self.raw, self.prevouts, self.spends = [], [], []
        if coinbase:
            cb = sh.Tx(1, [sh.TxIn(b"\0" * 32, 0xFFFFFFFF, b"\x03\x01\x02\x03", 0xFFFFFFFF)],
                       [sh.TxOut(50 * 10**8, sh.p2pkh_script(keys[0].h160))], [], 0)
            self.raw.append(sh.tx_serialize(cb))
            self.prevouts.append([])
            self.spends.append([("coinbase", None)])
        utxo = []   # (outpoint, kind, who, value, parent index)

        def fresh():
            kind = rng.choice(KINDS)
            who = rng.sample(keys, 3) if kind == "p2sh_ms" else rng.choice(keys if kind == "p2pkh" else ckeys)
            return kind, who

        for _ in range(n):
            t = len(self.raw)
            picked, entries = [], []
            for _ in range(rng.choice([1, 2, 2, 3])):
                if utxo and rng.random() < 0.6:
                    picked.append(utxo.pop(rng.randrange(len(utxo))))
                else:
                    kind, who = fresh()
                    ext = (rng.randbytes(32) + struct.pack("<I", rng.randrange(4)), kind, who, rng.randrange(1, 2**45), None)
                    picked.append(ext)
                    entries.append((ext[0], _spk(kind, who), ext[3]))
            outs, made = [], []
            for _ in range(rng.choice([2, 3])):
                kind, who = fresh()
                outs.append(sh.TxOut(rng.randrange(1, 2**40), _spk(kind, who)))
                made.append((kind, who))
            tx = sh.Tx(2, [sh.TxIn(p[0][:32], struct.unpack("<I", p[0][32:])[0], b"", 0xFFFFFFFF) for p in picked],
                       outs, [[] for _ in picked], rng.randrange(600000))
            for j, (_, kind, who, value, _) in enumerate(picked):
                _sign_input(rng, tx, j, kind, who, value, forkid)
            raw = sh.tx_serialize(tx)
            h = tx_hash(raw)
            rng.shuffle(entries)
            self.raw.append(raw)
            self.prevouts.append(entries)
            self.spends.append([(p[1], p[4]) for p in picked])
            utxo += [(h + struct.pack("<I", k), kind, who, outs[k].value, t) for k, (kind, who) in enumerate(made)]

    def children_of(self, p: int) -> List[int]:
        return [t for t, s in enumerate(self.spends) if any(parent == p for _, parent in s)]
