"""Shared inputs and expectations of the txHash / whole-block tests
(test_txids.py, test_gpu_txids.py). Test infrastructure.

The expected txid is always the oracle composition

    txid(raw) = sighash_oracle.sha256d(tx_serialize(tx_parse(raw), with_witness=False))

(haskoin-core txHash hashes the decoded and re-serialised tx); stripped_txid
is the same hash built from a Tx object with hashlib alone, never parsed.
"""
from __future__ import annotations

import hashlib
import json
import os
import random
from typing import Dict, List, Optional, Sequence

import merkle_oracle as mo
import sighash_oracle as sh
import txgen
from conftest import GOLDEN

ZERO32 = bytes(32)


def oracle_txid(raw: bytes) -> bytes:
    return sh.sha256d(sh.tx_serialize(sh.tx_parse(raw), with_witness=False))


def stripped_txid(tx: sh.Tx) -> bytes:
    b = sh.tx_serialize(tx, with_witness=False)
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


def kats() -> List[dict]:
    return json.load(open(os.path.join(GOLDEN, "txid_kats.json")))["txs"]


def fixture_wire_blocks() -> List[bytes]:
    """The 15 bchRegTest fixture blocks of ref_blocks.bin, one wire block each
    (one coinbase tx per block, every varint a single byte)."""
    raw = open(os.path.join(GOLDEN, "ref_blocks.bin"), "rb").read()
    off, out = 0, []
    while off < len(raw):
        b0 = off
        assert raw[off + 80] == 1
        off += 81 + 4
        nin = raw[off]; off += 1
        for _ in range(nin):
            off += 36; sl = raw[off]; off += 1 + sl + 4
        nout = raw[off]; off += 1
        for _ in range(nout):
            off += 8; sl = raw[off]; off += 1 + sl
        off += 4
        out.append(raw[b0:off])
    return out


def wire_block(header: bytes, raw_txs: Sequence[bytes]) -> bytes:
    return header + sh.put_varint(len(raw_txs)) + b"".join(raw_txs)


# --- non-canonical varints -----------------------------------------------------

def put_varint_as(n: int, form: Optional[str]) -> bytes:
    """n as a varint of the given form (None: canonical; "fd" / "fe" / "ff":
    that prefix with zero high bytes)."""
    if form is None:
        return sh.put_varint(n)
    w = {"fd": 2, "fe": 4, "ff": 8}[form]
    return bytes([{"fd": 0xFD, "fe": 0xFE, "ff": 0xFF}[form]]) + n.to_bytes(w, "little")


def serialize_forms(tx: sh.Tx, forms: Dict[object, str]) -> bytes:
    """Wire form of tx (witness form when it has witness data) with chosen
    varints re-encoded. Keys: "nin", ("slen", j), "nout", ("olen", k),
    ("wcnt", j), ("wlen", j, i)."""
    seg = any(len(w) for w in tx.witness)
    out = [tx.version.to_bytes(4, "little")]
    if seg:
        out.append(b"\x00\x01")
    out.append(put_varint_as(len(tx.inputs), forms.get("nin")))
    for j, ti in enumerate(tx.inputs):
        out += [ti.outpoint(), put_varint_as(len(ti.script), forms.get(("slen", j))), ti.script,
                ti.sequence.to_bytes(4, "little")]
    out.append(put_varint_as(len(tx.outputs), forms.get("nout")))
    for k, to in enumerate(tx.outputs):
        out += [to.value.to_bytes(8, "little"), put_varint_as(len(to.script), forms.get(("olen", k))), to.script]
    if seg:
        for j in range(len(tx.inputs)):
            stack = tx.witness[j] if j < len(tx.witness) else []
            out.append(put_varint_as(len(stack), forms.get(("wcnt", j))))
            for i, item in enumerate(stack):
                out += [put_varint_as(len(item), forms.get(("wlen", j, i))), item]
    out.append(tx.locktime.to_bytes(4, "little"))
    return b"".join(out)


# --- the tx sets ------------------------------------------------------------------

def random_txs(seed: int = 100) -> List[bytes]:
    """The recipe of test_sighash_random_vs_oracle: 300 random txs, every third
    one segwit, plus one with 0xFD / 0xFE script lengths."""
    rng = random.Random(seed)
    txs = []
    for k in range(300):
        nin, nout = rng.choice([1, 1, 2, 3, 5, 17]), rng.choice([0, 1, 2, 3, 9])
        txs.append(sh.tx_serialize(txgen.rand_tx(rng, nin, nout, segwit=(k % 3 == 0))))
    txs.append(sh.tx_serialize(txgen.rand_tx(rng, 3, 3, big_scripts=True)))
    return txs


def padding_tx(s: int, witness: bool = False) -> sh.Tx:
    """1 input with an empty scriptSig, 1 output with an s-byte script: the
    stripped serialisation is 60 + s bytes."""
    rng = random.Random(1000 + s)
    tx = sh.Tx(2, [sh.TxIn(txgen.rand_script(rng, 32), 1, b"", 0xFFFFFFFE)],
               [sh.TxOut(rng.randrange(2**64), txgen.rand_script(rng, s))],
               [[b"\x01\x02"]] if witness else [], rng.randrange(2**32))
    assert len(sh.tx_serialize(tx, with_witness=False)) == 60 + s
    return tx


def merkle_header(rng: random.Random, txids: Sequence[bytes]) -> bytes:
    """80 random header bytes with the oracle's merkle root at [36,68)."""
    h = bytearray(rng.randbytes(80))
    h[36:68] = mo.merkle_root(txids)[0]
    return bytes(h)
