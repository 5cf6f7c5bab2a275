"""A Python restatement of the spend rule of hkv_block_spends_device
(include/hkv.h), on tests/blocktx_model.py's resolution (src and amount of
every input), tests/stdtx_model.py's parse and the oracle's tx codec, plus the
batches the spend tests share (test infrastructure, never the product).

Input i of tx t is g = input_first[t] + i; a tx that does not parse has none.
  spender[g]  the smallest g' with the same 36 outpoint bytes (a dict), g
              itself for the null outpoint, which is never indexed;
  per tx with inputs: the exact integer sums of the resolved amounts and of
  the outputs' amounts, each replaced by 2^64 - 1 once an amount or a running
  sum exceeds max_money, and the flag byte from them, src and spender.
"""
from __future__ import annotations

import random
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import blocktx_model as bm
import sighash_oracle as sh
import stdtx_model as model

RESOLVED, FIRST, IN_RANGE, OUT_RANGE, BALANCED, COINBASE, OK = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x1F
SUM_NONE = 2**64 - 1
EMPTY = 0xFFFFFFFF
NULL_OUTPOINT = b"\0" * 32 + b"\xff" * 4
MAX_MONEY = 2_100_000_000_000_000   # Bitcoin's maxSatoshi
Entry = model.Entry


def input_offsets(raw: bytes) -> List[int]:
    """The offset within raw of each input's outpoint, by a walk of the wire
    bytes of a tx that parses."""
    off = model.inputs_start(raw)
    out = []
    for _ in sh.tx_parse(raw).inputs:
        out.append(off)
        sl, off = sh.get_varint(raw, off + 36)
        off += sl + 4
    return out


def range_sum(amounts: Sequence[int], max_money: int) -> Tuple[int, bool]:
    """(sum, in range): the exact sum while every amount and every running sum
    is <= max_money; (2^64 - 1, False) from the first that is not."""
    total = 0
    for a in amounts:
        if a > max_money or total + a > max_money:
            return SUM_NONE, False
        total += a
    return total, True


class Spends:
    """What hkv_block_spends_device must write for a batch: first[n_tx + 1],
    and per input off (from the batch's first byte), spender, src, value; per
    tx sums[t] = (in_sum, out_sum) and flags[t]."""

    def __init__(self, raw_txs: Sequence[bytes], prevouts: Sequence[Sequence[Entry]], max_money: int):
        self.first, rows = bm.resolve(raw_txs, prevouts)
        self.src = [r[2] for r in rows]
        self.value = [r[5] for r in rows]
        self.tx_off = [0]
        for r in raw_txs:
            self.tx_off.append(self.tx_off[-1] + len(r))
        self.off: List[int] = []
        self.spender: List[int] = []
        self.outpoint: List[bytes] = []
        seen: Dict[bytes, int] = {}
        for t, raw in enumerate(raw_txs):
            if model.parse_or_none(raw) is None:
                continue
            for o in input_offsets(raw):
                g = len(self.off)
                op = raw[o:o + 36]
                self.off.append(self.tx_off[t] + o)
                self.outpoint.append(op)
                self.spender.append(g if op == NULL_OUTPOINT else seen.setdefault(op, g))
        assert len(self.off) == self.first[-1]
        self.sums: List[Tuple[int, int]] = []
        self.flags: List[int] = []
        for t, raw in enumerate(raw_txs):
            b, e = self.first[t], self.first[t + 1]
            if e == b:
                self.sums.append((0, 0))
                self.flags.append(0)
                continue
            in_sum, in_ok = range_sum(self.value[b:e], max_money)
            out_sum, out_ok = range_sum([v for (_, _, v) in bm.output_refs(raw)], max_money)
            resolved = all(s != bm.SRC_NONE for s in self.src[b:e])
            first = all(self.spender[g] == g for g in range(b, e))
            balanced = resolved and in_ok and out_ok and in_sum >= out_sum
            coinbase = e - b == 1 and self.outpoint[b] == NULL_OUTPOINT
            self.sums.append((in_sum, out_sum))
            self.flags.append((RESOLVED if resolved else 0) | (FIRST if first else 0) | (IN_RANGE if in_ok else 0) |
                              (OUT_RANGE if out_ok else 0) | (BALANCED if balanced else 0) |
                              (COINBASE if coinbase else 0))

    def pairs(self) -> List[List[Tuple[int, int]]]:
        """Per tx, (tx, input) of each input's first spender."""
        t_of = []
        for t in range(len(self.first) - 1):
            t_of += [t] * (self.first[t + 1] - self.first[t])
        flat = [(t_of[s], s - self.first[t_of[s]]) for s in self.spender]
        return [flat[self.first[t]:self.first[t + 1]] for t in range(len(self.first) - 1)]


# --- directed amounts ---------------------------------------------------------------

def _amount_tx(rng: random.Random, in_values: Sequence[int], out_values: Sequence[int]) -> Tuple[bytes, List[Entry]]:
    """A tx whose inputs are listed with in_values and whose outputs pay out_values."""
    ops = [rng.randbytes(36) for _ in in_values]
    ins = [sh.TxIn(o[:32], struct.unpack("<I", o[32:])[0], rng.randbytes(3), 0xFFFFFFFF) for o in ops]
    outs = [sh.TxOut(v, rng.randbytes(22)) for v in out_values]
    raw = sh.tx_serialize(sh.Tx(2, ins, outs, [], 0))
    return raw, [(o, b"\x51" + rng.randbytes(3), v) for o, v in zip(ops, in_values)]


def directed_amounts(max_money: int = MAX_MONEY):
    """(raw txs, prevouts, {name: (tx index, expected flags, expected sums)}):
    every edge of the two range flags and of the balance."""
    rng = random.Random(4009)
    m = max_money
    cases = [
        ("out_sum_is_max", [m], [m - 5, 5], OK, (m, m)),
        ("out_sum_is_max_plus_1", [m], [m, 1], RESOLVED | FIRST | IN_RANGE, (m, SUM_NONE)),
        ("one_output_2_64_minus_1", [m], [1, 2**64 - 1, 1], RESOLVED | FIRST | IN_RANGE, (m, SUM_NONE)),
        ("in_equals_out", [700, 300], [1000], OK, (1000, 1000)),
        ("in_is_out_minus_1", [700, 299], [1000], RESOLVED | FIRST | IN_RANGE | OUT_RANGE, (999, 1000)),
        ("no_outputs", [5], [], OK, (5, 0)),
        ("in_sum_is_max_plus_1", [m, 1], [1], RESOLVED | FIRST | OUT_RANGE, (SUM_NONE, 1)),
        ("one_input_above_max", [1, m + 1], [1], RESOLVED | FIRST | OUT_RANGE, (SUM_NONE, 1)),
        ("both_out_of_range", [2**64 - 1], [m + 1], RESOLVED | FIRST, (SUM_NONE, SUM_NONE)),
        ("wraps_if_not_sticky", [1], [2**63, 2**63, 1], RESOLVED | FIRST | IN_RANGE, (1, SUM_NONE)),
    ]
    raws, prevouts, want = [], [], {}
    for name, ins, outs, flags, sums in cases:
        raw, entries = _amount_tx(rng, ins, outs)
        want[name] = (len(raws), flags, sums)
        raws.append(raw)
        prevouts.append(entries)
    # an unresolved input: in range, covered, yet not balanced
    raw, entries = _amount_tx(rng, [10, 10], [5])
    want["unresolved"] = (len(raws), FIRST | IN_RANGE | OUT_RANGE, (10, 5))
    raws.append(raw)
    prevouts.append(entries[:1])
    return raws, prevouts, want


# --- batches of chosen outpoints ------------------------------------------------------

def outpoint_batch(seed: int, n_inputs: int, pool: Optional[Sequence[bytes]] = None):
    """(raw txs, prevouts) with exactly n_inputs inputs whose outpoints are
    drawn from a pool a fifth that size; the pool starts with the directed
    pairs: equal hash with another index, equal index with hashes that differ
    only in the last byte, equal first 8 bytes and index with other bytes
    behind them (one slot hash: a forced collision), and the null outpoint.
    Txs of 1-4 inputs (a duplicate inside one tx is common), every fifth with
    witness data; no prevout lists."""
    rng = random.Random(seed)
    if pool is None:
        h = rng.randbytes(32)
        pool = [h + struct.pack("<I", 1), h + struct.pack("<I", 2),
                h[:31] + bytes([h[31] ^ 1]) + struct.pack("<I", 1),
                h[:8] + rng.randbytes(24) + struct.pack("<I", 1), NULL_OUTPOINT]
        pool += [rng.randbytes(36) for _ in range(max(0, n_inputs // 5 - len(pool)))]
        pool = pool[:max(1, n_inputs // 5)]
    raws, left = [], n_inputs
    while left:
        k = min(left, rng.randrange(1, 5))
        ops = [rng.choice(pool) for _ in range(k)]
        if k >= 2 and rng.random() < 0.3:
            ops[1] = ops[0]     # a duplicate inside one tx
        raws.append(sh.tx_serialize(bm._tx(rng, ops, witness=rng.random() < 0.2)))
        left -= k
    return raws, [[] for _ in raws]


def walk_batch(seed: int = 77):
    """(raw txs, prevouts) for the walk: a tx of 300 inputs and 300 outputs
    (the 0xFD count form), a BIP144 tx, a tx with a non-canonical input-count
    varint, 0xFD-length scriptSigs and output scripts, and a tx that does not
    parse between parsing ones."""
    rng = random.Random(seed)
    ext = lambda: rng.randbytes(36)
    raws = [sh.tx_serialize(bm._tx(rng, [ext() for _ in range(300)], out_lens=(25,) * 300))]
    raws.append(sh.tx_serialize(bm._tx(rng, [ext(), ext()], witness=True)))
    canon = sh.tx_serialize(bm._tx(rng, [ext()], out_lens=(25, 25)))
    raws.append(canon[:4] + b"\xfd\x01\x00" + canon[5:])
    raws.append(sh.tx_serialize(bm._tx(rng, [ext(), ext()], out_lens=(300, 253, 25), sig_lens=(253, 300))))
    raws.append(sh.tx_serialize(bm._tx(rng, [ext()]))[:-1])
    raws.append(sh.tx_serialize(bm._tx(rng, [ext(), ext(), ext()], witness=True)))
    assert raws[1][4:6] == b"\x00\x01" and model.parse_or_none(raws[4]) is None
    assert all(model.parse_or_none(r) is not None for r in raws[:4] + raws[5:])
    return raws, [[] for _ in raws]


# --- a signed chain whose amounts balance --------------------------------------------------

class BalancedChain:
    """bm.SignedChain's construction behind a coinbase, with amounts a
    validator accepts: each of n txs spends 1-3 prevouts (earlier outputs of
    the chain, not listed, and listed external ones) and pays 2-3 outputs that
    sum to its inputs less a fee; tx 1 pays fee 0. spends[t][i] = (kind,
    parent tx or None), as there."""

    def __init__(self, seed: int, forkid: Optional[int], n: int = 24):
        import secp256k1_oracle as o
        import txgen
        rng = random.Random(seed)
        keys = [txgen.Key(rng.randrange(1, o.N), compressed=(k % 3 != 0)) for k in range(8)]
        ckeys = [k for k in keys if len(k.pub) == 33]
        cb = sh.Tx(1, [sh.TxIn(b"\0" * 32, 0xFFFFFFFF, b"\x03\x01\x02\x03", 0xFFFFFFFF)],
                   [sh.TxOut(50 * 10**8, sh.p2pkh_script(keys[0].h160))], [], 0)
        self.raw, self.prevouts, self.spends = [sh.tx_serialize(cb)], [[]], [[("coinbase", None)]]
        utxo = []   # (outpoint, kind, who, value, parent index)

        def fresh():
            kind = rng.choice(bm.KINDS)
            return kind, (rng.sample(keys, 3) if kind == "p2sh_ms" else rng.choice(keys if kind == "p2pkh" else ckeys))

        for _ in range(n):
            t = len(self.raw)
            picked, entries = [], []
            for _ in range(rng.choice([1, 2, 2, 3])):
                if utxo and rng.random() < 0.6:
                    picked.append(utxo.pop(rng.randrange(len(utxo))))
                else:
                    kind, who = fresh()
                    ext = (rng.randbytes(32) + struct.pack("<I", rng.randrange(4)), kind, who,
                           rng.randrange(10**6, 2**45), None)
                    picked.append(ext)
                    entries.append((ext[0], bm._spk(kind, who), ext[3]))
            total = sum(p[3] for p in picked)
            k = rng.choice([2, 3])
            rest = total - (0 if t == 1 else rng.randrange(min(total - k, 10**4)))
            parts = [rest // k] * k
            parts[0] += rest - sum(parts)
            made = [fresh() for _ in range(k)]
            outs = [sh.TxOut(v, bm._spk(kind, who)) for v, (kind, who) in zip(parts, made)]
            tx = sh.Tx(2, [sh.TxIn(p[0][:32], struct.unpack("<I", p[0][32:])[0], b"", 0xFFFFFFFF) for p in picked],
                       outs, [[] for _ in picked], rng.randrange(600000))
            for j, (_, kind, who, value, _) in enumerate(picked):
                bm._sign_input(rng, tx, j, kind, who, value, forkid)
            raw = sh.tx_serialize(tx)
            h = bm.tx_hash(raw)
            rng.shuffle(entries)
            self.raw.append(raw)
            self.prevouts.append(entries)
            self.spends.append([(p[1], p[4]) for p in picked])
            utxo += [(h + struct.pack("<I", j), kind, who, outs[j].value, t) for j, (kind, who) in enumerate(made)]


# --- the case file of tests/spends_host.cpp -------------------------------------------

def emit_cases(raw_txs: Sequence[bytes], prevouts: Sequence[Sequence[Entry]], max_money: int) -> Tuple[bytes, int]:
    """The batch and the model's answers as one little-endian blob:
      u32 n_tx | (n_tx + 1) x u32 tx offsets | the tx bytes | (n_tx + 1) x u32 input_first | u64 max_money |
      per input: u64 amount | u32 src | u32 outpoint offset | u32 spender |
      per tx: u64 in_sum | u64 out_sum | u32 flags.
    Returns (blob, inputs)."""
    s = Spends(raw_txs, prevouts, max_money)
    n = s.first[-1]
    blob = (struct.pack("<I", len(raw_txs)) + struct.pack(f"<{len(s.tx_off)}I", *s.tx_off) + b"".join(raw_txs) +
            struct.pack(f"<{len(s.first)}I", *s.first) + struct.pack("<Q", max_money) +
            b"".join(struct.pack("<QIII", s.value[g], s.src[g], s.off[g], s.spender[g]) for g in range(n)) +
            b"".join(struct.pack("<QQI", a, b, f) for (a, b), f in zip(s.sums, s.flags)))
    return blob, n
