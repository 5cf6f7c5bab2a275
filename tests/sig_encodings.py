"""The signature-encoding case table (test infrastructure, pure Python, no
randomness): every DER, hashtype and push-form branch of the input parsers
(hkv_sighash_dev.h der_read_len / der_parse_int / der_parse_sig /
decode_tx_sig / read_push and their call sites in std_parse, ms_parse and
ms_emit_lane), carried by every single-signature template and by 2-of-3
multisig in its four wraps.

cases(forkid) returns a list of Case tuples (name, tx, job, expectation, ...).
`expectation` is "accept" or "reject": whether the input's signature decode
(and so its template decode) succeeds. It is written here from the rule the
case exercises, never computed by the oracle; tests/test_sig_encodings.py
checks the oracle against it. For multisig inputs it states the decode; the
verdict comes from the oracle's countMulSig walk.

Signing uses fixed keys and four fixed nonces chosen for the length of r
(33 bytes with its 00, 32, 31 and 21 bytes), so a variant costs one modular
multiply and no point multiplication. Every value-preserving (VP) variant
re-encodes a signature that verifies in canonical form (its `twin`): a parser
site that wrongly accepts the encoding produces a true verdict the oracle
does not.

Not representable: "the needed 00 dropped" for s. A low s is below 2^255, so
its top bit is never set; the case exists for r only (nonce r33, r >= 2^255).
"""
from __future__ import annotations

import functools
import hashlib
import itertools
from typing import List, NamedTuple, Optional, Tuple

import secp256k1_oracle as o
import sighash_oracle as sh
import txgen

N = o.N
HALF_N = N // 2
MAX_CASES = 16 * 256     # alone, the table is one block-kernel batch


class Case(NamedTuple):
    name: str
    tx: sh.Tx
    job: Tuple[int, int, bytes, int]   # (0, input, prevout script, value); tx index 0 = this case's tx
    expectation: str                   # "accept" / "reject": the decode
    kind: str                          # "single" / "multisig"
    blobs: Tuple[bytes, ...]           # the non-empty signature items (DER || hashtype) the input carries
    verifies: Optional[bool]           # the verdict where the construction fixes it; None: the oracle's
    twin: Optional[str]                # VP variants: the case holding the same signature in canonical form


# --- keys and nonces -----------------------------------------------------------

def _d(tag: str) -> int:
    return int.from_bytes(hashlib.sha256(b"sig_encodings " + tag.encode()).digest(), "big") % (N - 1) + 1


@functools.lru_cache(maxsize=None)
def key(tag: str, compressed: bool = True) -> txgen.Key:
    return txgen.Key(_d("key " + tag), compressed)


# nonce -> the byte length of r's DER content
NONCES = {
    "r33": 0x7C8A8BD4CD07F0B2249746462EE0110BC62B08552392B46B29BDF828658C55EF,   # r >= 2^255: 00-led
    "r32": 0x7C8A8BD4CD07F0B2249746462EE0110BC62B08552392B46B29BDF828658C55F0,
    "r31": 0x7C8A8BD4CD07F0B2249746462EE0110BC62B08552392B46B29BDF828658C55FD,
    "r21": (N + 1) // 2,    # r = 0x3b78ce563f89a0ed9414f5aa28ad0d96d6795f9c63
}
R_LEN = {"r33": 33, "r32": 32, "r31": 31, "r21": 21}


@functools.lru_cache(maxsize=None)
def _nonce(name: str) -> Tuple[int, int]:
    k = NONCES[name]
    r = o.point_mul(k, o.G)[0] % N
    assert len(enc_int(r)) == R_LEN[name], name
    return pow(k, -1, N), r


def sign(k: txgen.Key, msg32: bytes, nonce: str = "r33") -> Tuple[int, int]:
    kinv, r = _nonce(nonce)
    s = kinv * (int.from_bytes(msg32, "big") + r * k.d) % N
    return r, (N - s if s > HALF_N else s)


# --- DER pieces ------------------------------------------------------------------

def enc_int(v: int) -> bytes:
    """The minimal content bytes of a non-negative DER INTEGER (any size)."""
    b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
    return b"\x00" + b if b[0] & 0x80 else b


def tlv(tag: int, content: bytes) -> bytes:
    assert len(content) < 128
    return bytes([tag, len(content)]) + content


def der(r: int, s: int) -> bytes:
    return tlv(0x30, tlv(2, enc_int(r)) + tlv(2, enc_int(s)))


def header_variants(r: int, s: int, ht: int) -> List[Tuple[str, bytes]]:
    """The named rejects: (name, blob) re-encodings of the canonical
    signature (r, s) with r >= 2^255, each broken in one way."""
    R, S = enc_int(r), enc_int(s)
    assert len(R) == 33 and R[0] == 0
    ri, si = tlv(2, R), tlv(2, S)
    body = ri + si
    L = len(body)
    h = bytes([ht])
    z = b"\x00"
    out = [
        ("seq_tag_31", b"\x31" + bytes([L]) + body),
        ("seq_tag_b0", b"\xb0" + bytes([L]) + body),
        ("seq_len_81_short", b"\x30\x81" + bytes([L]) + body),            # long form below 128
        ("seq_len_82_lead0", b"\x30\x82\x00" + bytes([L]) + body),        # leading zero in the length
        ("seq_len_indefinite", b"\x30\x80" + body),
        ("seq_len_indefinite_eoc", b"\x30\x80" + body + z * 2),
        ("seq_len_ff", b"\x30\xff" + body),
        ("seq_len_89_zeros", b"\x30\x89" + z * 8 + bytes([L]) + body),    # nine length bytes
        ("seq_len_89_nonzero", b"\x30\x89\x01" + z * 7 + bytes([L]) + body),
        ("seq_len_88_zeros", b"\x30\x88" + z * 7 + bytes([L]) + body),
        ("seq_len_88_huge", b"\x30\x88\x01" + z * 6 + bytes([L]) + body),  # a length past the end
        ("seq_len_84_cut", b"\x30\x84\x01"),                               # the length bytes run out
        ("seq_len_plus1", bytes([0x30, L + 1]) + body),
        ("seq_len_plus1_byte_inside", bytes([0x30, L + 1]) + body + z),    # trailing byte inside the sequence
        ("seq_len_minus1", bytes([0x30, L - 1]) + body),
        ("seq_len_minus1_cut", bytes([0x30, L - 1]) + body[:-1]),          # s runs past the end
        ("seq_trailing_after", bytes([0x30, L]) + body + z),               # trailing byte after the sequence
        ("seq_empty", b"\x30\x00"),
        ("seq_only_r", tlv(0x30, ri)),
        ("seq_three_ints", tlv(0x30, ri + si + si)),
        ("seq_r_tag_at_end", b"\x30\x01\x02"),
        ("seq_s_tag_at_end", tlv(0x30, ri + b"\x02")),
        ("seq_only_r_len_plus1", tlv(0x30, bytes([2, len(R) + 1]) + R)),   # r's value runs past the end
    ]
    # well-formed long-form lengths (sequence and integer): the parse succeeds, r overflows to 0
    big = b"\x02\x81\x82" + b"\x01" * 130 + si
    out.append(("r_130_bytes_long_form", b"\x30\x81" + bytes([len(big)]) + big))
    for nm, V, other, first in (("r", R, si, True), ("s", S, ri, False)):
        def put(x, other=other, first=first):
            return tlv(0x30, x + other if first else other + x)
        V32 = (r if first else s).to_bytes(32, "big")
        out += [
            (nm + "_tag_03", put(tlv(3, V))),
            (nm + "_len_81", put(b"\x02\x81" + bytes([len(V)]) + V)),
            (nm + "_len_0", put(b"\x02\x00")),
            (nm + "_len_plus1", put(bytes([2, len(V) + 1]) + V)),            # s: past the end; r: eats s's tag
            (nm + "_pad_00", put(tlv(2, z + V))),                              # a 00 where none is needed
            (nm + "_33_bytes_nonzero_lead", put(tlv(2, b"\x01" + V32))),
        ]
    out.append(("r_drop_00", tlv(0x30, tlv(2, R[1:]) + si)))                # the needed 00 dropped: negative
    blobs = [(nm, d + h) for nm, d in out]
    blobs += [("empty_sig", b""), ("only_hashtype", h)]
    return blobs


# --- carriers ----------------------------------------------------------------------

SINGLE_TEMPLATES = ("p2pk33", "p2pk65", "p2pkh", "p2wpkh", "p2sh_p2wpkh", "p2sh_p2pk", "p2sh_p2pkh",
                    "p2wsh_p2pk", "p2wsh_p2pkh", "p2sh_p2wsh_p2pkh")
FULL_CARRIERS = ("p2pkh", "p2wpkh")     # scriptSig carrier, witness carrier
MS_WRAPS = ("bare", "p2sh", "p2wsh", "p2sh_p2wsh")
LOCKTIME = 500000


def _h(tag: str, n: int) -> bytes:
    return hashlib.sha256(b"sig_encodings " + tag.encode()).digest()[:n]


class _Base:
    """A two-output tx skeleton around one spent input; the sighash depends
    on the locktime and the hashtype, never on the scriptSig or witness."""
    segwit = False
    code = b""
    prev = b""

    def __init__(self, tag: str, forkid: Optional[int], nin: int, nout: int, inp: int):
        self.tag, self.forkid, self.nin, self.nout, self.inp = tag, forkid, nin, nout, inp
        self.value = 1 + int.from_bytes(_h(tag + " value", 6), "big")
        self.ht = 0x41 if forkid is not None else 0x01

    def skeleton(self, locktime: int) -> sh.Tx:
        ins = [sh.TxIn(_h(f"{self.tag} in {j}", 32), j, b"", 0xFFFFFFFE) for j in range(self.nin)]
        outs = [sh.TxOut(1000 + j, sh.p2pkh_script(_h(f"{self.tag} out {j}", 20))) for j in range(self.nout)]
        return sh.Tx(2, ins, outs, [[] for _ in ins], locktime)

    def msg(self, shb: int, locktime: int = LOCKTIME) -> bytes:
        tx = self.skeleton(locktime)
        if self.segwit:
            return sh.sighash_forkid(tx, self.code, self.value, self.inp, shb, self.forkid)
        return sh.sighash_legacy(tx, self.code, self.value, self.inp, shb, self.forkid)

    def job(self):
        return (0, self.inp, self.prev, self.value)

    def grind_s(self, k: txgen.Key, nonce: str, s_len: int, shb: int) -> Tuple[int, int, int]:
        """The first locktime whose signature has an s of s_len content bytes."""
        for lt in range(LOCKTIME, LOCKTIME + 20000):
            r, s = sign(k, self.msg(shb, lt), nonce)
            if len(enc_int(s)) == s_len:
                return lt, r, s
        raise AssertionError("no locktime found")


class Single(_Base):
    def __init__(self, template: str, forkid: Optional[int], nin: int = 2, nout: int = 2, inp: int = 0,
                 tag: str = ""):
        super().__init__(f"{template}{tag} {forkid}", forkid, nin, nout, inp)
        self.template = template
        self.key = k = key("single65", False) if template == "p2pk65" else key("single")
        p2pk = txgen.push(k.pub) + b"\xac"
        p2pkh = sh.p2pkh_script(k.h160)
        self.with_pub = template not in ("p2pk33", "p2pk65", "p2sh_p2pk", "p2wsh_p2pk")
        self.inner = p2pkh if self.with_pub else p2pk
        self.segwit = "p2w" in template
        self.code = self.inner
        self.wprog = b"\x00\x20" + hashlib.sha256(self.inner).digest()
        if template in ("p2pk33", "p2pk65", "p2pkh"):
            self.prev = self.inner
        elif template == "p2wpkh":
            self.prev = sh.p2wpkh_script(k.h160)
        elif template == "p2sh_p2wpkh":
            self.prev = txgen.p2sh_script(sh.p2wpkh_script(k.h160))
        elif template in ("p2sh_p2pk", "p2sh_p2pkh"):
            self.prev = txgen.p2sh_script(self.inner)
        elif template in ("p2wsh_p2pk", "p2wsh_p2pkh"):
            self.prev = self.wprog
        else:
            assert template == "p2sh_p2wsh_p2pkh"
            self.prev = txgen.p2sh_script(self.wprog)

    def n_pushes(self) -> int:
        return {"p2pk33": 1, "p2pk65": 1, "p2pkh": 2, "p2sh_p2pk": 2, "p2sh_p2pkh": 3, "p2sh_p2wpkh": 1}.get(
            self.template, 0)

    def install(self, blob: bytes, locktime: int = LOCKTIME, forms=None, script: Optional[bytes] = None) -> sh.Tx:
        """The tx with `blob` as the signature item (forms: one push form per
        scriptSig push; script: the whole scriptSig, verbatim). An empty item
        in a scriptSig is pushed as 4c 00: a bare 00 is OP_0, not a push."""
        tx = self.skeleton(locktime)
        t, k = self.template, self.key
        stack = [blob] + ([k.pub] if self.with_pub else [])
        if t in ("p2pk33", "p2pk65", "p2pkh"):
            pushes = stack
        elif t in ("p2sh_p2pk", "p2sh_p2pkh"):
            pushes = stack + [self.inner]
        elif t == "p2sh_p2wpkh":
            pushes = [sh.p2wpkh_script(k.h160)]
        elif t == "p2sh_p2wsh_p2pkh":
            pushes = [self.wprog]
        else:
            pushes = []
        forms = list(forms) if forms is not None else [None] * len(pushes)
        assert len(forms) == len(pushes)
        if self.segwit:
            tx.witness[self.inp] = stack if "wpkh" in t else stack + [self.inner]
        elif not blob and forms[0] is None:
            forms[0] = "4c"
        ss = b"".join(txgen.push(x, f) for x, f in zip(pushes, forms))
        tx.inputs[self.inp].script = ss if script is None else script
        return tx


class Multi(_Base):
    """2-of-3 multisig: signature items in key order, signers keys 0 and 1."""

    def __init__(self, wrap: str, forkid: Optional[int], tag: str = ""):
        super().__init__(f"ms {wrap}{tag} {forkid}", forkid, 2, 2, 1)
        self.wrap = wrap
        self.keys = [key("ms0"), key("ms1", False), key("ms2")]
        self.code = txgen.multisig_script(2, [k.pub for k in self.keys])
        self.segwit = wrap in ("p2wsh", "p2sh_p2wsh")
        self.wprog = b"\x00\x20" + hashlib.sha256(self.code).digest()
        self.prev = {"bare": self.code, "p2sh": txgen.p2sh_script(self.code), "p2wsh": self.wprog,
                     "p2sh_p2wsh": txgen.p2sh_script(self.wprog)}[wrap]

    def install(self, items: List[bytes], locktime: int = LOCKTIME, forms=None, empty: bytes = b"\x00") -> sh.Tx:
        """items: signature items in order, b"" = TxSignatureEmpty (scriptSig:
        the bytes `empty`); forms: one per non-empty scriptSig push (the
        redeem push last)."""
        tx = self.skeleton(locktime)
        if self.segwit:
            tx.witness[self.inp] = [b""] + list(items) + [self.code]
            tx.inputs[self.inp].script = txgen.push(self.wprog) if self.wrap == "p2sh_p2wsh" else b""
            return tx
        pushes = [x for x in items if x] + ([self.code] if self.wrap == "p2sh" else [])
        forms = iter(forms if forms is not None else [None] * len(pushes))
        ss = b"\x00" + b"".join(txgen.push(x, next(forms)) if x else empty for x in items)
        if self.wrap == "p2sh":
            ss += txgen.push(self.code, next(forms))
        tx.inputs[self.inp].script = ss
        return tx


# --- the table -----------------------------------------------------------------------

def hashtype_ok(b: int, forkid: Optional[int]) -> bool:
    """decodeTxSig's hashtype rule: a known base type, FORKID only on a fork-id network."""
    return (b & 0x1F) in (1, 2, 3) and not (forkid is None and (b & 0x40))


def _acc(flag: bool) -> str:
    return "accept" if flag else "reject"


class _Slot:
    """One place a signature item can stand: a single-signature carrier, or
    item `pos` of a multisig carrier (the other items canonical and valid)."""

    def __init__(self, c: _Base, name: str, signer: txgen.Key, pos: Optional[int] = None):
        self.c, self.name, self.signer, self.pos = c, name, signer, pos
        self.kind = "single" if pos is None else "multisig"

    def sig(self, nonce: str = "r33", shb: Optional[int] = None, locktime: int = LOCKTIME) -> Tuple[int, int]:
        return sign(self.signer, self.c.msg(self.c.ht if shb is None else shb, locktime), nonce)

    def case(self, variant: str, blob: bytes, accept: bool, verifies: Optional[bool], twin: Optional[str] = None,
             locktime: int = LOCKTIME, **kw) -> Case:
        c = self.c
        if self.pos is None:
            tx = c.install(blob, locktime, **kw)
            blobs = (blob,) if blob else ()
        else:
            ks = c.keys
            canon = [der(*sign(ks[j], c.msg(c.ht, locktime), "r32")) + bytes([c.ht]) for j in range(2)]
            items = {0: [blob, canon[1]], 1: [canon[0], blob], 3: canon + [b"", blob]}[self.pos]
            tx = c.install(items, locktime, **kw)
            blobs = tuple(x for x in items if x)
            if not blob:            # an empty item is TxSignatureEmpty: the decode succeeds
                accept, verifies, twin = True, None, None
        return Case(f"{self.name}/{variant}", tx, c.job(), _acc(accept), self.kind, blobs,
                    verifies if accept else False, f"{self.name}/{twin}" if twin else None)


def _named(slot: _Slot) -> List[Case]:
    """Canonical shapes (accept, verify) and the named rejects."""
    c = slot.c
    h = bytes([c.ht])
    out = []
    for nonce in ("r33", "r32", "r31", "r21"):
        out.append(slot.case("canon_" + nonce, der(*slot.sig(nonce)) + h, True, True))
    for s_len in (32, 31):
        lt, r, s = c.grind_s(slot.signer, "r32", s_len, c.ht)
        out.append(slot.case(f"canon_s{s_len}", der(r, s) + h, True, True, locktime=lt))
    r, s = slot.sig("r33")
    for nm, blob in header_variants(r, s, c.ht):
        out.append(slot.case(nm, blob, False, False, twin="canon_r33"))
    # (r33's content starts 00 8x: padded once more it still overflows 32 bytes after the one 00 the
    # parser drops, whatever the padding rule; an r with the top bit clear shows the rule alone)
    r, s = slot.sig("r32")
    blob = tlv(0x30, tlv(2, b"\x00" + enc_int(r)) + tlv(2, enc_int(s))) + h
    out.append(slot.case("r32_pad_00", blob, False, False, twin="canon_r32"))
    return out


def _prefixes(slot: _Slot) -> List[Case]:
    blob = der(*slot.sig("r33")) + bytes([slot.c.ht])
    return [slot.case(f"prefix_{k}", blob[:k], False, False, twin="canon_r33") for k in range(len(blob))]


def _int_tlv(v: int) -> bytes:
    return tlv(2, enc_int(v))


def _value_sweep(slot: _Slot) -> List[Case]:
    """r and s values at every content length; the ECDSA verdict is the
    oracle's (the point is the record's r / s bytes and accept / reject)."""
    h = bytes([slot.c.ht])
    r0, s0 = slot.sig("r32")
    out = []

    def add(nm, ri, si, accept):
        out.append(slot.case(nm, tlv(0x30, ri + si) + h, accept, None))

    for k in range(1, 33):
        v = (1 << (8 * k)) - 1
        add(f"r_2p{8 * k}m1", _int_tlv(v), _int_tlv(s0), 1 <= v < N)
    for nm, v in (("1", 1), ("7f", 0x7F), ("80", 0x80), ("100", 0x100), ("2p32", 1 << 32), ("2p64m1", (1 << 64) - 1),
                  ("2p255", 1 << 255), ("n_m1", N - 1), ("0", 0), ("n", N), ("n_p1", N + 1), ("p", o.P),
                  ("2p256m1", (1 << 256) - 1), ("2p256", 1 << 256)):
        add("r_is_" + nm, _int_tlv(v), _int_tlv(s0), 1 <= v < N)
    for raw in (b"\x02\x01\x80", b"\x02\x01\xff", b"\x02\x02\xff\x80", b"\x02\x02\x00\x7f"):
        add("r_raw_" + raw.hex(), raw, _int_tlv(s0), False)
    for nm, v in (("1", 1), ("80", 0x80), ("2p32", 1 << 32), ("half_n", HALF_N), ("0", 0), ("half_n_p1", HALF_N + 1),
                  ("n_m1", N - 1), ("n", N)):
        add("s_" + nm, _int_tlv(r0), _int_tlv(v), 1 <= v <= HALF_N)
    return out


def _hashtype_sweep(slot: _Slot) -> List[Case]:
    out = []
    for b in range(256):
        ok = hashtype_ok(b, slot.c.forkid)
        out.append(slot.case(f"hashtype_{b:02x}", der(*slot.sig("r32", b)) + bytes([b]), ok, True))
    return out


FORMS = (None, "4c", "4d", "4e")


def _fname(forms) -> str:
    return "_".join(f or "min" for f in forms)


def _push_cases(forkid: Optional[int]) -> List[Case]:
    out = []
    for t in ("p2pk33", "p2pkh", "p2sh_p2pk", "p2sh_p2pkh", "p2sh_p2wpkh"):
        c = Single(t, forkid, tag=" push")
        slot = _Slot(c, "push:" + t, c.key)
        blob = der(*slot.sig("r32")) + bytes([c.ht])
        for forms in itertools.product(FORMS, repeat=c.n_pushes()):
            out.append(slot.case("forms_" + _fname(forms), blob, True, True, forms=forms))
    for t in ("p2pk33", "p2pkh", "p2sh_p2pkh"):
        c = Single(t, forkid, tag=" push")
        slot = _Slot(c, "push:" + t, c.key)
        blob = der(*slot.sig("r32")) + bytes([c.ht])
        good = c.install(blob).inputs[c.inp].script
        rest = good[1 + len(blob):]             # the pushes after the signature's
        last = c.key.pub if t == "p2pkh" else (c.inner if t == "p2sh_p2pkh" else blob)
        for nm, ss in (("end_4c", good + b"\x4c"), ("end_4d_xx", good + b"\x4d\x01"),
                       ("end_4e_xx_xx_xx", good + b"\x4e\x01\x00\x00"),
                       ("len_one_past_end", good[:len(good) - len(last) - 1] + bytes([len(last) + 1]) + last),
                       ("sig_4c_00", b"\x4c\x00" + rest), ("sig_op_0", b"\x00" + rest)):
            out.append(slot.case(nm, blob, False, False, twin="forms_" + _fname([None] * c.n_pushes()), script=ss))
    for t in ("p2wpkh", "p2wsh_p2pkh", "p2sh_p2wpkh"):
        c = Single(t, forkid, tag=" push")
        slot = _Slot(c, "push:" + t, c.key)
        out.append(slot.case("witness_sig_empty", b"", False, False))
    return out


def _single_no_output(forkid: Optional[int]) -> List[Case]:
    """SIGHASH_SINGLE on input 1 of a 2-input, 1-output tx: the legacy
    message is the integer one, the BIP143 hashOutputs is zero."""
    out = []
    for t in ("p2pkh", "p2wpkh"):
        c = Single(t, forkid, nin=2, nout=1, inp=1, tag=" single")
        slot = _Slot(c, "single_no_output:" + t, c.key)
        for b in (0x03, 0x83, 0x43, 0xC3):
            out.append(slot.case(f"hashtype_{b:02x}", der(*slot.sig("r32", b)) + bytes([b]),
                                 hashtype_ok(b, forkid), True))
    return out


def _multisig_cases(forkid: Optional[int]) -> List[Case]:
    out = []
    for wrap in MS_WRAPS:
        c = Multi(wrap, forkid)
        for pos, label in ((0, "item0"), (1, "item1"), (3, "past_n")):
            out += _named(_Slot(c, f"ms:{wrap}@{label}", c.keys[min(pos, 2)], pos))
    for wrap in ("bare", "p2wsh"):
        c = Multi(wrap, forkid, tag=" sweep")
        out += _hashtype_sweep(_Slot(c, f"ms:{wrap}@item0", c.keys[0], 0))
    for wrap in ("bare", "p2sh"):
        c = Multi(wrap, forkid, tag=" push")
        slot = _Slot(c, f"ms_push:{wrap}", c.keys[0], 0)
        blob = der(*slot.sig("r32")) + bytes([c.ht])
        for forms in itertools.product(FORMS, repeat=3 if wrap == "p2sh" else 2):
            out.append(slot.case("forms_" + _fname(forms), blob, True, True, forms=forms))
        # an empty item first (it consumes key 0), then keys 1 and 2 sign
        sigs = [der(*sign(c.keys[j], c.msg(c.ht), "r32")) + bytes([c.ht]) for j in (1, 2)]
        for nm, e in (("op_0", b"\x00"), ("4c_00", b"\x4c\x00"), ("4d_00_00", b"\x4d\x00\x00"),
                      ("4e_00_00_00_00", b"\x4e" + bytes(4))):
            out.append(Case(f"ms_push:{wrap}/empty_item_{nm}", c.install([b""] + sigs, empty=e), c.job(), "accept",
                            "multisig", tuple(sigs), True, None))
    return out


@functools.lru_cache(maxsize=None)
def cases(forkid: Optional[int] = None) -> List[Case]:
    """The whole table for one network (forkid None: no fork id). Callers
    must not change the list or its transactions."""
    out: List[Case] = []
    for t in SINGLE_TEMPLATES:
        c = Single(t, forkid)
        slot = _Slot(c, t, c.key)
        out += _named(slot)
        if t in FULL_CARRIERS:
            out += _prefixes(slot) + _value_sweep(slot)
            out += _hashtype_sweep(_Slot(Single(t, forkid, tag=" sweep"), t, c.key))
    out += _single_no_output(forkid)
    out += _push_cases(forkid)
    out += _multisig_cases(forkid)
    names = [c.name for c in out]
    assert len(set(names)) == len(names), "duplicate case names"
    assert len(out) <= MAX_CASES, len(out)
    return out


def batch(table: List[Case], base: int = 0):
    """(txs, jobs) of the table, one tx per case, tx indices from `base`."""
    return [c.tx for c in table], [(base + k, c.job[1], c.job[2], c.job[3]) for k, c in enumerate(table)]
