"""The Verify actor — the Python mirror of ``withVerifyActor`` in
haskell/Haskoin/Node/Verify.hs, policy for policy.

The node hands the actor the blocks and txs its peers send
(``PeerEvent (PeerMessage _ (MBlock b))`` / ``(MTx t)``, which
``Haskoin.Node.peerEvents`` drops at /root/reference/src/Haskoin/Node.hs:172);
the actor idiom is ``withChain`` (/root/reference/src/Haskoin/Node/Chain.hs:277-307):
a mailbox drained by one loop.

* **Batching.** A block is one ``verify_std_inputs`` call. Mempool txs are
  coalesced: the loop takes the first tx, then drains the mailbox until the
  batch holds ``max_inputs`` inputs (16,384 by default: the pair kernel's
  range) or ``max_wait_s`` has passed since the first tx, and
  makes ONE call for the whole batch (tx k of the batch is tx index k of the
  call). A message that does not fit (a block, or a tx past the bound) is held
  over and handled next, so the mailbox order is kept.
* **Whole txs.** ``verify_std_tx`` posts a tx with an outpoint-keyed prevout
  list (haskoin-core ``verifyStdTx``): the outpoint match, the inputs'
  verdicts and the tx verdict come from one ``verify_std_txs_detail`` call, so
  the caller numbers no inputs. It is its own call, in mailbox order; a failed
  call is re-submitted like any other, but there is no CPU fallback for it.
* **Whole blocks.** ``verify_std_block`` posts a block's raw txs with, per tx,
  the prevouts the caller's UTXO set has; inputs that spend outputs created
  earlier in the block find them on the device (``verify_block_txs_detail``,
  one call, in mailbox order, the retry policy of ``verify_std_tx``). It
  publishes ``BlockVerified`` or ``BlockRejected`` with the failing (tx, input)
  pairs; with ``skip_coinbase`` tx 0 is not judged.
* **Whole blocks with their spends.** ``check_std_block`` is
  ``verify_std_block`` with the spend stage behind the signature verdicts
  (``check_block_txs``, one call, the same retry policy): an outpoint spent
  twice within the block and a tx that pays out more than it takes in (or an
  amount beyond ``max_money``) reject the block. It publishes ``BlockVerified``
  or ``BlockSpendRejected`` with the failing inputs, the double spends and the
  unbalanced txs; ``verify_std_block`` itself looks at signatures only.
* **Errors.** A failed call (``HkvError``: HKV_E_INTERNAL when the call's
  multisig tail gave up, a device error) is re-submitted to the GPU up to
  ``retries`` times, then handed to ``fallback`` — in the Haskell actor,
  haskoin-core's own per-input ``verifyStdInput``, the CPU path the drop-in
  replaces; this package has no CPU verifier of its own, so the caller
  supplies it. With no fallback, or a fallback that raises, the batch's
  messages get ``VerifyFailed``. Nothing is raised into the loop: a verify
  failure never stops the actor (the Haskell actor runs under ``link``). A
  bug in the loop itself (e.g. ``publish`` raising) ends it; ``stop`` re-raises
  it and later posts raise at once instead of queueing unanswered.
"""
from __future__ import annotations

import queue
import threading
import time
from dataclasses import dataclass, field
from typing import Any, Callable, List, Optional, Sequence, Tuple

from .lib import HKV_SPEND_BALANCED, HKV_SPEND_COINBASE, HKV_SPEND_OK, HKV_SPEND_RESOLVED, HkvError
from .sighash import verify_std_inputs
from .blocktx import verify_block_txs_detail
from .spends import check_block_txs
from .stdtx import verify_std_txs_detail

# Outcomes published per message (VerifyEvent in the Haskell module).


@dataclass(frozen=True)
class BlockVerified:
    key: Any


@dataclass(frozen=True)
class BlockRejected:
    key: Any
    bad: Tuple[Tuple[int, int], ...]  # (tx index, input index) of each failing input


@dataclass(frozen=True)
class BlockSpendRejected:
    key: Any
    bad: Tuple[Tuple[int, int], ...]  # as BlockRejected.bad
    # (tx, input, first tx, first input): the input's outpoint was already spent by (first tx, first input)
    double_spent: Tuple[Tuple[int, int, int, int], ...]
    unbalanced: Tuple[int, ...]  # txs whose resolved inputs do not cover their outputs within max_money


@dataclass(frozen=True)
class TxVerified:
    key: Any


@dataclass(frozen=True)
class TxRejected:
    key: Any
    bad: Tuple[int, ...]  # input indices that fail verifyStdInput


@dataclass(frozen=True)
class VerifyFailed:
    key: Any
    error: str  # the GPU call failed after every retry and no fallback was given


@dataclass
class _Tx:
    key: Any
    tx: bytes
    inputs: Sequence[Tuple[int, bytes, int]]  # (input index, prevout scriptPubKey, prevout value)


@dataclass
class _Block:
    key: Any
    txs: Sequence[bytes]
    inputs: Sequence[Tuple[int, int, bytes, int]]  # (tx index, input index, prevout scriptPubKey, value)


@dataclass
class _StdTx:
    key: Any
    tx: bytes
    prevouts: Sequence[Tuple[bytes, bytes, int]]  # (36-byte wire outpoint, prevout scriptPubKey, value), any order


@dataclass
class _StdBlock:
    key: Any
    txs: Sequence[bytes]  # the block's txs in block order
    prevouts: Sequence[Sequence[Tuple[bytes, bytes, int]]]  # per tx: the prevouts the caller has (its UTXO hits)
    skip_coinbase: bool


@dataclass
class _CheckBlock:
    key: Any
    txs: Sequence[bytes]
    prevouts: Sequence[Sequence[Tuple[bytes, bytes, int]]]
    max_money: int
    skip_coinbase: bool


_STOP = object()

Fallback = Callable[[Sequence[bytes], Sequence[Tuple[int, int, bytes, int]], Optional[int]], Sequence[bool]]


@dataclass
class VerifyActorConfig:
    """VerifyConfig of the Haskell module (net -> forkid)."""
    forkid: Optional[int] = None
    max_inputs: int = 16384
    max_wait_s: float = 0.002
    retries: int = 1
    fallback: Optional[Fallback] = None


@dataclass
class ActorStats:
    gpu_calls: int = 0          # verify_std_inputs calls, retries included
    gpu_failures: int = 0       # of which raised HkvError
    fallback_calls: int = 0
    batch_inputs: List[int] = field(default_factory=list)  # inputs per successful batch, in order
    errors: List[str] = field(default_factory=list)


class VerifyActor:
    """One verifier's actor: ``verify_tx`` / ``verify_block`` post messages,
    ``publish`` receives one outcome per message, in mailbox order. ``start``
    runs the loop on a thread; ``stop`` handles every message posted before it
    and joins."""

    def __init__(self, verifier, publish: Callable[[Any], None], config: VerifyActorConfig | None = None):
        self.v = verifier
        self.publish = publish
        self.cfg = config or VerifyActorConfig()
        if self.cfg.max_inputs < 1 or self.cfg.retries < 0:
            raise ValueError("max_inputs >= 1 and retries >= 0")
        self.stats = ActorStats()
        self._q: "queue.Queue" = queue.Queue()
        self._thread: Optional[threading.Thread] = None
        self._crash: Optional[BaseException] = None

    # -- the mailbox ------------------------------------------------------------
    def verify_tx(self, key, tx: bytes, inputs: Sequence[Tuple[int, bytes, int]]) -> None:
        self._post(_Tx(key, tx, list(inputs)))

    def verify_block(self, key, txs: Sequence[bytes], inputs: Sequence[Tuple[int, int, bytes, int]]) -> None:
        self._post(_Block(key, list(txs), list(inputs)))

    def verify_std_tx(self, key, tx: bytes, prevouts: Sequence[Tuple[bytes, bytes, int]]) -> None:
        """verifyStdTx: the prevouts are matched to the tx's inputs by
        outpoint on the device; publishes TxVerified, or TxRejected with the
        inputs that fail or found no prevout (none for a tx without inputs
        or one that does not parse)."""
        self._post(_StdTx(key, tx, list(prevouts)))

    def verify_std_block(self, key, txs: Sequence[bytes], prevouts: Sequence[Sequence[Tuple[bytes, bytes, int]]],
                         skip_coinbase: bool = True) -> None:
        """verifyStdTx for every tx of a block, from the raw txs in block order
        and, per tx, the prevouts the caller's UTXO set has: an input that
        spends an output created earlier in the block finds it on the device
        (``verify_block_txs_detail``). Publishes BlockVerified, or
        BlockRejected with the (tx, input) pairs that fail or found no
        prevout; a rejected tx without a failing input (it does not parse, or
        has no inputs) is named as (tx, -1). With skip_coinbase tx 0 is not
        judged (a coinbase has no prevout and verifyStdTx rejects it)."""
        if len(prevouts) != len(txs):
            raise ValueError("one prevout list per tx")
        self._post(_StdBlock(key, list(txs), [list(p) for p in prevouts], skip_coinbase))

    def check_std_block(self, key, txs: Sequence[bytes], prevouts: Sequence[Sequence[Tuple[bytes, bytes, int]]],
                        max_money: int, skip_coinbase: bool = True) -> None:
        """verify_std_block plus the block's spends (``check_block_txs``, one
        call): publishes BlockVerified when every judged tx has its verdict
        bit and HKV_SPEND_OK (every input resolved and the first spender of
        its outpoint in the block, amounts within max_money, inputs >=
        outputs) and, with skip_coinbase, tx 0 has the coinbase form and no
        later tx has it. Otherwise BlockSpendRejected: ``bad`` as
        BlockRejected's (a tx 0 that is no coinbase, under skip_coinbase, is
        named as (0, -1)), ``double_spent`` the inputs whose outpoint an
        earlier input of the block carries, with that input, ``unbalanced``
        the txs with every input resolved that still lack HKV_SPEND_BALANCED.
        With skip_coinbase tx 0 is not judged otherwise."""
        if len(prevouts) != len(txs):
            raise ValueError("one prevout list per tx")
        self._post(_CheckBlock(key, list(txs), [list(p) for p in prevouts], int(max_money), skip_coinbase))

    def _post(self, msg) -> None:
        if self._crash is not None:
            raise RuntimeError("verify actor stopped on an error") from self._crash
        self._q.put(msg)

    def start(self) -> "VerifyActor":
        if self._thread is None:
            self._thread = threading.Thread(target=self._loop, name="hkv-verify-actor", daemon=True)
            self._thread.start()
        return self

    def stop(self, timeout: float = 600.0) -> None:
        self._q.put(_STOP)
        self.start()
        self._thread.join(timeout)
        if self._thread.is_alive():
            raise TimeoutError("verify actor did not drain its mailbox")
        if self._crash is not None:
            raise self._crash

    def __enter__(self):
        return self.start()

    def __exit__(self, *exc):
        self.stop()

    # -- the loop ---------------------------------------------------------------
    def _loop(self) -> None:
        try:
            held = None
            while True:
                msg = held if held is not None else self._q.get()
                held = None
                if msg is _STOP:
                    return
                if isinstance(msg, _Block):
                    self._handle_block(msg)
                    continue
                if isinstance(msg, _StdTx):
                    self._handle_std_tx(msg)
                    continue
                if isinstance(msg, _StdBlock):
                    self._handle_std_block(msg)
                    continue
                if isinstance(msg, _CheckBlock):
                    self._handle_check_block(msg)
                    continue
                batch, n = [msg], len(msg.inputs)
                deadline = time.monotonic() + self.cfg.max_wait_s
                while n < self.cfg.max_inputs:
                    try:
                        nxt = self._q.get(timeout=max(0.0, deadline - time.monotonic()))
                    except queue.Empty:
                        break
                    if not isinstance(nxt, _Tx) or n + len(nxt.inputs) > self.cfg.max_inputs:
                        held = nxt
                        break
                    batch.append(nxt)
                    n += len(nxt.inputs)
                self._handle_txs(batch)
        except BaseException as e:  # a bug, not a verify failure: surfaced by stop()
            self._crash = e

    def _verify(self, txs, inputs) -> Tuple[Optional[List[bool]], Optional[str]]:
        err = None
        for _ in range(1 + self.cfg.retries):
            self.stats.gpu_calls += 1
            try:
                ok = verify_std_inputs(self.v, txs, inputs, self.cfg.forkid)
                self.stats.batch_inputs.append(len(inputs))
                return ok, None
            except HkvError as e:
                self.stats.gpu_failures += 1
                err = str(e)
                self.stats.errors.append(err)
        if self.cfg.fallback is not None:
            self.stats.fallback_calls += 1
            try:
                ok = [bool(x) for x in self.cfg.fallback(txs, inputs, self.cfg.forkid)]
            except Exception as e:  # the CPU path failed too: the batch is unverified
                err = f"{err}; fallback: {e!r}"
                self.stats.errors.append(err)
                return None, err
            if len(ok) != len(inputs):
                err = f"{err}; fallback returned {len(ok)} verdicts for {len(inputs)} inputs"
                self.stats.errors.append(err)
                return None, err
            return ok, None
        return None, err

    def _handle_std_tx(self, m: _StdTx) -> None:
        err = None
        for _ in range(1 + self.cfg.retries):
            self.stats.gpu_calls += 1
            try:
                ok, per_input = verify_std_txs_detail(self.v, [m.tx], [m.prevouts], self.cfg.forkid)
            except HkvError as e:
                self.stats.gpu_failures += 1
                err = str(e)
                self.stats.errors.append(err)
                continue
            self.stats.batch_inputs.append(len(per_input[0]))
            bad = tuple(i for i, v in enumerate(per_input[0]) if not v)
            self.publish(TxVerified(m.key) if ok[0] else TxRejected(m.key, bad))
            return
        self.publish(VerifyFailed(m.key, err))

    def _handle_std_block(self, m: _StdBlock) -> None:
        err = None
        for _ in range(1 + self.cfg.retries):
            self.stats.gpu_calls += 1
            try:
                ok, per_input, _ = verify_block_txs_detail(self.v, m.txs, m.prevouts, self.cfg.forkid)
            except HkvError as e:
                self.stats.gpu_failures += 1
                err = str(e)
                self.stats.errors.append(err)
                continue
            self.stats.batch_inputs.append(sum(len(p) for p in per_input))
            bad = []
            for t in range(1 if m.skip_coinbase else 0, len(m.txs)):
                if ok[t]:
                    continue
                failing = [(t, i) for i, v in enumerate(per_input[t]) if not v]
                bad += failing or [(t, -1)]
            self.publish(BlockRejected(m.key, tuple(bad)) if bad else BlockVerified(m.key))
            return
        self.publish(VerifyFailed(m.key, err))

    def _handle_check_block(self, m: _CheckBlock) -> None:
        err = None
        for _ in range(1 + self.cfg.retries):
            self.stats.gpu_calls += 1
            try:
                ok, per_input, _, spender, _, flags = check_block_txs(self.v, m.txs, m.prevouts, self.cfg.forkid,
                                                                      m.max_money)
            except HkvError as e:
                self.stats.gpu_failures += 1
                err = str(e)
                self.stats.errors.append(err)
                continue
            self.stats.batch_inputs.append(sum(len(p) for p in per_input))
            bad, double_spent, unbalanced = [], [], []
            if m.skip_coinbase and m.txs and not flags[0] & HKV_SPEND_COINBASE:
                bad.append((0, -1))
            for t in range(1 if m.skip_coinbase else 0, len(m.txs)):
                if ok[t] and flags[t] & HKV_SPEND_OK == HKV_SPEND_OK and not (
                        m.skip_coinbase and flags[t] & HKV_SPEND_COINBASE):
                    continue
                failing = [(t, i) for i, v in enumerate(per_input[t]) if not v]
                twice = [(t, i) + first for i, first in enumerate(spender[t]) if first != (t, i)]
                short = bool(flags[t] & HKV_SPEND_RESOLVED) and not flags[t] & HKV_SPEND_BALANCED
                double_spent += twice
                if short:
                    unbalanced.append(t)
                # (a rejected tx that none of the three names: it does not parse, has no inputs,
                # or is a second coinbase)
                bad += failing or ([] if twice or short else [(t, -1)])
            if bad or double_spent or unbalanced:
                self.publish(BlockSpendRejected(m.key, tuple(bad), tuple(double_spent), tuple(unbalanced)))
            else:
                self.publish(BlockVerified(m.key))
            return
        self.publish(VerifyFailed(m.key, err))

    def _handle_block(self, m: _Block) -> None:
        ok, err = self._verify(m.txs, m.inputs) if m.inputs else ([], None)
        if ok is None:
            self.publish(VerifyFailed(m.key, err))
            return
        bad = tuple((t, i) for (t, i, _, _), v in zip(m.inputs, ok) if not v)
        self.publish(BlockRejected(m.key, bad) if bad else BlockVerified(m.key))

    def _handle_txs(self, batch: List[_Tx]) -> None:
        txs = [m.tx for m in batch]
        inputs = [(k, i, spk, val) for k, m in enumerate(batch) for (i, spk, val) in m.inputs]
        ok, err = self._verify(txs, inputs) if inputs else ([], None)
        at = 0
        for m in batch:
            if ok is None:
                self.publish(VerifyFailed(m.key, err))
                continue
            vs = ok[at: at + len(m.inputs)]
            at += len(m.inputs)
            bad = tuple(i for (i, _, _), v in zip(m.inputs, vs) if not v)
            self.publish(TxRejected(m.key, bad) if bad else TxVerified(m.key))


__all__ = ["VerifyActor", "VerifyActorConfig", "ActorStats", "BlockVerified", "BlockRejected", "BlockSpendRejected",
           "TxVerified", "TxRejected", "VerifyFailed"]
