"""CPU tests of the Verify actor's verify_std_tx mailbox method (whole txs with
outpoint-keyed prevouts, haskoin-core verifyStdTx): the GPU call is a stub, so
what is checked is the actor's own part — the events it publishes from the tx
bit and the per-input bits, mailbox order beside the other messages, and the
retry policy."""
import hkv.actor as actor
from hkv.actor import TxRejected, TxVerified, VerifyActor, VerifyActorConfig, VerifyFailed
from hkv.lib import HkvError


class StubStdTx:
    """verify_std_txs_detail stand-in: the tx's first byte is its input count,
    the following bytes its per-input verdicts; fails the calls in `fail`."""

    def __init__(self, fail=()):
        self.calls, self.fail = [], set(fail)

    def __call__(self, v, txs, prevouts, forkid):
        self.calls.append((len(txs), [len(p) for p in prevouts], forkid))
        if len(self.calls) in self.fail:
            raise HkvError(-5, "hkv_verify_std_txs_device")
        per = [[bool(b) for b in tx[1:1 + tx[0]]] for tx in txs]
        return [bool(p) and all(p) for p in per], per


def run(monkeypatch, posts, cfg=None, fail=()):
    stub = StubStdTx(fail)
    monkeypatch.setattr(actor, "verify_std_txs_detail", stub)
    monkeypatch.setattr(actor, "verify_std_inputs", lambda v, txs, ins, forkid: [True] * len(ins))
    out = []
    a = VerifyActor(None, out.append, cfg or VerifyActorConfig(forkid=0, max_wait_s=0.0))
    for p in posts:
        p(a)
    a.start()
    a.stop()
    return a, stub, out


def test_events_from_the_tx_bit_and_the_input_bits(monkeypatch):
    entry = (b"\x11" * 36, b"\x51", 7)
    posts = [lambda a: a.verify_std_tx("ok", bytes([2, 1, 1]), [entry, entry]),
             lambda a: a.verify_std_tx("bad1", bytes([3, 1, 0, 1]), [entry]),
             lambda a: a.verify_std_tx("noinputs", bytes([0]), [entry]),
             lambda a: a.verify_std_tx("bad02", bytes([3, 0, 1, 0]), [])]
    a, stub, out = run(monkeypatch, posts)
    assert out == [TxVerified("ok"), TxRejected("bad1", (1,)), TxRejected("noinputs", ()), TxRejected("bad02", (0, 2))]
    assert stub.calls == [(1, [2], 0), (1, [1], 0), (1, [1], 0), (1, [0], 0)]   # one call per tx, the config's forkid
    assert a.stats.gpu_calls == 4 and a.stats.batch_inputs == [2, 3, 0, 3]


def test_mailbox_order_beside_other_messages(monkeypatch):
    posts = [lambda a: a.verify_tx("t0", b"\x01", [(0, b"\x51", 1)]),
             lambda a: a.verify_std_tx("s0", bytes([1, 1]), []),
             lambda a: a.verify_tx("t1", b"\x02", [(0, b"\x51", 1)]),
             lambda a: a.verify_block("b0", [b"\x03"], [(0, 0, b"\x51", 1)]),
             lambda a: a.verify_std_tx("s1", bytes([1, 0]), [])]
    _, _, out = run(monkeypatch, posts, VerifyActorConfig(max_wait_s=0.5))
    assert [e.key for e in out] == ["t0", "s0", "t1", "b0", "s1"]
    assert isinstance(out[1], TxVerified) and out[4] == TxRejected("s1", (0,))


def test_failed_call_is_resubmitted_then_reported(monkeypatch):
    posts = [lambda a: a.verify_std_tx("s0", bytes([1, 1]), []), lambda a: a.verify_std_tx("s1", bytes([1, 1]), [])]
    a, stub, out = run(monkeypatch, posts, VerifyActorConfig(retries=1, max_wait_s=0.0), fail={1, 3, 4})
    assert out[0] == TxVerified("s0")                      # call 1 failed, call 2 answered
    assert isinstance(out[1], VerifyFailed) and out[1].key == "s1" and "HKV_E_INTERNAL" in out[1].error
    assert a.stats.gpu_calls == 4 and a.stats.gpu_failures == 3
    # the actor keeps running after the failure
    assert a._crash is None
