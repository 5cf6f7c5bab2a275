"""The Verify actor's verify_std_block on the real library (MI355X): a signed
block whose txs spend each other (tests/blocktx_model.py SignedChain behind a
coinbase) gives BlockVerified; with one in-block spend broken BlockRejected
names exactly the inputs that lost their prevout; without skip_coinbase the
coinbase's input is named too."""
import pytest

import blocktx_model as bm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ver():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import hkv
    v = hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1))
    yield v
    v.close()


def test_verify_std_block_events(ver):
    from hkv.actor import BlockRejected, BlockVerified, VerifyActor, VerifyActorConfig
    c = bm.SignedChain(9300, None, n=24, coinbase=True)
    assert c.spends[0] == [("coinbase", None)]
    # the parent with the most in-block children, moved behind them: their inputs on it find nothing
    p = max(range(1, len(c.raw)), key=lambda t: len(c.children_of(t)))
    kids = c.children_of(p)
    assert kids
    order = [t for t in range(len(c.raw)) if t != p] + [p]
    lost = tuple(sorted((order.index(t), i) for t in kids for i, (_, parent) in enumerate(c.spends[t]) if parent == p))
    out = []
    with VerifyActor(ver, out.append, VerifyActorConfig(forkid=None)) as a:
        a.verify_std_block("good", c.raw, c.prevouts)
        a.verify_std_block("late parent", [c.raw[t] for t in order], [c.prevouts[t] for t in order])
        a.verify_std_block("coinbase judged", c.raw, c.prevouts, skip_coinbase=False)
        a.verify_std_block("garbage", [c.raw[0], c.raw[1][:-1]], [[], c.prevouts[1]])
    assert out == [BlockVerified("good"), BlockRejected("late parent", lost), BlockRejected("coinbase judged", ((0, 0),)),
                   BlockRejected("garbage", ((1, -1),))]
    assert a.stats.gpu_calls == 4 and a.stats.gpu_failures == 0
