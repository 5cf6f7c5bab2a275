"""The Verify actor's check_std_block on the real library (MI355X): a signed,
balanced block behind a coinbase gives BlockVerified; the same block with one
tx replayed gives BlockSpendRejected naming the copy's inputs and their first
spenders; with one output amount raised above the tx's inputs it names the tx
as unbalanced. verify_std_block on the same three blocks still publishes what
it does today: it accepts the replay."""
import pytest

import blocktx_model as bm
import sighash_oracle as sh
import spends_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ver():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import hkv
    v = hkv.Verifier(hkv.VerifierConfig(device_ids=[0], flags=1))
    yield v
    v.close()


def test_check_std_block_events(ver):
    from hkv.actor import BlockRejected, BlockSpendRejected, BlockVerified, VerifyActor, VerifyActorConfig
    c = sm.BalancedChain(9400, None, n=24)
    good = sm.Spends(c.raw, c.prevouts, sm.MAX_MONEY)
    assert good.flags[0] & sm.COINBASE and all(f == sm.OK for f in good.flags[1:])
    assert good.sums[1][0] == good.sums[1][1] and all(a > b for a, b in good.sums[2:])   # fee 0 once, then fees
    assert any(parent is not None for s in c.spends for _, parent in s)
    # one tx replayed at the end of the block
    u = next(t for t in range(1, len(c.raw)) if len(c.spends[t]) >= 2)
    replay = (c.raw + [c.raw[u]], c.prevouts + [c.prevouts[u]])
    copy = len(c.raw)
    twice = tuple((copy, i, u, i) for i in range(len(c.spends[u])))
    # the last tx (no children in the block) with its first output raised above its inputs: its
    # signatures no longer verify either
    last = len(c.raw) - 1
    tx = sh.tx_parse(c.raw[last])
    tx.outputs[0].value = good.sums[last][0] + 1
    raised = (c.raw[:last] + [sh.tx_serialize(tx)], c.prevouts)
    assert not sm.Spends(*raised, sm.MAX_MONEY).flags[last] & sm.BALANCED
    lost = tuple((last, i) for i in range(len(c.spends[last])))
    out = []
    with VerifyActor(ver, out.append, VerifyActorConfig(forkid=None)) as a:
        a.check_std_block("good", c.raw, c.prevouts, sm.MAX_MONEY)
        a.check_std_block("replay", *replay, sm.MAX_MONEY)
        a.check_std_block("raised", *raised, sm.MAX_MONEY)
        a.check_std_block("small money", c.raw, c.prevouts, 1000)
        a.verify_std_block("good", c.raw, c.prevouts)
        a.verify_std_block("replay", *replay)
        a.verify_std_block("raised", *raised)
    assert out[:3] == [BlockVerified("good"), BlockSpendRejected("replay", (), twice, ()),
                       BlockSpendRejected("raised", lost, (), (last,))]
    # every external prevout is worth at least 10^6: with max_money 1000 every tx is out of range
    assert out[3] == BlockSpendRejected("small money", (), (), tuple(range(1, len(c.raw))))
    assert out[4:] == [BlockVerified("good"), BlockVerified("replay"), BlockRejected("raised", lost)]
    assert a.stats.gpu_calls == 7 and a.stats.gpu_failures == 0
