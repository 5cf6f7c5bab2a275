"""GPU test of the launch shapes' edges (haskoin-node_amd/csrc/hkv_launch_plan.h,
the switch of the launch wrappers at the end of hkv_kernels.hip): a record
batch on each side of every threshold of an MI355X (256 CUs, a resident grid
of 262,144 lanes) — 4,096 | 4,097 the block and the pair kernel (the latter
padded to 4,352), 32,768 | 32,769 the pair kernel and the mid-size instance,
131,072 | 131,073 the mid-size instance at its full grid of 512 blocks and the
table / chain launches. The library reports that shape for the batch
(hkv_debug_launch_shape), and in both modes every verdict equals the
libsecp256k1-class host checker's (oracle/secp_fast.c) on every record."""
import numpy as np
import pytest

import launch_shapes
from conftest import fast_batch, host_threads
from test_gpu_table_chain import gen_batch, verify_bits
from test_gpu_table_chain import torch, ver  # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu

SEED = 0x45444745

# n -> (shape, padded length)
EDGES = {
    4_096: (launch_shapes.BLOCK, 4_096),
    4_097: (launch_shapes.PAIR, 4_352),
    32_768: (launch_shapes.PAIR, 32_768),
    32_769: (launch_shapes.MID, 33_024),
    131_072: (launch_shapes.MID, 131_072),
    131_073: (launch_shapes.TABLE_CHAIN, 131_328),
}


@pytest.mark.parametrize("n", sorted(EDGES))
def test_batch_on_each_side_of_every_edge(torch, ver, secpfast, n):  # noqa: F811
    shape, n_pad = EDGES[n]
    assert launch_shapes.records(ver, n) == (shape, 0, n_pad, 1)
    d = gen_batch(torch, ver, n, seed=SEED + n)
    host = d.cpu().numpy()
    for mode in (0, 1):
        exp = fast_batch(secpfast, host, mode, threads=host_threads())
        assert 0.04 < 1 - exp.mean() < 0.06
        got = verify_bits(torch, ver, d, n, mode)
        mism = np.nonzero(got != exp)[0]
        assert mism.size == 0, (mode, mism[:10])
