"""The joint table build by co-Z additions (tests/coz_walk.py walk_coz: the
big-integer restatement of csrc/hkv_kernels.hip qtable_build_joint) beside the
build by mixed additions it replaces (walk_mixed): the same z-ratios, entries
and Zg mod p on 1,000 seeded random keys, keys k G, x just below p, small x
and the special pool's keys; and every entry is its orbit's multiple of Q."""
import pytest

import coz_walk as cw
import secp256k1_oracle as o
from conftest import GOLDEN

SEED = 0x434F5A


@pytest.fixture(scope="module")
def keys():
    """[(name, Q)]: Q' of the table launch for a key given by x, Q = k G itself for a scalar"""
    ks = [("x=%x" % x, cw.lane_q(x)) for x in cw.edge_xs(GOLDEN) + cw.random_xs(1000, SEED)]
    ks += [("k=%x" % k, o.point_mul(k, o.G)) for k in (1, 2, 3, o.N - 1, o.N - 2, o.LAMBDA, SEED)]
    return ks


@pytest.fixture(scope="module")
def walks(keys):
    return [(name, q, cw.walk_mixed(q), cw.walk_coz(q)) for name, q in keys]


def test_key_sets(keys):
    assert cw.P == o.P
    assert pow(cw.BETA, 3, cw.P) == 1 and cw.BETA != 1
    assert len(keys) >= 1000 + 7 + 7 + 2  # random, x edges, scalars, and keys of the pool
    assert len(cw.STEPS) == 10 and cw.STEPS[0] == (0, 0)
    assert [j for j in range(2, 11) if cw.STEPS[j - 1][0]] == [4, 7, 9]  # hkv_joint_digits.h JD_STEP_E


def test_z_ratios_agree(walks):
    for name, _, old, new in walks:
        assert sorted(new.H) == list(range(2, 11)), name
        assert old.H == new.H, name


def test_entries_agree(walks):
    for name, _, old, new in walks:
        assert old.entries == new.entries, name


def test_zg_agrees(walks):
    for name, _, old, new in walks:
        assert old.Zg == new.Zg, name


def test_qc_is_entry_0_rescaled(walks):
    for name, _, old, new in walks:
        assert new.qc == old.entries[0], name


def test_entries_are_the_orbit_multiples(walks):
    for name, q, _, new in walks:
        for j, entry in enumerate(new.entries):
            assert cw.affine(entry, new.Zg) == cw.orbit_multiple(j, q), (name, j)


def test_small_order_twist_key_is_degenerate_in_both():
    assert not cw.on_curve(cw.TWIST_X)
    q = cw.lane_q(cw.TWIST_X)
    assert q == (0, 49) and cw.aff_add(cw.aff_add(q, q), q) is None
    for walk in (cw.walk_mixed, cw.walk_coz):
        with pytest.raises(cw.Degenerate):
            walk(q)
