"""The two numpy references of tests/balance_cases.py against the reference's golden vectors and against each other (CPU): the
literal loop reproduces tests/golden/neighbors.npz, and the fixed-point iteration reaches the loop's integers on the goldens and
on every constructed case the GPU tests use.  The new entry points' argument checks need no device either."""
import numpy as np
import pytest

import balance_cases as bc


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("tag,rounds", [("bal", 6), ("balc", 6), ("pad", 5), ("nd", 6)])
def test_references_reproduce_the_goldens(golden, tag, rounds):
    g = golden("neighbors")
    dsi, dist, maxl, k, groups = bc.golden_case(g, tag)
    loop = bc.reference_loop(dsi, dist, maxl, k, groups)
    assert np.array_equal(loop[1], g[f"{tag}_dsi_new"]) and np.array_equal(loop[2], g[f"{tag}_l"])
    assert np.array_equal(loop[0], g[f"{tag}_dist_new"])
    fp = bc.fixed_point(dsi, dist, maxl, k, groups)
    assert same(loop, fp[:3]) and fp[3] == rounds
    if tag == "pad":
        assert ((loop[1][:, 1:] == np.arange(220)[:, None]).any(1)).sum() == 184


CASES = bc.walk_cases() + bc.constructed_cases() + [(f"chain-{n}", bc.chain(n), None, 1, 1, None) for n in (64, 200)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_fixed_point_equals_the_loop(case):
    _, dsi, dist, maxl, k, groups = case
    loop = bc.reference_loop(dsi, dist, maxl, k, groups)
    fp = bc.fixed_point(dsi, dist, maxl, k, groups)
    assert same(loop, fp[:3])
    if maxl >= dsi.shape[0] - 1 and groups is None:           # the cap never binds: round 1 is final, round 2 confirms it
        assert fp[3] == 2


def test_walk_shapes_cover_the_edges():
    shapes = bc.walk_shapes()
    assert {s[0] for s in shapes} == set(bc.WALK_N) and {s[2] for s in shapes} == set(bc.WALK_K)
    for k in bc.WALK_K:
        assert {K for K in (k, k + 1, 63, 64, 65, 128, 129, 241) if K >= k} <= {s[1] for s in shapes if s[2] == k}
    assert all(K <= n for n, K, _ in shapes)


def test_chain_round_counts():
    assert bc.fixed_point(bc.chain(64), None, 1, 1)[3] == 31
    assert bc.fixed_point(bc.chain(200), None, 1, 1)[3] == 99


def test_constructed_cases_reach_their_edges():
    n, K, k = 65, 20, 9
    h = bc.hub(n, K)
    lsi = bc.processing_order(h)
    _, dsi_new, l = bc.reference_loop(h, None, 9, k)
    takers = np.nonzero((dsi_new[:, 1:] == 0).any(1))[0]
    first = [c for c in lsi if c != 0][:9]                    # the first maxl cells in lsi order other than node 0 itself
    assert l[0] == 9 and sorted(takers) == sorted(first)
    padded = lambda g: (bc.reference_loop(h, None, 9, k, g)[1][:, 1:] == np.arange(n)[:, None]).any(1)
    assert padded(bc.own_groups(n)).all() and not padded(bc.two_groups(n)).all()
    some = padded(bc.scarce_groups(n, h, k))
    assert some.any() and not some.all()
    for at, lo in ((0, 0), (3, 1), (11, 1), (None, 40)):      # the -1 of column 0: cells whose walk stops before it meets them
        col0 = bc.reference_loop(bc.random_lists(40, 12, 3, at), None, 39, 3)[1][:, 0]
        assert (col0 == -1).sum() >= lo and ((col0 == -1).sum() == 0) == (at == 0)


def test_abi_refuses_bad_arguments_before_any_launch():
    """NULL pointers, K < k, a pitch below K, n or K beyond int32 and maxl < 1: -1 and a message, without a device."""
    import velocyto_amd
    velocyto_amd.build()
    from velocyto_amd import _lib
    L = _lib.lib()
    p = 1                                                     # a non-NULL pointer that is never followed: every call below is refused first
    assert L.vcy_balance_select(None, 4, p, None, None, None, p, p, p, 10, 4, 2, None) == -1 and b"null pointer" in L.vcy_last_error()
    assert L.vcy_balance_select(p, 4, p, None, None, None, p, p, p, 10, 4, 5, None) == -1 and b"bigger than k" in L.vcy_last_error()
    assert L.vcy_balance_select(p, 3, p, None, None, None, p, p, p, 10, 4, 2, None) == -1 and b"pitch" in L.vcy_last_error()
    assert L.vcy_balance_select(p, 4, p, None, None, None, p, p, p, 1 << 31, 4, 2, None) == -1 and b"2^31" in L.vcy_last_error()
    assert L.vcy_balance_select(p, 1 << 31, p, None, None, None, p, p, p, 10, 1 << 31, 2, None) == -1
    assert L.vcy_balance_select(p, 4, p, None, None, p, p, p, p, 10, 4, 2, None) == -1          # sel and prev the same buffer
    assert L.vcy_balance_thresholds(None, p, p, 10, 2, 3, None) == -1
    assert L.vcy_balance_thresholds(p, p, p, 1 << 31, 2, 3, None) == -1
    assert L.vcy_balance_thresholds(p, p, p, 10, 2, 0, None) == -1
    assert L.vcy_balance_finish(p, 4, None, p, p, p, p, 10, 4, 2, None) == -1
    assert L.vcy_balance_finish(p, 4, p, p, p, p, p, 10, 4, 5, None) == -1
    assert L.vcy_balance_finish(p, 4, p, p, p, p, p, 1 << 31, 4, 2, None) == -1
