"""ops.balance_knn_device (csrc/balance.hip: the balanced kNN selection as a fixed-point iteration on the device) against the
literal loop of tests/balance_cases.py and, through it, the reference's golden vectors.  Everything is integer work and a gather:
dist_new, dsi_new and l must be bit-equal, dtypes included.  The loop's result for a case is computed once and shared."""
import functools

import numpy as np
import pytest
import torch

import balance_cases as bc

pytestmark = pytest.mark.gpu

WALK = {c[0]: c for c in bc.walk_cases()}
CONSTRUCTED = {c[0]: c for c in bc.constructed_cases()}


@functools.lru_cache(maxsize=None)
def loop_result(name):
    _, dsi, dist, maxl, k, groups = (WALK.get(name) or CONSTRUCTED[name])
    return bc.reference_loop(dsi, dist, maxl, k, groups)


def on_device(dsi, dist, pitch=0):
    """The lists as the search leaves them: int32 (C, K) and fp64 (C, K) on the device; pitch > 0 pads every row of the lists."""
    dev = torch.device("cuda", 0)
    idx = torch.from_numpy(np.ascontiguousarray(dsi, dtype=np.int32)).to(dev)
    if pitch:
        wide = torch.full((idx.shape[0], idx.shape[1] + pitch), -7, dtype=torch.int32, device=dev)   # never read: -7 would be refused
        wide[:, :idx.shape[1]] = idx
        idx = wide[:, :idx.shape[1]]
    return idx, None if dist is None else torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float64)).to(dev)


def run(dsi, dist, maxl, k, groups=None, pitch=0, **kw):
    from velocyto_amd import ops
    idx, d = on_device(dsi, dist, pitch)
    stats = {}
    out = ops.balance_knn_device(idx, d, maxl, k, groups, stats=stats, **kw)
    assert all(t.is_cuda for t in out)
    return tuple(t.cpu().numpy() for t in out), stats


def assert_same(got, want):
    for g, w, name in zip(got, want, ("dist_new", "dsi_new", "l")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("with_dist", [True, False], ids=["dist", "nodist"])
@pytest.mark.parametrize("tag", ["bal", "balc", "pad", "nd"])
def test_golden_vectors(golden, tag, with_dist):
    g = golden("neighbors")
    dsi, dist, maxl, k, groups = bc.golden_case(g, tag)
    if with_dist and dist is None:
        dist = g["bal_dist"]
    if not with_dist:
        dist = None
    got, stats = run(dsi, dist, maxl, k, groups)
    assert_same(got, bc.reference_loop(dsi, dist, maxl, k, groups))
    assert not stats["fell_back"] and stats["rounds"] == {"bal": 6, "balc": 6, "pad": 5, "nd": 6}[tag]
    assert np.array_equal(got[1], g[f"{tag}_dsi_new"]) and np.array_equal(got[2], g[f"{tag}_l"])      # the selection ignores distances
    if with_dist == (tag != "nd"):                            # the way the golden was recorded: its distances too
        assert np.array_equal(got[0], g[f"{tag}_dist_new"])


@pytest.mark.parametrize("name", list(WALK))
def test_walk_chunk_edges(name):
    """K, k and n around the 64-entry chunk of the walk, maxl in {1, k, n - 1}, on lists with a padded row pitch."""
    _, dsi, dist, maxl, k, _ = WALK[name]
    n = dsi.shape[0]
    got, stats = run(dsi, dist, maxl, k, pitch=5)
    assert_same(got, loop_result(name))
    assert not stats["fell_back"]
    if maxl >= n - 1:                                         # the cap never binds: the plain first-k lists, one round and its confirmation
        assert stats["rounds"] == 2
        first = dsi[:, 1:k + 1] if dsi.shape[1] > k else np.concatenate([dsi[:, 1:], np.arange(n)[:, None]], 1)
        assert np.array_equal(got[1][:, 1:], first) and np.array_equal(got[1][:, 0], np.arange(n))


@pytest.mark.parametrize("name", list(CONSTRUCTED))
def test_constructed_lists(name):
    """The hub (descending-index tie rule), two groups, one group per cell (every row padded), a group that exhausts some rows, and the
    cell itself at position 0, 3, K - 1 or absent (the -1 of column 0); fed directly, not searched."""
    _, dsi, dist, maxl, k, groups = CONSTRUCTED[name]
    got, stats = run(dsi, dist, maxl, k, groups)
    assert_same(got, loop_result(name))
    assert not stats["fell_back"]
    n = dsi.shape[0]
    if name == "hub":
        first = [c for c in bc.processing_order(dsi) if c != 0][:maxl]
        assert sorted(np.nonzero((got[1][:, 1:] == 0).any(1))[0]) == sorted(first) and got[2][0] == maxl
    if name == "own-groups":
        assert np.array_equal(got[1][:, 1:], np.broadcast_to(np.arange(n)[:, None], (n, k))) and not got[2].any()
        assert np.array_equal(got[0][:, 1:], np.broadcast_to(dist[:, :1], (n, k)))
    if name.startswith("self-at-None"):
        assert (got[1][:, 0] == -1).all()


@pytest.mark.parametrize("n", [64, 200])
def test_chain_rounds_and_fallback(n):
    """The worst case is real: the chain takes n / 2 rounds.  Under a large cap it converges on the device in the CPU's number of
    rounds; under a small one the same lists go through the host loop and give the same arrays."""
    dsi = bc.chain(n)
    want = bc.fixed_point(dsi, None, 1, 1)
    assert want[3] == {64: 31, 200: 99}[n]
    assert_same(want[:3], bc.reference_loop(dsi, None, 1, 1))
    got, stats = run(dsi, None, 1, 1, max_rounds=256)
    assert_same(got, want[:3])
    assert stats == {"rounds": want[3], "fell_back": False}
    dist = np.tile(np.array([0.0, 0.5, 1.5]), (n, 1))
    got, stats = run(dsi, dist, 1, 1, max_rounds=8)
    assert stats == {"rounds": 8, "fell_back": True}
    assert_same(got, bc.reference_loop(dsi, dist, 1, 1))
    got2, stats = run(dsi, dist, 1, 1, max_rounds=256)
    assert not stats["fell_back"]
    assert_same(got2, got)


def test_repeatable_and_workspace_contents_do_not_matter(golden):
    from velocyto_amd import ops
    g = golden("neighbors")
    dsi, dist, maxl, k, groups = bc.golden_case(g, "balc")
    first, _ = run(dsi, dist, maxl, k, groups)
    again, _ = run(dsi, dist, maxl, k, groups)
    assert_same(again, first)
    ws = torch.full((ops.balance_workspace_bytes(dsi.shape[0], k),), 0xFF, dtype=torch.uint8, device="cuda:0")
    dirty, stats = run(dsi, dist, maxl, k, groups, workspace=ws)
    assert_same(dirty, first)
    assert stats == {"rounds": 6, "fell_back": False}
    assert_same(first, (g["balc_dist_new"], g["balc_dsi_new"], g["balc_l"]))


def test_refusals():
    """K < k, NULL pointers, sizes beyond int32 and list entries outside 0 .. n-1 are refused (the ABI's before any launch)."""
    from velocyto_amd import _lib, ops
    L = _lib.lib()
    dsi = bc.random_lists(10, 4, 1)
    with pytest.raises(AssertionError):
        run(dsi, None, 3, 5)
    bad = dsi.copy()
    bad[3, 2] = 10
    with pytest.raises(ValueError):
        run(bad, None, 3, 2)
    with pytest.raises(ValueError):
        ops.balance_knn_device(torch.zeros((4, 3), dtype=torch.int64, device="cuda:0"), None, 2, 2)
    one = 1
    assert L.vcy_balance_select(None, 4, one, None, None, None, one, one, one, 10, 4, 2, None) == -1
    assert L.vcy_balance_select(one, 4, one, None, None, None, one, one, one, 10, 4, 5, None) == -1           # K < k
    assert L.vcy_balance_select(one, 4, one, None, None, None, one, one, one, 1 << 31, 4, 2, None) == -1
    assert L.vcy_balance_select(one, 1 << 31, one, None, None, None, one, one, one, 10, 1 << 31, 2, None) == -1
    assert L.vcy_balance_select(one, 3, one, None, None, None, one, one, one, 10, 4, 2, None) == -1           # pitch below K
    assert L.vcy_balance_thresholds(None, one, one, 10, 2, 3, None) == -1
    assert L.vcy_balance_thresholds(one, one, one, 1 << 31, 2, 3, None) == -1
    assert L.vcy_balance_thresholds(one, one, one, 10, 2, 0, None) == -1
    assert L.vcy_balance_finish(one, 4, None, one, one, one, one, 10, 4, 2, None) == -1
    assert L.vcy_balance_finish(one, 4, one, one, one, one, one, 10, 4, 5, None) == -1
    assert L.vcy_balance_finish(one, 4, one, one, one, one, one, 1 << 31, 4, 2, None) == -1


def test_balanced_knn_device_equals_host(golden):
    """BalancedKNN(balance="device") against the default on the golden space (k = 9, sight 40, maxl 14, as test_oracle_golden)."""
    from velocyto_amd.neighbors import BalancedKNN
    g = golden("neighbors")
    for constraint in (None, g["groups"]):
        host = BalancedKNN(k=9, sight_k=40, maxl=14, constraint=constraint).fit(g["space"]).kneighbors()
        b = BalancedKNN(k=9, sight_k=40, maxl=14, constraint=constraint, balance="device").fit(g["space"])
        got = b.kneighbors()
        assert all(isinstance(a, np.ndarray) for a in got)
        assert_same(got, host)
        assert b.balance_stats == {"rounds": 6, "fell_back": False}
        assert np.array_equal(b.kneighbors_graph().indices, BalancedKNN(k=9, sight_k=40, maxl=14, constraint=constraint).fit(g["space"]).kneighbors_graph().indices)
    with pytest.raises(ValueError):
        BalancedKNN(balance="gpu")
