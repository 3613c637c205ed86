"""The numpy restatement of the adaptive-tree repulsion (tests/tsne_atree_cases.py) pinned, on the CPU, on the f64 all-pairs sum (at
angle 0 it IS that sum), on a recursive build of the same tree and - where scikit-learn imports - on the error scikit-learn's own
Barnes-Hut gradient makes at the same angle.  tests/test_gpu_tsne_atree.py holds the kernels to this restatement."""
import numpy as np
import pytest

import tsne_atree_cases as ac


def case_id(c):
    return f"{c[0]}-{c[1]}-leaf{c[2]}-d{c[3]}"


def test_keys_and_nodes_by_hand():
    """Four points on the corners of a square and one in the middle, depth 1: x in the even bit, y in the odd one, the maximum
    clamped into the last cell; the middle point (t = 1.0 exactly) falls into the upper cell of both axes.  leaf_size 1: the root
    splits into four children, the last a leaf of two points only because the depth ends there."""
    Y = np.asarray([[0, 0], [2, 0], [0, 2], [2, 2], [1, 1]], np.float32)
    t = ac.tree(Y, 1, 1)
    assert t["keys"].dtype == np.int64 and t["keys"].tolist() == [0, 1, 2, 3, 3] and t["order"].tolist() == [0, 1, 2, 3, 4]
    assert t["level"].tolist() == [0, 1, 1, 1, 1] and t["start"].tolist() == [0, 0, 1, 2, 3] and t["count"].tolist() == [5, 1, 1, 1, 2]
    assert t["skip"].tolist() == [5, 2, 3, 4, 5] and t["leaf"].tolist() == [False, True, True, True, True]
    assert np.array_equal(t["com"], np.asarray([[1, 1], [0, 0], [2, 0], [0, 2], [1.5, 1.5]], np.float32))
    o = ac.repulsion(Y, 1, 1, 1.0, t)
    # point 0: the root (w2 = 4 < d2 = 2) is opened; cells 1 and 2 (w2 = 1 < 4) and cell 3 (1 < 4.5) are accepted, its own cell is summed
    assert o["visits"].tolist()[0] == [3, 0]
    q1, q3 = 1.0 / 5.0, 1.0 / (1.0 + 4.5)
    assert abs(o["W"][0] - (2 * q1 + 2 * q3)) <= 1e-15
    # leaf_size 5: the root is a leaf, everything is summed directly; depth 2 at leaf_size 1: the two points of cell 3 part
    assert ac.tree(Y, 5, 1)["level"].tolist() == [0] and ac.repulsion(Y, 5, 1, 1.0)["visits"].tolist() == [[0, 4]] * 5
    assert ac.tree(Y, 1, 2)["level"].tolist() == [0, 1, 1, 1, 1, 2, 2]
    # 16 bits per axis cross 32 key bits
    k = ac.keys(np.asarray([[0, 0], [1, 1]], np.float32), 16)[0]
    assert k.tolist() == [0, 2 ** 32 - 1] and ac.keys(np.asarray([[0, 0], [1, 1]], np.float32), 24)[0].tolist() == [0, 2 ** 48 - 1]


@pytest.mark.parametrize("c", ac.distinct_cases(), ids=case_id)
def test_numbering_by_flags_and_scan_is_the_recursive_build(c):
    kind, N, ls, D = c
    _, t, _ = ac.case(kind, N, ls, D, 0.5)
    sk = t["keys"][t["order"]]
    r = ac.build_recursive(sk, ls, D)
    assert all(np.array_equal(t[f], r[f]) for f in r)
    nn = len(t["level"])
    assert 1 <= nn <= ac.node_bound(N, ls, D)
    # the definition, node by node
    assert t["level"][0] == 0 and t["count"][0] == N and t["skip"][0] == nn
    assert np.array_equal(t["leaf"], (t["count"] <= ls) | (t["level"] == D))
    assert t["count"][t["leaf"]].sum() == N                              # the leaves partition the points
    ch = t["children"]
    has = ch >= 0
    assert np.array_equal(has.any(1), ~t["leaf"])
    par = np.repeat(np.arange(nn), has.sum(1))
    kid = ch[has]
    assert np.array_equal(np.sort(kid), np.arange(1, nn))                # every node but the root is one node's child
    assert np.all(t["level"][kid] == t["level"][par] + 1)
    assert np.array_equal(np.bincount(par, weights=t["count"][kid], minlength=nn)[~t["leaf"]], t["count"][~t["leaf"]])


def test_depth_follows_the_density():
    """The table of DESIGN.md section 9: 15 levels (what int32 keys hold) leave clumps whole, 24 resolve them to the cap, or to what
    float32 positions resolve."""
    for kind, at15, at24 in (("clumps3", 178, 8), ("clusters", 158, 8), ("clumps5", 250, 26)):
        Y = ac.points(kind, 3000)
        for D, want in ((15, at15), (24, at24)):
            t = ac.tree(Y, 8, D)
            assert int(t["count"][t["leaf"]].max()) == want, (kind, D)
    Y = ac.embedding("coincident", 100)
    t = ac.tree(Y, 8, 24)                                                # a chain of 24 internal nodes and one leaf of all points
    assert t["level"].tolist() == list(range(25)) and np.all(t["count"] == 100) and t["leaf"].tolist() == [False] * 24 + [True]
    t = ac.tree(ac.embedding("duplicates", 64), 1, 24)                   # exact copies part only at the depth's end
    assert int(t["count"][t["leaf"]].max()) == 2 and np.all(t["level"][t["count"] == 2][t["leaf"][t["count"] == 2]] == 24)


@pytest.mark.parametrize("c", [c for c in ac.distinct_cases() if c[1] <= 3000], ids=case_id)
def test_angle_zero_is_the_exact_sum_and_the_error_grows_with_the_angle(c):
    kind, N, ls, D = c
    ex = ac.exact_case(kind, N)
    err = {}
    for angle in (0.0, 0.2, 0.5, 0.8):
        Y, t, o = ac.case(kind, N, ls, D, angle)
        err[angle] = ac.rel_error(o, ex)
        if angle == 0.0:                                   # the same pairs, summed in another order: equal to rounding
            assert not o["visits"][:, 0].any() and np.all(o["visits"][:, 1] == N - 1)
            assert np.all(np.abs(o["rep"] - ex["rep"]) <= 1e-12 * ex["A"])
            assert np.all(np.abs(o["W"] - ex["W"]) <= 1e-12 * ex["W"]) and abs(o["Z"] - ex["Z"]) <= 1e-12 * ex["Z"]
    assert err[0.0] <= 1e-13
    assert err[0.0] <= err[0.2] + 1e-13 and err[0.2] <= err[0.5] + 1e-13 and err[0.5] <= err[0.8] + 1e-13, err


@pytest.mark.parametrize("N,ls,D", [(N, ls, d) for N, ls, d in ac.COINCIDENT if N <= 1000])
def test_coincident_points(N, ls, D):
    ls = ac.leaf_of(N, ls)
    Y = ac.embedding("coincident", N)
    t = ac.tree(Y, ls, D)
    chain = 1 if N <= ls else D + 1
    assert t["side"] == 0.0 and not t["keys"].any() and t["level"].tolist() == list(range(chain)) and np.all(t["count"] == N)
    for angle in (0.0, 1.0):
        o = ac.repulsion(Y, ls, D, angle, t)
        assert not o["rep"].any() and o["Z"] == N * (N - 1.0) and not o["visits"][:, 0].any() and np.all(o["visits"][:, 1] == N - 1)


def test_error_against_scikit_learns_own():
    bh = pytest.importorskip("sklearn.manifold._barnes_hut_tsne")
    N = ac.PIN_N
    worst = {}
    for kind in ac.PIN_KINDS:
        Y = ac.embedding(kind, N, 0)
        ex = ac.exact_repulsion(Y)
        ge = ex["rep"] / ex["Z"]
        for angle in ac.PIN_ANGLES:
            forces = np.zeros((N, 2), np.float32)
            bh.gradient(np.zeros(0, np.float32), Y, np.zeros(0, np.int64), np.zeros(N + 1, np.int64), forces, angle, 2, 0, dof=1.0,
                        compute_error=False, num_threads=1)
            e_sk = float(np.linalg.norm(-forces.astype(np.float64) - ge) / np.linalg.norm(ge))
            assert e_sk > 0
            for ls in ac.PIN_LEAVES:
                e = ac.rel_error(ac.repulsion(Y, ls, ac.MAX_DEPTH, angle), ex)
                worst[kind] = max(worst.get(kind, 0.0), e / e_sk)
                assert e <= (ac.RATIO_MAX + ac.RATIO_MARGIN) * e_sk, (kind, angle, ls, e, e_sk)
    print("\nlargest error ratio to scikit-learn's, per embedding:", {k: round(v, 3) for k, v in worst.items()},
          "recorded for seed 0:", {k: v[0] for k, v in ac.RATIO_MEASURED.items()})
