"""The numpy restatement of the tree repulsion (tests/tsne_tree_cases.py) pinned, on the CPU, on the f64 all-pairs sum (at angle 0 it
IS that sum) and - where scikit-learn imports - on the error scikit-learn's own Barnes-Hut gradient makes at the same angle.
tests/test_gpu_tsne_tree.py holds the kernels to this restatement."""
import numpy as np
import pytest

import tsne_tree_cases as tc


def case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}"


def test_automatic_depth():
    assert [tc.auto_depth(N) for N in (2, 4, 5, 16, 17, 4096, 4097, 10 ** 6, 4 ** 11, 4 ** 11 + 1, 2 ** 29)] == [1, 1, 1, 1, 2, 5, 6, 9, 10, 11, 11]


def test_keys_and_pyramid_by_hand():
    """Four points on the corners of a square and one in the middle, depth 1: x in the even bit, y in the odd one, the maximum
    clamped into the last cell; the middle point (t = 1.0 exactly) falls into the upper cell of both axes."""
    Y = np.asarray([[0, 0], [2, 0], [0, 2], [2, 2], [1, 1]], np.float32)
    p = tc.pyramid(Y, 1)
    assert p["keys"].tolist() == [0, 1, 2, 3, 3] and p["order"].tolist() == [0, 1, 2, 3, 4] and p["start"].tolist() == [0, 1, 2, 3, 5]
    assert p["count"][1].tolist() == [1, 1, 1, 2] and p["count"][0].tolist() == [5]
    assert np.array_equal(p["com"][1], np.asarray([[0, 0], [2, 0], [0, 2], [1.5, 1.5]], np.float32))
    assert np.array_equal(p["com"][0], np.asarray([[1, 1]], np.float32))
    o = tc.tree_repulsion(Y, 1, 1.0, p)
    # point 0: the root (w2 = 4 < d2 = 2) is opened; cells 1 and 2 (w2 = 1 < 4) and cell 3 (1 < 4.5) are accepted, its own cell is summed
    assert o["visits"].tolist()[0] == [3, 0]
    q1, q3 = 1.0 / 5.0, 1.0 / (1.0 + 4.5)
    assert abs(o["W"][0] - (2 * q1 + 2 * q3)) <= 1e-15


@pytest.mark.parametrize("c", tc.distinct_cases(), ids=case_id)
def test_angle_zero_is_the_exact_sum_and_the_error_grows_with_the_angle(c):
    kind, N, L = c
    ex = tc.exact_case(kind, N)
    err = {}
    for angle in (0.0, 0.2, 0.5, 0.8):
        Y, _, pyr, o = tc.case(kind, N, L, angle)
        err[angle] = tc.rel_error(o, ex)
        assert np.all(o["visits"].sum(1) >= 0)
        if angle == 0.0:                                   # the same pairs, summed in another order: equal to rounding
            assert not o["visits"][:, 0].any() and np.all(o["visits"][:, 1] == N - 1)
            assert np.all(np.abs(o["rep"] - ex["rep"]) <= 1e-12 * ex["A"])
            assert np.all(np.abs(o["W"] - ex["W"]) <= 1e-12 * ex["W"]) and abs(o["Z"] - ex["Z"]) <= 1e-12 * ex["Z"]
    assert err[0.0] <= 1e-13
    assert err[0.0] <= err[0.2] + 1e-13 and err[0.2] <= err[0.5] + 1e-13 and err[0.5] <= err[0.8] + 1e-13, err


@pytest.mark.parametrize("N,depth", [(N, d) for N, d in tc.COINCIDENT if N <= 1000])
def test_coincident_points(N, depth):
    L = tc.auto_depth(N) if depth is None else depth
    Y = tc.embedding("coincident", N)
    p = tc.pyramid(Y, L)
    assert p["side"] == 0.0 and not p["keys"].any() and all(int(p["count"][l][0]) == N for l in range(L + 1))
    for angle in (0.0, 1.0):
        o = tc.tree_repulsion(Y, L, angle, p)
        assert not o["rep"].any() and o["Z"] == N * (N - 1.0) and not o["visits"][:, 0].any() and np.all(o["visits"][:, 1] == N - 1)


def test_error_against_scikit_learns_own():
    bh = pytest.importorskip("sklearn.manifold._barnes_hut_tsne")
    N, L0 = tc.PIN_N, tc.auto_depth(tc.PIN_N)
    worst = {}
    for kind in tc.PIN_KINDS:
        Y = tc.embedding(kind, N, 0)
        ex = tc.exact_repulsion(Y)
        ge = ex["rep"] / ex["Z"]
        for angle in tc.PIN_ANGLES:
            forces = np.zeros((N, 2), np.float32)
            bh.gradient(np.zeros(0, np.float32), Y, np.zeros(0, np.int64), np.zeros(N + 1, np.int64), forces, angle, 2, 0, dof=1.0,
                        compute_error=False, num_threads=1)
            e_sk = float(np.linalg.norm(-forces.astype(np.float64) - ge) / np.linalg.norm(ge))
            assert e_sk > 0
            for L in (L0 - 1, L0, L0 + 1):
                e = tc.rel_error(tc.tree_repulsion(Y, L, angle), ex)
                worst[kind] = max(worst.get(kind, 0.0), e / e_sk)
                assert e <= (tc.RATIO_MAX + tc.RATIO_MARGIN) * e_sk, (kind, angle, L, e, e_sk)
    print("\nlargest error ratio to scikit-learn's, per embedding:", {k: round(v, 3) for k, v in worst.items()},
          "recorded for seed 0:", {k: v[0] for k, v in tc.RATIO_MEASURED.items()})
