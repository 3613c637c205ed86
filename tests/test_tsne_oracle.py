"""The f64 t-SNE oracle (oracle/oracle.py: tsne_binary_search_perplexity, tsne_joint_p, tsne_objective, tsne_step) pinned on
closed forms, which need nothing but numpy, and - where scikit-learn imports - on scikit-learn's own private functions, the code
the device t-SNE restates.  No GPU: tests/test_gpu_tsne_kernels.py holds the kernels to this oracle."""
import inspect

import numpy as np
import pytest
from scipy import sparse
from scipy.spatial.distance import squareform


def degenerate_rows(k):
    """The rows the bisection cannot satisfy or that take its sum_P == 0 branch, at width k."""
    rows = [np.zeros(k), np.full(k, 2.5), np.full(k, 1e10), np.full(k, 3e38)]
    r = np.full(k, 1e12)
    r[: min(5, max(k - 1, 1))] = 0.0
    rows.append(r)
    r = np.full(k, 3e38)
    r[0] = 1e-30
    rows.append(r)
    rows.append(np.round(np.random.default_rng(k).uniform(0.0, 6.0, k) * 2.0) / 2.0)        # exact ties
    return np.asarray(rows, dtype=np.float32)


def random_rows(n, k, seed, sort=False):
    rng = np.random.default_rng(seed)
    d = rng.gamma(3.0, 1.0, (n, k)) * 10.0 ** rng.uniform(-2.0, 2.0, (n, 1))
    return (np.sort(d, 1) if sort else d).astype(np.float32)


def knn_lists(N, k, seed):
    """Neighbour lists (every row's columns distinct, never the row itself, sorted) with squared distances."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, 4))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    idx = np.sort(np.argsort(d2, 1)[:, :k], 1)
    return idx, np.take_along_axis(d2, idx, 1).astype(np.float32)


def joint_p32(oracle, N, k, perplexity, seed):
    """A symmetric joint P as the kernels read it: CSR with values rounded to f32."""
    idx, sqd = knn_lists(N, k, seed)
    cond, _, _ = oracle.tsne_binary_search_perplexity(sqd, perplexity)
    indptr, indices, val = oracle.tsne_joint_p(idx, cond)
    return indptr, indices, val.astype(np.float32)


# ---------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("D", [1, 2])
def test_two_points_at_distance_one(oracle, D):
    Y = np.zeros((2, D), np.float32)
    Y[1, 0] = 1.0
    o = oracle.tsne_objective(Y, np.zeros(3, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), D)
    assert np.array_equal(o["W"], [0.5, 0.5]) and o["Z"] == 1.0 and o["Z_raw"] == 1.0
    want = np.zeros((2, D))
    want[:, 0] = [-0.25, 0.25]                                           # w^2 (y_i - y_j)
    assert np.array_equal(o["rep"], want) and np.array_equal(o["A_rep"], np.abs(want))
    assert np.array_equal(o["grad"], -4.0 * want) and o["KL"] == 0.0


def test_two_points_at_dof_two(oracle):
    Y = np.zeros((2, 3), np.float32)
    Y[1, 1] = 2.0                                                        # d^2 = 4: t = 2 / 6, w = t^1.5, force weight t^3
    o = oracle.tsne_objective(Y, np.zeros(3, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 3)
    t = 1.0 / 3.0
    np.testing.assert_allclose(o["W"], [t ** 1.5] * 2, rtol=1e-15)
    np.testing.assert_allclose(o["rep"][:, 1], [-2.0 * t ** 3, 2.0 * t ** 3], rtol=1e-15)
    np.testing.assert_allclose(o["grad"][:, 1], 3.0 * 2.0 * t ** 3 / (2.0 * t ** 1.5) * np.array([1.0, -1.0]), rtol=1e-15)


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("N", [2, 3, 257, 600])
def test_coincident_points(oracle, N, D):
    Y = np.tile(np.asarray([1.5, -2.25, 3.0], np.float32)[:D], (N, 1))
    o = oracle.tsne_objective(Y, np.zeros(N + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), D)
    assert np.array_equal(o["W"], np.full(N, N - 1.0)) and o["Z"] == N * (N - 1.0)
    assert not o["rep"].any() and not o["grad"].any() and not o["A_rep"].any()


def test_far_pair_takes_the_floor_of_z(oracle):
    Y = np.asarray([[0.0, 0.0], [1e20, 0.0]], np.float32)
    o = oracle.tsne_objective(Y, np.asarray([0, 1, 2]), np.asarray([1, 0]), np.asarray([0.5, 0.5], np.float32), 2)
    assert o["Z"] == float(np.float32(np.finfo(np.float64).eps)) and o["Z_raw"] < 1e-39
    assert np.all(np.isfinite(o["grad"])) and np.abs(o["grad"]).max() <= 1e-15 and np.isfinite(o["KL"])


def test_attraction_and_error_terms(oracle):
    # three points on a line, P = {(0, 1): 0.25, (1, 0): 0.25, (0, 0): 0.5 (a self-loop), (2, 1): 1e-40 (below FLT_MIN)}
    Y = np.asarray([[0.0], [1.0], [3.0]], np.float32)
    pv = np.asarray([0.5, 0.25, 0.25, 1e-40], np.float32)
    o = oracle.tsne_objective(Y, np.asarray([0, 2, 3, 4]), np.asarray([0, 1, 0, 1]), pv, 1)
    w01, w02, w12 = 0.5, 0.1, 0.2
    Z = 2.0 * (w01 + w02 + w12)
    assert o["Z"] == pytest.approx(Z, rel=1e-15)
    np.testing.assert_allclose(o["attr"][:, 0], [0.25 * w01 * -1.0, 0.25 * w01 * 1.0, float(pv[3]) * w12 * 2.0], rtol=1e-15)
    np.testing.assert_allclose(o["A_attr"][:, 0], np.abs(o["attr"][:, 0]), rtol=1e-15)
    tiny = float(np.finfo(np.float32).tiny)
    f32 = lambda x: float(np.float32(x))
    kl = 0.5 * np.log(0.5 / f32(1.0 / Z)) + 2 * 0.25 * np.log(0.25 / f32(w01 / Z)) + float(pv[3]) * np.log(tiny / f32(w12 / Z))
    assert o["KL"] == pytest.approx(kl, rel=1e-15)
    assert o["sum_p"] == pytest.approx(1.0, rel=1e-15)


def test_kl_at_a_given_z(oracle):
    Y = np.random.default_rng(0).normal(0.0, 2.0, (50, 2)).astype(np.float32)
    indptr, indices, pv = joint_p32(oracle, 50, 7, 3.0, 1)
    o = oracle.tsne_objective(Y, indptr, indices, pv, 2)
    assert oracle.tsne_kl(Y, indptr, indices, pv, o["Z"]) == o["KL"]
    # no clamp is active here: KL(Z') - KL(Z) = sum(p) log(Z' / Z), up to the f32 rounding of every q / Z (2^-24 each way)
    shifted = oracle.tsne_kl(Y, indptr, indices, pv, 1.25 * o["Z"])
    assert abs(shifted - o["KL"] - o["sum_p"] * np.log(1.25)) <= 2.0 ** -23 * o["sum_p"]


def test_bisection_closed_forms(oracle):
    for k in (2, 5, 30):                                                 # equal distances, perplexity == k: uniform at once
        P, steps, margin = oracle.tsne_binary_search_perplexity(np.full((3, k), 2.5, np.float32), float(k))
        np.testing.assert_allclose(P, 1.0 / k, rtol=1e-15)              # v / (v + ... + v), summed in order
        assert np.all(steps == 1) and np.all(margin > 9e-6)
    P, steps, _ = oracle.tsne_binary_search_perplexity(np.asarray([[0.0], [2.5], [1e10]], np.float32), 2.0)      # k = 1
    assert np.array_equal(P, np.ones((3, 1))) and np.all(steps == 0)
    for k, perplexity in ((3, 2.0), (16, 5.0), (16, 30.0)):             # duplicate cells: all distances 0
        P, steps, _ = oracle.tsne_binary_search_perplexity(np.zeros((2, k), np.float32), perplexity)
        assert np.array_equal(P, np.full((2, k), 1.0 / k)) and np.all(steps == 0)
    # rows of 1e10 with more neighbours than the perplexity: uniform wherever exp() does not underflow, which is too flat, and 0
    # where it does - the bisection ends on the underflowing side, in the sum_P == 0 branch
    for k, perplexity in ((16, 5.0), (91, 30.0)):
        P, steps, margin = oracle.tsne_binary_search_perplexity(np.full((2, k), 1e10, np.float32), perplexity)
        assert not P.any() and np.all(steps == 0) and np.all(margin > 0.1)


def test_bisection_meets_the_perplexity(oracle):
    for perplexity in (5.0, 30.0):
        sqd = random_rows(64, 91, 3)
        P, steps, margin = oracle.tsne_binary_search_perplexity(sqd, perplexity)
        assert np.all(steps > 0) and np.all(margin >= 0)
        np.testing.assert_allclose(P.sum(1), 1.0, rtol=0, atol=1e-14)
        H = -np.sum(P * np.log(np.where(P > 0, P, 1.0)), 1)
        assert np.all(np.abs(H - np.log(perplexity)) <= float(np.float32(1e-5)) + 1e-12)


def test_joint_p_small(oracle):
    # 0 -> 1 (0.5), 1 -> 0 (0.25): mutual; 2 -> 0 (1.0): one-sided; 3 -> 2 with conditional P exactly 0: dropped
    indptr, indices, val = oracle.tsne_joint_p(np.asarray([[1], [0], [0], [2]]), np.asarray([[0.5], [0.25], [1.0], [0.0]]))
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and val.dtype == np.float64
    assert np.array_equal(indptr, [0, 2, 3, 4, 4]) and np.array_equal(indices, [1, 2, 0, 0])
    np.testing.assert_allclose(val, np.asarray([0.75, 1.0, 0.75, 1.0]) / 3.5, rtol=1e-15)
    indptr, indices, val = oracle.tsne_joint_p(np.asarray([[1], [0]]), np.zeros((2, 1)))
    assert np.array_equal(indptr, [0, 0, 0]) and indices.size == 0 and val.size == 0


def test_step_rule(oracle):
    f = np.float32
    Y = np.asarray([[1.0], [2.0], [3.0], [4.0], [5.0]], f)
    update = np.asarray([[0.0], [1.0], [-1.0], [1.0], [0.0]])
    grad = np.asarray([[0.5], [0.5], [0.5], [-0.5], [-0.5]])
    gains = np.asarray([[1.0], [1.0], [1.0], [0.0101], [0.0125]], f)
    Yo, u, g, gg = oracle.tsne_step(Y, update, gains, grad, 0.5, 10.0, 0.01)
    assert Yo.dtype == f and g.dtype == f and u.dtype == np.float64
    want = np.asarray([f(1.0) * f(0.8), f(1.0) * f(0.8), f(1.0) + f(0.2), f(0.0101) + f(0.2), f(0.0125) * f(0.8)], f)[:, None]
    assert np.array_equal(g, want) and g[4, 0] > f(0.01)
    assert np.array_equal(gg, grad * want.astype(np.float64)) and np.array_equal(u, 0.5 * update - 10.0 * gg)
    assert np.array_equal(Yo, (Y.astype(np.float64) + u).astype(f))
    # the floor: 0.0101 x 0.8 is below both floors, 0.0125 x 0.8 only below 0.05, a gain at the floor stays there
    for mg in (0.01, 0.05):
        _, _, g, _ = oracle.tsne_step(Y[:3], np.zeros((3, 1)), np.asarray([[0.0101], [0.0125], [mg]], f), grad[:3], 0.8, 10.0, mg)
        assert g[0, 0] == f(mg) and g[2, 0] == f(mg) and g[1, 0] == (f(0.05) if mg == 0.05 else f(0.0125) * f(0.8))


# ---------------------------------------------------------------------------------------------- scikit-learn
@pytest.mark.parametrize("k", [1, 2, 3, 16, 91])
def test_bisection_against_scikit_learn(oracle, k):
    _utils = pytest.importorskip("sklearn.manifold._utils")
    sqd = np.ascontiguousarray(np.concatenate([degenerate_rows(k), random_rows(100, k, 10 + k), random_rows(100, k, 20 + k, sort=True)]))
    assert sqd.shape[0] > k                    # with as many columns as rows scikit-learn reads a dense matrix and skips its diagonal
    for perplexity in (2.0, 5.0, 30.0, 100.0):
        P, steps, _ = oracle.tsne_binary_search_perplexity(sqd, perplexity)
        ref = _utils._binary_search_perplexity(sqd, perplexity, 0)
        np.testing.assert_allclose(P, ref, rtol=0, atol=1e-15)


@pytest.mark.parametrize("N,k,perplexity", [(300, 16, 5.0), (200, 91, 30.0), (40, 1, 2.0)])
def test_joint_p_against_scikit_learn(oracle, N, k, perplexity):
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    idx, sqd = knn_lists(N, k, 30 + k)
    if k == 16:
        sqd[7] = 1e10                          # a row whose conditional P is exactly 0: its entries leave the pattern
    D = sparse.csr_matrix((sqd.ravel().astype(np.float64), idx.ravel(), np.arange(0, N * k + 1, k)), shape=(N, N))
    ref = sk._joint_probabilities_nn(D, perplexity, 0)
    ref.sort_indices()
    cond, _, _ = oracle.tsne_binary_search_perplexity(sqd, perplexity)
    if k == 16:
        assert not cond[7].any()
    indptr, indices, val = oracle.tsne_joint_p(idx, cond)
    assert np.array_equal(indptr, ref.indptr) and np.array_equal(indices, ref.indices)
    # the conditional P agree to 1e-15 absolute; then one addition, one division, and the order of the normalising sum
    np.testing.assert_allclose(val, ref.data, rtol=1e-13, atol=2e-15 / N)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_gradient_against_scikit_learn_exact(oracle, D):
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    N = 150
    indptr, indices, pv = joint_p32(oracle, N, 16, 5.0, 40 + D)
    Y = np.random.default_rng(50 + D).normal(0.0, 1.0, (N, D)).astype(np.float32)
    dense = sparse.csr_matrix((pv.astype(np.float64), indices, indptr), shape=(N, N)).toarray()
    assert np.array_equal(dense, dense.T) and not dense.diagonal().any()
    dof = max(D - 1, 1)
    _, g_ref = sk._kl_divergence(Y.astype(np.float64).ravel(), squareform(dense), dof, N, D)
    o = oracle.tsne_objective(Y, indptr, indices, pv, D)
    # scikit-learn floors every Q_ij at DBL_EPSILON; this embedding stays far above that floor
    assert (o["W"].min() / (N - 1)) / o["Z"] > 1e-12
    np.testing.assert_allclose(o["grad"], g_ref.reshape(N, D), rtol=1e-10)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_kl_against_scikit_learn_barnes_hut(oracle, D):
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    N = 400
    indptr, indices, pv = joint_p32(oracle, N, 31, 10.0, 60 + D)
    Y = np.random.default_rng(70 + D).normal(0.0, 3.0, (N, D)).astype(np.float32)
    P = sparse.csr_matrix((pv.astype(np.float64), indices, indptr), shape=(N, N))
    kw = {"num_threads": 1} if "num_threads" in inspect.signature(sk._kl_divergence_bh).parameters else {}
    kl_ref, g_ref = sk._kl_divergence_bh(Y.ravel(), P, max(D - 1, 1), N, D, angle=0.0, **kw)
    o = oracle.tsne_objective(Y, indptr, indices, pv, D)
    np.testing.assert_allclose(o["KL"], kl_ref, rtol=1e-4)              # scikit-learn sums KL in f32
    g_ref = g_ref.reshape(N, D)
    assert np.abs(o["grad"] - g_ref).max() <= 1e-5 * np.abs(g_ref).max()  # its tree sums the forces in f32
