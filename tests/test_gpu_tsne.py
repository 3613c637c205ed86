"""Device t-SNE (csrc/tsne.hip, velocyto_amd.tsne.DeviceTSNE, perform_TSNE(backend="hip")) against scikit-learn's own private
functions - the code the reference's perform_TSNE runs (analysis.py:1441-1450): the perplexity bisection, the joint P, the
objective at angle = 0 (the exact gradient the device computes), a stretch of the optimiser, and whole fits scored by one
referee.  Data: seeded, tie-free clusters (12 N(0, 1) blobs in 30 dimensions)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sk_tsne = pytest.importorskip("sklearn.manifold._t_sne")
from sklearn.manifold import TSNE, _utils, trustworthiness  # noqa: E402
from sklearn.neighbors import NearestNeighbors  # noqa: E402
from sklearn.utils import check_random_state  # noqa: E402

THREADS = 8


@pytest.fixture(scope="module")
def vcy():
    import velocyto_amd
    from velocyto_amd import ops
    ops.require_gpu()
    return velocyto_amd


def blobs(n, seed, d=30, centers=12):
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 4.0, (centers, d))
    return c[rng.integers(0, centers, n)] + rng.normal(size=(n, d))


def sk_graph(X, k):
    """What TSNE._fit hands _joint_probabilities_nn: the kNN distance graph, squared (_t_sne.py:967-1002)."""
    D = NearestNeighbors(n_neighbors=k).fit(X).kneighbors_graph(mode="distance")
    D.data **= 2
    return D


def entropy(P):
    return -np.sum(P * np.log(np.where(P > 0, P, 1.0)), 1)


@pytest.mark.parametrize("perplexity", [5.0, 30.0, 50.0])
def test_conditional_and_joint_p(vcy, perplexity):
    from velocyto_amd import ops
    from velocyto_amd.tsne import DeviceTSNE
    N = 3000
    X = blobs(N, 1)
    k = min(N - 1, int(3 * perplexity + 1))
    D = sk_graph(X, k)
    Ds = D.copy()
    Ds.sort_indices()
    sqd = Ds.data.reshape(N, k).astype(np.float32)
    ref = _utils._binary_search_perplexity(sqd, perplexity, 0)
    got, steps = ops.tsne_perplexity(torch.from_numpy(sqd), perplexity)
    got, steps = got.cpu().numpy(), steps.cpu().numpy()
    dP = np.abs(got - ref).max(1)
    assert np.mean(dP <= 1e-12) >= 0.999, np.sort(dP)[-5:]
    assert np.all(dP <= 1e-4 * ref.max(1))                       # a row may stop one bisection step apart at the tolerance edge
    tol = float(np.float32(1e-5)) + 1e-12
    conv = steps > 0
    assert np.all(np.abs(entropy(got)[conv] - np.log(perplexity)) <= tol)
    # rows that used all 100 steps here used them in scikit-learn too (up to the same tolerance edge)
    assert np.mean(np.abs(entropy(ref)[~conv] - np.log(perplexity)) > tol - 1e-12) >= 0.999 if (~conv).any() else True

    # the same through DeviceTSNE's own kNN and symmetrisation
    aff = DeviceTSNE(perplexity=perplexity)._affinities(torch.from_numpy(X).cuda())
    assert np.array_equal(aff["idx"].cpu().numpy(), Ds.indices.reshape(N, k))     # same neighbour sets, both in index order
    # rows whose inputs or stopping step differ: an f32 distance an ulp apart, or the bisection stopped a step apart
    off = np.any(aff["sqd"].cpu().numpy() != sqd, 1) | (np.abs(aff["cond"].cpu().numpy() - ref).max(1) > 1e-12)
    assert off.mean() <= 0.005
    Pref = sk_tsne._joint_probabilities_nn(D.copy(), perplexity, 0)
    Pref.sort_indices()
    ip, ix, pv = aff["indptr"].cpu().numpy(), aff["indices"].cpu().numpy(), aff["P"].cpu().numpy()
    assert np.array_equal(ip, Pref.indptr) and np.array_equal(ix, Pref.indices)     # the same sparsity pattern
    rows = np.repeat(np.arange(N), np.diff(ip))
    clean = ~(off[rows] | off[ix])
    np.testing.assert_allclose(pv[clean], Pref.data[clean], rtol=1e-9)
    np.testing.assert_allclose(pv, Pref.data, rtol=1e-4)


@pytest.mark.parametrize("nc", [2, 3])
def test_objective_matches_barnes_hut_at_angle_zero(vcy, nc):
    from velocyto_amd.tsne import DeviceTSNE
    N = 2000
    X = blobs(N, 2)
    P = sk_tsne._joint_probabilities_nn(sk_graph(X, 91), 30.0, 0)
    Y = np.random.default_rng(3).normal(0.0, 5.0, (N, nc)).astype(np.float32)
    dof = max(nc - 1, 1)
    kl_ref, g_ref = sk_tsne._kl_divergence_bh(Y.ravel(), P, dof, N, nc, angle=0.0, num_threads=THREADS)
    g_ref = g_ref.reshape(N, nc)
    kl, g = DeviceTSNE(n_components=nc)._objective(Y, P)
    assert g.dtype == np.float32 and g.shape == (N, nc)
    assert np.abs(g - g_ref).max() <= 1e-5 * np.abs(g_ref).max()
    np.testing.assert_allclose(kl, kl_ref, rtol=1e-4)          # scikit-learn sums its error in f32
    # an f64 dense restatement of the same formulas
    Y64 = Y.astype(np.float64)
    d2 = ((Y64[:, None, :] - Y64[None, :, :]) ** 2).sum(-1)
    w = (dof / (dof + d2)) ** ((dof + 1) / 2)
    np.fill_diagonal(w, 0.0)
    Z = w.sum()
    p = P.data.astype(np.float32).astype(np.float64)
    q = w[np.repeat(np.arange(N), np.diff(P.indptr)), P.indices] / Z
    tiny = float(np.finfo(np.float32).tiny)
    kl64 = float(np.sum(p * np.log(np.maximum(p, tiny) / np.maximum(q, tiny))))
    np.testing.assert_allclose(kl, kl64, rtol=1e-6)


def test_descent_matches_gradient_descent(vcy):
    """Phase 1 of the optimiser from scikit-learn's start against its _gradient_descent at angle = 0.
    The two gradients agree to ~3e-7 of max |grad|, and the trajectories agree to ~1e-4 of the embedding's spread while every
    gain takes the same branch.  The gain rule branches on the sign of update * grad, and early exaggeration grows any
    difference by about 1.5x per iteration, so a near-zero component eventually takes the other branch on one side.  That
    point then moves by the ratio of the two gains and pulls its cluster with it.  In a replay of this case with an exact f64
    gradient the first such branch comes at iteration 24, and by iteration 30 it has moved 8 % of the points by more than
    1e-3 of the spread.  So every point is held to 1e-3 of the spread at 20 iterations.  At 30 iterations the bounds are on
    the gains and the median point."""
    from velocyto_amd.tsne import DeviceTSNE
    N, nc, n_strict, n_it = 2000, 2, 20, 30
    X = blobs(N, 4)
    P_ex = sk_tsne._joint_probabilities_nn(sk_graph(X, 91), 30.0, 0) * 12.0        # phase 1: P x early_exaggeration
    Y0 = 1e-4 * check_random_state(5).standard_normal(size=(N, nc)).astype(np.float32)
    lr = np.maximum(N / 12.0 / 4, 50)
    kw = {"angle": 0.0, "skip_num_points": 0, "verbose": 0, "num_threads": THREADS}
    p_ref, _, _ = sk_tsne._gradient_descent(sk_tsne._kl_divergence_bh, Y0.ravel(), 0, n_it, n_iter_check=50, n_iter_without_progress=250,
                                            momentum=0.5, learning_rate=lr, min_gain=0.01, min_grad_norm=1e-7, args=[P_ex, 1, N, nc],
                                            kwargs=dict(kw))
    # _gradient_descent does not return its gains: the same rule replayed on the same objective (it lands on p_ref exactly)
    p, update, gains = Y0.ravel().copy(), np.zeros(N * nc, np.float32), np.ones(N * nc, np.float32)
    snap = {}
    for i in range(n_it):
        _, grad = sk_tsne._kl_divergence_bh(p, P_ex, 1, N, nc, compute_error=False, **kw)
        inc = update * grad < 0.0
        gains[inc] += 0.2
        gains[~inc] *= 0.8
        np.clip(gains, 0.01, np.inf, out=gains)
        grad *= gains
        update = 0.5 * update - lr * grad
        p += update
        if i + 1 in (n_strict, n_it):
            snap[i + 1] = (p.reshape(N, nc).copy(), gains.copy())
    assert np.array_equal(p, p_ref)
    t = DeviceTSNE(n_components=nc)
    t.learning_rate_ = lr
    for n, (ref, g_ref) in sorted(snap.items()):
        Y, _, it, g_dev = t._descend(Y0, P_ex, 0, n, 0.5, 250)
        assert it == n - 1
        gap, spread = np.abs(Y - ref).max(1), ref.std()
        if n == n_strict:
            assert np.mean(g_dev.ravel() == g_ref) >= 0.999
            assert gap.max() <= 1e-3 * spread, (gap.max() / spread, np.argsort(gap)[-5:])
        else:
            assert np.mean(g_dev.ravel() == g_ref) >= 0.99
            assert np.median(gap) <= 1e-3 * spread, np.median(gap) / spread


def test_fit_end_to_end_against_scikit_learn(vcy):
    from velocyto_amd.tsne import DeviceTSNE
    N = 4000
    X = blobs(N, 6)
    t = DeviceTSNE(random_state=7)
    Y0 = t._initial_embedding(N)
    assert Y0.dtype == np.float32
    assert np.array_equal(Y0, 1e-4 * check_random_state(7).standard_normal(size=(N, 2)).astype(np.float32))   # _t_sne.py:1024-1026
    Yd = t.fit_transform(X)
    assert Yd.dtype == np.float32 and Yd.shape == (N, 2) and np.all(np.isfinite(Yd))
    assert t.n_iter_ >= 250 and np.isfinite(t.kl_divergence_) and t.n_features_in_ == 30 and t.learning_rate_ == np.maximum(N / 12.0 / 4, 50)
    Ys = TSNE(n_components=2, perplexity=30.0, init="random", random_state=7, max_iter=1000).fit_transform(X)   # default angle 0.5
    P = sk_tsne._joint_probabilities_nn(sk_graph(X, 91), 30.0, 0)
    score = lambda Y: sk_tsne._kl_divergence_bh(np.asarray(Y, np.float32).ravel(), P, 1, N, 2, angle=0.0, num_threads=THREADS)[0]
    kl_d, kl_s = score(Yd), score(Ys)
    assert kl_d <= 1.02 * kl_s, (kl_d, kl_s)
    tw_d, tw_s = trustworthiness(X, Yd, n_neighbors=10), trustworthiness(X, Ys, n_neighbors=10)
    assert tw_d >= tw_s - 0.01, (tw_d, tw_s)


def test_scale_determinism_and_exact_repulsion(vcy):
    from velocyto_amd import ops
    from velocyto_amd.tsne import DeviceTSNE
    N = 50_000                                     # not a multiple of the 512-target blocks, the 256-source tiles or the splits
    X = blobs(N, 8)
    a = DeviceTSNE(random_state=9)
    Ya = a.fit_transform(X)
    b = DeviceTSNE(random_state=9)
    Yb = b.fit_transform(X)
    assert np.array_equal(Ya, Yb) and a.n_iter_ == b.n_iter_ and a.kl_divergence_ == b.kl_divergence_
    # one evaluation of the repulsion on the fitted embedding: with an empty P the gradient is -c rep / Z (c = 4 at dof = 1)
    dev = torch.device("cuda", torch.cuda.current_device())
    Y = torch.from_numpy(Ya).to(dev)
    indptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    grad, stats = ops.tsne_gradient(Y, indptr, torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev),
                                    compute_error=False)
    Z = float(stats[0])
    sel = torch.from_numpy(np.random.default_rng(10).choice(N, 256, replace=False)).to(dev)
    rep = (-grad.double()[sel] / 4.0 * Z).cpu().numpy()
    Y64 = Y.double()
    ref = torch.empty((256, 2), dtype=torch.float64, device=dev)
    for s in range(0, 256, 32):
        t = sel[s:s + 32]
        diff = Y64[t, None, :] - Y64[None, :, :]
        w = 1.0 / (1.0 + (diff * diff).sum(-1))
        w[torch.arange(t.numel(), device=dev), t] = 0.0
        ref[s:s + 32] = ((w * w)[..., None] * diff).sum(1)
    Zref = 0.0
    for s in range(0, N, 500):
        diff = Y64[s:s + 500, None, :] - Y64[None, :, :]
        w = 1.0 / (1.0 + (diff * diff).sum(-1))
        Zref += float(w.sum()) - w.shape[0]        # w_ii = 1 exactly
    np.testing.assert_allclose(Z, Zref, rtol=1e-6)
    ref = ref.cpu().numpy()
    np.testing.assert_allclose(rep, ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max())


def _loom(vcy, golden):
    g = golden("pipeline")
    vlm = vcy.analysis.VelocytoLoom.from_arrays(g["S"], g["U"])
    vlm.normalize("both", size=True, log=True)
    vlm.pcs = g["pcs"]
    vlm.Sx_sz, vlm.Ux_sz = g["Sx"], g["Ux"]
    vlm.gammas, vlm.q = g["gammas"], g["q"]
    vlm.predict_U(); vlm.calculate_velocity(); vlm.calculate_shift(); vlm.extrapolate_cell_at_t()
    return vlm, g


def test_perform_tsne_hip_backend(vcy, golden):
    from velocyto_amd.tsne import DeviceTSNE
    vlm, g = _loom(vcy, golden)
    C = g["pcs"].shape[0]
    np.random.seed(11)
    vlm.perform_TSNE(backend="hip")
    ts = vlm.ts
    assert ts.dtype == np.float32 and ts.shape == (C, 2)
    np.random.seed(11)
    assert np.array_equal(ts, DeviceTSNE(n_components=2, perplexity=30, angle=0.5, init="random", max_iter=1000).fit_transform(g["pcs"]))
    vlm.estimate_transition_prob(hidim="Sx_sz", embed="ts", transform="sqrt", n_neighbors=40, knn_random=True, sampled_fraction=0.5,
                                 calculate_randomized=False, threads=1)
    vlm.calculate_embedding_shift(sigma_corr=0.05)
    assert vlm.delta_embedding.shape == (C, 2) and np.all(np.isfinite(vlm.delta_embedding))
    # initial_pos is honoured
    init = (10.0 * np.random.default_rng(12).normal(size=(C, 2))).astype(np.float32)
    vlm.perform_TSNE(initial_pos=init, n_pca_dim=5, max_iter=300, backend="hip")
    ref = DeviceTSNE(init=init, max_iter=300).fit_transform(g["pcs"][:, :5])
    assert np.array_equal(vlm.ts, ref) and not np.array_equal(vlm.ts[:, :2], ts)
