"""Host side of the gene selection from CSR count layers: the numpy helpers the facade and the atlas route share
(preprocess.detection_mask, cv_vs_mean_from_stats, cluster_averages, cluster_expression_mask), the threshold table of
atlas.default_gene_filter and the `keep` / `remap` checks of CsrCounts.select_genes.  No device.

The helpers are fed per-gene statistics computed here with numpy's int64 sums from the recorded input layers of
tests/golden/preprocess.npz and must reproduce what the reference left there: masks and averages exactly (integer statistics, one
division), the CV-vs-mean score with scikit-learn's SVR standing in for the device's at the bar of tests/test_gpu_preprocess.py (5e-3:
two libsvm-style solutions each stopped at tol = 1e-3 of the target).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _stats(M):
    """(4, G) float64 [sum, sum of squares, count(x > 0), max] of a (genes, cells) count array: exact integers."""
    M = np.asarray(M, dtype=np.int64)
    return np.stack([M.sum(1), (M * M).sum(1), (M > 0).sum(1), M.max(1) if M.shape[1] else np.zeros(M.shape[0])]).astype(np.float64)


@pytest.fixture(scope="module")
def g(golden):
    return golden("preprocess")


def test_detection_mask_reproduces_the_recorded_selection(g):
    from velocyto_amd.preprocess import detection_mask
    m = detection_mask(_stats(g["S"]), _stats(g["U"]), min_expr_counts=40, min_cells_express=20, min_expr_counts_U=15, min_cells_express_U=10)
    assert m.dtype == bool and np.array_equal(m, g["detection_level_selected"])
    assert np.array_equal(np.flatnonzero(m), g["genes_after_detection"])


def test_detection_mask_on_a_hand_computed_case():
    from velocyto_amd.preprocess import detection_mask
    # rows: sum, sum of squares, expressing cells, max; columns: four genes
    sS = np.array([[50., 49., 50., 0.], [9., 9., 9., 0.], [20., 20., 19., 0.], [5., 5., 5., 0.]])
    sU = np.array([[7., 7., 6., 7.], [9., 9., 9., 0.], [3., 3., 3., 2.], [5., 5., 5., 0.]])
    assert list(detection_mask(sS, sU)) == [True, False, False, False]                      # thresholds are inclusive: 50 counts, 20 cells
    assert list(detection_mask(sS, sU, 0, 0, 7, 3)) == [True, True, False, False]           # the unspliced pair alone


def test_cluster_averages_reproduce_the_recorded_ones(g):
    from velocyto_amd.preprocess import cluster_averages, cluster_expression_mask
    genes, ix = g["genes_after_detection"], g["cluster_ix"]
    S, U = g["S"][genes].astype(np.int64), g["U"][genes].astype(np.int64)
    sizes = np.bincount(ix, minlength=len(g["cluster_uid"]))
    assert (sizes <= 40).any() and (sizes > 40).any()                                      # both branches
    asked = []

    def cluster_sums(i):
        asked.append(i)
        return U[:, ix == i].sum(1).astype(np.float64), S[:, ix == i].sum(1).astype(np.float64)
    overall_calls = []

    def overall_sums():
        overall_calls.append(1)
        return U.sum(1).astype(np.float64), S.sum(1).astype(np.float64)
    U_avgs, S_avgs = cluster_averages(sizes, S.shape[1], S.shape[0], cluster_sums, overall_sums, size_limit=40)
    assert asked == [i for i, n in enumerate(sizes) if n > 40] and len(overall_calls) == 1
    # the reference takes np.mean over float64 copies: a sum of integers (exact either way) and one division
    assert np.array_equal(U_avgs, g["U_avgs"]) and np.array_equal(S_avgs, g["S_avgs"])
    assert np.array_equal(cluster_expression_mask(U_avgs, S_avgs, 0.02, 0.08), g["clu_avg_selected"])


def test_cv_vs_mean_from_stats_with_sklearn_standing_in_for_the_device_svr(g, monkeypatch):
    svm = pytest.importorskip("sklearn.svm")
    from velocyto_amd import preprocess
    monkeypatch.setattr(preprocess, "DeviceSVR", lambda gamma: svm.SVR(gamma=gamma))
    genes = g["genes_after_detection"]
    st = _stats(g["S"][genes])
    C = g["S"].shape[1]
    for kw, name, N in ((dict(N=200, max_expr_avg=40), "", 200),
                        (dict(N=120, max_expr_avg=40, sort_inverse=True, min_expr_cells=5, min_expr_avg=0.05), "_inverse", 120)):
        score, mask = preprocess.cv_vs_mean_from_stats(st, C, **kw)
        ref, ref_mask = g["cv_mean_score" + name], g["cv_mean_selected" + name]
        assert score.shape == ref.shape and np.all(np.abs(score - ref) <= 5e-3), float(np.abs(score - ref).max())
        assert mask.dtype == bool and mask.sum() >= N + 1 and (mask != ref_mask).sum() <= max(2, int(0.02 * N))
        assert np.array_equal(mask, score >= np.sort(score[score > score.min()])[::-1][N])
    # the unspliced layer
    score, mask = preprocess.cv_vs_mean_from_stats(_stats(g["U"][genes]), C, N=150, max_expr_avg=30)
    assert np.all(np.abs(score - g["Ucv_mean_score"]) <= 5e-3) and (mask != g["Ucv_mean_selected"]).sum() <= 3
    # `moments`: detection from `st`, mean and variance from the other statistics
    st2 = st.copy()
    st2[1] *= 1.5
    s_a, _ = preprocess.cv_vs_mean_from_stats(st, C, N=200, max_expr_avg=40, moments=st2)
    s_b, _ = preprocess.cv_vs_mean_from_stats(st2, C, N=200, max_expr_avg=40)
    assert np.array_equal(s_a, s_b) and not np.array_equal(s_a, preprocess.cv_vs_mean_from_stats(st, C, N=200, max_expr_avg=40)[0])


@pytest.mark.parametrize("cells", [1, 500, 4444, 8000, 33333, 100000, 1_000_000])
def test_default_gene_thresholds_are_the_facades(cells):
    from velocyto_amd import atlas
    from velocyto_amd.preprocess import PreprocessMixin
    ref = PreprocessMixin._default_thresholds(cells)
    t = atlas.default_gene_thresholds(cells)
    assert set(t) == {"min_expr_counts", "min_cells_express", "N", "min_avg_U", "min_avg_S"}
    assert all(t[k] == ref[k] for k in t)
    t2 = atlas.default_gene_thresholds(cells, N=321, min_avg_U=None)
    assert t2["N"] == 321 and t2["min_avg_U"] == ref["min_avg_U"] and t2["min_expr_counts"] == ref["min_expr_counts"]
    with pytest.raises(TypeError):
        atlas.default_gene_thresholds(cells, max_expr_avg=3)


def test_gene_remap_of_masks_and_lists():
    from velocyto_amd import ops
    r, n = ops.gene_remap(np.array([True, False, True, True, False]), 5)
    assert n == 3 and r.dtype == np.int32 and list(r) == [0, -1, 1, 2, -1]
    r, n = ops.gene_remap([1, 4], 5)
    assert n == 2 and list(r) == [-1, 0, -1, -1, 1]
    r, n = ops.gene_remap(np.zeros(5, dtype=bool), 5)
    assert n == 0 and list(r) == [-1] * 5
    r, n = ops.gene_remap(np.array([], dtype=np.int64), 5)
    assert n == 0 and list(r) == [-1] * 5
    r, n = ops.gene_remap(torch.tensor([0, 4]).numpy(), 5)
    assert n == 2 and list(r) == [0, -1, -1, -1, 1]


@pytest.mark.parametrize("keep", [np.ones(4, dtype=bool), np.ones(6, dtype=bool), [0, 5], [-1, 2], [2, 1], [1, 1], [0.0, 1.0], np.ones((5, 1), dtype=bool)],
                         ids=["short-mask", "long-mask", "past-G", "negative", "descending", "repeat", "floats", "2d"])
def test_bad_keep_is_rejected(keep):
    from velocyto_amd import ops
    with pytest.raises(ValueError):
        ops.gene_remap(keep, 5)


def test_bad_remap_is_rejected():
    from velocyto_amd import ops
    assert list(ops.check_remap(np.array([1, -1, 0, -1]), 4, 2)) == [1, -1, 0, -1]          # a permutation of the kept ones passes the check
    for remap, G, G_new in (([0, 0, -1, 1], 4, 2), ([0, 2, -1, 1], 4, 2), ([0, 1, -1], 4, 2)):
        with pytest.raises(ValueError):
            ops.check_remap(np.array(remap), G, G_new)
