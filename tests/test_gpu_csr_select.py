"""Gene selection from CSR count layers (csrc/csr_select.hip -> ops.csr_gene_stats, CsrCounts.select_genes -> atlas.score_* /
default_gene_filter).  Every kernel call goes through the C ABI on cuda:0.

Nothing here has a tolerance: the statistics are sums of integers accumulated as integers (exact, independent of order and of the
cell blocking) and the arithmetic behind the masks is shared with the facade, so every comparison is bit for bit / array_equal -
against ops.gene_stats on the densified layer, against scipy's int64 column sums, against scipy's `a[:, keep]`, against the facade's
own attributes, and between the one-rank run and the ranks of a sharded one.
"""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker_module():
    spec = importlib.util.spec_from_file_location("gene_select_worker", os.path.join(ROOT, "tests", "gene_select_worker.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


@pytest.fixture(scope="module")
def L():
    import velocyto_amd
    from velocyto_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def B(L):
    return int(L.vcy_csr_gene_stats_block_cells())


@pytest.fixture(scope="module")
def SLAB(L):
    s = int(L.vcy_csr_slab_genes())
    assert s == 2048
    return s


VALUES = {"u8": np.array([1, 2, 3, 7, 100, 255]), "u16": np.array([1, 2, 3, 7, 255, 256, 4000, 65535])}


def _row_lengths(rng, C, G):
    """Rows with 0, 1, 3, 4, 5 stored elements, a full row (G stored), 63 / 64 / 65, then random lengths (the layout of
    tests/test_gpu_csr_pca.py with the full row added)."""
    lens = [0, 1, 3, 4, 5, G, 0, 64, 65, 63][:C]
    lens += list(rng.integers(0, min(G, 40) + 1, C - len(lens)))
    return rng.permutation(np.minimum(lens, G)) if C > 1 else np.array([min(3, G)])


def _layer(rng, lens, G, values):
    lens = np.minimum(np.asarray(lens, dtype=np.int64), G)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(G, n, replace=False)) for n in lens] + [np.empty(0, dtype=np.int64)]).astype(np.int32)
    data = rng.choice(values, int(indptr[-1])).astype(np.int64)
    return sp.csr_matrix((data, indices, indptr), shape=(len(lens), G))


def _device(ops, a, width):
    c = ops.CsrCounts.from_scipy(a, G=a.shape[1], narrow=(width == "u8"))
    assert c.data.dtype == (torch.uint8 if width == "u8" else torch.int16)
    return c


def _scipy_stats(a, mask=None):
    """(4, G) float64 from scipy's int64 arithmetic: column sums of a, of a*a, of (a > 0) and the column maxima over the masked rows."""
    a = sp.csr_matrix(a, dtype=np.int64)
    if mask is not None:
        a = a[np.flatnonzero(np.asarray(mask))]
    G = a.shape[1]
    if a.shape[0] == 0:
        return np.zeros((4, G))
    s, ss, n = (np.asarray(m.sum(0)).ravel() for m in (a, a.multiply(a), (a > 0).astype(np.int64)))
    assert s.dtype == np.int64 and ss.dtype == np.int64
    return np.stack([s, ss, n, a.max(0).toarray().ravel()]).astype(np.float64)


def _same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


def _check_stats(ops, a, cnt, mask=None, dense=True):
    got_t = ops.csr_gene_stats(cnt, mask)
    got = got_t.cpu().numpy()
    assert got.shape == (4, a.shape[1]) and got_t.dtype == torch.float64
    m = mask.cpu().numpy() if isinstance(mask, torch.Tensor) else mask
    assert _same_bits(got, _scipy_stats(a, m))
    if dense and a.shape[0] and (m is None or np.any(m)):           # with no cell selected the dense kernel's maximum is -inf, by its contract
        assert torch.equal(got_t, ops.gene_stats(cnt.to_dense(), cell_mask=mask))
    assert torch.equal(got_t, ops.csr_gene_stats(cnt, mask))              # the same call twice: the same bits
    return got


# ------------------------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("width", ["u8", "u16"])
@pytest.mark.parametrize("Gk", ["1", "slab-1", "slab", "slab+1", "2slab+1"])
@pytest.mark.parametrize("Ck", ["1", "B-1", "B", "B+1", "2B+3"])
def test_stats_equal_the_dense_kernel_and_scipy_bit_for_bit(ops, B, SLAB, Ck, Gk, width):
    C = {"1": 1, "B-1": B - 1, "B": B, "B+1": B + 1, "2B+3": 2 * B + 3}[Ck]
    G = {"1": 1, "slab-1": SLAB - 1, "slab": SLAB, "slab+1": SLAB + 1, "2slab+1": 2 * SLAB + 1}[Gk]
    rng = np.random.default_rng(C * 7 + G + (width == "u16"))
    a = _layer(rng, _row_lengths(rng, C, G), G, VALUES[width])
    cnt = _device(ops, a, width)
    _check_stats(ops, a, cnt)
    if C > 1:                                                             # the mask cases on every shape with more than one cell
        alt = np.arange(C) % 2 == 0
        whole_tiles = np.arange(C) >= min(B, C - 1)                       # empties the first tile (all but the last cell when C <= B)
        for mask in (np.ones(C, bool), np.zeros(C, bool), alt, whole_tiles, torch.as_tensor(alt, device=cnt.indptr.device)):
            got = _check_stats(ops, a, cnt, mask, dense=Gk in ("slab-1", "2slab+1"))
            if not bool(mask.any()):
                assert not got.any()


@pytest.mark.parametrize("nnz", [0, 1, 3, 4, 5])
def test_stats_of_layers_with_next_to_nothing_stored(ops, nnz):
    rng = np.random.default_rng(nnz)
    C, G = 4, 6
    dense = np.zeros(C * G, dtype=np.int64)
    dense[rng.choice(C * G, nnz, replace=False)] = rng.choice(VALUES["u16"], nnz)
    for width in ("u8", "u16"):
        a = sp.csr_matrix((np.minimum(dense, 255) if width == "u8" else dense).reshape(C, G))
        cnt = _device(ops, a, width)
        assert cnt.nnz == nnz
        _check_stats(ops, a, cnt)
        _check_stats(ops, a, cnt, np.array([1, 0, 0, 1], dtype=bool))


def test_stats_of_a_layer_without_cells(ops):
    dev = ops.require_gpu()
    cnt = ops.CsrCounts(torch.zeros(1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                        torch.empty(0, dtype=torch.uint8, device=dev), 2500)
    st = ops.csr_gene_stats(cnt)
    assert st.shape == (4, 2500) and not bool(st.any())
    assert not bool(ops.csr_gene_stats(cnt, np.zeros(0, dtype=bool)).any())


@pytest.mark.parametrize("width,top", [("u8", 255), ("u16", 65535)])
def test_one_gene_at_the_top_of_the_count_range_in_every_cell(ops, B, SLAB, width, top):
    """The largest sum of squares the format holds: C cells of `top` in one gene (2 B + 3 cells: three tiles)."""
    C, G = 2 * B + 3, SLAB + 5
    rng = np.random.default_rng(top)
    a = _layer(rng, rng.integers(0, 6, C), G, VALUES[width]).tolil()
    a[:, SLAB + 1] = top
    a = sp.csr_matrix(a)
    cnt = _device(ops, a, width)
    got = _check_stats(ops, a, cnt)
    assert got[0, SLAB + 1] == float(C * top) and got[1, SLAB + 1] == float(C * top * top) and got[2, SLAB + 1] == C and got[3, SLAB + 1] == top


def test_an_explicitly_stored_zero_counts_in_nothing(ops):
    dev = ops.require_gpu()
    # 3 cells x 5 genes through the raw constructor: zeros stored at (0, 1), (1, 4) and as the only element of gene 3
    indptr = np.array([0, 3, 5, 7])
    indices = np.array([0, 1, 2, 0, 4, 2, 3], dtype=np.int32)
    for dt, npdt in ((torch.uint8, np.uint8), (torch.int16, np.int16)):
        data = np.array([5, 0, 7, 1, 0, 2, 0]).astype(npdt)
        cnt = ops.CsrCounts(torch.as_tensor(indptr, device=dev), torch.as_tensor(indices, device=dev), torch.as_tensor(data, device=dev), 5)
        assert cnt.nnz == 7
        got = ops.csr_gene_stats(cnt).cpu().numpy()
        ref = np.array([[6, 0, 9, 0, 0], [26, 0, 53, 0, 0], [2, 0, 2, 0, 0], [5, 0, 7, 0, 0]], dtype=np.float64)
        assert _same_bits(got, ref)
        assert torch.equal(ops.csr_gene_stats(cnt), ops.gene_stats(cnt.to_dense()))


# ------------------------------------------------------------------------------------------------------------------ select_genes
def _same_csr(c, ref, dtype):
    ref = sp.csr_matrix(ref)
    ref.sort_indices()
    assert (c.C, c.G, c.nnz) == (ref.shape[0], ref.shape[1], ref.nnz)
    assert c.data.dtype == dtype and c.indptr.dtype == torch.int64 and c.indices.dtype == torch.int32
    assert np.array_equal(c.indptr.cpu().numpy(), ref.indptr)
    assert np.array_equal(c.indices.cpu().numpy(), ref.indices)
    vals = c.data.cpu().numpy()
    assert np.array_equal(vals.view(np.uint16) if vals.dtype == np.int16 else vals, ref.data)


@pytest.mark.parametrize("width", ["u8", "u16"])
@pytest.mark.parametrize("C,G", [(1, 5), (37, 130), (301, 4097)])
def test_select_genes_equals_scipy_column_indexing(ops, L, C, G, width):
    rng = np.random.default_rng(C + G + (width == "u16"))
    a = _layer(rng, _row_lengths(rng, C, G), G, VALUES[width])
    if G > int(L.vcy_csr_spmm_chunk()):
        assert np.diff(a.indptr).max() == G                               # a row longer than the chunk of the CSR products (rows are not cut here)
    cnt = _device(ops, a, width)
    half = rng.random(G) < 0.5
    only_empty_rows_left = np.zeros(G, dtype=bool)
    only_empty_rows_left[a[1 % C].indices[:1]] = True                     # a gene of one short row: most rows become empty
    keeps = {"all": np.ones(G, bool), "none": np.zeros(G, bool), "one": np.arange(G) == G // 2, "ends": np.isin(np.arange(G), [0, G - 1]),
             "half": half, "rows-empty": only_empty_rows_left}
    for name, keep in keeps.items():
        sub = cnt.select_genes(keep)
        _same_csr(sub, a[:, np.flatnonzero(keep)], cnt.data.dtype)
        assert sub.G == int(keep.sum()) and sub._slabptr is None and sub._max_row is None
        assert np.array_equal(sub.row_sums().cpu().numpy(), np.asarray(sp.csr_matrix(a, dtype=np.int64)[:, np.flatnonzero(keep)].sum(1)).ravel())
    assert cnt.select_genes(keeps["none"]).G == 0 and cnt.select_genes(keeps["none"]).nnz == 0
    lst = np.flatnonzero(half)
    for keep in (lst, list(lst), torch.as_tensor(lst), lst.astype(np.int32)):
        _same_csr(cnt.select_genes(keep), a[:, lst], cnt.data.dtype)
    assert torch.equal(cnt.select_genes(half).indices, cnt.select_genes(half).indices)
    # the selection of a selection, and its statistics
    sub = cnt.select_genes(half)
    if sub.G > 2:
        k2 = rng.random(sub.G) < 0.5
        _same_csr(sub.select_genes(k2), a[:, lst][:, np.flatnonzero(k2)], cnt.data.dtype)
        assert _same_bits(ops.csr_gene_stats(sub).cpu().numpy(), _scipy_stats(a[:, lst]))


def test_select_genes_of_a_layer_with_next_to_nothing_stored(ops):
    a = sp.csr_matrix(np.array([[0, 3, 0, 0], [0, 0, 0, 0], [9, 0, 0, 2]]))
    cnt = _device(ops, a, "u8")
    for keep in ([True, False, False, True], [False, True, False, False], [False, False, True, False]):
        keep = np.array(keep)
        _same_csr(cnt.select_genes(keep), a[:, np.flatnonzero(keep)], torch.uint8)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_selected_layer_is_a_valid_pooling_operand(ops, dtype):
    """knn_pool_csr on the selected layer (slab table rebuilt, padding contract kept) against pooling the selected dense layer."""
    rng = np.random.default_rng(5)
    C, G, k = 150, 5001, 9
    a = sp.csr_matrix((rng.poisson(1.5, (C, G)) * (rng.random((C, G)) < 0.1)).astype(np.int64))
    cnt = _device(ops, a, "u8")
    scale = torch.as_tensor(rng.gamma(4.0, 0.25, C))
    lens = rng.integers(1, k + 2, C)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([rng.choice(C, n, replace=False) for n in lens]).astype(np.int32)
    w = rng.random(indices.size)
    for keep in (rng.random(G) < 0.45, np.arange(G) == 4000, np.arange(G) < 3):          # the last two leave fewer than 4 stored elements or few
        sub = cnt.select_genes(keep)
        dense = ops.CountMatrix.from_genes_major(np.ascontiguousarray(a[:, np.flatnonzero(keep)].toarray().T))
        ref = ops.knn_pool_counts(dense, None, scale, None, indptr, indices, w, dtype=dtype)
        got = ops.knn_pool_csr(sub, scale, indptr, indices, w, dtype=dtype)
        assert torch.equal(got.t, ref.t)


# ------------------------------------------------------------------------------------------------------------------ arguments
def test_argument_validation_at_the_abi(ops, L):
    dev = ops.require_gpu()
    a = sp.csr_matrix(np.array([[0, 3, 0, 1], [2, 0, 0, 0], [9, 0, 0, 2]]))
    c = _device(ops, a, "u8")
    st = torch.empty((4, 4), dtype=torch.float64, device=dev)
    ws = torch.empty(int(L.vcy_csr_gene_stats_workspace_bytes(3, 4)) // 8, dtype=torch.int64, device=dev)
    assert ws.numel() * 8 == 4 * 24
    good = [c.indptr.data_ptr(), c._istore.data_ptr(), c._dstore.data_ptr(), c.slabptr.data_ptr(), None, st.data_ptr(), ws.data_ptr(), 3, 4, ops.U8, None]
    assert L.vcy_csr_gene_stats(*good) == 0
    for i in (0, 1, 2, 3, 5, 6):
        bad = list(good)
        bad[i] = None
        assert L.vcy_csr_gene_stats(*bad) == -1 and b"null pointer" in L.vcy_last_error()
    for code in (ops.F32, ops.F64, 17, -1):
        bad = list(good)
        bad[9] = code
        assert L.vcy_csr_gene_stats(*bad) == -1 and b"count_dtype" in L.vcy_last_error()
    assert L.vcy_csr_gene_stats(*(good[:7] + [-1, 4, ops.U8, None])) == -1
    remap = torch.tensor([0, -1, -1, 1], dtype=torch.int32, device=dev)
    row_len = torch.empty(3, dtype=torch.int64, device=dev)
    good = [c.indptr.data_ptr(), c._istore.data_ptr(), remap.data_ptr(), row_len.data_ptr(), 3, 4, None]
    assert L.vcy_csr_select_count(*good) == 0 and row_len.tolist() == [1, 1, 2]
    for i in range(4):
        bad = list(good)
        bad[i] = None
        assert L.vcy_csr_select_count(*bad) == -1 and b"null pointer" in L.vcy_last_error()
    ptr = torch.tensor([0, 1, 2, 4], dtype=torch.int64, device=dev)
    io, do = torch.empty(4, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.uint8, device=dev)
    good = [c.indptr.data_ptr(), c._istore.data_ptr(), c._dstore.data_ptr(), remap.data_ptr(), ptr.data_ptr(), io.data_ptr(), do.data_ptr(), 3, 4, ops.U8, None]
    assert L.vcy_csr_select_fill(*good) == 0 and io.tolist() == [1, 0, 0, 1] and do.tolist() == [1, 2, 9, 2]
    for i in range(7):
        bad = list(good)
        bad[i] = None
        assert L.vcy_csr_select_fill(*bad) == -1 and b"null pointer" in L.vcy_last_error()
    bad = list(good)
    bad[9] = ops.F32
    assert L.vcy_csr_select_fill(*bad) == -1 and b"count_dtype" in L.vcy_last_error()
    # the wrapper's own checks
    with pytest.raises(ValueError, match="more than one gene"):
        ops.csr_select(c, np.array([0, 0, -1, 1]), 2)
    with pytest.raises(ValueError, match="new G"):
        ops.csr_select(c, np.array([0, 2, -1, 1]), 2)
    with pytest.raises(ValueError):
        c.select_genes([2, 1])
    with pytest.raises(ValueError):
        ops.csr_gene_stats(c, np.ones(2, dtype=bool))


# ------------------------------------------------------------------------------------------------------------------ the facade
@functools.lru_cache(maxsize=None)
def _dataset():
    S, U, ix = _worker_module().make_dataset()
    for arr in (S, U, ix):
        arr.setflags(write=False)
    return S, U, ix


@functools.lru_cache(maxsize=None)
def _one_rank_route():
    """The atlas route on the whole dataset in this process: computed once, shared, never modified."""
    from velocyto_amd import atlas, ops
    wm = _worker_module()
    S, U, ix = _dataset()
    cS, cU = ops.CsrCounts.from_scipy(sp.csr_matrix(S), G=S.shape[1]), ops.CsrCounts.from_scipy(sp.csr_matrix(U), G=U.shape[1])
    res = wm.atlas_route(atlas, cS, cU, ix, 3)
    for v in res.values():
        v.setflags(write=False)
    return res


def test_the_atlas_route_equals_the_facade_bit_for_bit(ops):
    from velocyto_amd.analysis import VelocytoLoom
    wm = _worker_module()
    S, U, ix = _dataset()
    C, G = S.shape
    assert C == 600 and G == 2500 and tuple(np.bincount(ix)) == (30, 200, 370)
    # on the host first: more than N + 1 genes pass detection (and the CV filter's own detection), so that an IndexError in both routes
    # cannot pass for agreement; the dataset holds all-zero genes and genes seen in one or two cells
    det_host = (S.sum(0) >= wm.DETECTION["min_expr_counts"]) & ((S > 0).sum(0) >= wm.DETECTION["min_cells_express"])
    assert det_host.sum() > wm.N_CV + 1 + 10 and (S.sum(0) == 0).sum() >= 40 and (((S > 0).sum(0) >= 1) & ((S > 0).sum(0) <= 2)).sum() >= 40
    Sd = S[:, det_host]
    assert (((Sd > 0).sum(0) > 2) & (Sd.mean(0) < 40) & (Sd.mean(0) > 0)).sum() > wm.N_CV + 1
    res = _one_rank_route()

    vlm = VelocytoLoom.from_arrays(S.T.astype(np.float64), U.T.astype(np.float64))
    vlm.set_clusters(np.array(["a", "b", "c"])[ix])
    assert np.array_equal(vlm.cluster_ix, ix)
    vlm.score_detection_levels(**wm.DETECTION)
    assert np.array_equal(res["detection"], det_host) and np.array_equal(res["detection"], vlm.detection_level_selected)
    vlm.filter_genes(by_detection_levels=True)
    vlm.score_cv_vs_mean(N=wm.N_CV, max_expr_avg=40)
    assert _same_bits(res["cv_score"], vlm.cv_mean_score) and np.array_equal(res["cv_selected"], vlm.cv_mean_selected)
    assert wm.N_CV + 1 <= res["cv_selected"].sum() < res["cv_selected"].size
    vlm.score_cluster_expression()
    assert _same_bits(res["U_avgs"], vlm.U_avgs) and _same_bits(res["S_avgs"], vlm.S_avgs)
    assert np.array_equal(res["clu_selected"], vlm.clu_avg_selected)
    assert np.array_equal(res["S_avgs"][:, 0], Sd.sum(0) / C) and not np.array_equal(res["S_avgs"][:, 1], res["S_avgs"][:, 0])   # the small cluster
    # the whole sequence, the facade's filter_genes calls in the order of default_filter_and_norm with the same thresholds
    t = {**VelocytoLoom._default_thresholds(C), **wm.DETECTION, "N": wm.N_CV}
    vlm.filter_genes(by_cv_vs_mean=True)
    half = lambda x: int(x / 2) + 1
    vlm.score_detection_levels(min_expr_counts=0, min_cells_express=0, min_expr_counts_U=half(t["min_expr_counts"]),
                               min_cells_express_U=half(t["min_cells_express"]))
    vlm.score_cluster_expression(min_avg_U=t["min_avg_U"], min_avg_S=t["min_avg_S"])
    vlm.filter_genes(by_detection_levels=True, by_cluster_expression=True)
    assert res["kept"].dtype == np.int64 and 0 < res["kept"].size <= res["cv_selected"].sum()
    assert np.array_equal(res["kept"], vlm.ra["Gene"])
    assert np.array_equal(res["kept_row_sums"], np.stack([S[:, res["kept"]].sum(1), U[:, res["kept"]].sum(1)]))


def test_default_gene_filter_without_clusters_and_with_default_thresholds(ops):
    from velocyto_amd import atlas
    from velocyto_amd.analysis import VelocytoLoom
    S, U, _ = _dataset()
    C = S.shape[0]
    cS, cU = ops.CsrCounts.from_scipy(sp.csr_matrix(S), G=S.shape[1]), ops.CsrCounts.from_scipy(sp.csr_matrix(U), G=U.shape[1])
    fS, fU, kept = atlas.default_gene_filter(cS, cU, N=300)
    t = {**VelocytoLoom._default_thresholds(C), "N": 300}
    vlm = VelocytoLoom.from_arrays(S.T.astype(np.float64), U.T.astype(np.float64))
    vlm.score_detection_levels(min_expr_counts=t["min_expr_counts"], min_cells_express=t["min_cells_express"])
    vlm.filter_genes(by_detection_levels=True)
    vlm.score_cv_vs_mean(N=t["N"], max_expr_avg=40)
    vlm.filter_genes(by_cv_vs_mean=True)
    half = lambda x: int(x / 2) + 1
    vlm.score_detection_levels(min_expr_counts=0, min_cells_express=0, min_expr_counts_U=half(t["min_expr_counts"]),
                               min_cells_express_U=half(t["min_cells_express"]))
    vlm.filter_genes(by_detection_levels=True)
    assert np.array_equal(kept, vlm.ra["Gene"]) and kept.size > 0
    _same_csr(fS, sp.csr_matrix(S)[:, kept], cS.data.dtype)
    _same_csr(fU, sp.csr_matrix(U)[:, kept], cU.data.dtype)


def test_winsorize_is_not_implemented_on_csr_layers(ops):
    from velocyto_amd import atlas
    c = _device(ops, sp.csr_matrix(np.array([[0, 3], [1, 0]])), "u8")
    with pytest.raises(NotImplementedError, match="percentiles"):
        atlas.score_cv_vs_mean(c, winsorize=True)


# ------------------------------------------------------------------------------------------------------------------ sharded
def _run_worker(world, out, cfg, port):
    env = dict(os.environ, VCY_SINGLE_DEVICE="1", VCY_DIST_BACKEND="gloo", MASTER_PORT=str(port), MASTER_ADDR="127.0.0.1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "gene_select_worker.py"), out, json.dumps(cfg)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return dict(np.load(out))


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_selection_equals_the_one_rank_run(ops, tmp_path, world):
    """Cells sharded over 2 and 3 ranks on one GPU (gloo transport): the all-reduced integer statistics give every rank the masks,
    scores and kept list of the one-rank run, bit for bit.  With 3 ranks the last shard holds no cell of clusters 0 and 1."""
    one = _one_rank_route()
    many = _run_worker(world, str(tmp_path / "many.npz"), dict(expect_missing_cluster=(world == 3)), port=29881 + world)
    assert int(many["world"]) == world
    for name in ("detection", "cv_score", "cv_selected", "U_avgs", "S_avgs", "clu_selected", "kept"):
        ref = one[name].astype(np.float64) if one[name].dtype == bool else one[name]
        assert many[name].shape == (world,) + ref.shape, name
        for rk in range(world):
            got = many[name][rk]
            assert got.dtype == ref.dtype and np.array_equal(np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(ref).view(np.int64)), (name, rk)
    assert np.array_equal(many["kept_row_sums"], one["kept_row_sums"])
