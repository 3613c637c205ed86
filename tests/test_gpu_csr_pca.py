"""PCA straight from CSR count layers (csrc/csr_pca.hip -> ops.LogNormCsr -> DevicePCA.fit_transform_csr -> atlas.pca_from_counts).
Every kernel call goes through the C ABI on cuda:0; references are numpy / scipy.sparse / scikit-learn in float64 on the host.

Bars:
  * exact inputs (counts in {1, 3, 7, 15, 255, 65535}, scale 1, pcount 1 -> x = log2(c + 1) a small integer; integer B): every sum
    is exact in f64, so the products and the moments must equal scipy's BIT FOR BIT, in both orientations, across the chunk rule;
  * general inputs: per element (n + 2 + 2 E_LOG) 2^-53 sum_p (|log2 v_p| + |log2 pcount|) |B_pj|, n the row's stored elements:
    a rounding per accumulated term, one each for the difference log2 v - log2 pcount and the product, and E_LOG ulps (of at most
    2^-52 relative each) between the kernel's log2 and numpy's;
  * the fit against scikit-learn's full solver and against the dense subspace route at the bounds of
    test_gpu_preprocess.test_pca_subspace_iteration_matches_the_exact_route.
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

# log2 error of the kernel in ulps: the maximum measured on the device against numpy's float64 log2 over every count 1..65535 times
# seven size factors (test_direct_case_measures_the_log2_error prints it; DESIGN.md section 10 records it: 1 ulp), rounded up, plus
# 1 ulp because numpy's own log2 is within 1 ulp and not correctly rounded
E_LOG = 1 + 1


def _worker_module():
    spec = importlib.util.spec_from_file_location("csr_pca_worker", os.path.join(ROOT, "tests", "csr_pca_worker.py"))
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
def chunk():
    import velocyto_amd
    from velocyto_amd import _lib
    return int(_lib.lib().vcy_csr_spmm_chunk())


EXACT_VALUES = {"u8": np.array([1, 3, 7, 15, 255]), "u16": np.array([1, 3, 7, 15, 255, 65535])}


def _layer_from_lengths(rng, lens, N, values):
    """scipy CSR with lens[r] stored elements in row r (distinct sorted columns) drawn from `values`."""
    lens = np.minimum(np.asarray(lens, dtype=np.int64), N)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(N, n, replace=False)) for n in lens] + [np.empty(0, dtype=np.int64)]).astype(np.int32)
    data = rng.choice(values, int(indptr[-1])).astype(np.int64)
    return sp.csr_matrix((data, indices, indptr), shape=(len(lens), N))


def _row_lengths(rng, R, N):
    """Rows with 0, 1, 3, 4, 5 and 200 stored elements (what fits N), then random lengths."""
    lens = [0, 1, 3, 4, 5, 200, 0, 64, 65, 63][:R]
    lens += list(rng.integers(0, min(N, 40) + 1, R - len(lens)))
    return rng.permutation(np.minimum(lens, N)) if R > 1 else np.array([min(3, N)])


def _device(ops, a, width):
    c = ops.CsrCounts.from_scipy(a, G=a.shape[1], narrow=(width == "u8"))
    assert c.data.dtype == (torch.uint8 if width == "u8" else torch.int16)
    return c


def _x_of(a, s_rows, pc):
    """The transformed layer on the host: scipy CSR of log2(c * s + pc) - log2(pc) over the stored elements (s per row)."""
    a = sp.csr_matrix(a, dtype=np.float64)
    v = a.data * np.repeat(s_rows, np.diff(a.indptr)) + pc
    return sp.csr_matrix((np.log2(v) - np.log2(pc), a.indices, a.indptr), shape=a.shape), v


def _int_B(rng, N, L):
    return rng.integers(-8, 9, (N, L)).astype(np.float64)


@pytest.mark.parametrize("width", ["u8", "u16"])
@pytest.mark.parametrize("L", [1, 2, 7, 50, 64, 65, 70])
@pytest.mark.parametrize("R,N", [(1, 5), (37, 130), (300, 1153)])
def test_exact_inputs_match_scipy_bit_for_bit_in_both_orientations(ops, R, N, L, width):
    rng = np.random.default_rng(R * 131 + L * 7 + (width == "u16"))
    a = _layer_from_lengths(rng, _row_lengths(rng, R, N), N, EXACT_VALUES[width])
    x, _ = _x_of(a, np.ones(R), 1.0)
    assert np.array_equal(x.data, np.rint(x.data))
    cnt = _device(ops, a, width)
    dev = cnt.indptr.device
    one_r = torch.ones(R, dtype=torch.float64, device=dev)
    # rows = cells: the projection, scale taken by row
    B = _int_B(rng, N, L)
    out = ops.csr_lognorm_spmm(cnt, one_r, torch.as_tensor(B, device=dev), scale_on="row")
    assert np.array_equal(out.cpu().numpy(), x @ B)
    # the gene-major copy: the contraction, scale taken by index
    cntT = cnt.transposed()
    assert (cntT.C, cntT.G, cntT.nnz) == (N, R, cnt.nnz)
    B2 = _int_B(rng, R, L)
    b2 = torch.as_tensor(B2, device=dev)
    out2 = ops.csr_lognorm_spmm(cntT, one_r, b2, scale_on="index")
    assert np.array_equal(out2.cpu().numpy(), x.T.tocsr() @ B2)
    assert torch.equal(out2, ops.csr_lognorm_spmm(cntT, one_r, b2, scale_on="index"))            # the same call twice: the same bits
    # an output with padded rows and an operand that is a column slice of a wider buffer (what the fit hands over)
    wide = torch.full((R, L + 3), 7.0, dtype=torch.float64, device=dev)
    Bw = torch.zeros((N, L + 5), dtype=torch.float64, device=dev)
    Bw[:, :L] = torch.as_tensor(B, device=dev)
    ops.csr_lognorm_spmm(cnt, one_r, Bw[:, :L], scale_on="row", out=wide[:, :L])
    assert torch.equal(wide[:, :L], out) and bool((wide[:, L:] == 7.0).all())
    # the moments of both copies
    st = ops.csr_lognorm_stats(cntT, one_r).cpu().numpy()
    assert np.array_equal(st[0], np.asarray(x.sum(0)).ravel()) and np.array_equal(st[1], np.asarray(x.multiply(x).sum(0)).ravel())
    st_r = ops.csr_lognorm_stats(cnt, one_r, scale_on="row").cpu().numpy()
    assert np.array_equal(st_r[0], np.asarray(x.sum(1)).ravel()) and np.array_equal(st_r[1], np.asarray(x.multiply(x).sum(1)).ravel())


@pytest.mark.parametrize("nnz", [0, 1, 3, 4, 5])
def test_layers_with_next_to_nothing_stored(ops, nnz):
    rng = np.random.default_rng(nnz)
    R, N, L = 4, 6, 3
    dense = np.zeros(R * N, dtype=np.int64)
    dense[rng.choice(R * N, nnz, replace=False)] = rng.choice(EXACT_VALUES["u16"], nnz)
    a = sp.csr_matrix(dense.reshape(R, N))
    x, _ = _x_of(a, np.ones(R), 1.0)
    for width in ("u8", "u16"):
        if width == "u8" and dense.max() > 255:
            a8 = sp.csr_matrix(np.minimum(dense, 255).reshape(R, N))
            xa, aa = _x_of(a8, np.ones(R), 1.0)[0], a8
        else:
            xa, aa = x, a
        cnt = _device(ops, aa, width)
        dev = cnt.indptr.device
        ones = torch.ones(R, dtype=torch.float64, device=dev)
        B, B2 = _int_B(rng, N, L), _int_B(rng, R, L)
        assert np.array_equal(ops.csr_lognorm_spmm(cnt, ones, torch.as_tensor(B, device=dev)).cpu().numpy(), xa @ B)
        cntT = cnt.transposed()
        assert cntT.nnz == nnz
        assert np.array_equal(ops.csr_lognorm_spmm(cntT, ones, torch.as_tensor(B2, device=dev), scale_on="index").cpu().numpy(), xa.T.tocsr() @ B2)
        st = ops.csr_lognorm_stats(cntT, ones).cpu().numpy()
        assert np.array_equal(st[0], np.asarray(xa.sum(0)).ravel()) and np.array_equal(st[1], np.asarray(xa.multiply(xa).sum(0)).ravel())


def _chunk_layer(rng, chunk, values):
    """Cells x 9 genes whose gene-major copy has columns exactly chunk, chunk + 1 and 2 chunk + 3 long beside empty ones (and a short
    one): every way a row can meet the chunk rule - one full chunk and nothing after it, one element after it, two full chunks and a tail."""
    C = 2 * chunk + 40
    lens = {1: chunk, 3: chunk + 1, 4: 5, 6: 2 * chunk + 3, 7: chunk - 1}            # genes 0, 2, 5, 8 stay empty
    rows, cols = [], []
    for g, n in lens.items():
        rows.append(np.sort(rng.choice(C, n, replace=False)))
        cols.append(np.full(n, g))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    a = sp.csr_matrix((rng.choice(values, rows.size).astype(np.int64), (rows, cols)), shape=(C, 9))
    a.sort_indices()
    assert list(np.diff(a.tocsc().indptr)) == [0, chunk, 0, chunk + 1, 5, 0, 2 * chunk + 3, chunk - 1, 0]
    return a


@pytest.mark.parametrize("width", ["u8", "u16"])
@pytest.mark.parametrize("L", [1, 50, 70])
def test_exact_inputs_across_the_chunk_rule(ops, chunk, L, width):
    rng = np.random.default_rng(L + (width == "u16"))
    a = _chunk_layer(rng, chunk, EXACT_VALUES[width])
    C, G = a.shape
    x, _ = _x_of(a, np.ones(C), 1.0)
    cnt = _device(ops, a, width)
    dev = cnt.indptr.device
    cntT = cnt.transposed()
    t = a.T.tocsr()
    t.sort_indices()
    assert np.array_equal(cntT.indptr.cpu().numpy(), t.indptr) and np.array_equal(cntT.indices.cpu().numpy(), t.indices)
    ones = torch.ones(C, dtype=torch.float64, device=dev)
    Y = _int_B(rng, C, L)
    y = torch.as_tensor(Y, device=dev)
    out = ops.csr_lognorm_spmm(cntT, ones, y, scale_on="index")
    assert np.array_equal(out.cpu().numpy(), x.T.tocsr() @ Y)
    assert torch.equal(out, ops.csr_lognorm_spmm(cntT, ones, y, scale_on="index"))
    st = ops.csr_lognorm_stats(cntT, ones)
    assert np.array_equal(st.cpu().numpy(), np.stack([np.asarray(x.sum(0)).ravel(), np.asarray(x.multiply(x).sum(0)).ravel()]))
    assert torch.equal(st, ops.csr_lognorm_stats(cntT, ones))
    # the same long rows with the scale taken by row: the gene-major copy read as a layer of its own
    Z = _int_B(rng, C, L)
    onesG = torch.ones(G, dtype=torch.float64, device=dev)
    assert np.array_equal(ops.csr_lognorm_spmm(cntT, onesG, torch.as_tensor(Z, device=dev), scale_on="row").cpu().numpy(), x.T.tocsr() @ Z)


def _ulps(got, ref):
    return np.abs(got - ref) / np.spacing(np.abs(ref))


def test_direct_case_measures_the_log2_error(ops):
    """One stored element per row, L = 1, B = 1: the output IS the transformed value.  Every count 1..65535 times seven size factors
    against numpy's float64 log2 of the same v (products and sums rounded one by one on both sides: v is the same double)."""
    s = np.array([1.0, 0.37, 2.9, 1.0 / 3.0, 17.123, 0.0625, 1234.5])
    c = np.tile(np.arange(1, 65536), len(s))
    scale = np.repeat(s, 65535)
    R = c.size
    a = sp.csr_matrix((c, np.zeros(R, dtype=np.int32), np.arange(R + 1)), shape=(R, 1))
    cnt = _device(ops, a, "u16")
    dev = cnt.indptr.device
    out = ops.csr_lognorm_spmm(cnt, torch.as_tensor(scale, device=dev), torch.ones((1, 1), dtype=torch.float64, device=dev)).cpu().numpy()[:, 0]
    ref = np.log2(c * scale + 1.0)
    err = _ulps(out, ref)
    exact = np.log2(np.asarray(c * scale + 1.0, dtype=np.longdouble))
    print(f"\nlog2 on the device: max {err.max():.3f} ulp against numpy's float64 log2 (mean {err.mean():.4f}); against an 80-bit log2: "
          f"device max {float((np.abs(out - exact) / np.spacing(np.abs(ref))).max()):.3f} ulp, "
          f"numpy max {float((np.abs(ref - exact) / np.spacing(np.abs(ref))).max()):.3f} ulp")
    assert err.max() <= E_LOG
    # the stats entry sees the same values
    st = ops.csr_lognorm_stats(cnt, torch.as_tensor(scale, device=dev), scale_on="row").cpu().numpy()
    assert np.array_equal(st[0], out)


def _general_check(ops, a, s, pc, L, rng, width):
    """Both orientations of one layer with non-integer size factors against the host, at the bound of the module docstring."""
    C, G = a.shape
    x, v = _x_of(a, s, pc)
    absx = sp.csr_matrix((np.abs(np.log2(v)) + abs(np.log2(pc)), x.indices, x.indptr), shape=x.shape)
    cnt = _device(ops, a, width)
    dev = cnt.indptr.device
    sc = torch.as_tensor(s, device=dev)
    worst = 0.0
    for ori, m, am, c in (("row", x, absx, cnt), ("index", x.T.tocsr(), absx.T.tocsr(), cnt.transposed())):
        B = rng.normal(size=(m.shape[1], L))
        got = ops.csr_lognorm_spmm(c, sc, torch.as_tensor(B, device=dev), scale_on=ori, pcount=pc).cpu().numpy()
        n = np.diff(m.indptr)[:, None]
        bound = (n + 2 + 2 * E_LOG) * 2.0 ** -53 * (am @ np.abs(B))
        err = np.abs(got - m @ B)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (ori, float((err / np.maximum(bound, 1e-300)).max()))
    # moments of the gene-major copy: the sums as a product with B = 1; a square carries twice the relative error of its x
    st = ops.csr_lognorm_stats(cnt.transposed(), sc, pcount=pc).cpu().numpy()
    xt, at = x.T.tocsr(), absx.T.tocsr()
    n = np.diff(xt.indptr)
    s1, s2 = np.asarray(xt.sum(1)).ravel(), np.asarray(xt.multiply(xt).sum(1)).ravel()
    assert np.all(np.abs(st[0] - s1) <= (n + 2 + 2 * E_LOG) * 2.0 ** -53 * np.asarray(at.sum(1)).ravel())
    assert np.all(np.abs(st[1] - s2) <= 2 * (n + 2 + 2 * E_LOG) * 2.0 ** -53 * np.asarray(at.multiply(at).sum(1)).ravel())
    return worst


@pytest.mark.parametrize("pc", [1.0, 0.5, 3.0])
@pytest.mark.parametrize("R,N,L,width", [(300, 1153, 50, "u8"), (37, 130, 7, "u16"), (300, 1153, 65, "u16")])
def test_general_inputs_within_the_rounding_bound(ops, R, N, L, width, pc):
    rng = np.random.default_rng(int(pc * 10) + R + L)
    vals = np.arange(1, 256) if width == "u8" else np.concatenate([np.arange(1, 40), [255, 256, 4000, 65535]])
    a = _layer_from_lengths(rng, _row_lengths(rng, R, N), N, vals)
    _general_check(ops, a, np.exp(0.4 * rng.normal(size=R)), pc, L, rng, width)


@pytest.mark.parametrize("pc", [1.0, 3.0])
def test_general_inputs_across_the_chunk_rule(ops, chunk, pc):
    rng = np.random.default_rng(int(pc))
    a = _chunk_layer(rng, chunk, np.arange(1, 30))
    _general_check(ops, a, np.exp(0.4 * rng.normal(size=a.shape[0])), pc, 50, rng, "u8")


# ------------------------------------------------------------------------------------------------------------------ the fit
@functools.lru_cache(maxsize=None)
def _pca_case(C, G, r, k, pc):
    """Input, its dense log-normalised form and scikit-learn's exact PCA of it: computed once, shared, never modified."""
    from sklearn.decomposition import PCA
    S, f = _worker_module().make_input(C, G, r)
    X = np.log2(S * f[:, None] + pc)
    sk = PCA(n_components=k, svd_solver="full")
    p = sk.fit_transform(X)
    for arr in (S, f, X, p):
        arr.setflags(write=False)
    return S, f, X, sk, p


def _fit_csr(ops, S, f, k, pc):
    from velocyto_amd.preprocess import DevicePCA
    pca = DevicePCA(n_components=k)
    pcs = pca.fit_transform_csr(ops.CsrCounts.from_scipy(sp.csr_matrix(S), G=S.shape[1]), np.array(f), pcount=pc)
    assert isinstance(pcs, torch.Tensor) and pcs.is_cuda and pcs.dtype == torch.float64 and pcs.shape == (S.shape[0], k)
    return pca, pcs.cpu().numpy()


def _same_fit(pca, pcs, ref, ref_pcs):
    """The bounds of test_pca_subspace_iteration_matches_the_exact_route."""
    np.testing.assert_allclose(pca.explained_variance_, ref.explained_variance_, rtol=1e-8)
    np.testing.assert_allclose(pca.explained_variance_ratio_, ref.explained_variance_ratio_, rtol=1e-8)
    np.testing.assert_allclose(np.abs(np.sum(pca.components_ * ref.components_, 1)), 1.0, atol=1e-8)
    np.testing.assert_allclose(pca.components_, ref.components_, atol=1e-6)
    np.testing.assert_allclose(pcs, ref_pcs, atol=1e-5 * np.abs(ref_pcs).max())
    np.testing.assert_allclose(pca.mean_, ref.mean_, rtol=1e-13)


@pytest.mark.parametrize("C,G,r,k,pc", [(1500, 900, 6, 6, 1.0), (700, 1200, 5, 5, 1.0), (1500, 900, 6, 6, 0.5)])
def test_fit_from_csr_matches_sklearn_and_the_dense_subspace_route(ops, C, G, r, k, pc):
    from velocyto_amd.preprocess import DevicePCA
    S, f, X, sk, p_sk = _pca_case(C, G, r, k, pc)
    assert 0.1 < (S != 0).mean() < 0.3
    pca, pcs = _fit_csr(ops, S, f, k, pc)
    assert pca.converged_ and pca.n_iter_ < 60
    assert (pca.n_components_, pca.n_samples_, pca.n_features_in_) == (k, C, G)
    _same_fit(pca, pcs, sk, p_sk)
    np.testing.assert_allclose(pca.singular_values_, sk.singular_values_, rtol=1e-8)
    dense = DevicePCA(n_components=k, svd_solver="subspace")
    p_dense = dense.fit_transform(ops.CellMatrix.from_cells_major(np.array(X), torch.float64))
    assert dense.n_iter_ < 60
    _same_fit(pca, pcs, dense, p_dense)
    # two fits of one input: the same bits
    again, pcs2 = _fit_csr(ops, S, f, k, pc)
    assert np.array_equal(again.components_, pca.components_) and np.array_equal(pcs2, pcs) and again.n_iter_ == pca.n_iter_


def test_fit_at_the_exact_limit_of_the_block(ops):
    """k + 20 > min(C, G): the block spans the whole space, l = min(C, G), and the iteration is exact."""
    C, G, r, k = 60, 40, 5, 25
    S, f, X, sk, p_sk = _pca_case(C, G, r, k, 1.0)
    pca, pcs = _fit_csr(ops, S, f, k, 1.0)
    assert pca.n_iter_ < 60
    _same_fit(pca, pcs, sk, p_sk)


def _run_worker(world, out, cfg, port):
    env = dict(os.environ, VCY_SINGLE_DEVICE="1", VCY_DIST_BACKEND="gloo", MASTER_PORT=str(port), MASTER_ADDR="127.0.0.1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "csr_pca_worker.py"), out, json.dumps(cfg)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_fit_equals_the_one_rank_fit(ops, tmp_path, world):
    """Cells sharded over 2 and 3 ranks on one GPU (gloo transport): the all-reduced contraction, moments and column sums give every
    rank the components of the one-rank fit, and the gathered scores are its scores."""
    C, G, r, k = 1500, 900, 6, 6
    S, f, X, sk, p_sk = _pca_case(C, G, r, k, 1.0)
    one, pcs_one = _fit_csr(ops, S, f, k, 1.0)
    many = _run_worker(world, str(tmp_path / "many.npz"), dict(C=C, G=G, r=r, k=k, pcount=1.0), port=29871 + world)
    assert int(many["world"]) == world and int(many["n_iter"]) < 60
    comps = many["components_every_rank"]
    assert comps.shape == (world, k, G)
    for rk in range(1, world):
        assert np.array_equal(comps[rk], comps[0]), f"rank {rk} holds other components than rank 0"
    np.testing.assert_allclose(many["explained_variance"], one.explained_variance_, rtol=1e-8)
    np.testing.assert_allclose(many["explained_variance_ratio"], one.explained_variance_ratio_, rtol=1e-8)
    np.testing.assert_allclose(np.abs(np.sum(comps[0] * one.components_, 1)), 1.0, atol=1e-8)
    np.testing.assert_allclose(comps[0], one.components_, atol=1e-6)
    np.testing.assert_allclose(many["pcs"], pcs_one, atol=1e-5 * np.abs(pcs_one).max())
    np.testing.assert_allclose(many["mean"], one.mean_, rtol=1e-13)


def test_pcs_from_counts_feed_the_atlas_path(ops):
    """atlas.pca_from_counts -> AtlasPath(pcs=...): shapes, dtypes and layout of the hand-over.  The run equals the resident dense
    path fed the same pcs (the PCA itself is checked above)."""
    from velocyto_amd import atlas
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_atlas import _dense_reference
    dev = ops.require_gpu()
    C, G, k = 4000, 1500, 10
    cS, cU, totS, totU, _, emb = atlas.synth_atlas(C, G, 12, dev, density=0.08)
    fS, fU = atlas.size_factors(totS, totU, C)
    pcs, pca = atlas.pca_from_counts(cS, fS, n_components=10)
    assert pcs.is_cuda and pcs.dtype == torch.float64 and pcs.shape == (C, 10) and pcs.is_contiguous()
    assert pca.components_.shape == (10, G) and pca.n_samples_ == C and bool(torch.isfinite(pcs).all())
    assert np.all(np.diff(pca.explained_variance_) <= 0) and pca.explained_variance_[-1] > 0
    path = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, k=k, n_neighbors=60, sampled_fraction=0.5, block_cells=0, knn="brute")
    corr = path.run()
    Sx, Ux, gamma, neigh, ref = _dense_reference(ops, atlas, cS, cU, fS, fU, pcs, emb, k, 60, 0.5)
    assert torch.equal(path.neigh, neigh) and torch.equal(path.gamma, gamma)
    assert torch.equal(torch.nan_to_num(corr, nan=7.0), torch.nan_to_num(ref, nan=7.0))
