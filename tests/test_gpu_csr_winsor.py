"""Winsorised gene selection from CSR count layers (csrc/csr_quantiles.hip, the clipped statistics of csrc/csr_select.hip ->
ops.csr_gene_quantiles / CsrGeneQuantiles, ops.csr_gene_stats(lo=, hi=) -> atlas.gene_percentiles, winsorized_gene_stats,
score_cv_vs_mean(winsor_perc=), default_gene_filter(winsor_perc=)).  Every kernel call goes through the C ABI on cuda:0.

The percentiles are order statistics of integers and the clipped moments one fixed float64 expression of integer sums, so nearly
every comparison is bit for bit: against np.percentile on the dense integer matrix, against the exact-integer formula in numpy
(tests/csr_winsor_cases.py; both pinned on the host by tests/test_csr_winsor_host.py), against the dense kernels, between cell
blockings and between the one-rank run and the ranks of a sharded one.  The two comparisons that carry a tolerance say where it
comes from.
"""
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sp = pytest.importorskip("scipy.sparse")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import csr_winsor_cases as cases  # noqa: E402

PERC = (1, 99.5)
same_bits = cases.same_bits


def _worker_module():
    spec = importlib.util.spec_from_file_location("csr_winsor_worker", os.path.join(ROOT, "tests", "csr_winsor_worker.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd  # noqa: F401
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


@pytest.fixture(scope="module")
def atlas(ops):
    from velocyto_amd import atlas as _atlas
    return _atlas


def _mask(C, kind):
    if kind == "all":
        return None
    rng = np.random.default_rng(C)
    m = rng.random(C) < 0.6
    m[rng.integers(C)] = True
    return m


# ------------------------------------------------------------------------------------------------------------------ 1. percentiles
def test_the_launch_edges_are_where_the_cases_sit(ops):
    import velocyto_amd  # noqa: F401
    from velocyto_amd import _lib
    L = _lib.lib()
    assert int(L.vcy_csr_quantiles_block_cells()) == 4096 and int(L.vcy_csr_gene_stats_block_cells()) == 2048 and int(L.vcy_csr_slab_genes()) == 2048
    assert L.vcy_csr_quantiles_passes(ops.U8) == 1 and L.vcy_csr_quantiles_passes(ops.U16) == 2
    # the state held: G x 256 uint32 x (1 + distinct ranks) for uint16 counts, one table for uint8, and two words per rank and gene
    assert L.vcy_csr_quantiles_hist_bytes(30000, 4, ops.U16) == 30000 * 256 * 4 * 5 and L.vcy_csr_quantiles_hist_bytes(30000, 4, ops.U8) == 30000 * 256 * 4
    assert L.vcy_csr_quantiles_state_bytes(30000, 4) == 30000 * 4 * 8


@pytest.mark.parametrize("masked", ["all", "masked"])
@pytest.mark.parametrize("wide", [False, True], ids=["u8", "u16"])
@pytest.mark.parametrize("C,G", cases.SIZE_PAIRS)
def test_percentiles_equal_np_percentile_bit_for_bit(ops, C, G, wide, masked):
    rng = np.random.default_rng(C * 31 + G + wide)
    dense = cases.random_dense(rng, C, G, wide)
    mask = _mask(C, masked)
    cnt = cases.device_layer(ops, dense, wide)
    for name, qs in cases.PERCENTILE_SETS.items():
        got = ops.csr_gene_quantiles(cnt, qs, mask)
        assert got.dtype == torch.float64 and tuple(got.shape) == (len(qs), G)
        assert same_bits(got.cpu().numpy(), cases.np_percentiles(dense, qs, mask)), name


# ------------------------------------------------------------------------------------------------------------------ 2. constructed genes
@pytest.mark.parametrize("wide", [False, True], ids=["u8", "u16"])
def test_constructed_genes(ops, wide):
    dense, cells = cases.constructed_dense(wide)
    C, G = dense.shape
    assert (dense > 0).sum(1).max() > 192                                      # the tail loop of the element walk
    rng = np.random.default_rng(5)
    stored_zeros = rng.random(dense.shape) < 0.3                               # explicitly stored zeros, in the all-zero gene too
    one_cell = np.zeros(C, dtype=bool)
    one_cell[cells[0]] = True
    sets = dict(cases.PERCENTILE_SETS, straddle=(50.25,), shared=(50.25, 50.3, 49.9))
    if wide:                                                                   # what the genes were built for, on the host first
        ref = cases.np_percentiles(dense, (50.25,))[0]
        assert ref[5] > 0 and np.percentile(dense[:, 5], 50) == 0              # rank 100 is a zero, rank 101 a positive count
        assert 0x00FF < ref[6] < 0x0100                                        # the two ranks differ in the high byte
        assert set(dense[:, 4]) == {0x00FF, 0x0100, 0x01FF, 0xFF00, 0xFFFF} and set(dense[:, 3]) == {255, 256, 257}
    for zeros in (None, stored_zeros):
        cnt = cases.device_layer(ops, dense, wide, zeros)
        assert cnt.nnz == int(((dense > 0) | (zeros if zeros is not None else False)).sum())
        for mask in (None, _mask(C, "masked"), one_cell):
            for name, qs in sets.items():
                got = ops.csr_gene_quantiles(cnt, qs, mask).cpu().numpy()
                assert same_bits(got, cases.np_percentiles(dense, qs, mask)), (name, zeros is not None)
            if mask is one_cell:
                assert np.array_equal(got[0], dense[cells[0]].astype(np.float64))
        lo, hi = ops.csr_gene_quantiles(cnt, PERC)
        assert same_bits(ops.csr_gene_stats(cnt, None, lo, hi).cpu().numpy(), cases.clipped_stats(dense, lo.cpu().numpy(), hi.cpu().numpy()))
        assert torch.equal(ops.csr_gene_stats(cnt), ops.csr_gene_stats(cases.device_layer(ops, dense, wide)))


# ------------------------------------------------------------------------------------------------------------------ 3. the dense select
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("wide", [False, True], ids=["u8", "u16"])
def test_percentiles_equal_the_dense_kernel_bit_for_bit(ops, wide, dtype):
    rng = np.random.default_rng(77 + wide)
    C, G = 700, 130
    dense = cases.random_dense(rng, C, G, wide)
    cnt = cases.device_layer(ops, dense, wide)
    M = ops.CellMatrix.from_cells_major(dense.astype(np.float64), dtype=getattr(torch, dtype))
    for qs in (PERC, (0, 100), (50,), (5, 33.3, 50.25, 66.6, 99)):
        assert torch.equal(ops.csr_gene_quantiles(cnt, qs), ops.gene_quantiles(M, list(qs)))
    keep = _mask(C, "masked")
    assert torch.equal(ops.csr_gene_quantiles(cnt, PERC, keep), ops.gene_quantiles(ops.select_cells(M, torch.as_tensor(keep)), list(PERC)))
    assert torch.equal(ops.csr_gene_quantiles(cnt, PERC), ops.gene_quantiles(cnt.to_dense().to_float(getattr(torch, dtype)), list(PERC)))


# ------------------------------------------------------------------------------------------------------------------ 4. winsorised statistics
@pytest.mark.parametrize("masked", ["all", "masked"])
@pytest.mark.parametrize("wide", [False, True], ids=["u8", "u16"])
@pytest.mark.parametrize("C,G", [(201, 2049), (2001, 300), (2049, 7), (4097, 130), (65, 4100), (1, 7)])
def test_winsorised_statistics(ops, C, G, wide, masked):
    rng = np.random.default_rng(C + 3 * G + wide)
    dense = cases.random_dense(rng, C, G, wide)
    mask = _mask(C, masked)
    n = C if mask is None else int(mask.sum())
    cnt = cases.device_layer(ops, dense, wide)
    lo_t, hi_t = ops.csr_gene_quantiles(cnt, PERC, mask)
    lo, hi = lo_t.cpu().numpy(), hi_t.cpu().numpy()
    got_t = ops.csr_gene_stats(cnt, mask, lo=lo_t, hi=hi_t)
    got = got_t.cpu().numpy()
    assert got_t.dtype == torch.float64 and got.shape == (4, G)
    # the reference formula, and its integer parts, bit for bit
    parts = ops.csr_gene_stats_parts(cnt, mask, lo_t, hi_t)
    assert parts.dtype == torch.int64 and np.array_equal(parts.cpu().numpy(), cases.integer_parts(dense, lo, hi, mask))
    assert same_bits(got, cases.clipped_stats(dense, lo, hi, mask))
    assert torch.equal(got_t, ops.csr_gene_stats_clip(parts, n, lo_t, hi_t)) and torch.equal(got_t, ops.csr_gene_stats(cnt, mask, lo=lo, hi=hi))
    # the dense kernel
    ref = ops.gene_stats(cnt.to_dense(), lo=lo_t, hi=hi_t, cell_mask=mask).cpu().numpy()
    assert np.array_equal(got[2:], ref[2:])
    if masked == "all" and C in (201, 2001):
        # (C - 1) q / 100 is an integer in float64 for both percentiles: the bounds are counts, every sum an exact integer below 2^53
        assert np.array_equal(lo, np.rint(lo)) and np.array_equal(hi, np.rint(hi))
        assert same_bits(got, ref)
    else:
        # the dense kernel rounds once per cell (n non-negative terms: at most n x 2^-53 relative), the formula four times; some slack
        tol = (n + 8) * 2.0 ** -53
        err = np.abs(got[:2] - ref[:2]) / np.maximum(ref[:2], 1e-300)
        print(f"C={C} G={G}: worst relative difference to the dense kernel {err.max() / 2.0 ** -53:.2f} x 2^-53, bound {n + 8}")
        assert np.all(np.abs(got[:2] - ref[:2]) <= tol * ref[:2])
    # no bounds: today's statistics, whichever way they are asked for
    plain = ops.csr_gene_stats(cnt, mask)
    assert torch.equal(plain, ops.csr_gene_stats_clip(ops.csr_gene_stats_parts(cnt, mask), n))
    assert same_bits(plain.cpu().numpy(), cases.clipped_stats(dense, None, None, mask))


# ------------------------------------------------------------------------------------------------------------------ 5. order independence
@pytest.mark.parametrize("wide", [False, True], ids=["u8", "u16"])
def test_cell_blocking_and_repetition_do_not_change_a_bit(ops, wide):
    rng = np.random.default_rng(91 + wide)
    C, G = 4500, 2100
    dense = cases.random_dense(rng, C, G, wide)
    mask = _mask(C, "masked")
    whole = cases.device_layer(ops, dense, wide)
    qs = cases.Q16
    one = ops.csr_gene_quantiles(whole, qs, mask)
    assert torch.equal(one, ops.csr_gene_quantiles(whole, qs, mask))
    assert same_bits(one.cpu().numpy(), cases.np_percentiles(dense, qs, mask))
    # three uneven pieces, each with a select of its own as a rank would hold it: the histograms of a pass are added, every piece gets
    # the sum, and only then is the next digit fixed
    cuts = [0, 37, 4133, C]
    pieces = [cases.device_layer(ops, dense[a:b], wide) for a, b in zip(cuts[:-1], cuts[1:])]
    masks = [mask[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    n = int(mask.sum())
    sels = [ops.CsrGeneQuantiles(G, qs, n, wide) for _ in pieces]
    assert sels[0].passes == (2 if wide else 1) and sels[0].state_bytes == sels[0].state.numel() * 4 + sels[0].hist.numel() * 4
    while not sels[0].done:
        for s, p, m in zip(sels, pieces, masks):
            s.add_block(p, m)
        total = sum(s.pass_hist.clone() for s in sels)
        cells = sum(s.cells_in_pass for s in sels)
        for s in sels:
            s.pass_hist.copy_(total)
            s.cells_in_pass = cells
            s.advance()
    for s in sels:
        assert torch.equal(s.result(), one)
    # the integer parts of the clipped statistics likewise
    lo, hi = ops.csr_gene_quantiles(whole, PERC, mask)
    parts = [ops.csr_gene_stats_parts(p, m, lo, hi) for p, m in zip(pieces, masks)]
    summed = torch.cat([sum(p[:5] for p in parts), torch.stack([p[5] for p in parts]).max(0).values[None]])
    assert torch.equal(summed, ops.csr_gene_stats_parts(whole, mask, lo, hi))
    assert torch.equal(ops.csr_gene_stats_clip(summed, n, lo, hi), ops.csr_gene_stats(whole, mask, lo, hi))


@functools.lru_cache(maxsize=None)
def _dataset():
    S, U_ = cases.selection_dataset()
    S.setflags(write=False)
    U_.setflags(write=False)
    return S, U_


@functools.lru_cache(maxsize=None)
def _one_rank_route():
    from velocyto_amd import atlas, ops
    wm = _worker_module()
    S, _ = _dataset()
    cS = ops.CsrCounts.from_scipy(sp.csr_matrix(S), G=S.shape[1])
    res = wm.winsor_route(atlas, cS, wm.cell_mask(S.shape[0]))
    for v in res.values():
        v.setflags(write=False)
    return res


def test_sharded_run_equals_the_one_rank_run(ops, tmp_path):
    """Cells sharded over 3 ranks on one GPU (gloo transport); the first shard holds uint16 counts, the others uint8.  The all-reduced
    histograms and integer parts give every rank the one-rank arrays, bit for bit."""
    one = _one_rank_route()
    S, _ = _dataset()
    wm = _worker_module()
    assert same_bits(one["percentiles"], cases.np_percentiles(S, cases.Q16))
    assert same_bits(one["bounds_masked"], cases.np_percentiles(S, (2.5, 97.25), wm.cell_mask(S.shape[0])))
    world, out, port = 3, str(tmp_path / "many.npz"), 29893
    env = dict(os.environ, VCY_SINGLE_DEVICE="1", VCY_DIST_BACKEND="gloo", MASTER_PORT=str(port), MASTER_ADDR="127.0.0.1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "csr_winsor_worker.py"), out]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    many = dict(np.load(out))
    assert int(many["world"]) == world and set(many) == set(one) | {"world"}
    for name, ref in one.items():
        ref = ref.astype(np.float64)
        assert many[name].shape == (world,) + ref.shape, name
        for rk in range(world):
            assert same_bits(many[name][rk], ref), (name, rk)


# ------------------------------------------------------------------------------------------------------------------ 6. end to end
def test_score_cv_vs_mean_against_the_reference_output(ops, atlas, golden):
    """The golden vectors are the reference's own output; the bars are those test_gpu_preprocess.py::test_filters_and_scores holds the
    dense facade to: scores within 5e-3 (libsvm's stopping tolerance), at most max(2, 2 % of N) = 3 genes differing in the mask."""
    g = golden("preprocess")
    S = g["S"][g["genes_after_detection"]].astype(np.int64)                    # (genes, cells)
    c = ops.CsrCounts.from_scipy(sp.csr_matrix(S.T), G=S.shape[0])
    score, selected = atlas.score_cv_vs_mean(c, N=150, max_expr_avg=40, winsor_perc=PERC, svr_gamma=0.4)
    diff = np.abs(score - g["cv_mean_score_winsor"]).max()
    n_diff = int((selected != g["cv_mean_selected_winsor"]).sum())
    print(f"score: worst absolute difference {diff:.3e} (bar 5e-3); mask: {n_diff} genes differ (bar 3)")
    assert score.shape == g["cv_mean_score_winsor"].shape and diff <= 5e-3
    assert selected.shape == g["cv_mean_selected_winsor"].shape and n_diff <= max(2, int(0.02 * 150))


def _facade(S, U_):
    from velocyto_amd.analysis import VelocytoLoom
    return VelocytoLoom.from_arrays(S.T.astype(np.float64), U_.T.astype(np.float64))


def test_score_and_filter_equal_the_facade_bit_for_bit(ops, atlas):
    S, U_ = _dataset()
    C, G = S.shape
    assert (C, G) == (2001, 300)
    cS, cU = ops.CsrCounts.from_scipy(sp.csr_matrix(S), G=G), ops.CsrCounts.from_scipy(sp.csr_matrix(U_), G=G)
    vlm = _facade(S, U_)
    vlm.score_cv_vs_mean(N=cases.N_CV, max_expr_avg=40, winsorize=True, winsor_perc=PERC)
    one = _one_rank_route()
    assert same_bits(one["cv_score"], vlm.cv_mean_score) and np.array_equal(one["cv_selected"], vlm.cv_mean_selected)
    assert cases.N_CV + 1 <= one["cv_selected"].sum() < G
    plain = atlas.score_cv_vs_mean(cS, N=cases.N_CV, max_expr_avg=40)
    assert not np.array_equal(plain[1], one["cv_selected"])                   # the cells of extreme counts do move the selection
    # the reference's upgrade of min_expr_cells (with the gene count, as it has it) is applied: 0.5 % of 2001 cells is above the default 2
    moments = atlas.winsorized_gene_stats(cS, PERC)[0]
    from velocyto_amd.preprocess import cv_vs_mean_from_stats
    up = cv_vs_mean_from_stats(atlas.gene_stats(cS), C, N=cases.N_CV, min_expr_cells=int(np.ceil(0.5 * G * 0.01)) + 2, max_expr_avg=40, moments=moments)
    assert same_bits(up[0], one["cv_score"])
    # the whole filter, the facade's calls in the order of default_filter_and_norm with the winsorised step in the middle
    fS, fU, kept = atlas.default_gene_filter(cS, cU, N=cases.N_CV, winsor_perc=PERC, **cases.DETECTION)
    t = {**type(vlm)._default_thresholds(C), **cases.DETECTION, "N": cases.N_CV}
    vlm = _facade(S, U_)
    vlm.score_detection_levels(min_expr_counts=t["min_expr_counts"], min_cells_express=t["min_cells_express"])
    vlm.filter_genes(by_detection_levels=True)
    vlm.score_cv_vs_mean(N=t["N"], max_expr_avg=40, winsorize=True, winsor_perc=PERC)
    vlm.filter_genes(by_cv_vs_mean=True)
    half = lambda x: int(x / 2) + 1
    vlm.score_detection_levels(min_expr_counts=0, min_cells_express=0, min_expr_counts_U=half(t["min_expr_counts"]),
                               min_cells_express_U=half(t["min_cells_express"]))
    vlm.filter_genes(by_detection_levels=True)
    assert np.array_equal(kept, vlm.ra["Gene"]) and 0 < kept.size < G and fS.G == fU.G == kept.size
    assert not np.array_equal(kept, atlas.default_gene_filter(cS, cU, N=cases.N_CV, **cases.DETECTION)[2])


# ------------------------------------------------------------------------------------------------------------------ 7. interface
def test_interface(ops, atlas):
    S, U_ = _dataset()
    S, U_ = S[:400], U_[:400]
    cS, cU = ops.CsrCounts.from_scipy(sp.csr_matrix(S), G=S.shape[1]), ops.CsrCounts.from_scipy(sp.csr_matrix(U_), G=S.shape[1])
    for bad in ((99.5, 1), (1,), (1, 50, 99), (-1, 99), (1, 100.5), (1, float("nan")), 5, "ab"):
        with pytest.raises(ValueError, match="winsor_perc"):
            atlas.score_cv_vs_mean(cS, N=50, winsor_perc=bad)
        with pytest.raises(ValueError, match="winsor_perc"):
            atlas.winsorized_gene_stats(cS, bad)
        with pytest.raises(ValueError, match="winsor_perc"):
            atlas.default_gene_filter(cS, cU, N=50, winsor_perc=bad)
    wrong = np.ones(cS.C + 1, dtype=bool)
    for call in (lambda: ops.csr_gene_quantiles(cS, PERC, wrong), lambda: atlas.gene_percentiles(cS, PERC, wrong),
                 lambda: atlas.winsorized_gene_stats(cS, PERC, wrong), lambda: ops.csr_gene_stats_parts(cS, wrong),
                 lambda: ops.csr_gene_stats(cS, wrong, lo=np.zeros(cS.G), hi=np.ones(cS.G))):
        with pytest.raises(ValueError, match="cell_mask"):
            call()
    with pytest.raises(ValueError, match="no cell"):
        ops.csr_gene_quantiles(cS, PERC, np.zeros(cS.C, dtype=bool))
    with pytest.raises(ValueError, match="no cell"):
        atlas.gene_percentiles(cS, PERC, np.zeros(cS.C, dtype=bool))
    for qs in ((), (101,), (-0.5, 50), (float("nan"),), tuple(range(17))):
        with pytest.raises(ValueError):
            ops.csr_gene_quantiles(cS, qs)
    with pytest.raises(ValueError, match="together"):
        ops.csr_gene_stats(cS, lo=np.zeros(cS.G))
    with pytest.raises(ValueError, match="per gene"):
        ops.csr_gene_stats(cS, lo=np.zeros(3), hi=np.zeros(3))
    with pytest.raises(NotImplementedError, match="winsor_perc="):
        atlas.score_cv_vs_mean(cS, N=50, winsorize=True)
    # winsor_perc alone switches it on; winsorize beside it changes nothing
    a = atlas.score_cv_vs_mean(cS, N=50, max_expr_avg=40, winsor_perc=PERC)
    b = atlas.score_cv_vs_mean(cS, N=50, max_expr_avg=40, winsor_perc=PERC, winsorize=True)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    # None: the functions as they were
    from velocyto_amd.preprocess import cv_vs_mean_from_stats
    old = cv_vs_mean_from_stats(atlas.gene_stats(cS), cS.C, N=50, max_expr_avg=40)
    new = atlas.score_cv_vs_mean(cS, N=50, max_expr_avg=40, winsor_perc=None)
    assert same_bits(old[0], new[0]) and np.array_equal(old[1], new[1]) and not same_bits(new[0], a[0])
    k0 = atlas.default_gene_filter(cS, cU, N=50, **cases.DETECTION)
    k1 = atlas.default_gene_filter(cS, cU, N=50, winsor_perc=None, **cases.DETECTION)
    assert np.array_equal(k0[2], k1[2]) and torch.equal(k0[0].data, k1[0].data) and torch.equal(k0[1].indices, k1[1].indices)
    # percentile values and moments come back as host arrays
    p, (m, bnd) = atlas.gene_percentiles(cS, PERC), atlas.winsorized_gene_stats(cS)
    assert isinstance(p, np.ndarray) and p.shape == (2, cS.G) and m.shape == (4, cS.G) and same_bits(bnd, p)
