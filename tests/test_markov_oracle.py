"""The long-double references of stage E/F and the Markov chain (oracle.transition_prob_reference, markov_reference,
markov_factors_reference, gauss_step_reference) pinned on the oracle's f64 restatements of the reference and on the golden vectors,
before test_gpu_markov_kernels.py holds a kernel to them; and the constants of that file's bounds (markov_cases.MARKOV_K, TP_C),
measured here on the CPU."""
import numpy as np
import pytest

import markov_cases as mc

f64 = lambda a: np.asarray(a, dtype=np.float64)


def test_markov_reference_against_the_f64_restatement(oracle):
    P, emb = mc.prepare_problem(600, 2, empty_row=True)
    for direction in ("forward", "backwards"):
        Pd = mc.directed(P, direction)
        ref = oracle.markov_reference(Pd.indptr, Pd.indices, Pd.data, emb, 0.9, 1.6)
        with np.errstate(all="ignore"):
            want = oracle.prepare_markov(P.toarray(), emb, 0.9, 1.6, direction)
        empty = np.flatnonzero(np.diff(Pd.indptr) == 0)
        assert (empty.size == 1) == (direction == "forward")                      # row 2 of P; its transpose has no empty row here
        assert np.array_equal(np.isnan(f64(ref)), np.isnan(want))
        assert np.isnan(want[empty]).all() and np.isnan(want).sum() == empty.size * 600
        ok = ~np.isnan(want)
        np.testing.assert_allclose(f64(ref)[ok], want[ok], rtol=1e-13, atol=0)
        assert float(np.abs(ref[ok].reshape(-1, 600).sum(1) - 1).max()) < 1e-17
    assert P[7, 7] == 50.0 and P[5].nnz == 1 and P[3].nnz == 300                 # the case stores diagonals of every kind


def test_markov_reference_against_the_golden_chain(oracle, golden):
    from scipy import sparse
    g = golden("pipeline")
    for direction in ("forward", "backwards"):
        Pd = mc.directed(sparse.csr_matrix(g["transition_prob"]), direction)
        ref = oracle.markov_reference(Pd.indptr, Pd.indices, Pd.data, g["ts"], 2.0, 4.0)
        np.testing.assert_allclose(f64(ref), g[f"tr_{direction}"], rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("edim", [1, 2, 3, 4])
def test_gauss_step_reference_is_a_step_of_the_dense_chain(oracle, edim):
    p = mc.chain_problem(257, edim, 100.0)
    args = (p["indptr"], p["indices"], p["pval"], p["emb"], mc.SIGMA_D, mc.SIGMA_W)
    tr = oracle.markov_reference(*args)
    colptr, rowidx, scsc, tot, kw = oracle.markov_factors_reference(*args)
    es = oracle.markov_scaled_coords(p["emb"], mc.SIGMA_W)
    y, S = oracle.gauss_step_reference(p["x"], tot, kw, colptr, rowidx, scsc, es, mc.SIGMA_W)
    want = np.asarray(p["x"], dtype=np.longdouble) @ tr
    assert float((np.abs(y - want) / want).max()) < 1e-15
    assert np.all(S > 0)
    assert int(np.diff(colptr).max()) > 200                                       # cell 1's column


def test_transition_prob_reference_against_the_f64_restatement_and_golden(oracle, golden):
    g = golden("pipeline")
    ixs, emb, corr = g["neigh_ixs"], g["ts"], g["corrcoef_sqrt"]
    C = corr.shape[0]
    compact = corr[np.arange(C)[:, None], ixs]
    tp, wd, de, cond = oracle.transition_prob_reference(compact, ixs, emb, 0.05)
    dense = np.zeros((C, C))
    dense[np.arange(C)[:, None], ixs] = f64(tp)
    np.testing.assert_allclose(dense, g["transition_prob"], rtol=1e-12, atol=1e-15)
    tp2, _, de2, _ = oracle.transition_prob_reference(compact, ixs, emb, 0.1)
    np.testing.assert_allclose(f64(de2), g["delta_embedding_noscale"], rtol=1e-9, atol=1e-12)
    tpo, deo, _ = oracle.calculate_embedding_shift(corr, ixs, emb, sigma_corr=0.1, expression_scaling=False)
    np.testing.assert_allclose(f64(de2), deo, rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(f64(tp2), tpo[np.arange(C)[:, None], ixs], rtol=1e-13)
    np.testing.assert_allclose(f64(cond), np.abs(f64(tp) - 1.0 / ixs.shape[1]).sum(1), rtol=1e-12)
    # a block of rows with global indices, a list that names its own cell, and a twin: rows of the full answer
    sub = slice(41, 60)
    tps, wds, des, _ = oracle.transition_prob_reference(compact[sub], ixs[sub], emb, 0.05, cell0=41)
    assert np.array_equal(tps, tp[sub]) and np.array_equal(des, de[sub])
    cs = next(c for c in mc.tp_cases("float64", 0.005) if c["n"] == 65 and c["C_out"] == 130)
    assert np.isnan(f64(cs["de"][0])).all() and not np.isnan(f64(cs["de"][2:])).any()      # cell0 and its twin: only they can list each other
    assert np.isfinite(f64(cs["tp"])).all() and float(np.abs(cs["tp"].sum(1) - 1).max()) < 1e-17   # exp(200) never formed


def test_the_k_of_the_step_bound_is_what_the_cpu_measures(oracle):
    """K of test_gpu_markov_kernels.py's bound 4 K u S_j: the largest |emulated - reference| / (u S_j) of the Gaussian half of one
    factored step in numpy arithmetic of the compute type, over M = 6 ... 1e4 and edim 1 ... 4 at n = 600 (markov_cases.MARKOV_K says what is seen)."""
    for dtype in ("float32", "float64"):
        k, rel = 0.0, {}
        for M in mc.SWEEP_M:
            for edim in (1, 2, 3, 4):
                p = mc.chain_problem(600, edim, M)
                fac = oracle.markov_factors_reference(p["indptr"], p["indices"], p["pval"], p["emb"], mc.SIGMA_D, mc.SIGMA_W)
                colptr, rowidx, scsc, tot, kw = (f64(a) if a.dtype == np.longdouble else a for a in fac)
                es = f64(oracle.markov_scaled_coords(p["emb"], mc.SIGMA_W))
                y, S = oracle.gauss_step_reference(p["x"], tot, kw, colptr, rowidx, scsc, es, mc.SIGMA_W)
                ys, T, terms = oracle.sparse_half_reference(p["x"], tot, colptr, rowidx, scsc)
                gg = oracle.gauss_step_emulated(p["x"], tot, kw, colptr, rowidx, scsc, es, mc.SIGMA_W, dtype, gauss_only=True)
                k = max(k, float((f64(np.abs(gg - (y - ys))) / (mc.U[dtype] * f64(S))).max()))
                got = oracle.gauss_step_emulated(p["x"], tot, kw, colptr, rowidx, scsc, es, mc.SIGMA_W, dtype)
                err = f64(np.abs(got - y))
                assert np.all(err <= mc.step_bound(S, dtype, 600, 0.0, None, T, terms))        # the whole step is inside its whole bound
                rel[M] = max(rel.get(M, 0.0), float((err / f64(y)).max()))
        print(dtype, "measured K", k, "worst relative error per M", rel)
        assert mc.MARKOV_K[dtype] / 1.1 <= k <= mc.MARKOV_K[dtype]
        if dtype == "float32":                                                    # the error follows M: the figures DESIGN section 12 quotes
            r = [rel[M] for M in mc.SWEEP_M]                                      # (the exact figures depend on numpy's float32 exp2)
            assert all(a < b for a, b in zip(r, r[1:])) and all(rel[M] <= 1.5 * mc.F32_REL[M] for M in mc.SWEEP_M), rel
            assert rel[1e4] >= 1e3 * rel[6.0]


def test_the_c_of_the_delta_embedding_bound_is_what_the_cpu_measures(oracle):
    c, ulps = 0.0, 0.0
    for dtype in ("float32", "float64"):
        for sigma in (0.05, 0.005):
            for cs in mc.tp_cases(dtype, sigma):
                p, de = mc.tp_formula_f64(cs["corr"], cs["ixs"], cs["emb"], sigma, cs["cell0"])
                ref = f64(cs["de"])
                assert np.array_equal(np.isnan(de), np.isnan(ref))
                ulps = max(ulps, float((f64(np.abs(p - cs["tp"])) / mc.ulp(cs["tp"], "float64")).max()))
                ok = ~np.isnan(ref).any(1) & (f64(cs["cond"]) > 0)
                if ok.any():
                    err = f64(np.abs(de - cs["de"]))[ok].max(1)
                    c = max(c, float((err / (cs["n"] * 2.0 ** -53 * f64(cs["cond"])[ok])).max()))
    print("measured c", c, "worst f64 ulps of tp in the device's formula", ulps)
    assert mc.TP_C / 1.1 <= c <= mc.TP_C
    assert ulps < 4.0                                                                 # (2.3: the formula can meet the 4 ulps it is held to)
