"""The oracle of the PCA products (tests/pca_cases.py) pinned without a GPU: the extended-precision references against exact rational
arithmetic, both of their arithmetic paths (np.longdouble where it has 64 mantissa bits, double-double everywhere), the integer cases
against int64, the case lists against what they claim to contain, and a plain numpy fp64 evaluation of every product against the derived
bounds - the bounds hold for fp64 arithmetic before any kernel is held to them."""
from fractions import Fraction

import numpy as np
import pytest

import pca_cases as pc

PATHS = ["double-double"] + (["longdouble"] if pc.HAVE_LONGDOUBLE else [])


@pytest.fixture(params=PATHS)
def path(request, monkeypatch):
    monkeypatch.setattr(pc, "FORCE_DD", request.param == "double-double")
    return request.param


def _frac(a):
    return np.vectorize(Fraction, otypes=[object])(np.asarray(a, dtype=np.float64))


def _pair_frac(pair):
    return _frac(pair[0]) + _frac(pair[1])


def _tol(path, K, S):
    """The issue's K 2^-63 S for longdouble (every tiny shape here has K + c <= 2 K), 2^-100 K S for double-double."""
    return Fraction(K) * Fraction(2) ** (-63 if path == "longdouble" else -100) * Fraction(float(S))


def _assert_close(pair, exact, S, K, path, what):
    got = _pair_frac(pair)
    for idx in np.ndindex(exact.shape):
        assert abs(got[idx] - exact[idx]) <= _tol(path, K, S[idx]), (what, idx, float(got[idx] - exact[idx]), float(S[idx]))


@pytest.mark.parametrize("C,G,L,kind", [(3, 2, 3, "recipe"), (5, 4, 2, "ill"), (17, 3, 1, "recipe"), (4, 3, 2, "exact")])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_gram_references_against_rational_arithmetic(path, C, G, L, kind, dtype):
    X, mean, Y = pc.gram_inputs(C, G, L, kind, dtype)
    Xf, Yf = _frac(X), _frac(Y)
    for m in (mean, None):
        A = Xf - _frac(mean)[None, :] if m is not None else Xf
        absA = np.vectorize(abs, otypes=[object])(A)
        ref, S = pc.gram_reference(X, m)
        exact = A.T @ A
        assert np.all(_frac(S) >= absA.T @ absA), "the absolute-term sum must not fall below the exact one"
        assert np.all(_frac(S) <= (absA.T @ absA) * (1 + Fraction(2) ** -39))
        _assert_close(ref, exact, S, C, path, "gram")
        ref, S = pc.gram_tn_reference(X, m, Y)
        _assert_close(ref, A.T @ Yf, S, C, path, "gram_tn")
    (pair, S) = pc.col_means_reference(X)
    exact = Xf.sum(0) / C
    got = _pair_frac(pair)
    for g in range(G):
        assert abs(got[g] - exact[g]) <= _tol(path, C, S[g]) + Fraction(2) ** (-63 if path == "longdouble" else -100) * abs(exact[g])


@pytest.mark.parametrize("M,N,K,kind", [(2, 3, 3, "recipe"), (3, 2, 17, "ill"), (1, 1, 5, "recipe"), (3, 3, 4, "exact")])
@pytest.mark.parametrize("ta,tb", pc.TYPE_PAIRS)
def test_gemm_nt_reference_against_rational_arithmetic(path, M, N, K, kind, ta, tb):
    A, B, rc, cc, c0 = pc.gemm_inputs(M, N, K, kind, ta, tb)
    exact = _frac(A) @ _frac(B).T
    absS = np.vectorize(abs, otypes=[object])(_frac(A)) @ np.vectorize(abs, otypes=[object])(_frac(B)).T
    ref, S = pc.gemm_nt_reference(A, B)
    _assert_close(ref, exact, S, K, path, "plain")
    if rc is not None:
        exact = exact - _frac(rc)[:, None]
        absS = absS + np.vectorize(abs, otypes=[object])(_frac(rc))[:, None]
    if cc is not None:
        exact = exact - _frac(cc)[None, :]
        absS = absS + np.vectorize(abs, otypes=[object])(_frac(cc))[None, :]
    exact, absS = exact + Fraction(c0), absS + abs(Fraction(c0))
    ref, S = pc.gemm_nt_reference(A, B, rc, cc, c0)
    assert np.all(_frac(S) >= absS)
    _assert_close(ref, exact, S, K, path, "corrected")


def test_references_are_exact_on_the_integer_cases(path):
    for C, G, L in ((1, 1, 1), (17, 5, 3), (49, 129, 65), (2049, 20, 3)):
        X, mean, Y = pc.gram_inputs(C, G, L, "exact", "float32")
        assert np.array_equal(X, np.round(X)) and np.abs(X).max() <= 8 and np.array_equal(X, pc.stored(X, "float32"))
        for centred in (True, False):
            want = pc.gram_expect(C, G, L, "exact", "float32", centred)
            (hi, lo), _ = pc.gram_reference(X, mean if centred else None)
            assert np.array_equal(hi, want["gram"][0].astype(np.float64)) and not lo.any()
            assert np.array_equal(want["gram"][0], want["gram"][0].T)
            (hi, lo), _ = pc.gram_tn_reference(X, mean if centred else None, Y)
            assert np.array_equal(hi, want["tn"][0].astype(np.float64)) and not lo.any()
    for M, N, K in ((1, 1, 1), (5, 3, 17), (65, 64, 33), (9, 129, 161)):
        for ta, tb in pc.TYPE_PAIRS:
            A, B, rc, cc, c0 = pc.gemm_inputs(M, N, K, "exact", ta, tb)
            for corrected in (True, False):
                want, none = pc.gemm_expect(M, N, K, "exact", ta, tb, corrected)
                (hi, lo), _ = pc.gemm_nt_reference(A, B, *((rc, cc, c0) if corrected else ()))
                assert none is None and np.array_equal(hi, want.astype(np.float64)) and not lo.any()


def test_exact_cases_differ_in_every_row_and_column():
    """A moved lane, a swapped mirror or a dropped slab must change an integer result: no two rows and no two columns of an expected matrix
    agree, no expected matrix is its own transpose-with-Y, and every slab of 16 cells contributes to it."""
    for C, G, L in ((49, 129, 65), (33, 257, 64), (2049, 130, 63)):
        X, mean, Y = pc.gram_inputs(C, G, L, "exact", "float64")
        want = pc.gram_expect(C, G, L, "exact", "float64")
        for name in ("gram", "tn"):
            W = want[name][0]
            assert len({r.tobytes() for r in W}) == W.shape[0] and len({c.tobytes() for c in W.T}) == W.shape[1], name
        Xi = X.astype(np.int64) - mean.astype(np.int64)[None, :]
        for c0 in range(0, C, 16 * max(1, C // 160)):
            assert (Xi[c0:c0 + 16].T @ Y[c0:c0 + 16].astype(np.int64)).any() and (Xi[c0:c0 + 16].T @ Xi[c0:c0 + 16]).any()
    for M, N, K in ((65, 129, 33), (257, 64, 161)):
        W = pc.gemm_expect(M, N, K, "exact", "float64", "float64")[0]
        assert len({r.tobytes() for r in W}) == M and len({c.tobytes() for c in W.T}) == N


def _exit_of(n):
    """The exit of k_gram_dma's double-buffer loop a split of n cells takes: (pairs of slabs run, odd extra slab, tail slab)."""
    return (n // 32 > 0, n % 32 >= 16, n % 16 > 0)


def test_case_lists_contain_what_they_claim():
    # the double-buffer loop: every residue class of the cell count modulo 32 that takes another exit, with and without whole pairs before it
    exits = {_exit_of(C) for C in pc.SMALL_C}
    assert exits == {(False, False, True), (False, True, False), (False, True, True), (True, False, False), (True, False, True),
                     (True, True, False), (True, True, True)}
    assert {C % 32 for C in pc.SMALL_C} >= {1, 15, 16, 17, 31, 0}
    # both sides of every tile edge; the triangular walk with 1, 2, 3 and 5 tiles a side
    Gs = {G for _, G, _ in pc.GRAM_SMALL}
    assert Gs >= {1, 2, 127, 128, 129, 257, 513} and {(G + 127) // 128 for G in Gs} == {1, 2, 3, 5}
    assert len(pc.GRAM_SMALL) == len(pc.SMALL_C) * len(pc.SMALL_G) + 1 == len(set(pc.GRAM_SMALL))
    for C in pc.SMALL_C:
        assert {G for c, G, _ in pc.GRAM_SMALL if c == C} >= set(pc.SMALL_G)
    for L in pc.THIN_L:                                                # every thin width meets cell counts of several exits and several G
        part = [(C, G) for C, G, l in pc.GRAM_SMALL if l == L]
        assert len({_exit_of(C) for C, _ in part}) >= 4 and len({G for _, G in part}) == len(pc.SMALL_G)
    assert set(pc.THIN_L) == {1, 63, 64, 65, 128, 129}
    # the split: the first cell count that splits, a split that ends on a slab and one cell past it, two -> three splits
    assert tuple(C for C, _, _ in pc.GRAM_SPLIT) == pc.SPLIT_C == (2048, 2049, 2063, 2064, 2065, 2080, 2081, 3072, 3073)
    assert all(G == 130 for _, G, _ in pc.GRAM_SPLIT)
    assert {L for _, _, Ls in pc.GRAM_SPLIT for L in Ls} == set(pc.THIN_L) and all(len(set(Ls)) == 2 for _, _, Ls in pc.GRAM_SPLIT)
    # gemm_nt: every listed value, each with a small and a large partner in both other dimensions; 1 .. 5 slabs of K in both slab widths
    assert len(pc.GEMM_NT) == len(set(pc.GEMM_NT)) and 24 <= len(pc.GEMM_NT) <= 72
    for name, pos, values in (("M", 0, pc.NT_M), ("N", 1, pc.NT_N), ("K", 2, pc.NT_K)):
        assert {t[pos] for t in pc.GEMM_NT} == set(values), name
        for v in values:
            mine = [t for t in pc.GEMM_NT if t[pos] == v]
            for other, opos in (("M", 0), ("N", 1), ("K", 2)):
                if other != name:
                    assert {t[opos] for t in mine} & set(pc.NT_SMALL[other]) and {t[opos] for t in mine} & set(pc.NT_LARGE[other]), (name, v, other)
    for ksl in (16, 32):
        slabs = {(K + ksl - 1) // ksl for K in pc.NT_K}
        assert slabs >= {1, 2, 3, 4, 5}, ksl
        assert {K % ksl for K in pc.NT_K} >= {0, 1, ksl - 1}, ksl
    assert set(pc.MEANS) == {(C, G) for C in (1, 2, 63, 64, 65, 129) for G in (1, 255, 256, 257)}
    # what the children of the other kernel forms run
    assert {_exit_of(C if C < 2048 else 1) for C, _, _ in pc.WORKER_GRAM_BOUNDED} >= {(False, True, True), (True, False, True), (True, True, False)}
    assert any(C >= 2048 for C, _, _ in pc.WORKER_GRAM_BOUNDED) and {(K + 31) // 32 for _, _, K in pc.WORKER_GEMM_BOUNDED} >= {1, 2, 3, 5}


def _fp64_worst(got, expect):
    return pc.check(got, expect, "numpy fp64")


@pytest.mark.parametrize("kind", ["recipe", "ill"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_plain_fp64_evaluation_stays_within_the_bounds(kind, dtype):
    """numpy's own fp64 products (BLAS: blocked, vectorised, fused - yet another order of summation) of the same inputs."""
    worst = {"gram": 0.0, "tn": 0.0, "gemm_nt": 0.0, "col_means": 0.0}
    for C, G, L in ((17, 129, 65), (49, 257, 64), (33, 513, 127), (2049, 130, 63), (3073, 130, 1)):
        X, mean, Y = pc.gram_inputs(C, G, L, kind, dtype)
        for centred in (True, False):
            A = X - mean[None, :] if centred else X
            exp = pc.gram_expect(C, G, L, kind, dtype, centred)
            worst["gram"] = max(worst["gram"], _fp64_worst(A.T @ A, exp["gram"]))
            worst["tn"] = max(worst["tn"], _fp64_worst(A.T @ Y, exp["tn"]))
            # a split into three partial sums folded afterwards, as the cell split does
            parts = [A[a:a + (C + 2) // 3].T @ A[a:a + (C + 2) // 3] for a in range(0, C, (C + 2) // 3)]
            worst["gram"] = max(worst["gram"], _fp64_worst(sum(parts[1:], parts[0]), exp["gram"]))
    ta, tb = ("float64", "float64") if dtype == "float64" else ("float32", "float64")
    for M, N, K in pc.WORKER_GEMM_BOUNDED:
        A, B, rc, cc, c0 = pc.gemm_inputs(M, N, K, kind, ta, tb)
        out = A @ B.T
        if rc is not None:
            out = out - rc[:, None]
        out = out - cc[None, :] + c0
        worst["gemm_nt"] = max(worst["gemm_nt"], _fp64_worst(out, pc.gemm_expect(M, N, K, kind, ta, tb)))
    for C, G in ((1, 1), (65, 257), (129, 255)):
        X = pc.means_inputs(C, G, kind, dtype)
        ref, S = pc.col_means_reference(X)
        worst["col_means"] = max(worst["col_means"], _fp64_worst(X.sum(0) / C, (ref, pc.col_means_bound(S, C))))
    print(f"numpy fp64, {kind}, {dtype}: worst error / bound", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_ill_conditioned_bounds_still_say_something(dtype):
    """Mean 1e6, spread 1: the bound absorbs the cancellation and is still below 1e-6 of the largest entry."""
    for C, G, L in list(pc.WORKER_GRAM_BOUNDED) + [(49, 129, 65), (3073, 130, 129)]:
        exp = pc.gram_expect(C, G, L, "ill", dtype)
        for name in ("gram", "tn"):
            (hi, _), bound = exp[name]
            assert 0 < bound.max() < 1e-6 * np.abs(hi).max(), (C, G, L, name, bound.max(), np.abs(hi).max())
    ta, tb = ("float64", "float64") if dtype == "float64" else ("float32", "float32")
    for M, N, K in pc.WORKER_GEMM_BOUNDED:
        (hi, _), bound = pc.gemm_expect(M, N, K, "ill", ta, tb)
        assert 0 < bound.max() < 1e-6 * np.abs(hi).max(), (M, N, K, bound.max(), np.abs(hi).max())
    for C, G in ((65, 257), (129, 255)):
        (hi, _), S = pc.col_means_reference(pc.means_inputs(C, G, "ill", dtype))
        assert pc.col_means_bound(S, C).max() < 1e-6 * np.abs(hi).max()


def test_gamma_and_the_bound_factors():
    assert pc.gamma(1) == pytest.approx(2.0 ** -53, rel=1e-12) and pc.gamma(3073) > 3073 * 2.0 ** -53
    assert pc.bound_factor(18) == pc.gamma(18) + 18 * 2.0 ** -64
    S = np.ones((2, 2))
    assert np.array_equal(pc.gram_bound(S, 16), pc.bound_factor(18) * S) and np.array_equal(pc.gram_bound(S, 16, False), pc.bound_factor(16) * S)
    assert np.array_equal(pc.gram_tn_bound(S, 16), pc.bound_factor(17) * S)
    assert np.array_equal(pc.gemm_nt_bound(S, 65), pc.bound_factor(128 + 3) * S) and np.array_equal(pc.col_means_bound(S, 9), pc.bound_factor(10) * S)
