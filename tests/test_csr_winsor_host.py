"""The two numpy references of the winsorised gene statistics of CSR layers (tests/csr_winsor_cases.py), pinned on the host against
numpy itself on the reference's data: tests/golden/preprocess.npz, the 387 detected genes x 260 cells, counts up to 373.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csr_winsor_cases as cases  # noqa: E402

U = cases.U
PERC = (1, 99.5)


@pytest.fixture(scope="module")
def data(golden):
    g = golden("preprocess")
    S = g["S"][g["genes_after_detection"]].astype(np.int64)          # (genes, cells), the reference's layout
    assert S.shape == (387, 260) and S.max() == 373
    down, up = np.percentile(S.astype(np.float64), PERC, 1)           # analysis.py:264, on the float64 layer as the reference holds it
    return S, down, up


def test_the_rank_rule_with_zeros_and_the_lerp_are_np_percentile(data):
    S, down, up = data
    got = cases.rank_rule_percentiles(S.T, PERC)
    assert cases.same_bits(got, np.stack([down, up])) and got.size == 774
    assert cases.same_bits(cases.np_percentiles(S.T, PERC), np.stack([down, up]))          # integer input: the same bits
    # the data exercises the rule: non-integer upper bounds (both lerp forms need them) and positive lower bounds beside zero ones
    assert 0.5 < np.mean(up != np.rint(up)) < 0.8 and 0.05 < np.mean(down > 0) < 0.2 and np.any(down == 0)
    for qs in ((0, 100), (50,), (33.3, 50.25, 66.6), cases.Q16):
        assert cases.same_bits(cases.rank_rule_percentiles(S.T, qs), np.percentile(S.astype(np.float64), qs, 1))
    mask = np.arange(260) % 3 != 1
    assert cases.same_bits(cases.rank_rule_percentiles(S.T, PERC, mask), np.percentile(S[:, mask].astype(np.float64), PERC, 1))


def test_the_moment_formula_is_the_sum_of_the_clipped_values(data):
    """sum = (lo nb + S1) + hi na: S1 and the counts are exact, so three separately rounded operations on non-negative terms - at most
    3 x 2^-53 relative - plus one of slack: 4 x 2^-53 against math.fsum (the correctly rounded sum) of np.clip(...), and of its square
    (one more rounding per square, lo lo and hi hi, inside the same slack: the squares of the middle values are exact integers)."""
    S, down, up = data
    st = cases.clipped_stats(S.T, down, up)
    clipped = np.clip(S.astype(np.float64), down[:, None], up[:, None])
    worst = 0.0
    for g in range(S.shape[0]):
        for got, vals in ((st[0, g], clipped[g]), (st[1, g], clipped[g] * clipped[g])):
            ref = math.fsum(vals)
            assert ref > 0
            worst = max(worst, abs(got - ref) / ref)
    print(f"worst relative error of the moment formula: {worst / U:.2f} x 2^-53")
    assert worst <= 4 * U
    assert np.array_equal(st[2], (clipped > 0).sum(1)) and np.array_equal(st[3], clipped.max(1))
    # without bounds the formula is the plain integer statistics
    plain = cases.clipped_stats(S.T, None, None)
    assert np.array_equal(plain, np.stack([S.sum(1), (S * S).sum(1), (S > 0).sum(1), S.max(1)]).astype(np.float64))


def test_mu_and_sigma_from_the_moments_match_the_reference(data):
    S, down, up = data
    C = S.shape[1]
    st = cases.clipped_stats(S.T, down, up)
    Sfw = np.clip(S.astype(np.float64), down[:, None], up[:, None])          # analysis.py:265-267
    mu_ref, sigma_ref = Sfw.mean(1), Sfw.std(1, ddof=1)
    mu = st[0] / C                                                           # preprocess.cv_vs_mean_from_stats
    var = (st[1] - C * mu * mu) / (C - 1)
    sigma = np.sqrt(np.maximum(var, 0.0))
    # mu: the sum is within 4u (the test above), the division adds 1u; numpy's mean is a pairwise sum of 260 non-negative terms (blocks
    # of 128 in 8 accumulators: at most 15 + 3 + 2 roundings on a path) and a division, 21u.  26u in all; asserted at 32u.
    assert np.all(np.abs(mu - mu_ref) <= 32 * U * mu_ref)
    # sigma: the numerator sum2 - C mu mu carries 4u sum2 from sum2, (2 x 5u + 2u) C mu^2 <= 12u sum2 from the product and 1u of its own
    # result: at most 17u sum2, whatever cancels; numpy's two-pass variance is relatively accurate, (2 x 21 + 22)u = 64u of var.  So
    # |var - var_ref| <= 17u sum2 / (C - 1) + 64u var_ref, and |sigma - sigma_ref| = |var - var_ref| / (sigma + sigma_ref), plus 1u for
    # the square root.  The cancellation shows as sum2 / ((C - 1) var) = 1 + 1 / CV^2 (up to ~60 on this data).
    var_ref = Sfw.var(1, ddof=1)
    bound_var = 17 * U * st[1] / (C - 1) + 64 * U * var_ref
    assert np.all(np.abs(var - var_ref) <= bound_var)
    assert np.all(sigma_ref > 0)
    assert np.all(np.abs(sigma - sigma_ref) <= bound_var / (sigma + sigma_ref) + 2 * U * sigma_ref)
