"""CPU pins of the independent fit reference (oracle.fit_box_reference, fit_kkt, r2_reference) that test_gpu_fit_kernels.py holds
the weighted-fit kernels to.  box_wls2 shares its raw-moment formula and its candidate order with csrc/fit.hip; the reference
here shares neither (long double, centred data, active set by enumeration), and is itself pinned on scipy's bounded least
squares, on box_wls2 where the expansion is harmless, on its own optimality conditions and on the golden L-BFGS-B results."""
import numpy as np
import pytest
import scipy.optimize

import fit_cases as fc

EPS = fc.EPS


def _genes(G=65, C=33, dtype="float64", wmode=0):
    for L in fc.region_launches(G, C, dtype, wmode):
        for g in range(G):
            yield L, g


def test_reference_against_scipy_bounded_least_squares(oracle):
    """lsq_linear(method="bvls") is an exact active-set solver: on these well-conditioned genes (kappa <= 200) both reach the
    minimiser to a few hundred eps; every region of the box occurs among them."""
    seen = set()
    for L, g in _genes():
        x, y, w = L["X"][g], L["Y"][g], L["W"][g]
        sq = np.sqrt(w)
        res = scipy.optimize.lsq_linear(np.stack([x, np.ones_like(x)], 1) * sq[:, None], y * sq,
                                        bounds=([L["lo"], 0.0], [L["up"][g], L["hi_q"][g]]), method="bvls", tol=1e-14)
        assert res.status > 0
        scale = max(1.0, abs(L["m"][g]), abs(L["q"][g]))
        assert abs(res.x[0] - L["m"][g]) <= 1e-11 * scale and abs(res.x[1] - L["q"][g]) <= 1e-11 * scale, (L["region"][g], res.x, L["m"][g], L["q"][g])
        seen.add(L["region"][g])
    assert seen == set(oracle.FIT_REGIONS)


def test_reference_against_box_wls2_where_the_expansion_is_harmless(oracle):
    n = 0
    for L, g in _genes():
        x, y, w = L["X"][g], L["Y"][g], L["W"][g]
        on = w > 0
        if x[on].mean() / x[on].std() > 3:
            continue
        m, q = oracle.box_wls2(x, y, w, L["lo"], L["up"][g], 0.0, L["hi_q"][g])
        scale = max(1.0, abs(L["m"][g]), abs(L["q"][g]))
        assert abs(m - L["m"][g]) <= 1e-12 * scale and abs(q - L["q"][g]) <= 1e-12 * scale, (L["region"][g], m, q)
        n += 1
    assert n >= 100


def test_reference_satisfies_its_own_optimality_conditions(oracle):
    """The reference's (m, q), rounded to f64, leaves a scaled KKT violation of a few f64 roundings (planted lines: 3e-16)."""
    worst = 0.0
    for L, g in _genes():
        worst = max(worst, oracle.fit_kkt(L["X"][g], L["Y"][g], L["W"][g], L["m"][g], L["q"][g], L["lo"], L["up"][g], 0.0, L["hi_q"][g]))
    print("largest KKT violation of the reference:", worst)
    assert worst <= 4 * EPS


def test_kkt_sees_a_wrong_active_set(oracle):
    """A feasible point that is not the minimiser has a violation far above rounding: the other corner, a free variable moved by
    1e-6, a variable left on the wrong bound."""
    for L, g in _genes(G=63):
        a = (L["X"][g], L["Y"][g], L["W"][g])
        box = (L["lo"], L["up"][g], 0.0, L["hi_q"][g])
        m, q, region = L["m"][g], L["q"][g], L["region"][g]
        rm, rq = region[2:4], region[7:9]
        if rm == "in":
            assert oracle.fit_kkt(*a, m * (1 + 1e-6) + 1e-9, q, *box) > 1e-9
        else:
            assert oracle.fit_kkt(*a, box[1] if rm == "lo" else box[0], q, *box) > 1e-6
        if rq != "in":
            assert oracle.fit_kkt(*a, m, box[3] if rq == "lo" else box[2], *box) > 1e-6
        assert oracle.fit_kkt(*a, box[1] + 1.0, q, *box) == float("inf")


@pytest.mark.parametrize("lg", [False, True])
def test_reference_on_the_golden_fits(oracle, golden, fit_parity, lg):
    """The golden L-BFGS-B results through SURVEY section 7's bar: parameters to rtol 1e-4, the objective never worse."""
    g = golden("fits")
    t = "lg" if lg else "nolg"
    G = g["Y"].shape[0]
    m, q = np.full(G, np.nan), np.zeros(G)
    regions = []
    for i in range(G):
        y, x, w = g["Y"][i], g["X"][i], g["W"][i]
        if not np.any(x) or not np.any(y):
            continue
        m[i], q[i], r = oracle.fit_box_reference(x, y, w, 1e-8, oracle._up_gamma(y, x, lg), 0.0, 2 * np.sum(y * w) / np.sum(w))
        regions.append(r)
    fit_parity(m, q, g[f"woffset_{t}_m"], g[f"woffset_{t}_q"], g["Y"], g["X"], g["W"], skip=(0, 1))
    assert "degenerate" not in regions


def test_degenerate_labels(oracle):
    x = np.array([1.0, 2.0, 3.0, 4.0])
    y = np.array([2.0, 1.0, 4.0, 3.0])
    assert oracle.fit_box_reference(x, y, np.zeros(4), 0, 20, 0, np.nan)[2] == "degenerate"          # Sw == 0, upper q bound 0/0
    assert oracle.fit_box_reference(x, y, [0, 0, 1, 0], 0, 20, 0, 8)[2] == "degenerate"              # one weighted cell
    m, q, r = oracle.fit_box_reference([2.0, 2.0, 3.0, 2.0], y, [1, 1, 0, 1], 0, 20, 0, 4)           # weighted x all equal
    assert r == "degenerate" and 0 <= m <= 20 and 0 <= q <= 4
    assert abs(oracle.fit_objective([2.0, 2.0, 3.0, 2.0], y, [1, 1, 0, 1], m, q) - 2.0) < 1e-15       # = sum (y - 2)^2 over the three cells
    assert oracle.fit_box_reference(x, y, np.ones(4), 0, 20, 0, 5)[2] == "m_in/q_in"


def test_r2_reference(oracle):
    rng = np.random.default_rng(5)
    x = rng.gamma(2.0, 1.0, 200)
    y = 0.7 * x + 0.3 + rng.normal(0, 0.2, 200)
    assert abs(oracle.r2_reference(0.7, 0.3, x, y) - oracle._r2(0.7, 0.3, x, y)) < 1e-14
    assert abs(oracle.r2_expansion(0.7, 0.3, x, y) - oracle._r2(0.7, 0.3, x, y)) < 1e-13
    assert oracle.r2_reference(1.0, 0.0, x, np.full(200, 3.0)) == -1e16                              # sstot == 0
    assert oracle.r2_reference(1.0, 0.0, [2.0], [2.0]) == -1e16                                      # one cell: 0/0
    assert oracle.r2_reference(np.nan, 0.0, x, y) == -1e16


def test_the_k_of_the_conditioning_bound_is_what_the_cpu_measures(oracle):
    """K of test_gpu_fit_kernels.py's conditioning sweep: the largest err / (C eps kappa) of the oracle's own f64 raw-moment
    expansion (box_wls2, r2_expansion) against the centred long-double reference over x = r + N(0, 1), r = 1 ... 1e5, C = 257.
    Measured: 0.0074 for m and q (numpy sums pairwise), 131 for R2, whose error is not the expansion's alone: R2 is evaluated at
    the solver's own (m, q), whose error grows with kappa as well (R2 per ratio: 0.008, 0.008, 0.02, 0.59, 2.6, 131)."""
    k_fit = k_r2 = 0.0
    for dtype in ("float64", "float32"):
        s = fc.sweep(dtype)
        assert set(s["region"]) == {"m_in/q_in"}
        G = s["X"].shape[0]
        got = np.empty((G, 3))
        for g in range(G):
            m, q = oracle.box_wls2(s["X"][g], s["Y"][g], s["W"][g], 1e-8, 20.0, 0.0, s["hi_q"][g])
            got[g] = m, q, oracle.r2_expansion(m, q, s["X"][g], s["Y"][g])
        bm, bq, br = fc.sweep_bounds(s, 1.0, 1.0)
        err = np.abs(got - s["ref"])
        k_fit = max(k_fit, float((err[:, 0] / bm).max()), float((err[:, 1] / bq).max()))
        k_r2 = max(k_r2, float((err[:, 2] / br).max()))
    print("measured K: fit", k_fit, "R2", k_r2)
    assert 0.5 * fc.FIT_K <= k_fit <= fc.FIT_K
    assert 0.5 * fc.FIT_K_R2 <= k_r2 <= fc.FIT_K_R2


def test_every_region_is_reached_from_the_reference_alone(oracle):
    for dtype, wmode in (("float64", 0), ("float32", 2)):
        n = fc.census(fc.region_launches(255, 33, dtype, wmode))
        assert n["degenerate"] == 0 and min(n[r] for r in oracle.FIT_REGIONS) >= 8, n
