"""The optimality certificate of svr_cases.py on the CPU, before test_gpu_svr_kernels.py holds the device solver to it: the
reference solutions (oracle.svr_rbf_fit, scikit-learn's libsvm) pass every condition, and solutions that are wrong in the ways the
device solver could be wrong - stopped early, a shifted intercept, a residual that missed an update, a coefficient off its
bound - do not.  A certificate that accepts everything proves nothing."""
import numpy as np
import pytest

import svr_cases as sv

TOL3 = [c for c in sv.CASES if sv.CASES[c][5] == 1e-3]
_FITS = {}


def _oracle_fit(oracle, name):
    """The oracle's solution of a case, fitted once and never modified."""
    if name not in _FITS:
        x, t, kw = sv.case(name)
        coef, b, it = oracle.svr_rbf_fit(x, t, **kw)
        coef.setflags(write=False)
        _FITS[name] = (coef, float(b), int(it))
    return _FITS[name]


def _check(x, t, kw, coef, b, it):
    cert = sv.certificate(x, t, coef, b, kw["C"], kw["epsilon"], kw["gamma"])
    return cert, sv.accept(cert, b, kw["C"], kw["tol"], it, len(x), t, coef)


@pytest.mark.parametrize("name", list(sv.CASES))
def test_the_oracle_solution_passes(oracle, name):
    x, t, kw = sv.case(name)
    coef, b, it = _oracle_fit(oracle, name)
    cert, bad = _check(x, t, kw, coef, b, it)
    print(f"{name}: steps {it} slack {sv.slack(it, kw['C'], t, coef):.2e} violation {float(cert.violation):.6e} "
          f"(violation - tol) / slack {sv.violation_ratio(cert, kw['C'], kw['tol'], it, t, coef):.4g} gap {float(cert.gap):.3e}")
    assert not bad, bad
    a = np.abs(coef)
    assert (name in sv.NONE_FREE) == (not ((a > 0) & (a < kw["C"])).any())          # the midpoint cases are exactly these
    if name in sv.NONE_FREE:
        print(f"{name}: |b - (L + U) / 2| = {abs(b - 0.5 * (float(cert.L) + float(cert.U))):.2e}")
    if name == "eps0":
        assert np.count_nonzero(coef) == len(x)
    if name in ("tinyC", "totals1025"):
        assert np.count_nonzero(coef) > len(x) // 2


@pytest.mark.parametrize("name", TOL3)
def test_the_libsvm_solution_passes(name):
    svm = pytest.importorskip("sklearn.svm")
    x, t, kw = sv.case(name)
    m = svm.SVR(**kw).fit(x[:, None], t)
    coef = np.zeros(len(x))
    coef[m.support_] = m.dual_coef_[0]
    it = int(np.ravel(m.n_iter_)[0])
    b = float(m.intercept_[0])
    cert = sv.certificate(x, t, coef, b, kw["C"], kw["epsilon"], kw["gamma"])
    bad = sv.accept(cert, b, kw["C"], kw["tol"], it, len(x), t, coef, row_eps=sv.FLOAT_ROWS)      # float kernel rows: see FLOAT_ROWS
    print(f"{name}: libsvm steps {it} (violation - tol) / slack {sv.violation_ratio(cert, kw['C'], kw['tol'], it, t, coef):.4g}")
    assert not bad, bad
    strict = sv.accept(cert, b, kw["C"], kw["tol"], it, len(x), t, coef)
    assert not strict or (name in ("tinyC", "totals1025") and len(strict) == 1 and "midpoint" in strict[0]), strict


@pytest.mark.parametrize("name", ["cv1300", "C100"])
def test_the_certificate_rejects_wrong_solutions(oracle, name):
    x, t, kw = sv.case(name)
    C, tol = kw["C"], kw["tol"]
    coef, b, it = _oracle_fit(oracle, name)
    cert, bad = _check(x, t, kw, coef, b, it)
    assert not bad
    # stopped at half the steps
    hc, hb, hit = oracle.svr_rbf_fit(x, t, max_iter=it // 2, **kw)
    assert hit == it // 2
    assert any("violation" in s for s in _check(x, t, kw, hc, hb, hit)[1])
    # the intercept 3 tol beyond either end of [U, L]
    lo, hi = sorted((float(cert.L), float(cert.U)))
    for moved in (hi + 3 * tol, lo - 3 * tol):
        assert any("intercept" in s for s in _check(x, t, kw, coef, moved, it)[1])
    # a residual that missed an update: the solution of targets in which one free support vector moved by 5 tol
    a = np.abs(coef)
    k = int(np.argmin(np.where((a > 0) & (a < C), np.abs(a - 0.5 * C), np.inf)))
    assert 0 < a[k] < C
    for sign in (1.0, -1.0):
        t2 = t.copy()
        t2[k] += sign * 5 * tol
        c2, b2, it2 = oracle.svr_rbf_fit(x, t2, **kw)
        assert not _check(x, t2, kw, c2, b2, it2)[1]                                  # a fine solution of ITS problem
        assert any("violation" in s for s in _check(x, t, kw, c2, b2, it2)[1])
    # a bound coefficient 1e-6 C inside: sum(coef) = 0 broken
    kb = int(np.flatnonzero(a == C)[0])
    off = np.array(coef)
    off[kb] -= np.sign(off[kb]) * 1e-6 * C
    assert any("sum coef" in s for s in _check(x, t, kw, off, b, it)[1])


def test_the_certificate_in_closed_form():
    # one point inside the tube: no support vector, [L, U] = [t - eps, t + eps], nothing to pay at b = t
    c = sv.certificate([0.0], [0.25], [0.0], 0.25, 1.0, 0.125, 2.0)
    assert (c.L, c.U, c.violation, c.gap, c.sum_coef, c.max_abs_coef) == (0.125, 0.375, -0.25, 0.0, 0.0, 0.0)
    # two points at x = 0 and 1 with coef = (C, -C): the sets of L are {k: coef < C} = {1} twice, those of U {0} twice
    K01 = np.exp(np.longdouble(-2))
    c = sv.certificate([0.0, 1.0], [3.0, -3.0], [1.0, -1.0], 0.0, 1.0, 0.125, 2.0)
    r0 = np.array([3 - (1 - K01), -3 + (1 - K01)])
    assert c.L == r0[1] + 0.125 and c.U == r0[0] - 0.125 and c.violation < 0
    assert abs(c.gap) < 1e-18 and c.max_abs_coef == 1 and c.sum_coef == 0      # each term C (|r0| - eps) + eps C - C |r0| = 0
    c = sv.certificate([0.0, 1.0], [3.0, -3.0], [1.0, -1.0], 0.5, 1.0, 0.125, 2.0)
    assert abs(c.gap - 0) < 1e-18                                              # ... and the b terms cancel while sum(coef) = 0
    c = sv.certificate([0.0, 1.0], [3.0, -3.0], [0.5, -0.5], 0.0, 1.0, 0.125, 2.0)
    assert abs(c.gap - 2 * 0.5 * (3 - 0.5 * (1 - K01) - 0.125)) < 1e-18        # half the box: C (|r| - eps) - |r|/2 + eps/2 per point
    # a set that is empty: the only point at +C leaves I_up empty
    c = sv.certificate([0.0], [3.0], [1.0], 0.0, 1.0, 0.125, 2.0)
    assert c.L == -np.inf and c.violation == -np.inf and np.isfinite(c.U)


def test_predict_reference_against_the_f64_restatement(oracle):
    x, t, kw = sv.case("cv1300")
    coef, b, _ = _oracle_fit(oracle, "cv1300")
    xq = np.concatenate([np.linspace(x.min() - 1, x.max() + 1, 101), x[:5]])
    ref = sv.predict_reference(x, coef, b, xq, kw["gamma"])
    err = np.abs(oracle.svr_rbf_predict(x, coef, b, xq, kw["gamma"]) - ref).astype(np.float64)
    bound = sv.predict_bound(x, coef, b, xq, kw["gamma"])
    print(f"predict: worst error / bound {float((err / bound).max()):.4g}")
    assert np.all(err <= bound)
    # the reference itself: a one-point model is coef exp(-gamma d^2) + b in closed form
    one = sv.predict_reference([1.0], [2.0], 0.5, [1.0, 3.0], 0.25)
    assert one.dtype == np.longdouble and one[0] == 2.5 and abs(one[1] - (2 * np.exp(np.longdouble(-1)) + 0.5)) < 1e-18
