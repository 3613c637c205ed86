"""The epsilon-SVR solver (csrc/svr.hip: k_svr_smo<E>, k_svr_finish, k_svr_predict) held to an optimality certificate that
needs none of the solver's state, and to a plain long-double sum.  numpy only; shared by test_svr_oracle.py (CPU: the
references pass, wrong solutions do not) and test_gpu_svr_kernels.py (the device).

The certificate.  With coef = alpha - alpha*, alpha = max(coef, 0), alpha* = max(-coef, 0) and the residuals without the
intercept r0 = t - K coef recomputed from coef alone in long double,
    L = max( max_{coef_k < C} (r0_k - eps),  max_{coef_k < 0} (r0_k + eps) )        libsvm's m(b): max over I_up of -y G
    U = min( min_{coef_k > -C}(r0_k + eps),  min_{coef_k > 0} (r0_k - eps) )        libsvm's M(b): min over I_low of -y G
violation = L - U is the quantity libsvm stops on (< tol); it does not move when every r0 is shifted by a constant.  Any
intercept in [U, L] (or [L, U]) satisfies the KKT conditions to `violation`; with no free variable libsvm takes the
midpoint.  gap = sum_k C max(0, |r0_k - b| - eps) + eps |coef_k| - coef_k (r0_k - b) is primal minus dual: every term is
>= 0 inside the box, and at a point whose violation is v it is at most 2 C v per support vector.

The slack.  The solver carries r incrementally: `it` updates of two fma-free terms each, every one rounding a number no
larger than max|t| + sum|coef| (+ the step's own 2C), so the carried residual is off the recomputed one by at most
16 u (it + 1) (max|t| + sum|coef| + 2C), u = 2^-53.  This is a bound on rounding, not on the solver: a residual that
missed an update is off by a multiple of tol.

Measured (violation - tol) / slack, negative = inside tol by that many slacks (the stop leaves headroom under tol; the
slack is what the certificate grants on top):

    case         slack (oracle's)  oracle.svr_rbf_fit  scikit-learn   device (MI355X)   steps oracle / device
    cv1300       1.75e-09          -2.85e+03           -6.53e+04      -9.56e+04         1050 / 1064
    tied1300     1.75e-09          -3.68e+03           -2.17e+04      -2.52e+04         1066 / 1260
    cv2100       3.77e-09          -8.69e+03           -4.45e+02      -8.55e+04         1342 / 1360
    cv300tight   3.18e-10          -7.37               (not run)      -21.97             794 / 810
    C100         7.83e-08          -1.18e+03           -5.09e+02      -45.36            4730 / 4648
    eps0         6.14e-10          -2.88e+05           -2.92e+05      -2.13e+05          602 / 598
    dupx         2.46e-12          -1.46e+08           -5.22e+07      -1.46e+08           37 / 37
    tinyC        1.96e-12          -2.76e+09           -2.76e+09      -2.76e+09          193 / 193
    gamma0       3.23e-11          -4.50e+08           -4.50e+08      -4.50e+08           93 / 93
    gammabig     5.96e-11          -1.63e+05           -8.04e+05      -1.63e+05          266 / 266
    totals1025   1.28e-08          -4.04e+07           -4.04e+07      -4.04e+07          687 / 687

(scikit-learn at tol = 1e-7 is not run: its float kernel rows leave it 3.8e-7 over.)  Where the step counts differ the device's
exp and libm's differ by an ulp somewhere and a near-tie went the other way; on tied1300, whose candidates are often equal up to
that ulp, the oracle itself takes 1241 to 1483 steps when a tenth of its exp values are moved by one ulp at random.

predict, worst error / predict_bound: oracle.svr_rbf_predict (numpy's pairwise sum) on cv1300 3.6e-4; k_svr_predict over the
n x m x gamma matrix of test_gpu_svr_kernels.py 0.674 (n = 1: 0, 2: 0.660, 1023: 0.674, 1024: 0.653, 1025: 0.657, 2049: 0.671; the
worst is at gamma = 1e6 for n >= 1023 and at gamma = 0.7 for n = 2: a handful of terms, so the bound has no n / 2 to spare).
"""
import math
from collections import namedtuple

import numpy as np

U53 = 2.0 ** -53
LD = np.longdouble
# libsvm keeps its kernel rows as float: every K_kl carries a relative rounding of 2^-24, so every gradient entry - and with it
# the rho libsvm derives from them - is off by up to 2^-24 sum|coef|.  Granted to scikit-learn's solution only (accept's row_eps);
# the oracle and the device compute fp64 rows and get none of it.  Without it libsvm's own midpoint rho misses the slack:
# tinyC |b - (L + U) / 2| = 3.9e-11 (slack 2.0e-12, this term 1.7e-8), totals1025 1.9e-7 (slack 1.3e-8, this term 1.8e-4);
# oracle.svr_rbf_fit on the same inputs: @ORACLE_MID@.
FLOAT_ROWS = 2.0 ** -24

Certificate = namedtuple("Certificate", "violation L U gap sum_coef max_abs_coef")


# ------------------------------------------------------------------------------------------------------------------ the inputs
def _cv_like(n, rng):
    x = np.log2(rng.gamma(0.5, 0.5, n) + 1e-3)
    return x, -0.5 * x + 0.3 * rng.normal(size=n) + 0.5 * np.exp(-x * x)


def _totals_like(n, rng):
    x = rng.gamma(5, 2000, n)
    return x, 0.3 * x * (1 + 0.2 * np.sin(x / 5000)) + rng.normal(0, 300, n)


def _tied(n, rng):
    """Genes with identical mean and CV: eleven distinct x, targets on a grid of 0.1 - many exact duplicates of (x, t), so the
    lowest-index rule of better_max / better_min / wave_best / gather decides most selections."""
    x = np.log2(rng.integers(1, 12, n) / 4)
    return x, np.round(-0.5 * x + 0.3 * rng.normal(size=n), 1)


def _dupx(n, rng):
    assert n == 40
    return np.repeat(np.arange(8.), 5), rng.normal(size=40)


_GEN = {"cv": _cv_like, "totals": _totals_like, "tied": _tied, "dupx": _dupx}

# name: (generator, n, C, gamma, epsilon, tol)
CASES = {
    "cv1300": ("cv", 1300, 1.0, 150. / 1300, 0.1, 1e-3),          # the launch-shape matrix
    "tied1300": ("tied", 1300, 1.0, 0.5, 0.1, 1e-3),              # tie-break decisive
    "cv2100": ("cv", 2100, 1.0, 0.05, 0.1, 1e-3),                 # per = 9 on one workgroup: <0> without the env switch
    "cv300tight": ("cv", 300, 1.0, 0.5, 0.1, 1e-7),               # a tolerance at which drift would show
    "C100": ("cv", 120, 100.0, 0.5, 0.1, 1e-3),                   # wide box, many free <-> bound transitions
    "eps0": ("cv", 65, 10.0, 2.0, 0.0, 1e-3),                     # every point a support vector
    "dupx": ("dupx", 40, 1.0, 1.0, 0.1, 1e-3),                    # zero curvature between duplicates (SVR_TAU)
    "tinyC": ("cv", 300, 1e-3, 0.5, 0.1, 1e-3),                   # every SV at the bound, none free: midpoint rho
    "gamma0": ("cv", 200, 1.0, 0.0, 0.1, 1e-3),                   # K = 1, SVR_TAU on every pair, none free
    "gammabig": ("cv", 200, 1.0, 1e6, 0.1, 1e-3),                 # K ~ identity
    "totals1025": ("totals", 1025, 3.0, 1e-7, 25.0, 1e-3),        # targets of 1e4, all at the bound
}
NONE_FREE = ("tinyC", "gamma0", "totals1025")


def case(name):
    """(x, t, kw) of a case; kw = dict(C, gamma, epsilon, tol) as ops.svr_fit and oracle.svr_rbf_fit take it."""
    kind, n, C, gamma, eps, tol = CASES[name]
    x, t = _GEN[kind](n, np.random.default_rng(n))
    return x, t, dict(C=C, gamma=gamma, epsilon=eps, tol=tol)


# ------------------------------------------------------------------------------------------------------------------ the certificate
def _kernel(xa, xb, gamma):
    d = np.asarray(xa, dtype=LD)[:, None] - np.asarray(xb, dtype=LD)[None, :]
    return np.exp(-LD(gamma) * d * d), d


def certificate(x, t, coef, b, C, eps, gamma):
    x, t, coef = (np.asarray(a, dtype=LD).ravel() for a in (x, t, coef))
    b, C, eps = LD(b), LD(C), LD(eps)
    K, _ = _kernel(x, x, gamma)
    r0 = t - K @ coef

    def ext(fn, empty, *parts):
        vals = np.concatenate([v[m] for v, m in parts])
        return fn(vals) if vals.size else LD(empty)

    L = ext(np.max, -np.inf, (r0 - eps, coef < C), (r0 + eps, coef < 0))
    U = ext(np.min, np.inf, (r0 + eps, coef > -C), (r0 - eps, coef > 0))
    rb = r0 - b
    gap = np.sum(C * np.maximum(LD(0), np.abs(rb) - eps) + eps * np.abs(coef) - coef * rb)
    return Certificate(L - U, L, U, gap, np.sum(coef), np.max(np.abs(coef)))


def slack(it, C, t, coef):
    return 16 * U53 * (it + 1) * (float(np.abs(t).max()) + float(np.abs(np.asarray(coef, dtype=np.float64)).sum()) + 2 * C)


def accept(cert, b, C, tol, it, n, t, coef, row_eps=0.0):
    """The conditions a converged fit meets.  Returns the list of those that do NOT hold (empty: accepted).  row_eps: the relative
    rounding of the solver's kernel rows where they are not fp64 (libsvm: FLOAT_ROWS); 0 for the oracle and for the device."""
    coef = np.asarray(coef, dtype=np.float64)
    s = slack(it, C, t, coef) + row_eps * float(np.abs(coef).sum())
    v, L, U, gap = (float(a) for a in cert[:4])
    bad = []
    if not v <= tol + s:
        bad.append(f"violation {v:.3e} > tol {tol:g} + slack {s:.2e}")
    if not float(cert.max_abs_coef) <= C:
        bad.append(f"max|coef| {float(cert.max_abs_coef)!r} > C {C!r}")
    if not abs(float(cert.sum_coef)) <= 4 * U53 * (it + n) * C:
        bad.append(f"|sum coef| {abs(float(cert.sum_coef)):.3e} > {4 * U53 * (it + n) * C:.3e}")
    b = float(b)
    if not min(L, U) - s <= b <= max(L, U) + s:
        bad.append(f"intercept {b!r} outside [{min(L, U)!r}, {max(L, U)!r}] +- {s:.2e}")
    a = np.abs(coef)
    if not ((a > 0) & (a < C)).any() and not abs(b - 0.5 * (L + U)) <= s:
        bad.append(f"no free variable, intercept {b!r} is not the midpoint {0.5 * (L + U)!r} +- {s:.2e}")
    hi = 2 * C * int(np.count_nonzero(coef)) * max(v, 0.0) + s * n
    if not -s * n <= gap <= hi:
        bad.append(f"duality gap {gap:.3e} outside [{-s * n:.2e}, {hi:.3e}]")
    return bad


def violation_ratio(cert, C, tol, it, t, coef):
    """(violation - tol) / slack: above 1 the certificate fails."""
    return (float(cert.violation) - tol) / slack(it, C, t, coef)


# ------------------------------------------------------------------------------------------------------------------ predict
def predict_reference(x, coef, b, xq, gamma):
    K, _ = _kernel(xq, x, gamma)
    return K @ np.asarray(coef, dtype=LD).ravel() + LD(b)


def predict_bound(x, coef, b, xq, gamma):
    """Per query u ( sum_k |coef_k| K_qk (4 + 2 gamma d_qk^2 + ceil(n/2)) + |out_q| ): the rounding of the argument -gamma d^2
    scaled through exp (relative error of exp = absolute error of its argument), a 1-ulp device exp and the product, the two fma
    chains of ceil(n/2) terms (each partial sum bounded by the sum of magnitudes), and the final adds."""
    K, d = _kernel(xq, x, gamma)
    ac = np.abs(np.asarray(coef, dtype=LD).ravel())
    n = ac.size
    w = K * (4 + 2 * LD(gamma) * d * d + math.ceil(n / 2))
    out = K @ np.asarray(coef, dtype=LD).ravel() + LD(b)
    return (U53 * (w @ ac + np.abs(out))).astype(np.float64)
