"""Inputs and measured constants for the tests of the fused fit_gammas weights (test_gpu_fit_fused_weights.py).

POW_W_ULPS: the largest distance, in f64 ulps of numpy's value, between the "maxmin_weighted" weight the device forms
(0.5 (R^pw + (1 - R)^pw) with the device's f64 pow; vcy_gamma_weights mode 2) and numpy's restatement of analysis.py:1186-1192 on
the inputs of `case` below, over pw in POWERS and every shape of the test.  Measured on an MI355X (2 ulps at every gene count of the test), not chosen: the
test prints what it measures and fails if the device ever exceeds it."""
import functools

import numpy as np

POWERS = (1.0, 15.0, 2.5)
POW_W_ULPS = 2.0
FIT_CB = 32                                    # cell blocks of the moments kernels (csrc/fit.hip)
CELLS = (1, 2, FIT_CB - 1, FIT_CB, FIT_CB + 1, 1201)
GENES = (1, 255, 256, 257)
PERC = (2.0, 98.0)


def stored(a, dtype):
    return np.asarray(a, dtype=np.float64) if dtype == "float64" else np.asarray(a, dtype=np.float32).astype(np.float64)


def _denominator(M):
    """analysis.py:1197-1202."""
    d = np.percentile(M, 99.9, 0)
    return np.where(d == 0, np.maximum(M.max(0), 0.001), d)


@functools.lru_cache(maxsize=None)
def case(C, G, dtype):
    """Cells-major (C, G) non-negative matrices as stored in `dtype` (f64 arrays) and the per-gene thresholds fit_gammas would take
    from them (np.percentile over the cells of the stored values): sparse pooled-count-like S, U, and X, Y of their own."""
    rng = np.random.default_rng(100003 * C + 17 * G + (dtype == "float32"))
    draw = lambda scale: stored(rng.gamma(0.7, scale, (C, G)) * (rng.random((C, G)) < 0.8), dtype)
    S, U, X, Y = draw(2.0), draw(1.0), draw(2.0), draw(1.0)
    t = np.float64 if dtype == "float64" else np.float32
    dS, dU = _denominator(S), _denominator(U)
    with np.errstate(all="ignore"):
        Z = (S.astype(t) / dS.astype(t)[None, :] + U.astype(t) / dU.astype(t)[None, :]).astype(np.float64)      # formed in the storage type
    zd, zu = np.percentile(Z, PERC, 0)
    sd, su = np.percentile(S, PERC, 0)
    return dict(S=S, U=U, X=X, Y=Y, Z=Z, p99_S=np.percentile(S, 99, 0), p99_U=np.percentile(U, 99, 0), down_S=sd, up_S=su, down_Z=zd, up_Z=zu,
                denom_S=dS, denom_U=dU)


def mode_args(c, mode):
    """(pa, pb, pc, pd, sa, sb) of vcy_gamma_weights / vcy_fit_weighted_moments_fused for the case's thresholds."""
    if mode in (0, 1):
        return c["p99_S"], c["p99_U"], None, None, None, None
    if mode == 2:
        return c["down_S"], c["up_S"], None, None, None, None
    return c["down_Z"], c["up_Z"], c["down_S"], c["up_S"], c["denom_S"], c["denom_U"]


def numpy_weights(c, mode, power=15.0):
    """analysis.py:1182-1192, 1208-1219 in numpy on the stored values (f64), cells-major, with the case's thresholds."""
    S, U = c["S"], c["U"]
    with np.errstate(all="ignore"):
        if mode == 0:
            return S / c["p99_S"][None, :] + U / c["p99_U"][None, :]
        if mode == 1:
            return (S / c["p99_S"][None, :]) * (U / c["p99_U"][None, :])
        if mode == 2:
            R = np.clip(S, c["down_S"][None, :], c["up_S"][None, :])
            R = R - R.min(0)[None, :]
            R = R / R.max(0)[None, :]
            return 0.5 * (R ** power + (1 - R) ** power)
        Z = c["Z"]
        W = ((Z <= c["down_Z"][None, :]) | (Z >= c["up_Z"][None, :])).astype(float)
        return W + ((S <= c["down_S"][None, :]) | (S >= c["up_S"][None, :])).astype(float)


def numpy_moments(c, W, keep=None):
    """The (10, G) moments [Sx Sy Sxx Sxy Syy | Sw Swx Swy Swxx Swxy] of x = X, y = Y, w = W over the kept cells, numpy's own sums."""
    X, Y = c["X"], c["Y"]
    if keep is not None:
        X, Y, W = X[keep], Y[keep], W[keep]
    with np.errstate(all="ignore"):
        return np.stack([X.sum(0), Y.sum(0), (X * X).sum(0), (X * Y).sum(0), (Y * Y).sum(0), W.sum(0), (W * X).sum(0), (W * Y).sum(0),
                         (W * X * X).sum(0), (W * X * Y).sum(0)])


def degenerate(dtype, C=67):
    """Eight constructed genes, cells-major (C, 8), and thresholds per mode that hit the divisions by zero:
    gene 0 ordinary; 1 all zero (every threshold 0); 2 constant (every threshold the constant); 3 S with p99 = 0 but a few non-zero
    cells; 4 down == up inside the data's range; 5 an ordinary gene with U all zero; 6 huge values; 7 tiny values."""
    rng = np.random.default_rng(5)
    S = rng.gamma(0.7, 2.0, (C, 8))
    U = rng.gamma(0.7, 1.0, (C, 8))
    S[:, 1] = U[:, 1] = 0.0
    S[:, 2], U[:, 2] = 1.25, 0.75
    S[:, 3] = 0.0
    S[:2, 3] = (3.0, 5.0)
    U[:, 5] = 0.0
    S[:, 6] *= 1e30
    S[:, 7] *= 1e-30
    S, U = stored(S, dtype), stored(U, dtype)
    X, Y = stored(rng.gamma(0.7, 2.0, (C, 8)), dtype), stored(rng.gamma(0.7, 1.0, (C, 8)), dtype)
    c = dict(S=S, U=U, X=X, Y=Y)
    pS, pU = np.percentile(S, 99, 0), np.percentile(U, 99, 0)
    pS[3] = 0.0
    sd, su = np.percentile(S, PERC, 0)
    sd[4] = su[4] = np.median(S[:, 4])
    dS, dU = _denominator(S), _denominator(U)
    t = np.float64 if dtype == "float64" else np.float32
    with np.errstate(all="ignore"):
        Z = (S.astype(t) / dS.astype(t)[None, :] + U.astype(t) / dU.astype(t)[None, :]).astype(np.float64)
    zd, zu = np.percentile(Z, PERC, 0)
    c.update(Z=Z, p99_S=pS, p99_U=pU, down_S=sd, up_S=su, down_Z=zd, up_Z=zu, denom_S=dS, denom_U=dU)
    return c
