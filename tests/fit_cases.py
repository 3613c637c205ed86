"""Constructed inputs for the tests of the weighted-fit kernels (test_fit_oracle.py on the CPU, test_gpu_fit_kernels.py on the
device).  Nothing here is sampled until it lands somewhere: every gene is built from a recipe that aims at one region of the box
[lo_gamma, up_gamma] x [0, 2 sum(wy)/sum(w)], and oracle.fit_box_reference alone says where it landed."""
import functools

import numpy as np

import oracle

LO_GAMMAS = (-1.0, 0.5, 1e-8)          # one launch each; up_gamma is per gene
# The K of the conditioning bound K C eps kappa: the largest err / (C eps kappa) of the oracle's own f64 raw-moment expansion against
# the centred long-double reference over the sweep below, measured on the CPU and pinned by test_fit_oracle.py (0.0074 for m and q,
# 131 for R2).  The kernel gets 4 K: as many roundings, summed in 32 blocks with fma and in another order.
FIT_K, FIT_K_R2 = 0.0075, 135.0
EPS = float(np.finfo(np.float64).eps)


def stored(a, dtype):
    """The values the device holds for `a` in storage type `dtype`, as f64."""
    return np.asarray(a, dtype=np.float64) if dtype == "float64" else np.asarray(a, dtype=np.float32).astype(np.float64)


def _wstats(x, y, w):
    sw = w.sum()
    xb, yb = (w * x).sum() / sw, (w * y).sum() / sw
    return xb, yb, (w * (x - xb) ** 2).sum() / sw, (w * x * y).sum() / (w * x * x).sum()


def _recipe(name, rng, C, w, lo):
    """One gene (x, y, up_gamma) of non-negative data aimed at region `name` for lower bound `lo`."""
    noise = lambda s: rng.normal(0.0, s, C)
    if name in ("m_in/q_in", "m_hi/q_in"):                  # a planted line with a positive offset; up_gamma above or below the slope
        m0 = rng.uniform(max(lo, 0.0) + 0.3, max(lo, 0.0) + 2.0)
        x = rng.uniform(0.2, 4.0, C)
        y = np.abs(m0 * x + rng.uniform(0.5, 2.0) + noise(0.2))
        return x, y, (3.0 * m0 if name == "m_in/q_in" else max(lo, 0.0) + 0.5 * (m0 - max(lo, 0.0)))
    if name == "m_in/q_lo":                                 # a negative intercept: q stops at 0, the slope is free
        m0 = rng.uniform(max(lo, 0.0) + 0.5, max(lo, 0.0) + 2.0)
        x = rng.uniform(0.2, 4.0, C)
        y = np.maximum(m0 * (x - 1.0) + noise(0.1), 0.0)
        return x, y, 20.0
    if name == "m_hi/q_lo":                                 # the same, with up_gamma between ybar/xbar and Sxy/Sxx
        x = rng.uniform(0.2, 4.0, C)
        y = np.maximum(rng.uniform(1.0, 2.0) * (x - 1.0) + noise(0.1), 0.0)
        xb, yb, _, mq0 = _wstats(x, y, w)
        return x, y, 0.5 * (max(yb / xb, lo) + mq0)
    if name == "m_lo/q_lo":                                 # lo above Sxy/Sxx, and ybar - lo xbar < 0
        x = rng.uniform(0.5, 4.0, C)
        y = np.abs(0.2 * lo * x * (1.0 + noise(0.1)))
        return x, y, 20.0
    if name == "m_lo/q_in":                                 # a slope below lo with a large offset
        x = rng.uniform(0.0, 1.0, C)
        y = np.abs(6.0 + (lo - 1.0) * x + noise(0.1))
        return x, y, 20.0
    # the q upper edge: lo < 0, falling lines through data with ybar < xbar
    x = rng.uniform(1.7, 2.3, C)                            # y = a - s x stays positive: x_max <= 1.33 xbar
    xb, _, vx, _ = _wstats(x, x, w)
    if name == "m_lo/q_hi":                                 # y = a - 3x with a in [4 xbar - 2 vx/xbar, 4 xbar] (KKT at the corner), lo = -1
        a = 4.0 * xb - vx / xb
        return x, a - 3.0 * x + noise(0.01), 20.0
    a = 1.3 * xb                                            # y = a - 0.8x: the free intercept a exceeds 2 ybar = 2a - 1.6 xbar
    y = a - 0.8 * x + noise(0.01)
    return x, y, (20.0 if name == "m_in/q_hi" else -0.7)


_RECIPES = {
    -1.0: ("m_in/q_in", "m_in/q_lo", "m_in/q_hi", "m_lo/q_in", "m_lo/q_hi", "m_hi/q_in", "m_hi/q_lo", "m_hi/q_hi"),
    0.5: ("m_in/q_in", "m_in/q_lo", "m_lo/q_in", "m_lo/q_lo", "m_hi/q_in", "m_hi/q_lo"),
    1e-8: ("m_in/q_in", "m_in/q_lo", "m_lo/q_in", "m_hi/q_in", "m_hi/q_lo"),
}


@functools.lru_cache(maxsize=None)
def region_launches(G, C, dtype, wmode):
    """The launches of one case: for each lo_gamma a dict with X, Y, W (G, C) as stored, up (G,) float32-representable, and the
    reference's answer per gene: m, q, region, hi_q.  wmode 0: a W matrix with zeros and unequal weights; wmode 2: w = 1."""
    rng = np.random.default_rng(1000 * G + 10 * C + (dtype == "float32") + 2 * wmode)
    out = []
    for lo in LO_GAMMAS:
        names = _RECIPES[lo]
        X, Y, W, up = np.empty((G, C)), np.empty((G, C)), np.ones((G, C)), np.empty(G)
        off = int(rng.integers(0, len(names))) if G < len(names) else 0      # fewer genes than recipes: start anywhere
        for g in range(G):
            if wmode == 0:
                W[g] = rng.choice([0.0, 0.5, 1.0, 2.0], C, p=[0.3, 0.2, 0.3, 0.2])
                W[g, rng.integers(0, C, 3)] = 1.0
            w = stored(W[g], dtype)
            x, y, u = _recipe(names[(g + off) % len(names)], rng, C, w, lo)
            # (the recipes that read the weighted statistics see them before the storage rounding: the reference below does not)
            X[g], Y[g], up[g] = x, np.maximum(y, 0.0), np.float32(u)
        X, Y, W = stored(X, dtype), stored(Y, dtype), stored(W, dtype)
        m, q, hi_q, region = np.empty(G), np.empty(G), np.empty(G), []
        for g in range(G):
            hi_q[g] = 2.0 * float((np.longdouble(W[g]) * Y[g]).sum() / np.longdouble(W[g]).sum())
            m[g], q[g], r = oracle.fit_box_reference(X[g], Y[g], W[g], lo, up[g], 0.0, hi_q[g])
            region.append(r)
        out.append(dict(lo=lo, X=X, Y=Y, W=W, up=up, m=m, q=q, hi_q=hi_q, region=np.array(region)))
    return out


def census(launches):
    r = np.concatenate([L["region"] for L in launches])
    return {name: int((r == name).sum()) for name in oracle.FIT_REGIONS + ("degenerate",)}


SWEEP_RATIOS = (1.0, 1e1, 1e2, 1e3, 1e4, 1e5)
SWEEP_C = 257


@functools.lru_cache(maxsize=None)
def sweep(dtype, per_ratio=40):
    """The conditioning sweep: x = r + N(0, 1), y a planted line inside the default box, C = 257, unequal weights; the
    reference's (m, q, R2) and the condition numbers per gene."""
    rng = np.random.default_rng(77)
    G, C = per_ratio * len(SWEEP_RATIOS), SWEEP_C
    ratio = np.repeat(SWEEP_RATIOS, per_ratio)
    X = np.abs(ratio[:, None] + rng.normal(size=(G, C)))
    m0 = rng.uniform(0.3, 2.0, G)
    Y = m0[:, None] * X + (0.3 * ratio + 1.0)[:, None] + rng.normal(0.0, 0.5, (G, C))
    W = rng.choice([0.0, 0.5, 1.0, 2.0], (G, C), p=[0.3, 0.2, 0.3, 0.2])
    X, Y, W = stored(X, dtype), stored(Y, dtype), stored(W, dtype)
    ref = np.empty((G, 3))
    cond = np.empty((G, 4))
    hi_q = np.empty(G)
    region = []
    for g in range(G):
        hi_q[g] = 2.0 * float((np.longdouble(W[g]) * Y[g]).sum() / np.longdouble(W[g]).sum())
        m, q, r = oracle.fit_box_reference(X[g], Y[g], W[g], 1e-8, 20.0, 0.0, hi_q[g])
        ref[g] = m, q, oracle.r2_reference(m, q, X[g], Y[g])
        cond[g] = oracle.fit_condition(X[g], Y[g], W[g])
        region.append(r)
    return dict(X=X, Y=Y, W=W, ratio=ratio, ref=ref, cond=cond, hi_q=hi_q, region=np.array(region))


def sweep_bounds(s, K, K_r2):
    """|m - m_ref|, |q - q_ref| <= K C eps kappa_fit (x scale_m, scale_q), |R2 - R2_ref| <= K_r2 C eps kappa_r2."""
    kf, kr, sm, sq = s["cond"].T
    u = SWEEP_C * EPS
    return K * u * kf * sm, K * u * kf * sq, K_r2 * u * kr
