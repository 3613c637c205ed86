"""Reference, error bound, branch classifier and constructed inputs for the tests of the kNN search (csrc/knn.hip, ops.knn_search /
ops.knn_query): test_knn_oracle.py on the CPU, test_gpu_knn_kernels.py on the device.  DESIGN section 13 states the contract.

Nothing here runs the code under test.  The reference is a plain f64 loop in feature order, the bound is computed from the data in
f64, and the classifier restates the documented selection rule of the row-free kernel in numpy; it is used only to assert that a
constructed input reaches the branch it was built for."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24                                         # unit roundoff of the candidate pass
INF_BITS = 0x7f800000
CONTRACT_MARGIN = 8                                      # ksel = min(k + 8, avail), whatever knn.hip's KNN_MARGIN says
UNDECIDABLE_CAP = 0.01                                   # of a case's queries, outside the designated ones


@functools.lru_cache(maxsize=None)
def constants():
    """KNN_QB, KNN_MAXSEL, KNN_MARGIN, KNN_NC as csrc/knn.hip declares them."""
    text = open(os.path.join(ROOT, "velocyto.py_amd", "csrc", "knn.hip")).read()
    c = dict((k, int(v)) for k, v in re.findall(r"constexpr int (KNN_[A-Z]+) = (\d+);", text))
    assert set(c) >= {"KNN_QB", "KNN_MAXSEL", "KNN_MARGIN", "KNN_NC"}, c
    return c


def plan(C, k, include_self=True):
    """The documented launch plan: candidates kept (ksel), sort length (nsort), sort in global memory (large), bits of the slice
    position (nb), and whether the search runs without distance rows (row_free)."""
    c = constants()
    avail = C if include_self else C - 1
    ksel = min(k + c["KNN_MARGIN"], avail)
    nsort = 128
    while nsort < 4 * ksel and nsort < c["KNN_MAXSEL"]:
        nsort <<= 1
    while nsort < ksel:
        nsort <<= 1
    large = nsort > c["KNN_MAXSEL"]
    nb = 1
    while (1 << nb) < (C + 255) // 256 + c["KNN_NC"]:
        nb += 1
    return dict(ksel=ksel, nsort=nsort, large=large, nb=nb, row_free=not (large or ksel > 128 or nb > 10))


# ---------------------------------------------------------------- reference
def _sq_dists(points, queries):
    """(Q, C) squared distances: sums of rounded squares in feature order, an explicit loop over the features."""
    X, Qm = np.asarray(points, dtype=np.float64), np.asarray(queries, dtype=np.float64)
    d2 = np.zeros((Qm.shape[0], X.shape[0]))
    for p in range(X.shape[1]):
        df = Qm[:, p][:, None] - X[:, p][None, :]
        d2 = d2 + df * df
    return d2


def knn_reference(points, queries, k, exclude=None):
    """(idx int64 (Q, k), dist (Q, k), d2 (Q, k)): the k nearest of `points` for every row of `queries`, ordered by (distance, index);
    exclude[i] is the candidate query i may not return (its own row), or None."""
    d2 = _sq_dists(points, queries)
    if exclude is not None:
        d2[np.arange(d2.shape[0]), np.asarray(exclude)] = np.inf
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]                     # stable: equal distances stay in index order
    s = np.take_along_axis(d2, idx, 1)
    assert np.isfinite(s).all()
    return idx, np.sqrt(s), s


# ---------------------------------------------------------------- the f32 pass and its bound
def frame(points):
    """(c, e): the per-feature midpoint of the point set and the exponent of its largest half-range m, 1 <= m 2^-e < 2; e is kept
    within the normal range of f64 (-1022 for a point set of zero or subnormal extent, at most 1022)."""
    X = np.asarray(points, dtype=np.float64)
    mn, mx = X.min(0), X.max(0)
    c = (mn + mx) * 0.5
    m = float((mx - mn).max() * 0.5)
    e = int(np.clip(np.frexp(m)[1] - 1, -1022, 1022)) if m > 0 else -1022
    return c, e


def f32_copy(points, queries=None):
    """The f32 images the candidate pass reads: (x - c) 2^-e rounded to f32, the queries in the frame of the POINT set."""
    c, e = frame(points)
    x32 = np.ldexp(np.asarray(points, dtype=np.float64) - c, -e).astype(np.float32)
    q32 = None if queries is None else np.ldexp(np.asarray(queries, dtype=np.float64) - c, -e).astype(np.float32)
    return x32, q32, e


def emulate_s32(x32, q32):
    """(Q, C) f32 squared distances as the kernel's pass forms them: df = q - x in f32, acc = fmaf(df, df, acc) in feature order.
    The fused step is done in f64 (the product of two f32 is exact there) and rounded once more to f32: a double rounding that can
    differ from a true fmaf by one ulp in rare cases, which is why no class is planted within an ulp of its boundary."""
    acc = np.zeros((q32.shape[0], x32.shape[0]), dtype=np.float32)
    for p in range(x32.shape[1]):
        df = (q32[:, p][:, None] - x32[:, p][None, :]).astype(np.float64)
        acc = (df * df + acc.astype(np.float64)).astype(np.float32)
    return acc


def f32_error_bound(points, queries):
    """(E, s), both (Q, C): |s32 - s| <= E for ANY f32 pass that takes differences of the centred coordinates first,
         e_p = u (|q_p| + |x_p| + |df_p|),   E = 2 [ sum_p (2 |df_p| e_p + e_p^2) + (P + 1) u s ],
    coordinates relative to the midpoint of the point set, u = 2^-24: one rounding of each coordinate, one of the difference, P
    roundings of the running sum and one to spare; the leading 2 covers the second-order terms."""
    X, Qm = np.asarray(points, dtype=np.float64), np.asarray(queries, dtype=np.float64)
    c, _ = frame(X)
    Xc, Qc = X - c, Qm - c
    P = X.shape[1]
    lin = np.zeros((Qm.shape[0], X.shape[0]))
    s = np.zeros_like(lin)
    for p in range(P):
        q, x = Qc[:, p][:, None], Xc[:, p][None, :]
        df = np.abs(q - x)
        e = U32 * (np.abs(q) + np.abs(x) + df)
        lin = lin + (2.0 * df * e + e * e)
        s = s + df * df
    return 2.0 * (lin + (P + 1) * U32 * s), s


def _mask_excluded(a, exclude, value):
    if exclude is not None:
        a[np.arange(a.shape[0]), np.asarray(exclude)] = value
    return a


def analyse(points, queries, k, exclude=None):
    """Everything the checks need, computed once: the reference lists, s and E, which queries are f32-decidable and the bound of
    property (b).  A query is decidable when #{ j : s_j - E_j <= max_{i in true top-k} (s_i + E_i) } <= ksel = min(k + 8, avail):
    no member of the true list can then be pushed past rank ksel by the f32 pass."""
    C = np.asarray(points).shape[0]
    avail = C if exclude is None else C - 1
    ksel = min(k + CONTRACT_MARGIN, avail)
    E, s = f32_error_bound(points, queries)
    lo = _mask_excluded(s - E, exclude, np.inf)
    hi = _mask_excluded(s + E, exclude, np.inf)
    full = _mask_excluded(_sq_dists(points, queries), exclude, np.inf)   # knn_reference's sums and order, sorted once to rank ksel
    order = np.argsort(full, axis=1, kind="stable")[:, :ksel]
    idx = order[:, :k]
    d2 = np.take_along_axis(full, idx, 1)
    dist = np.sqrt(d2)
    thr_k = np.take_along_axis(hi, idx, 1).max(1)
    count = (lo <= thr_k[:, None]).sum(1)
    thr_sel = np.take_along_axis(hi, order, 1).max(1)
    return dict(idx=idx, dist=dist, d2=d2, lo=lo, thr_sel=thr_sel, count=count, ksel=ksel, decidable=count <= ksel, k=k,
                points=np.asarray(points, dtype=np.float64), queries=np.asarray(queries, dtype=np.float64), exclude=exclude)


def decidable(points, queries, k, exclude=None):
    return analyse(points, queries, k, exclude)["decidable"]


def check_contract(an, idx, dist, designated=(), what=""):
    """Contract of DESIGN section 13 on one result.  (a) on every decidable query: the reference's lists, bit for bit.  (b) on every
    query: distances are the exact f64 distances of the returned indices, rows sorted by (distance, index), no repeats, the excluded
    candidate absent, and every returned j within the f32 reach of the true top-ksel.  `designated`: the queries the case was built
    to leave undecidable; outside them at most UNDECIDABLE_CAP of the queries may be undecidable.  Returns the number of queries
    whose lists differ from the reference (all of them undecidable)."""
    idx, dist = np.asarray(idx).astype(np.int64), np.asarray(dist, dtype=np.float64)
    Q, k = an["idx"].shape
    assert idx.shape == (Q, k) and dist.shape == (Q, k), what
    dec = an["decidable"]
    stray = np.setdiff1d(np.nonzero(~dec)[0], np.asarray(list(designated), dtype=np.int64))
    assert stray.size <= UNDECIDABLE_CAP * Q, (what, "undecidable outside the designated queries", stray[:10])

    # (a)
    assert np.array_equal(idx[dec], an["idx"][dec]), (what, "indices of a decidable query", np.nonzero((idx != an["idx"]).any(1) & dec)[0][:10])
    assert np.array_equal(dist[dec], an["dist"][dec]), (what, "distances of a decidable query")
    # (b)
    assert (idx >= 0).all() and (idx < an["points"].shape[0]).all(), what
    own = np.zeros((Q, k))
    for p in range(an["points"].shape[1]):
        df = an["queries"][:, p][:, None] - an["points"][idx, p]
        own = own + df * df
    assert np.array_equal(dist, np.sqrt(own)), (what, "distances are not those of the returned indices")
    if k > 1:
        dd, di = np.diff(own, axis=1), np.diff(idx, axis=1)
        assert ((dd > 0) | ((dd == 0) & (di > 0))).all(), (what, "rows not sorted by (distance, index), or an index repeats")
    if an["exclude"] is not None:
        assert (idx != np.asarray(an["exclude"])[:, None]).all(), (what, "the excluded query came back")
    reach = np.take_along_axis(an["lo"], idx, 1) <= an["thr_sel"][:, None]
    assert reach.all(), (what, "a returned candidate is beyond the f32 reach of the true top-ksel", np.nonzero(~reach.all(1))[0][:10])
    return int((idx != an["idx"]).any(1).sum())


# ---------------------------------------------------------------- branch classifier of the row-free kernel
def classify(points, q, k, include_self=False, query=None, jitter=None):
    """Which way the row-free kernel takes query `q` (a row of `points`; `query`: an external query vector instead, nothing excluded):
    `direct` (threshold from the two smallest words per thread, candidates from the four tracked words), `rescan` (1..8 threads whose
    fourth word is within the threshold hand their slice over), `row_overflow` (more than 8 such threads), `row_count` (more candidates
    within the threshold than the sort holds) or `row_inf` (fewer than ksel finite local minima).  jitter: a numpy Generator that moves
    every f32 distance by -1, 0 or +1 ulp - a class that survives it does not hang on the last bit of the emulation."""
    X = np.asarray(points, dtype=np.float64)
    C = X.shape[0]
    external = query is not None
    pl = plan(C, k, include_self or external)
    assert pl["row_free"], "the rule below is the row-free kernel's"
    nb, ksel, nsort = pl["nb"], pl["ksel"], pl["nsort"]
    x32, q32, _ = f32_copy(X, np.asarray(query, dtype=np.float64)[None, :] if external else X[q:q + 1])
    bits = emulate_s32(x32, q32)[0].view(np.uint32).astype(np.int64)
    finite = bits < INF_BITS
    if jitter is not None:
        bits = np.clip(bits + jitter.integers(-1, 2, size=C), 0, None)
    j = np.arange(C)
    lowmask = (1 << nb) - 1
    tracked = finite.copy()
    if not (include_self or external):
        tracked[q] = False
    words = np.where(tracked, (bits & ~lowmask) | (j >> 8), 0xffffffff)
    nslice = max((C + 255) // 256, 4)
    grid = np.full(nslice * 256, 0xffffffff, dtype=np.int64)
    grid[:C] = words
    four = np.sort(grid.reshape(nslice, 256), axis=0)[:4]                 # per thread (column): its four smallest words
    T = np.sort(four[:2].ravel())[ksel - 1]
    if T >= INF_BITS:
        return "row_inf"
    Tm = (T >> nb) + 1
    over = (four[3] >> nb) <= Tm
    nover = int(over.sum())
    if nover > 8:
        return "row_overflow"
    count = int(((four[:, ~over] >> nb) <= Tm).sum())
    hi = np.where(tracked, bits >> nb, 1 << 40)
    for t in np.nonzero(over)[0]:
        count += int((hi[t::256] <= Tm).sum())
    if count > nsort:
        return "row_count"
    return "rescan" if nover else "direct"


def classify_stable(points, q, k, **kw):
    """The class of classify(), asserted to survive three draws of one-ulp jitter."""
    cls = classify(points, q, k, **kw)
    for seed in range(3):
        assert classify(points, q, k, jitter=np.random.default_rng(seed), **kw) == cls, (cls, seed)
    return cls


# ---------------------------------------------------------------- constructed inputs
def _unit(rng, n, P):
    v = rng.normal(size=(n, P))
    return v / np.sqrt((v * v).sum(1))[:, None]


PLAN_C, PLAN_P, PLAN_Q0, PLAN_Q = 4500, 3, 1000, 19
PLAN_K = (24, 25, 120, 121, 504, 505, 1016, 1017, 4088, 4089)
PLAN_DUPES = (962, 1002)                                 # a block of 40 exact duplicates: queries 1000 and 1001 are two of them
PLAN_UNDECIDABLE = {24: (0, 1), 25: (0, 1)}               # by the count: 39 candidates at distance 0 against ksel = 32 / 33
PLAN_ROUNDED = (1010, 1310)                              # 300 points rounded to one decimal: queries 1010..1018 sit on that lattice


@functools.lru_cache(maxsize=None)
def plan_points():
    rng = np.random.default_rng(20)
    x = rng.normal(size=(PLAN_C, PLAN_P))
    x[PLAN_DUPES[0]:PLAN_DUPES[1]] = x[PLAN_DUPES[0]]
    a, b = PLAN_ROUNDED
    x[a:b] = np.round(0.3 * x[a:b], 1)
    x.setflags(write=False)
    return x


BLOCK_Q0, BLOCK_Q = 900, 203                             # the queries of the planted cases: rows 900..1102, the constructed one (row 1000) among them
OVER_C, OVER_P, OVER_K, OVER_Q = 2600, 6, 40, 1000
OVER_TIDS = (7, 19, 33, 58, 91, 120, 150, 201, 240)
OVER_CLASS = {0: "direct", 1: "rescan", 8: "rescan", 9: "row_overflow"}


@functools.lru_cache(maxsize=None)
def overflow_points(n):
    """Five near neighbours of query OVER_Q in the slice of each of the first n thread ids of OVER_TIDS."""
    rng = np.random.default_rng(31)
    x = rng.normal(size=(OVER_C, OVER_P)) * 5.0
    step = 0
    for t in OVER_TIDS[:n]:
        for m in (0, 2, 4, 6, 8):
            step += 1
            x[t + 256 * m] = x[OVER_Q] + 1e-3 * step * _unit(rng, 1, OVER_P)[0]
    x.setflags(write=False)
    return x


COUNT_C, COUNT_P, COUNT_K, COUNT_Q = 2600, 6, 12, 1000
COUNT_SHELL = 300


@functools.lru_cache(maxsize=None)
def count_points():
    """Twelve clear neighbours of query COUNT_Q, then 300 points within 5e-7 relative radius at ranks 13..312, at most two per slice:
    no thread tracks a fourth word within the threshold, but more words are within it than a sort of 128 holds.  The query sits on
    the midpoint of the point set, where the f32 images of its neighbours keep the shell as thin as it is (their coordinates ARE the
    displacements); elsewhere the rounding of the coordinates spreads the f32 distances of the shell over ten steps of the threshold."""
    rng = np.random.default_rng(32)
    x = rng.normal(size=(COUNT_C, COUNT_P)) * 5.0
    x[COUNT_Q] = (x.min(0) + x.max(0)) * 0.5
    clear = [3 + 20 * i for i in range(12)]                               # twelve different slices
    shell = [t + 256 * m for m in (1, 3) for t in range(256) if t + 256 * m != COUNT_Q][:COUNT_SHELL]
    assert not set(clear) & set(shell) and COUNT_Q not in clear
    for i, j in enumerate(clear):
        x[j] = x[COUNT_Q] + 0.01 * (1 + 0.1 * i) * _unit(rng, 1, COUNT_P)[0]
    radii = 0.1 * (1.0 + 5e-7 * rng.random(COUNT_SHELL))
    x[shell] = x[COUNT_Q] + radii[:, None] * _unit(rng, COUNT_SHELL, COUNT_P)
    x.setflags(write=False)
    return x


CAP_C, CAP_P, CAP_Q, CAP_K = 261120, 2, 16, (12, 120)
CAP_PLANT = {12: 40, 120: 140}


@functools.lru_cache(maxsize=None)
def cap_points(nplant):
    """CAP_C + 1 points (the first CAP_C are the row-free kernel's largest launch: slice positions up to 1019; all of them is the
    rows kernel's smallest that the position bits force).  Rows CAP_C - 16 .. CAP_C - 1 are the queries, on a circle of radius 5 far
    from everything else; `nplant` points within 0.5 of its centre sit at indices CAP_C - 1 - 256 m, m up to 1019: ONE thread's slice
    (CAP_PLANT: enough to fill the lists, few enough for the sort that k asks for)."""
    rng = np.random.default_rng(33)
    x = rng.random((CAP_C + 1, CAP_P)) * 1000.0
    centre = np.array([-300.0, -300.0])
    ang = 2 * np.pi * (np.arange(CAP_Q) + 0.25 * rng.random(CAP_Q)) / CAP_Q
    x[CAP_C - CAP_Q:CAP_C] = centre + 5.0 * np.stack([np.cos(ang), np.sin(ang)], 1)
    planted = CAP_C - 1 - 256 * (1019 - (970 // nplant) * np.arange(nplant))
    assert planted.min() == CAP_C - 1 - 256 * 1019 == 255 and np.unique(planted).size == nplant and planted.max() < CAP_C - CAP_Q and (planted % 256 == 255).all()
    x[planted] = centre + 0.5 * np.sqrt(rng.random(nplant))[:, None] * _unit(rng, nplant, CAP_P)
    x[CAP_C] = (2000.0, 2000.0)
    x.setflags(write=False)
    return x


SEGMENT = 1008 * 256                                     # ops.KNN_SEGMENT: the most candidates ops gives one launch
SEGMENT_Q, SEGMENT_K = 24, 12


@functools.lru_cache(maxsize=None)
def segment_points():
    """SEGMENT + 1 points: the last SEGMENT rows of cap_points before its far point (a shift by a multiple of 256: the planted
    neighbours stay in one slice), the last 24 of them the queries, then the far point."""
    x = cap_points(CAP_PLANT[SEGMENT_K])
    x = np.concatenate([x[CAP_C - SEGMENT:CAP_C], x[CAP_C:]])
    x.setflags(write=False)
    return x


def _dyadic(rng, C, P):
    return np.round(rng.normal(size=(C, P)) * 4096.0) / 4096.0           # unit spread on a 2^-12 grid


PRECISION_C, PRECISION_K = 1000, 30
# name -> (P, shift exponent, scale exponent): dyadic data + 2^shift, then x 2^scale; every operation exact in f64
TRANSLATED = {"2d_shift10": (2, 10, 0), "2d_shift20": (2, 20, 0), "6d_shift10": (6, 10, 0), "6d_shift20": (6, 20, 0)}
# (at 2^-70 the squares of an unscaled f32 copy are subnormal and still order the neighbours; at 2^-90 they are all zero)
SCALED = {f"{P}d_scale{s:+d}": (P, 10, s) for P in (2, 6) for s in (40, -40, 70, -70, 90, -90)}


@functools.lru_cache(maxsize=None)
def dyadic_points(name):
    P, shift, scale = {**TRANSLATED, **SCALED}[name]
    base = _dyadic(np.random.default_rng(40 + P), PRECISION_C, P)
    x = np.ldexp(base + 2.0 ** shift, scale)
    assert np.array_equal(np.ldexp(x, -scale) - 2.0 ** shift, base)       # exact: the neighbour lists are those of `base`
    x.setflags(write=False)
    return x


SHELL_C, SHELL_P, SHELL_K, SHELL_Q, SHELL_A = 1500, 6, 20, 1000, 3
SHELL_B = {"decidable": (8,), "undecidable": (9, 40)}


@functools.lru_cache(maxsize=None)
def shell_points(b):
    """Query SHELL_Q: k - a clear neighbours, then a + b points at radii 0.5 (1 + 1e-9 i) straddling rank k (a inside, b beyond)."""
    rng = np.random.default_rng(50 + b)
    x = rng.normal(size=(SHELL_C, SHELL_P)) * 5.0
    free = [j for j in rng.permutation(SHELL_C) if j != SHELL_Q]
    nclear, nshell = SHELL_K - SHELL_A, SHELL_A + b
    clear, shell = free[:nclear], free[nclear:nclear + nshell]
    x[clear] = x[SHELL_Q] + (0.1 + 0.2 * np.arange(nclear) / nclear)[:, None] * _unit(rng, nclear, SHELL_P)
    x[shell] = x[SHELL_Q] + (0.5 * (1.0 + 1e-9 * np.arange(nshell)))[:, None] * _unit(rng, nshell, SHELL_P)
    x.setflags(write=False)
    return x


STRICT_K = 125                                           # ksel = 133 > 128: the rows kernel, threshold from the local minima


@functools.lru_cache(maxsize=None)
def strict_shell_points():
    """The shell of 3 + 8 where the select is STRICT.  Query SHELL_Q, 122 clear neighbours and the shell all in different slices,
    so the rows kernel's threshold (the ksel-th of the two smallest per thread) IS the ksel-th smallest f32 distance and exactly
    ksel = k + 8 candidates pass: the 122, and the 11 of the shell.  The shell member that the f32 pass ranks LAST gets the smallest
    radius, so it belongs to the true list: one candidate fewer and it is lost.  strict_shell_margin() measures that on the CPU."""
    rng = np.random.default_rng(66)                       # a draw that leaves the last two of the f32 order 7 ulps apart
    x = rng.normal(size=(SHELL_C, SHELL_P)) * 5.0
    nclear, nshell = STRICT_K - SHELL_A, SHELL_A + SHELL_B["decidable"][0]
    near = np.array([i + 256 * (i % 5) for i in range(nclear + nshell)])             # one per slice
    assert SHELL_Q not in near and np.unique(near % 256).size == near.size and near.max() < SHELL_C
    clear, shell = near[:nclear], near[nclear:]
    x[clear] = x[SHELL_Q] + (0.1 + 0.2 * np.arange(nclear) / nclear)[:, None] * _unit(rng, nclear, SHELL_P)
    dirs = _unit(rng, nshell, SHELL_P)
    x[shell] = x[SHELL_Q] + 0.5 * dirs
    x32, q32, _ = f32_copy(x, x[SHELL_Q:SHELL_Q + 1])
    last_first = np.argsort(-emulate_s32(x32[shell], q32)[0], kind="stable")           # the f32 pass's last gets radius number 0
    radii = np.empty(nshell)
    radii[last_first] = 0.5 * (1.0 + 1e-9 * np.arange(nshell))
    x[shell] = x[SHELL_Q] + radii[:, None] * dirs
    x.setflags(write=False)
    return x


def strict_shell_margin():
    """(rank of the true list's last-ranked member in the emulated f32 order, 1-based; its distance in f32 ulps from the candidate
    ranked just before it) for query SHELL_Q of strict_shell_points()."""
    x = strict_shell_points()
    x32, q32, _ = f32_copy(x, x[SHELL_Q:SHELL_Q + 1])
    s32 = emulate_s32(x32, q32)[0]
    s32[SHELL_Q] = np.inf
    order = np.argsort(s32, kind="stable")
    truth = knn_reference(x, x[SHELL_Q:SHELL_Q + 1], STRICT_K, [SHELL_Q])[0][0]
    rank = int(np.nonzero(np.isin(order, truth))[0].max()) + 1
    bits = s32.view(np.uint32).astype(np.int64)
    return rank, int(bits[order[rank - 1]] - bits[order[rank - 2]])


LATTICE_N, LATTICE_INNER = 12, 512
LATTICE_K = {"decidable": 32, "undecidable": 35}


@functools.lru_cache(maxsize=None)
def lattice_points():
    """A 12^3 lattice of step 0.1, the 8^3 points at least two steps from every face first (rows 0..511, the queries).  Around such a
    point the shells hold 6, 12, 8, 6, 24 points: rank 32 ends a shell, rank 35 is three points into the shell of 24."""
    g = np.arange(LATTICE_N)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    inner = ((ijk >= 2) & (ijk <= LATTICE_N - 3)).all(1)
    ijk = np.concatenate([ijk[inner], ijk[~inner]])
    assert int(inner.sum()) == LATTICE_INNER
    x = ijk / 10.0
    x.setflags(write=False)
    return x


CLUSTER_C, CLUSTER_K = 1500, 20
CLUSTER_SPREAD = (2.0 ** -14, 2.0 ** -18)


@functools.lru_cache(maxsize=None)
def cluster_points(spread):
    """Two clusters at (+-2^8, +-2^8) of the given spread: the midpoint is between them, so the f32 images are quantised to 2^-16
    whatever the frame - coarser than the distances inside a cluster."""
    rng = np.random.default_rng(60)
    x = rng.normal(size=(CLUSTER_C, 2)) * spread
    x[::2] += 256.0
    x[1::2] -= 256.0
    x.setflags(write=False)
    return x


OUTSIDE_C, OUTSIDE_P, OUTSIDE_Q, OUTSIDE_K = 1000, 3, 64, 20


@functools.lru_cache(maxsize=None)
def outside_points():
    """(points, queries): the queries 30 to 60 spreads away from the point set, in every direction."""
    rng = np.random.default_rng(70)
    x = rng.normal(size=(OUTSIDE_C, OUTSIDE_P))
    q = (30.0 + 30.0 * rng.random(OUTSIDE_Q))[:, None] * _unit(rng, OUTSIDE_Q, OUTSIDE_P)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


STRIDE_C, STRIDE_P, STRIDE_K, STRIDE_NQ = 700, 5, 20, 40


@functools.lru_cache(maxsize=None)
def stride_points():
    """(points, external queries) of the stride tests."""
    rng = np.random.default_rng(90)
    x, q = rng.normal(size=(STRIDE_C, STRIDE_P)), rng.normal(size=(STRIDE_NQ, STRIDE_P))
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


FEATURE_C, FEATURE_K = 300, 20
FEATURE_P = (1, 4, 5, 257, 1024)


@functools.lru_cache(maxsize=None)
def feature_points(P):
    x = np.random.default_rng(80 + P).normal(size=(FEATURE_C, P))
    x.setflags(write=False)
    return x


def self_exclude(q0, Q):
    return np.arange(q0, q0 + Q)


@functools.lru_cache(maxsize=None)
def analysed(case, *args):
    """analyse() of a named self-search case (all queries unless said), made once and shared between the tests."""
    if case == "plan":                                                    # args: k, include_self
        k, inc = args
        x = plan_points()
        return analyse(x, x[PLAN_Q0:PLAN_Q0 + PLAN_Q], k, None if inc else self_exclude(PLAN_Q0, PLAN_Q))
    if case == "cap":                                                     # args: C, k
        C, k = args
        x = cap_points(CAP_PLANT[k])[:C]
        return analyse(x, x[CAP_C - CAP_Q:CAP_C], k, self_exclude(CAP_C - CAP_Q, CAP_Q))
    if case == "segment":                                                 # args: C
        x = segment_points()[:args[0]]
        return analyse(x, x[SEGMENT - SEGMENT_Q:SEGMENT], SEGMENT_K, self_exclude(SEGMENT - SEGMENT_Q, SEGMENT_Q))
    if case == "lattice":
        x = lattice_points()
        return analyse(x, x[:LATTICE_INNER], args[0], self_exclude(0, LATTICE_INNER))
    if case == "outside":
        x, q = outside_points()
        return analyse(x, q, OUTSIDE_K)
    if case == "cluster":
        x = cluster_points(*args)
        return analyse(x, x, CLUSTER_K, self_exclude(0, CLUSTER_C))
    if case == "dyadic":
        x = dyadic_points(*args)
        return analyse(x, x, PRECISION_K, self_exclude(0, PRECISION_C))
    if case == "feature":
        x = feature_points(*args)
        return analyse(x, x, FEATURE_K, self_exclude(0, FEATURE_C))
    x, k = {"overflow": lambda: (overflow_points(*args), OVER_K), "count": lambda: (count_points(), COUNT_K),
            "strict": lambda: (strict_shell_points(), STRICT_K), "shell": lambda: (shell_points(*args), SHELL_K)}[case]()
    return analyse(x, x[BLOCK_Q0:BLOCK_Q0 + BLOCK_Q], k, self_exclude(BLOCK_Q0, BLOCK_Q))
