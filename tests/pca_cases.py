"""Shared by tests/test_pca_products_oracle.py, tests/test_gpu_pca_kernels.py and tests/pca_products_worker.py: the extended-precision
references of the PCA products of csrc/gram.hip (vcy_col_means, vcy_gram, vcy_gram_tn, vcy_gemm_nt), their derived error bounds, the
inputs and the case lists.

The references work on the STORED values (f32 storage converted exactly) in np.longdouble where it carries 64 mantissa bits, else in
double-double arithmetic (TwoSum / Dekker's TwoProduct, vectorised over the output); `FORCE_DD` runs the second where the first exists.
A reference is returned as an unevaluated pair (hi, lo) of fp64 arrays, hi + lo = the extended value: the same type whichever
arithmetic produced it.  Its own error is (K + c) 2^-64 of the absolute-term sum S at most (longdouble: one rounding per product, per
addition and per centring) and far less in double-double.

The bounds.  u = 2^-53, gamma(n) = n u / (1 - n u).  K numbers t_k, each the fp64 result of c_k roundings applied to an exact term,
accumulated in fp64 in ANY order - in slabs, over lanes of a matrix instruction, split over workgroups and folded afterwards - give
    computed = sum_k t_k (1 + theta_k),   |theta_k| <= gamma(r_k),
r_k the number of roundings on the path of term k to the result (Higham, Accuracy and Stability, lemma 3.1 and section 4.2: the bound
holds for every order of summation).  A term passes through at most K - 1 additions however they are grouped (a split of the cells
into ks partial sums of at most K_s terms and a fold of ks partials is K_s - 1 + ks - 1 <= K - 1; adding to the zero an accumulator
starts from, or adding the exact zeros of padded slabs, rounds nothing), one rounding of its product and c roundings before it:
    |computed - exact| <= gamma(K + c) S,   S = sum_k |exact term k|.
    gram     term (x_ci - m_i)(x_cj - m_j):  c = 2, the two centring subtractions (c = 0 without a mean); K = C cells
    gram_tn  term (x_ci - m_i) y_cj:         c = 1 (0 without a mean); K = C
    gemm_nt  out = ((sum_g a_ig b_jg - rc_i) - cc_j) + c0: the three corrections are three further additions, each rounding everything
             summed before it, so c = 3 and S = sum_g |a_ig b_jg| + |rc_i| + |cc_j| + |c0|; K = the gene count padded to the 64-element
             row pitch (an upper limit of every slab width: the zeros beyond K add exactly).  A product centred by algebra
             (col_corr = B m) is held to the reference of the expression AS STATED, with the stored col_corr, and so to the UNCENTRED
             absolute sum - the expansion's own error, documented in the kernel's header.
    col_means  sum over ceil(C / nb) rows per block, a fold of nb <= C partials, one division: at most C + 1 roundings per term,
             |mean - exact| <= gamma(C + 1) sum_c |x_cg| / C.
The reference's own error is added: bound = (gamma(K + c) + (K + c) 2^-64) S.  S is evaluated in plain fp64 (relative error
gamma(K + 2) < 2^-40 for every K here) and multiplied by 1 + 2^-40.  Nothing in a bound is fitted to what a kernel returns.

Exact cases need no bound: integers |x| <= 8, integer means |m| <= 3, integer Y, B and corrections keep every product and every partial
sum an integer far below 2^53, so every order of summation in every kernel form must give the int64 result bit for bit."""
import functools

import numpy as np

U = 2.0 ** -53
HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63
FORCE_DD = False                   # tests/test_pca_products_oracle.py flips this to pin the double-double path where longdouble exists
S_SLACK = 1.0 + 2.0 ** -40


def gamma(n):
    return n * U / (1.0 - n * U)


def bound_factor(n):
    """gamma(n) of the fp64 kernel plus n 2^-64 of the reference itself."""
    return gamma(n) + n * 2.0 ** -64


# ------------------------------------------------------------------------------------------------------------- extended arithmetic
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    h = c - (c - a)
    return h, a - h


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _use_dd():
    return FORCE_DD or not HAVE_LONGDOUBLE


def _centred(X, m):
    """x - m as a pair (hi, lo): exact in double-double; the longdouble path adds the two (one rounding to 64 bits)."""
    X = np.asarray(X, dtype=np.float64)
    if m is None:
        return X, None
    return _two_sum(X, -np.asarray(m, dtype=np.float64)[None, :])


def _ext_tn(P, Plo, Q, Qlo):
    """sum_k (P + Plo)[k, i] (Q + Qlo)[k, j] -> (hi, lo)."""
    if not _use_dd():
        ld = np.longdouble
        Pe = P.astype(ld) if Plo is None else P.astype(ld) + Plo.astype(ld)
        Qe = Q.astype(ld) if Qlo is None else Q.astype(ld) + Qlo.astype(ld)
        R = Pe.T @ Qe
        hi = R.astype(np.float64)
        return hi, (R - hi.astype(ld)).astype(np.float64)
    hi = np.zeros((P.shape[1], Q.shape[1]))
    lo = np.zeros_like(hi)
    for k in range(P.shape[0]):
        a, b = P[k][:, None], Q[k][None, :]
        p, e = _two_prod(a, b)
        if Plo is not None:
            e = e + Plo[k][:, None] * b
        if Qlo is not None:
            e = e + a * Qlo[k][None, :]
        s, t = _two_sum(hi, p)
        lo = lo + (t + e)
        hi, lo = _two_sum(s, lo)
    return hi, lo


def _ext_add(pair, v):
    """pair + v, v an fp64 array that broadcasts."""
    hi, lo = pair
    v = np.broadcast_to(np.asarray(v, dtype=np.float64), hi.shape)
    if not _use_dd():
        ld = np.longdouble
        R = hi.astype(ld) + lo.astype(ld) + v.astype(ld)
        h = R.astype(np.float64)
        return h, (R - h.astype(ld)).astype(np.float64)
    s, t = _two_sum(hi, v)
    return _two_sum(s, lo + t)


def error_against(got, ref):
    """|got - (hi + lo)| in fp64: got - hi is exact wherever the two are within a factor of two (Sterbenz), and where they are not the
    difference is far above any bound anyway."""
    hi, lo = ref
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)


# ------------------------------------------------------------------------------------------------------------------ the references
def col_means_reference(X):
    """X (C, G) fp64 array of the stored values -> (mean pair, S = sum_c |x_cg| / C)."""
    X = np.asarray(X, dtype=np.float64)
    C = X.shape[0]
    ones = np.ones((C, 1))
    hi, lo = _ext_tn(X, None, ones, None)
    hi, lo = hi[:, 0], lo[:, 0]
    if not _use_dd():
        ld = np.longdouble
        R = (hi.astype(ld) + lo.astype(ld)) / ld(C)
        h = R.astype(np.float64)
        pair = (h, (R - h.astype(ld)).astype(np.float64))
    else:                                                            # (hi + lo) / C: quotient of the head, one correction from the remainder
        q = hi / C
        p, e = _two_prod(q, np.float64(C))
        r = ((hi - p) - e) + lo
        pair = _two_sum(q, r / C)
    return pair, np.abs(X).sum(0) / C * S_SLACK


def gram_reference(X, mean):
    Ph, Pl = _centred(X, mean)
    A = np.abs(Ph)
    return _ext_tn(Ph, Pl, Ph, Pl), (A.T @ A) * S_SLACK


def gram_tn_reference(X, mean, Y):
    Ph, Pl = _centred(X, mean)
    Y = np.asarray(Y, dtype=np.float64)
    return _ext_tn(Ph, Pl, Y, None), (np.abs(Ph).T @ np.abs(Y)) * S_SLACK


def gemm_nt_reference(A, B, rc=None, cc=None, c0=0.0):
    """A (M, K), B (N, K) -> (out pair (M, N), S)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    pair = _ext_tn(np.ascontiguousarray(A.T), None, np.ascontiguousarray(B.T), None)
    S = np.abs(A) @ np.abs(B).T
    if rc is not None:
        pair = _ext_add(pair, -np.asarray(rc, dtype=np.float64)[:, None])
        S = S + np.abs(rc)[:, None]
    if cc is not None:
        pair = _ext_add(pair, -np.asarray(cc, dtype=np.float64)[None, :])
        S = S + np.abs(cc)[None, :]
    pair = _ext_add(pair, np.float64(c0))
    return pair, (S + abs(float(c0))) * S_SLACK


def col_means_bound(S, C):
    return bound_factor(C + 1) * S


def gram_bound(S, C, centred=True):
    return bound_factor(C + (2 if centred else 0)) * S


def gram_tn_bound(S, C, centred=True):
    return bound_factor(C + (1 if centred else 0)) * S


def padded_genes(K):
    return (K + 63) // 64 * 64


def gemm_nt_bound(S, K):
    return bound_factor(padded_genes(K) + 3) * S


# ---------------------------------------------------------------------------------------------------------------------- case lists
SMALL_C = (1, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49)                 # every exit of the double-buffer loop: 0, 1, 2, 3 whole slabs with and without a tail
SMALL_G = (1, 2, 127, 128, 129, 257)
THIN_L = (1, 63, 64, 65, 128, 129)                                   # the 64- / 128-column tile of gram_tn and its second column of tiles
GRAM_SMALL = tuple((C, G, THIN_L[(i + j) % 6]) for i, C in enumerate(SMALL_C) for j, G in enumerate(SMALL_G)) + ((33, 513, 127),)
SPLIT_C = (2048, 2049, 2063, 2064, 2065, 2080, 2081, 3072, 3073)     # first split; a split ending on a slab, one cell past it; 2 -> 3 splits
SPLIT_G = 130
GRAM_SPLIT = tuple((C, SPLIT_G, (THIN_L[(2 * i) % 6], THIN_L[(2 * i + 3) % 6])) for i, C in enumerate(SPLIT_C))

NT_M = (1, 63, 64, 65, 127, 128, 129, 257)
NT_N = (1, 63, 64, 65, 128, 129)
NT_K = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 81, 160, 161) + (127, 128)   # (the last two: four slabs of 32 genes, f32 A)
NT_SMALL = {"M": (1, 63, 64, 65), "N": (1, 63, 64, 65), "K": (1, 15, 16, 17, 31, 32, 33)}
NT_LARGE = {"M": (127, 128, 129, 257), "N": (128, 129), "K": (63, 64, 65, 80, 81, 160, 161, 127, 128)}
TYPE_PAIRS = (("float64", "float64"), ("float32", "float64"), ("float32", "float32"))


def _thin_gemm():
    s, l = NT_SMALL, NT_LARGE
    pick = lambda seq, i: seq[i % len(seq)]
    out = []
    for i, K in enumerate(NT_K):
        out += [(pick(s["M"], i), pick(l["N"], i), K), (pick(l["M"], i), pick(s["N"], i), K)]
    for i, M in enumerate(NT_M):
        out += [(M, pick(s["N"], i), pick(l["K"], i)), (M, pick(l["N"], i), pick(s["K"], i))]
    for i, N in enumerate(NT_N):
        out += [(pick(s["M"], i), N, pick(l["K"], i + 3)), (pick(l["M"], i), N, pick(s["K"], i + 3))]
    return tuple(dict.fromkeys(out))


GEMM_NT = _thin_gemm()
MEANS = tuple((C, G) for C in (1, 2, 63, 64, 65, 129) for G in (1, 255, 256, 257))

# what a child process of another kernel form runs (tests/pca_products_worker.py): every exact case, a thinned bounded list
WORKER_GRAM_BOUNDED = ((17, 129, 65), (33, 257, 64), (48, 128, 129), (49, 127, 1), (2049, 130, 63), (2065, 130, 128), (3073, 130, 65))
WORKER_GEMM_BOUNDED = ((65, 129, 17), (257, 64, 33), (128, 65, 81), (63, 128, 161), (129, 1, 64), (1, 129, 160), (127, 63, 49))
KINDS = ("exact", "recipe", "ill")


# -------------------------------------------------------------------------------------------------------------------------- inputs
def stored(X, dtype):
    """The fp64 values a CellMatrix of `dtype` holds for X."""
    return X.astype(np.float32).astype(np.float64) if str(dtype).endswith("32") else np.asarray(X, dtype=np.float64)


def _values(rng, rows, cols, kind):
    """kind "exact": integers in [-8, 8]; "recipe": the recipe of test_gpu_preprocess.py - scales 0.5 .. 3 and means -2 .. 40 along the
    genes; "ill": mean 1e6, spread 1 (centring cancels six digits)."""
    if kind == "exact":
        return rng.integers(-8, 9, (rows, cols)).astype(np.float64)
    if kind == "ill":
        return 1e6 + rng.standard_normal((rows, cols))
    return rng.standard_normal((rows, cols)) * np.linspace(0.5, 3.0, cols)[None, :] + np.linspace(-2.0, 40.0, cols)[None, :]


@functools.lru_cache(maxsize=None)
def gram_X(C, G, kind, dtype):
    """X (C, G) as stored in `dtype` and the mean vector handed to the kernels - an input like any other: integer for the exact kind,
    the fp64 column mean of the stored values else."""
    rng = np.random.default_rng([C, G, KINDS.index(kind)])
    X = stored(_values(rng, C, G, kind), dtype)
    mean = rng.integers(-3, 4, G).astype(np.float64) if kind == "exact" else X.mean(0)
    X.setflags(write=False)
    mean.setflags(write=False)
    return X, mean


@functools.lru_cache(maxsize=None)
def gram_inputs(C, G, L, kind, dtype):
    """X, mean (gram_X) and the thin block Y (C, L) fp64, asymmetric: its columns grow with their number."""
    X, mean = gram_X(C, G, kind, dtype)
    rng = np.random.default_rng([C, G, L, KINDS.index(kind), 1])
    if kind == "exact":
        Y = rng.integers(-8, 9, (C, L)).astype(np.float64)
    else:
        Y = rng.standard_normal((C, L)) * np.arange(1, L + 1, dtype=np.float64)[None, :]
    Y.setflags(write=False)
    return X, mean, Y


@functools.lru_cache(maxsize=None)
def _gram_side(C, G, kind, dtype, centred):
    X, mean = gram_X(C, G, kind, dtype)
    if kind == "exact":
        Xi = X.astype(np.int64) - (mean.astype(np.int64)[None, :] if centred else 0)
        return Xi.T @ Xi, None
    ref, S = gram_reference(X, mean if centred else None)
    return ref, gram_bound(S, C, centred)


@functools.lru_cache(maxsize=None)
def _tn_side(C, G, L, kind, dtype, centred):
    X, mean, Y = gram_inputs(C, G, L, kind, dtype)
    if kind == "exact":
        Xi = X.astype(np.int64) - (mean.astype(np.int64)[None, :] if centred else 0)
        return Xi.T @ Y.astype(np.int64), None
    ref, S = gram_tn_reference(X, mean if centred else None, Y)
    return ref, gram_tn_bound(S, C, centred)


def gram_expect(C, G, L, kind, dtype, centred=True):
    """{"gram": (ref, bound), "tn": (ref, bound)}; the exact kind: ref is the int64 result and bound None.  (The integer inputs are the same
    in both storage types: computed once.)"""
    if kind == "exact":
        dtype = "float64"
    return {"gram": _gram_side(C, G, kind, dtype, centred), "tn": _tn_side(C, G, L, kind, dtype, centred)}


@functools.lru_cache(maxsize=None)
def gemm_inputs(M, N, K, kind, ta, tb):
    """A (M, K) as stored in ta, B (N, K) as stored in tb, rc (M), cc (N), c0.  "ill": the product centred by algebra, cc = B m with m = 1e6 the
    mean the rows of A were drawn around, no other correction."""
    rng = np.random.default_rng([M, N, K, KINDS.index(kind), TYPE_PAIRS.index((ta, tb))])
    A = stored(_values(rng, M, K, kind), ta)
    if kind == "exact":
        B = rng.integers(-8, 9, (N, K)).astype(np.float64)
        rc, cc, c0 = rng.integers(-50, 51, M).astype(np.float64), rng.integers(-50, 51, N).astype(np.float64), float(rng.integers(-9, 10))
    else:
        B = stored(rng.standard_normal((N, K)) * np.arange(1, N + 1, dtype=np.float64)[:, None], tb)
        if kind == "ill":
            rc, cc, c0 = None, B @ np.full(K, 1e6), 0.0
        else:
            rc, cc, c0 = rng.standard_normal(M) * 30.0, rng.standard_normal(N) * 30.0, float(rng.standard_normal() * 5.0)
    for a in (A, B, rc, cc):
        if a is not None:
            a.setflags(write=False)
    return A, B, rc, cc, c0


@functools.lru_cache(maxsize=None)
def gemm_expect(M, N, K, kind, ta, tb, corrected=True):
    A, B, rc, cc, c0 = gemm_inputs(M, N, K, kind, ta, tb)
    if not corrected:
        rc, cc, c0 = None, None, 0.0
    if kind == "exact":
        out = A.astype(np.int64) @ B.astype(np.int64).T
        if corrected:
            out = out - rc.astype(np.int64)[:, None] - cc.astype(np.int64)[None, :] + int(c0)
        return out, None
    ref, S = gemm_nt_reference(A, B, rc, cc, c0)
    return ref, gemm_nt_bound(S, K)


@functools.lru_cache(maxsize=None)
def means_inputs(C, G, kind, dtype):
    rng = np.random.default_rng([C, G, 77, KINDS.index(kind)])
    X = stored(_values(rng, C, G, kind), dtype)
    X.setflags(write=False)
    return X


# -------------------------------------------------------------------------------------------------------------------------- checks
def same_bits(a, b):
    """Bit for bit, NaNs matched by position (two fp64 arrays)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a, nan=7.0).view(np.int64),
                                                                                              np.nan_to_num(b, nan=7.0).view(np.int64))


def check(got, expect, what):
    """An exact case: the int64 result in every entry, no bit of it off (the sign of a zero is not part of an integer); a bounded one: |got - ref| <= bound in every
    entry.  Returns the worst error / bound (0 for an exact case)."""
    ref, bound = expect
    got = np.asarray(got)
    assert got.dtype == np.float64, (what, got.dtype)
    if bound is None:
        want = ref.astype(np.float64)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bad = np.argwhere(~(got == want))
        assert bad.size == 0, f"{what}: {len(bad)} entries differ from the int64 result, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
        return 0.0
    assert got.shape == ref[0].shape, (what, got.shape, ref[0].shape)
    err = error_against(got, ref)
    assert np.isfinite(got).all(), f"{what}: non-finite entries"
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max())
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert np.all(err <= bound), f"{what}: error / bound {worst:.3g} at {at} (error {err[at]:.3g}, bound {bound[at]:.3g})"
    return worst


# --------------------------------------------------------------------------------------------------- the device side (ops = velocyto_amd.ops)
def cell_matrix(ops, torch, X, dtype, pad_nan=True, extra=0):
    """X on the device as a CellMatrix of `dtype`, its row padding (at least one element: `extra` widens the pitch) NaN for the kernels
    that contract over the cells, zero for gemm_nt (pad_nan=False: the contraction runs over the zero padding)."""
    C, G = X.shape
    ld = ops.padded_ld(G + 1 if pad_nan else G) + extra
    t = torch.full((C, ld), float("nan") if pad_nan else 0.0, dtype=getattr(torch, dtype), device=ops.require_gpu())
    t[:, :G] = torch.as_tensor(np.array(X), device=t.device).to(t.dtype)
    return ops.CellMatrix(t, G)


def run_gram_case(ops, torch, C, G, L, kind, dtype, centred=True):
    X, mean, Y = gram_inputs(C, G, L, kind, dtype)
    M = cell_matrix(ops, torch, X, dtype)
    dev = M.t.device
    m = torch.as_tensor(np.array(mean), device=dev) if centred else None
    g = ops.gram(M, m)
    t = ops.gram_tn(M, m, torch.as_tensor(np.array(Y), device=dev))
    return {"gram": g.cpu().numpy(), "tn": t.cpu().numpy()}


def run_gemm_case(ops, torch, M, N, K, kind, ta, tb, corrected=True, out=None):
    A, B, rc, cc, c0 = gemm_inputs(M, N, K, kind, ta, tb)
    Am = cell_matrix(ops, torch, A, ta, pad_nan=False)
    dev = Am.t.device
    Bm = cell_matrix(ops, torch, B, tb, pad_nan=False) if (ta, tb) != ("float32", "float64") else torch.as_tensor(np.array(B), device=dev)
    if (ta, tb) == ("float64", "float64") and (M + N) % 2:            # both operand forms of the f64 pair: a CellMatrix and a plain fp64 tensor
        Bm = torch.as_tensor(np.array(B), device=dev)
    dv = lambda v: None if v is None else torch.as_tensor(np.array(v), device=dev)
    if not corrected:
        rc, cc, c0 = None, None, 0.0
    return ops.gemm_nt(Am, Bm, row_corr=dv(rc), col_corr=dv(cc), c0=c0, out=out).cpu().numpy()


# --------------------------------------------------------------------------------- what a child process of another kernel form runs
def key(*parts):
    return "|".join(str(p) for p in parts)


def worker_gram_jobs():
    """(C, G, L, kind, dtype): every exact case, the thinned bounded list in both bounded kinds."""
    jobs = []
    for dtype in ("float64", "float32"):
        jobs += [(C, G, L, "exact", dtype) for C, G, L in GRAM_SMALL]
        jobs += [(C, G, L, "exact", dtype) for C, G, Ls in GRAM_SPLIT for L in Ls]
        jobs += [(C, G, L, kind, dtype) for C, G, L in WORKER_GRAM_BOUNDED for kind in ("recipe", "ill")]
    return jobs


def worker_gemm_jobs():
    """(M, N, K, kind, ta, tb)."""
    jobs = []
    for ta, tb in TYPE_PAIRS:
        jobs += [(M, N, K, "exact", ta, tb) for M, N, K in GEMM_NT]
        jobs += [(M, N, K, kind, ta, tb) for M, N, K in WORKER_GEMM_BOUNDED for kind in ("recipe", "ill")]
    return jobs
