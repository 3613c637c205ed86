"""Constructed inputs and recorded constants for the tests of stage E/F and the Markov chain (test_markov_oracle.py on the CPU,
test_gpu_markov_kernels.py on the device).  Every reference comes from the long-double functions of oracle.py; the constants
below are measured on the CPU by test_markov_oracle.py, which fails when they drift."""
import functools

import numpy as np
from scipy import sparse

import oracle

U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}            # unit roundoff of the compute / storage types
SIGMA_D, SIGMA_W = 3.0, 1.0
SWEEP_M = (6.0, 1e2, 1e3, 1e4)
# K of the bound on one factored step,
#     |y - y_ref| <= 4 K u S_j + (terms_j / 64 + 10) 2^-52 T_j  [+ n max|u| 2^-cut for the culled transform],
# S_j the sensitivity of the Gaussian half (oracle.gauss_step_reference), T_j = sum_c |v_c s_cj| and terms_j the column length of the
# sparse half (oracle.sparse_half_reference), which is summed in f64 whatever the compute type: a wave-strided recursive sum, six
# butterfly steps, the roundings of v and of the final add - a textbook bound with no measured constant.  K is the largest
# error / (u S_j) of the GAUSSIAN half of oracle.gauss_step_emulated over M in SWEEP_M x edim 1..4 at n = 600, measured on the CPU and
# pinned by test_markov_oracle.py: 1.26 in f32 and 6.65 in f64 (the f64 accumulation of 600 terms against the one rounding S_j counts).  The kernels get 4 K: fma in place of multiply-add, v_exp_f32 in place of
# a correctly rounded exp2, the partial sums of the source parts in another order.
MARKOV_K = {"float32": 1.3, "float64": 7.0}
# The largest relative error per target of the f32 emulation at each M of the sweep (over edim 1..4): the error follows M.  test_markov_oracle.py
# holds the emulation below 1.5 times these and asserts that they rise with M; DESIGN section 12 quotes them.
F32_REL = {6.0: 5.47e-8, 1e2: 3.59e-6, 1e3: 1.02e-5, 1e4: 2.77e-4}
# c of the bound |delta_embedding - ref| <= 2 c n 2^-53 sum_n |p - 1/n|: the largest error / (n 2^-53 cond) of the device's formula
# in numpy (tp_formula_f64) over tp_cases, both sigmas, both storage types, measured on the CPU: 2.12, at n = 2, where p - 1/2
# cancels and the last bits of p and of the two unit vectors are all there is.  The kernel gets 2 c (its exp() is good to an ulp
# where the C library's is good to half of one, its sums run lane by lane): on an MI355X it uses 1.6 c.
TP_C = 2.3


def stored(a, dtype):
    """The values the device holds for `a` in storage type `dtype`, as f64."""
    return np.asarray(a, dtype=np.float64) if dtype == "float64" else np.asarray(a, dtype=np.float32).astype(np.float64)


def ulp(ref, dtype):
    """The spacing of `dtype` at |ref| (ref long double or f64), as f64."""
    t = np.float64 if dtype == "float64" else np.float32
    a = np.abs(np.asarray(ref)).astype(t)
    return np.spacing(np.maximum(a, np.finfo(t).tiny)).astype(np.float64)


# ---------------------------------------------------------------- stage E
TP_N = (1, 2, 63, 64, 65, 129, 300)
TP_COUT = (1, 3, 4, 5, 130)


@functools.lru_cache(maxsize=None)
def tp_cases(dtype, sigma):
    """Every (n, C_out) of TP_N x TP_COUT, edim and cell0 cycling through 1..4 and (0, 41).  ixs and emb are global; corr reaches
    +-1 exactly; every third row lists its own cell; with two rows or more, cell0 + 1 sits on cell0's coordinates and row 0 lists it
    (a NaN unit vector).  Each case carries the long-double reference."""
    out = []
    for i, (n, C_out) in enumerate((n, c) for n in TP_N for c in TP_COUT):
        rng = np.random.default_rng(1000 * n + C_out + (dtype == "float32"))
        edim, cell0 = 1 + i % 4, (0, 41)[(i // 4) % 2]
        C = max(cell0 + C_out, n) + 7
        emb = rng.normal(size=(C, edim)) * 5.0
        corr = rng.uniform(-1.0, 1.0, (C_out, n))
        corr[0, 0], corr[-1, -1] = 1.0, -1.0
        corr = stored(corr, dtype)
        ixs = np.stack([rng.choice(C, n, replace=False) for _ in range(C_out)]).astype(np.int32)
        for r in range(0, C_out, 3):                                    # the cell itself, once per list
            ixs[r][ixs[r] == cell0 + r] = (cell0 + r + 1) % C
            ixs[r, -1] = cell0 + r
        if C_out >= 2 and n >= 2:
            emb[cell0 + 1] = emb[cell0]
            ixs[0][ixs[0] == cell0 + 1] = (cell0 + 2) % C
            ixs[0, 0] = cell0 + 1
        tp, wd, de, cond = oracle.transition_prob_reference(corr, ixs, emb, sigma, cell0)
        out.append(dict(n=n, C_out=C_out, edim=edim, cell0=cell0, corr=corr, ixs=ixs, emb=emb, tp=tp, wd=wd, de=de, cond=cond))
    return out


def tp_formula_f64(corr, ixs, emb, sigma, cell0):
    """The device's formula in numpy (k_transition_prob): used to measure TP_C, never as a reference.  The (hi, lo) normaliser of
    two_sum carries about 106 bits; a long-double sum stands in for it here (both are exact to well below an f64 ulp)."""
    corr = np.asarray(corr, dtype=np.float64)
    R, n = corr.shape
    q = corr / sigma
    split = lambda a: ((a * 134217729.0) - ((a * 134217729.0) - a), a - ((a * 134217729.0) - ((a * 134217729.0) - a)))
    (qh, ql), (sh, sl) = split(q), split(np.float64(sigma))
    prod = q * sigma
    perr = ql * sl - (((prod - qh * sh) - ql * sh) - qh * sl)             # q sigma = prod + perr exactly (Dekker): the fma's residual
    e, dq = np.exp(q).astype(np.longdouble), (((corr - prod) - perr) / sigma).astype(np.longdouble)
    e = e * (1 + dq)                                                       # exp(q) (1 + d) / (zh + zl), rounded once (softmax_quot)
    p = (e / e.sum(1, keepdims=True)).astype(np.float64)
    cells = cell0 + np.arange(R)
    d = emb[ixs] - emb[cells][:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        unit = d / np.sqrt((d * d).sum(-1))[..., None]
    unit[ixs == cells[:, None]] = 0.0
    return p, ((p - 1.0 / n)[..., None] * unit).sum(1)


# ---------------------------------------------------------------- prepare_markov
PREP_N = (1, 2, 255, 256, 257, 600)


@functools.lru_cache(maxsize=None)
def prepare_problem(n, edim, empty_row=False):
    """P (scipy CSR, sorted, no duplicates) and an embedding a few kernel widths across.  Where n allows: row 3 stores 300 entries
    (the stride-256 loops wrap), row 5 only its diagonal, row 7 a diagonal that is its maximum, row 9 a diagonal that is not, cells
    11 and 12 share their coordinates; empty_row: row 2 stores nothing (a NaN row of the chain)."""
    rng = np.random.default_rng(31 * n + edim)
    emb = rng.normal(size=(n, edim)) * 2.0
    k = min(n, 7)
    lists = [np.union1d(rng.choice(n, k, replace=False), [(r + 1) % n, (r + 5) % n]) for r in range(n)]    # (no column left empty)
    vals = [rng.random(l.size) + 0.01 for l in lists]
    if n == 1:
        lists, vals = ([np.array([0])], [np.array([0.3])])
    if n >= 16:
        if n >= 300:
            lists[3] = np.sort(rng.choice(n, 300, replace=False))
            vals[3] = rng.random(300) + 0.01
        lists[5], vals[5] = np.array([5]), np.array([0.4])
        for r, dv in ((7, 50.0), (9, 1e-3)):
            lists[r] = np.union1d(lists[r], [r])
            vals[r] = rng.random(lists[r].size) + 0.5
            vals[r][lists[r] == r] = dv
        emb[12] = emb[11]
    if empty_row:
        assert n >= 16
        lists[2], vals[2] = np.array([], dtype=np.int64), np.array([])
    indptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    P = sparse.csr_matrix((np.concatenate(vals), np.concatenate(lists).astype(np.int32), indptr), shape=(n, n))
    return P, emb


def directed(P, direction):
    Pd = sparse.csr_matrix(P if direction == "forward" else P.T)
    Pd.sort_indices()
    return Pd


# ---------------------------------------------------------------- the factored chain
STEP_N = (1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1025, 2049)


@functools.lru_cache(maxsize=None)
def chain_problem(n, edim, M=6.0, seed=0, shift=0.0):
    """A clustered embedding whose scaled coordinates es = emb sqrt(log2 e / 2 sigma_W^2) reach about M (up to nine clusters 1.5
    sigma_W wide, their centres spread to M; M = 6 puts them on top of each other), translated by `shift` sigma_W along every axis.
    Cells are stored cluster by cluster.  P: a stored diagonal and up to 7 cells of the same cluster per row, no duplicates; from
    n = 256 on cell 1 is also listed by 200 rows (a column of s longer than a wave)."""
    rng = np.random.default_rng(7 * n + 100 * edim + seed + int(M))
    scale = float(np.sqrt(np.log2(np.e) / (2.0 * SIGMA_W ** 2)))
    ncl = min(9, max(1, n // 8))
    centres = rng.uniform(-1.0, 1.0, (ncl, edim))
    centres *= max(M - 4.5, 0.0) / np.abs(centres).max()
    lab = np.sort(rng.integers(0, ncl, n))
    emb = (centres[lab] / scale + rng.normal(size=(n, edim)) * 1.5 * SIGMA_W) + shift * SIGMA_W
    first, count = np.searchsorted(lab, lab), np.bincount(lab, minlength=ncl)[lab]
    lists = []
    for c in range(n):
        others = first[c] + rng.choice(count[c], min(7, count[c]), replace=False)
        lists.append(np.union1d(others, [c]))
    if n >= 256:
        for r in rng.choice(np.arange(2, n), 200, replace=False):
            lists[r] = np.union1d(lists[r], [1])
    indptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    indices = np.concatenate(lists).astype(np.int32)
    pval = rng.random(indices.size) + 0.01
    x = rng.random(n) + 1e-3
    return dict(n=n, edim=edim, emb=emb, indptr=indptr, indices=indices, pval=pval, x=x / x.sum(), lab=lab)


def scaled_M(emb, sigma_W=SIGMA_W):
    return float(np.abs(oracle.markov_scaled_coords(emb, sigma_W)).max())


def step_bound(S, dtype, n, umax, cut=None, T=0.0, terms=0):
    """4 K u S_j + the f64 sparse half's (terms_j / 64 + 10) 2^-52 T_j, plus what the culled transform leaves out: n max|u| 2^-cut."""
    b = 4.0 * MARKOV_K[dtype] * U[dtype] * np.asarray(S, dtype=np.float64) + (np.asarray(terms) / 64.0 + 10.0) * 2.0 ** -52 * np.asarray(T, dtype=np.float64)
    return b + (0.0 if cut is None else 2.0 ** -cut * n * float(umax))


def culled_box_census(es_sorted, cut):
    """What k_gauss_transform_culled's box tests decide, counted on the CPU from the sorted coordinates the device holds: blocks of
    256 targets against chunks of 32 sources, gap^2 summed over the axes, a chunk skipped when the sum exceeds cut.
    Returns (chunks skipped, chunks kept)."""
    es = np.asarray(es_sorted, dtype=np.float64)
    n = es.shape[0]
    box = lambda w: (np.stack([es[i:i + w].min(0) for i in range(0, n, w)]), np.stack([es[i:i + w].max(0) for i in range(0, n, w)]))
    tlo, thi = box(256)
    clo, chi = box(32)
    gap = np.maximum(np.maximum(clo[None] - thi[:, None], tlo[:, None] - chi[None]), 0.0)
    far = (gap * gap).sum(-1) > cut
    return int(far.sum()), int((~far).sum())
