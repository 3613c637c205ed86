"""Case builders and numpy references for the winsorised gene statistics of CSR count layers (tests/test_csr_winsor_host.py,
tests/test_gpu_csr_winsor.py, tests/csr_winsor_worker.py).

Two references, both on the dense integer matrix (cells, genes):
  * percentiles: np.percentile(dense, qs, axis=0) - the reference's own call (analysis.py:264);
  * clipped moments: the exact-integer formula of vcy_csr_gene_stats_clip, in numpy's float64 (every product and sum rounded on its own).
`rank_rule_percentiles` is the rule the kernels implement (zeros first, then the positive counts; numpy's lerp) written out on the
host, so that the host test can pin it against np.percentile without a GPU."""
import numpy as np

U = 2.0 ** -53          # unit roundoff of float64


# ------------------------------------------------------------------------------------------------------------------ references
def np_percentiles(dense, qs, mask=None):
    d = np.asarray(dense, dtype=np.int64)
    if mask is not None:
        d = d[np.asarray(mask, dtype=bool)]
    return np.percentile(d, list(qs), axis=0)


def lerp(a, b, t):
    """numpy's _lerp (function_base.py): a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = b - a
    r = a + d * t
    if t >= 0.5:
        r = b - d * (1.0 - t)
    return a.copy() if t == 0.0 else r


def rank_rule_percentiles(dense, qs, mask=None):
    """Per gene: z = n - p zeros, rank r is 0 when r < z and the (r - z)-th smallest positive count otherwise; h = (n - 1)(q / 100),
    lo = floor(h), hi = min(lo + 1, n - 1), t = h - lo; lerp."""
    d = np.asarray(dense, dtype=np.int64)
    if mask is not None:
        d = d[np.asarray(mask, dtype=bool)]
    n, G = d.shape
    out = np.empty((len(qs), G))
    pos = [np.sort(d[:, g][d[:, g] > 0]) for g in range(G)]

    def value(g, r):
        z = n - pos[g].size
        return 0.0 if r < z else float(pos[g][r - z])
    for i, q in enumerate(qs):
        h = float(n - 1) * (float(q) / 100.0)
        lo = int(np.floor(h))
        hi, t = min(lo + 1, n - 1), h - lo
        a = np.array([value(g, lo) for g in range(G)])
        b = np.array([value(g, hi) for g in range(G)])
        out[i] = lerp(a, b, t)
    return out


def integer_parts(dense, lo, hi, mask=None):
    """(6, G) int64 [positive counts < lo, counts > hi, sum and sum of squares of the other positive counts, positive counts, max]."""
    d = np.asarray(dense, dtype=np.int64)
    if mask is not None:
        d = d[np.asarray(mask, dtype=bool)]
    G = d.shape[1]
    if lo is None:
        lo, hi = np.full(G, -np.inf), np.full(G, np.inf)
    pos = d > 0
    above = pos & (d > hi[None, :])
    below = pos & ~above & (d < lo[None, :])
    mid = np.where(pos & ~above & ~below, d, 0)
    mx = d.max(0) if d.shape[0] else np.zeros(G, dtype=np.int64)
    return np.stack([below.sum(0), above.sum(0), mid.sum(0), (mid * mid).sum(0), pos.sum(0), mx]).astype(np.int64)


def clip_from_parts(parts, n, lo, hi):
    """(4, G) float64: sum = (lo (n_below + [lo > 0] z) + S1) + hi n_above; sum of squares = ((lo lo)(...) + S2) + (hi hi) n_above;
    count = [hi > 0](p + [lo > 0] z); max = min(max(largest, lo), hi).  numpy rounds every operation on its own."""
    parts = np.asarray(parts, dtype=np.int64)
    n_below, n_above, s1, s2, p, mx = parts
    if lo is None or n == 0:
        return np.stack([s1, s2, p, mx]).astype(np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    z = n - p
    nb = (n_below + np.where(lo > 0, z, 0)).astype(np.float64)
    na = n_above.astype(np.float64)
    s = (lo * nb + s1.astype(np.float64)) + hi * na
    ss = ((lo * lo) * nb + s2.astype(np.float64)) + (hi * hi) * na
    cnt = np.where(hi > 0, p + np.where(lo > 0, z, 0), 0).astype(np.float64)
    return np.stack([s, ss, cnt, np.minimum(np.maximum(mx.astype(np.float64), lo), hi)])


def clipped_stats(dense, lo, hi, mask=None):
    n = int(np.asarray(dense).shape[0] if mask is None else np.asarray(mask, dtype=bool).sum())
    return clip_from_parts(integer_parts(dense, lo, hi, mask), n, lo, hi)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


# ------------------------------------------------------------------------------------------------------------------ layers
Q16 = (0, 0.5, 1, 5, 10, 25, 33.3, 50, 50.25, 66.6, 75, 90, 95, 99, 99.5, 100)
PERCENTILE_SETS = {"winsor": (1, 99.5), "ends": (0, 100), "median": (50,), "sixteen": Q16, "repeated": (99.5, 1, 99.5)}

# (cells, genes): the cells at the edges of the wave batch (64), the workgroup batch (512) and the cell tiles (2048 of the statistics,
# 4096 of the select), the genes at the edges of the slab (2048); pairs, not the cross product
SIZE_PAIRS = ((1, 7), (2, 2049), (63, 1), (64, 2047), (65, 4100), (511, 2048), (512, 7), (513, 1), (2047, 7), (2048, 2049), (2049, 7),
              (4095, 1), (4096, 7), (4097, 2049))


def random_dense(rng, C, G, wide):
    """(C, G) int64 counts: per-gene densities from never stored to always stored, small counts with a heavy tail; wide: values up to
    65535 with every high byte seen."""
    dens = rng.choice([0.0, 0.01, 0.08, 0.3, 0.9, 1.0], G)
    x = rng.geometric(0.35, (C, G))
    tail = rng.random((C, G))
    if wide:
        x = np.where(tail < 0.05, rng.integers(200, 700, (C, G)), x)
        x = np.where(tail < 0.01, rng.integers(1, 65536, (C, G)), x)
    else:
        x = np.where(tail < 0.05, rng.integers(1, 256, (C, G)), x)
    x = np.minimum(x, 65535 if wide else 255)
    return np.where(rng.random((C, G)) < dens[None, :], x, 0).astype(np.int64)


def constructed_dense(wide):
    """201 cells x 300 genes: rows with ~270 stored elements in one slab (the tail loop of the element walk: more than 192), and in
    the first columns genes built for the select's edges.  With q = 50.25, h = 100.5: ranks 100 and 101."""
    rng = np.random.default_rng(1234 + wide)
    C, G = 201, 300
    d = np.where(rng.random((C, G)) < 0.9, rng.geometric(0.3, (C, G)), 0).astype(np.int64)
    cells = rng.permutation(C)
    d[:, 0] = 0                                                            # all zeros
    d[:, 1] = 7                                                            # every cell the same positive count
    d[:, 2] = 0
    d[cells[0], 2] = 300                                                   # one positive cell
    d[:, 3] = np.array([255, 256, 257])[np.arange(C) % 3]
    d[:, 4] = np.array([0x00FF, 0x0100, 0x01FF, 0xFF00, 0xFFFF])[np.arange(C) % 5]
    d[:, 5] = 0
    d[cells[:100], 5] = rng.integers(1, 50, 100)                           # 101 zeros: ranks 100 / 101 straddle the zero / positive boundary
    d[cells[:101], 6] = 0x00FF
    d[cells[101:], 6] = 0x0100                                             # ranks 100 / 101 have different high bytes
    d[:, 7] = 65535
    d[:, 8] = np.where(np.arange(C) % 2 == 0, 0x0300 + rng.integers(0, 256, C), 0)      # every positive count shares one high byte
    if not wide:
        d = np.minimum(d, 255)
    return d, cells


def csr_arrays(dense, stored_zeros=None):
    """(indptr int64, indices int32, data int64) of the cells-major CSR of `dense`; stored_zeros: a bool matrix of further positions to
    store (explicitly stored zeros where dense is 0)."""
    dense = np.asarray(dense, dtype=np.int64)
    stored = dense > 0
    if stored_zeros is not None:
        stored = stored | np.asarray(stored_zeros, dtype=bool)
    r, c = np.nonzero(stored)
    indptr = np.concatenate([[0], np.cumsum(stored.sum(1))]).astype(np.int64)
    return indptr, c.astype(np.int32), dense[r, c]


def device_layer(ops, dense, wide, stored_zeros=None):
    import torch
    indptr, indices, data = csr_arrays(dense, stored_zeros)
    dev = ops.require_gpu()
    dat = torch.from_numpy(data.astype(np.uint16).view(np.int16)) if wide else torch.from_numpy(data.astype(np.uint8))
    return ops.CsrCounts(torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev), dat.to(dev), int(np.asarray(dense).shape[1]))


# ------------------------------------------------------------------------------------------------------------------ the selection dataset
N_CV = 100
DETECTION = dict(min_expr_counts=30, min_cells_express=15)


def selection_dataset():
    """(S, U): Poisson counts (cells, genes) = (2001, 300) int64 with a few cells of extreme counts in a tenth of the genes - what the
    winsorisation is for.  2001 cells: the ranks of (1, 99.5) are exactly 20 and 1990, so every bound is a count.  The first cell
    holds a count above 255 and no other cell does: in a sharded run only the first shard keeps uint16 counts."""
    rng = np.random.Generator(np.random.PCG64(20181123))
    C, G = 2001, 300
    rate = np.exp(rng.normal(-0.3, 1.0, G))
    size = np.exp(0.25 * rng.normal(size=C))
    S = np.minimum(rng.poisson(rate[None, :] * size[:, None]), 200)
    U_ = np.minimum(rng.poisson(0.35 * rate[None, :] * size[:, None]), 200)
    for g in rng.choice(G, 30, replace=False):
        S[rng.choice(np.arange(1, C), 5, replace=False), g] = rng.integers(100, 250, 5)
    S[0, 5] = 300
    return S.astype(np.int64), U_.astype(np.int64)
