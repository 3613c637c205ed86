"""Constructed inputs for the tests of stage A, kNN pooling (test_pool_oracle.py on the CPU, test_gpu_pool_kernels.py on the device).
Every reference is oracle.pool_reference (long double), every tolerance oracle.pool_bound (derived, nothing measured).

Where the kernels change path, restated from the sources:
  csrc/pool.hip, k_knn_pool (float matrices): N = 4 (f32) / 2 (f64) genes per 16-byte vector.  slab = slab_genes or 512, rounded up
    to N, clipped to G rounded up to N; threads = 256 if slab / N >= 256, 128 if >= 128, else 64 - f32: 64 below 512 genes, 128
    from 512 (the default), 256 from 1024; f64: 128 from 256, 256 from 512.  Whole vectors of a slab take the 4-unrolled gather
    loop and its remainder (graph rows of 0 .. 3 and 4 .. 9 entries), the G % N last genes the scalar tail, which then is all
    the last slab holds when slab divides G - G % N.
  csrc/pool.hip, k_knn_pool_counts: NE = 16 (uint8) / 8 (uint16) genes per gather, default slab 1024 = 64 (uint8) or 128 (uint16)
    threads; 256 threads from slab 4096 / 2048.  The vector that straddles G is masked to zero past G and stored whole.
  csrc/poolcsr.hip, k_knn_pool_csr: slabs of 2048 genes; ceil(20480 / C_out) waves per cell, at most one per slab
    (vcy_knn_pool_csr_splits); graph rows in batches of 64 entries (partial sums reloaded from `out` from the second batch on);
    a lane owns four consecutive non-zeros of a slab segment, 256 per pass, longer segments take an element-wise loop."""
import functools

import numpy as np

import oracle

U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
NPT = {"float32": np.float32, "float64": np.float64}
DTYPES = ("float32", "float64")

# lengths of the first graph rows: what a block of C_out = 1, 7, 8 or 9 rows (from row 0 or from row BLOCK_CELL0) still holds.
# 0 .. 9: the 4-unrolled loop and its remainder; 64 / 65 / 128 / 129: the CSR kernel's batch boundaries; 81: one batch and a part
LEAD_LENGTHS = (5, 0, 64, 1, 65, 9, 0, 129, 3, 128, 81, 2, 6, 7, 8, 4)
BLOCK_CELL0 = 5
BLOCK_COUT = (1, 7, 8, 9)


def stored(a, dtype):
    """The values the device holds for `a` in the working type `dtype`, in that type."""
    return np.asarray(a, dtype=np.float64).astype(NPT[dtype])


@functools.lru_cache(maxsize=None)
def graph(C, seed=0, long_rows=True, signed=False):
    """Graph rows for C output cells over C source rows: (indptr int64, indices int32, w f64 in [0.5, 1], w2).  Row r has
    LEAD_LENGTHS[r] entries (rows of 64 and more only with long_rows, else r % 10), later rows 1 .. 9; entries are drawn with
    repeats, row 2 repeats its first entry for sure, row 3 names only itself, rows are NOT sorted (the kernels add in list order).
    w2: a second weight set of the same magnitudes with random signs (signed), else None."""
    rng = np.random.default_rng(9000 + 17 * C + seed)
    lens = [LEAD_LENGTHS[r] if r < len(LEAD_LENGTHS) else 1 + (r * 7) % 9 for r in range(C)]
    if not long_rows:
        lens = [l if l < 64 else r % 10 for r, l in enumerate(lens)]
    rows = [rng.integers(0, C, l) for l in lens]
    if C > 3:
        if rows[2].size > 1:
            rows[2][1] = rows[2][0]
        rows[3] = np.array([3])
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32) if indptr[-1] else np.zeros(0, dtype=np.int32)
    w = rng.uniform(0.5, 1.0, indices.size)
    w2 = rng.uniform(0.5, 1.0, indices.size) * rng.choice([-1.0, 1.0], indices.size) if signed else None
    for a in (indptr, indices, w) + ((w2,) if signed else ()):
        a.setflags(write=False)
    return indptr, indices, w, w2


def block(g, cell0, C_out):
    """Rows cell0 .. cell0 + C_out - 1 of a graph (indptr, indices, w, w2) as a graph of their own: the rows of a cell block."""
    indptr, indices, w, w2 = g
    a, b = int(indptr[cell0]), int(indptr[cell0 + C_out])
    return (indptr[cell0:cell0 + C_out + 1] - a, indices[a:b], w[a:b], None if w2 is None else w2[a:b])


def order_for(C_out, seed=0):
    """A random schedule order (permutation of range(C_out)) as int32."""
    return np.random.default_rng(77 + C_out + seed).permutation(C_out).astype(np.int32)


def row_terms(g):
    return np.diff(g[0])


def smallest_term(indptr, indices, w, data, scale=None):
    """Per output element the smallest NON-ZERO |w s x| among its terms (inf where there is none), in f64."""
    X = np.abs(np.asarray(data, dtype=np.float64))
    s = np.ones(X.shape[0]) if scale is None else np.abs(np.asarray(scale, dtype=np.float64))
    out = np.full((indptr.size - 1, X.shape[1]), np.inf)
    for r in range(indptr.size - 1):
        j = indices[indptr[r]:indptr[r + 1]]
        if j.size:
            t = (np.abs(np.asarray(w, dtype=np.float64)[indptr[r]:indptr[r + 1]]) * s[j])[:, None] * X[j]
            out[r] = np.where(t > 0, t, np.inf).min(0)
    return out


# ---------------------------------------------------------------- float matrices (vcy_knn_pool, _pool2, _pool_w2)
FLOAT_G = (1, 3, 5, 66, 257, 515, 1029)
# 0: the default (512).  1: rounded up to N.  6: rounded up to 8 in f32, a slab of 3 vectors in f64.  256 / 512 / 1024: the thread
# counts (f32: 64 / 128 / 256, f64: 128 / 256 / 256); with G = 257, 515, 1029 and slab 256, 512, 1024 the last slab holds nothing but
# the scalar tail (f32: G % 4 = 1, 3, 1 genes; f64: 1).  4096: clipped to G.
FLOAT_SLABS = (0, 1, 6, 256, 512, 1024, 4096)
FLOAT_C = 40


@functools.lru_cache(maxsize=None)
def float_case(G, dtype):
    """Two (C, G) matrices of the working type - values in [0.5, 4), three in ten exactly zero, gene G // 2 zero in every cell
    (an output that must be exactly 0), some negative entries in the second - and the signed graph.  Structural: the f32 bound
    resolves a single term."""
    rng = np.random.default_rng(100 + G)
    mats = []
    for m in range(2):
        a = rng.uniform(0.5, 4.0, (FLOAT_C, G)) * (rng.random((FLOAT_C, G)) >= 0.3)
        if m == 1:
            a = a * rng.choice([-1.0, 1.0], a.shape) + 0.0               # (+ 0.0: no -0 among the zeros)
        if G > 1:
            a[:, G // 2] = 0.0
        mats.append(stored(a, dtype))
    g = graph(FLOAT_C, seed=G, signed=True)
    g = (g[0], g[1], stored(g[2], dtype), stored(g[3], dtype))
    return dict(G=G, C=FLOAT_C, dtype=dtype, data=mats[0], data2=mats[1], graph=g, scale=None, structural=True)


# ---------------------------------------------------------------- dense count layers (vcy_knn_pool_counts)
COUNT_G = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1025, 4100)
# 0: the default (1024).  1: rounded up to NE.  8 / 24: one or three uint16 gathers, rounded up to 16 / 32 for uint8.  1024 / 2048 /
# 4096 / 8192: 64 / 128 / 256 / 256 threads for uint8, 128 / 256 / 256 / 256 for uint16; 8192 is clipped to G.
COUNT_SLABS = (0, 1, 8, 24, 1024, 2048, 4096, 8192)
COUNT_C = 40
EDGE_COUNTS = (0, 1, 255, 256, 32767, 32768, 65535)


def odd_scales(rng, n, lo, hi, pin=False):
    """Factors 2^e (1 + odd * 2^-40), e uniform in [lo, hi] (pin: the first two take lo and hi): no f32 holds one of them."""
    e = rng.integers(lo, hi + 1, n)
    if pin:
        e[:2] = lo, hi
    return np.ldexp(1.0 + (2 * rng.integers(1, 2 ** 38, n) + 1) * 2.0 ** -40, e)


@functools.lru_cache(maxsize=None)
def count_case(G, kind):
    """Two count layers (C, G), S with no count above 255 (held as uint8 or uint16), U of any count, per-cell factors, a graph.
      kind "structural": counts 0 .. 3 (half of them 0), factors in [0.5, 2), graph rows of up to 129 entries: the f32 bound
        resolves a single term.
      kind "range": every count of EDGE_COUNTS, factors over 2^-10 .. 2^10, graph rows of 0 .. 9 entries.  The magnitudes are kept
        apart BY GENE so that f64 still resolves a term next to the largest one of the same output: gene g holds, besides zeros,
        counts of ONE class (g + G) % 3 - {1, 2, 3}, {255, 256} (S: {254, 255}), {32767, 32768, 65535} (S: {1, 2, 3}).  f32 cannot
        resolve 2^-20 of a sum: the case is marked and runs against the bound all the same."""
    rng = np.random.default_rng(500 + G + (kind == "range"))
    C = COUNT_C
    nz = rng.random((2, C, G)) < 0.5
    if kind == "structural":
        S, Uc = (rng.integers(1, 4, (C, G)) * nz[0], rng.integers(1, 4, (C, G)) * nz[1])
        sS, sU = odd_scales(rng, C, -1, 0), odd_scales(rng, C, -1, 0)
        g = graph(C, seed=G)
    else:
        cls = (np.arange(G) + G) % 3
        pick = lambda sets: np.stack([rng.choice(np.asarray(sets[c]), C) for c in cls], 1)
        S = pick({0: (1, 2, 3), 1: (254, 255), 2: (1, 2, 3)}) * nz[0]
        Uc = pick({0: (1, 2, 3), 1: (255, 256), 2: (32767, 32768, 65535)}) * nz[1]
        sS, sU = odd_scales(rng, C, -10, 9, pin=True), odd_scales(rng, C, -10, 9, pin=True)
        g =graph(C, seed=G, long_rows=False)
    if G > 2:
        S[:, G // 2] = 0
        Uc[:, G // 2] = 0
    return dict(G=G, C=C, kind=kind, S=S.astype(np.int64), U=Uc.astype(np.int64), sS=sS, sU=sU, graph=g, structural=kind == "structural")


def case_graph(cs, dtype):
    """The case's graph with the weights as the device holds them in `dtype`."""
    g = cs["graph"]
    return (g[0], g[1], stored(g[2], dtype), None if g[3] is None else stored(g[3], dtype))


# ---------------------------------------------------------------- CSR count layers (vcy_csr_slab_ptr, vcy_knn_pool_csr)
CSR_SLAB = 2048                      # vcy_csr_slab_genes(), asserted by the GPU test
CSR_G = (700, 2048, 2049, 4097)
CSR_SEGMENTS = (1, 2, 3, 4, 5, 255, 256, 257, 300)      # non-zeros of one row inside one slab: the quads of 4, one pass of 256, the tail loop
CSR_PLANTED = (0, 2047, 2048, 4095, 4096)


@functools.lru_cache(maxsize=None)
def csr_case(G, wide):
    """A CSR layer of C rows x G genes as (indptr, indices, data) with genes ascending inside a row, factors and a graph with rows
    of up to 129 entries.  Row 0: non-zeros at the genes of CSR_PLANTED below G and at G - 1.  Row 1: empty.  Rows 2 .. 10: exactly
    CSR_SEGMENTS[i] non-zeros in slab 0 and, where G reaches it, CSR_SEGMENTS[-1 - i] in slab 1.  Row 11: every gene (2048 per
    slab).  Rows 12 .. C - 2: 5 % of the genes.  Row C - 1: ONE non-zero, gene G - 1: the last element of the arrays (its quad is
    pulled back inside them).  Counts 1 .. 3; `wide`: a uint16 layer in which every count of the rows 0, 4, 9, 11, 13 and C - 1 lies
    in 256 .. 1000 (f32 cannot resolve a count of 1 next to them: marked)."""
    rng = np.random.default_rng(800 + G + wide)
    C = 30
    genes = []
    genes.append(np.unique([g for g in CSR_PLANTED if g < G] + [G - 1]))
    genes.append(np.zeros(0, dtype=np.int64))
    for i, m in enumerate(CSR_SEGMENTS):
        seg = [np.sort(rng.choice(min(G, CSR_SLAB), min(m, G), replace=False))]
        if G > CSR_SLAB:
            m1 = min(CSR_SEGMENTS[-1 - i], G - CSR_SLAB)
            seg.append(CSR_SLAB + np.sort(rng.choice(min(G - CSR_SLAB, CSR_SLAB), m1, replace=False)))
        genes.append(np.concatenate(seg))
    genes.append(np.arange(G))
    while len(genes) < C - 1:
        genes.append(np.sort(rng.choice(G, max(1, G // 20), replace=False)))
    genes.append(np.array([G - 1]))
    vals = [rng.integers(1, 4, g.size) for g in genes]
    if wide:
        for r in (0, 4, 9, 11, 13, C - 1):
            vals[r] = rng.integers(256, 1001, genes[r].size)
    indptr = np.concatenate([[0], np.cumsum([g.size for g in genes])]).astype(np.int64)
    indices, data = np.concatenate(genes).astype(np.int32), np.concatenate(vals).astype(np.int64)
    dense = np.zeros((C, G), dtype=np.int64)
    dense[np.repeat(np.arange(C), np.diff(indptr)), indices] = data
    return dict(G=G, C=C, wide=wide, indptr=indptr, indices=indices, data=data, dense=dense, scale=odd_scales(rng, C, -1, 0),
                graph=graph(C, seed=G + 1), structural=not wide)


def slab_ptr_reference(indptr, indices, G):
    """What vcy_csr_slab_ptr fills: per row the number of its non-zeros with gene < s * CSR_SLAB, s = 0 .. nslab."""
    nslab = (G + CSR_SLAB - 1) // CSR_SLAB
    keys = np.arange(nslab + 1) * CSR_SLAB
    return np.stack([np.searchsorted(indices[indptr[r]:indptr[r + 1]], keys, side="left") for r in range(indptr.size - 1)]).astype(np.int32)


# ---------------------------------------------------------------- CSR, several slabs per wave
# About the smallest shapes at which vcy_knn_pool_csr_splits(C_out, G) < ceil(G / 2048) leaves a range of two slabs AND a shorter
# one: three slabs need G >= 4097, and ceil(20480 / C_out) < 3 needs C_out >= 10240 (below, every slab has its own wave).  C_out = 10241: 2 waves per cell, slab ranges [0, 2) and [2, 3) - a hand-over and a
# short last range; C_out = 20480: 1 wave walks all three slabs, the production arrangement (nsplit = 1).
MULTI_G = 4097
MULTI_SHAPES = ((10241, 2, ("float32", "float64")), (20480, 1, ("float32",)))       # (C_out, expected splits, working types)
MULTI_C = 20480
MULTI_K = 5


@functools.lru_cache(maxsize=None)
def multi_case():
    """A uint8 layer of MULTI_C x MULTI_G at about 2 % density (a block of 1024 generated rows, repeated), counts 1 .. 3, with the
    planted genes of CSR_PLANTED in row 0, a slab-1 segment of 300 non-zeros in row 1 and a full row 2; a graph of the cell itself
    + MULTI_K random cells per row, rows 0 .. 3 of 64, 65, 129 and 1 entries instead; factors in [0.5, 2).  `sample`: the output rows
    the long-double reference is computed for (the first 8, the rows around the C_out = 10241 boundary, the last, 40 random)."""
    rng = np.random.default_rng(4097)
    blk = (rng.integers(1, 4, (1024, MULTI_G)) * (rng.random((1024, MULTI_G)) < 0.02)).astype(np.uint8)
    blk[0, [g for g in CSR_PLANTED if g < MULTI_G] + [MULTI_G - 1]] = 3
    blk[1, CSR_SLAB + rng.choice(CSR_SLAB, 300, replace=False)] = 2
    blk[2] = rng.integers(1, 4, MULTI_G)
    dense = np.tile(blk, (MULTI_C // 1024, 1))
    rows = [np.concatenate([[r], rng.integers(0, MULTI_C, MULTI_K)]) for r in range(MULTI_C)]
    for r, l in ((0, 64), (1, 65), (2, 129), (3, 1)):
        rows[r] = rng.integers(0, MULTI_C, l)
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    w = rng.uniform(0.5, 1.0, indices.size)
    sample = np.unique(np.concatenate([np.arange(8), [10239, 10240, 10241, MULTI_C - 1], rng.integers(0, MULTI_C, 40)]))
    return dict(G=MULTI_G, C=MULTI_C, dense=dense, scale=odd_scales(rng, MULTI_C, -1, 0), graph=(indptr, indices, w, None), sample=sample)


def graph_rows(g, rows):
    """The listed rows of a graph as a graph of their own (for a reference of a sample of the output)."""
    indptr, indices, w, _ = g
    sel = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in rows])
    ptr = np.concatenate([[0], np.cumsum([indptr[r + 1] - indptr[r] for r in rows])]).astype(np.int64)
    return ptr, indices[sel], w[sel], None
