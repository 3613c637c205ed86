"""The scaled root of the f64 partial-sqrt rule of stage D (csrc/coldeltacor.hip): under RULES_PARTIAL the element accumulates
A' = 2 sign(t) sqrt(|t| + psc), formed from the f32 seed Y = v_rsq_f32((float)x) by one Newton step in its reciprocal-root form,
u = x Y, w = 3 - u Y, A' = u w.  Pearson's r is unchanged when every A of a pair carries the same power of two, so nothing outside the
kernel sees the factor.  Everything goes through the C ABI on cuda:0 and is compared with long-double restatements made here.

Bounds (none is taken from what the kernels return):
  * element: with Y = (1 + e) / sqrt(x), |e| <= 2^-23 + 2^-25 (v_rsq_f32 to one ulp; the rounding of x to f32, 2^-24, half of which
    reaches the seed), u w / (2 sqrt x) = 1 - 1.5 e^2 - 0.5 e^3.  Roundings: that of |t| + psc and that of u each reach the result by half
    (d(u w)/du = 3 - 2 u Y = 1 at u = sqrt x, against a result of 2 sqrt x): 2^-54 each; the fma's w (near 2) and the last product 2^-53 each.
    DELTA = 1.5 (2^-23 + 2^-25)^2 + 3 2^-53 = 2^-44.7.  A pair whose cells differ in two genes only has A = (a1, a2, 0, ..., 0) and r is a
    closed form of the two roots; a relative error delta on each root moves r by at most 2 delta sqrt(sum A^2 / sum (A - mean A)^2)
    (Cauchy-Schwarz on the centred, normalised vectors, as in ops.partial_rules_for).  The kernel's own f64 arithmetic between the roots
    and r is the term tests/test_gpu_cdc_root.py derives: at most 16 rounded operations, each amplified by at most the product of the two
    cancellation ratios, 16 max(ratio_A, ratio_b)^2 2^-53.
  * homogeneity: e and psc times 4 make x' = 4 x, (float)x' = 4 (float)x, Y' = Y / 2, u' = 2 u, w' = w, A'' = 2 A', the three moments
    times 2, 4 and 2, and every intermediate of pearson_from_moments an exact power-of-two multiple (its square root sees 4 va vb): r is
    the same bits.  No rounding is involved anywhere, so any constant or halving that does not scale with the data shows.
  * edges: the project's f64 bar against the long-double restatement (1e-10 absolute) and its NaN pattern.
  * dual against single: the d-moment bound tests/test_gpu_cdc_root.py derives, G 2^-53 (1.5 ratio_b^2 + ratio_A ratio_b).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

L = np.longdouble
PSC = 1e-10
DELTA = 1.5 * (2.0 ** -23 + 2.0 ** -25) ** 2 + 3 * 2.0 ** -53
SHAPES = [(7, 5), (26, 9)]                      # (cells, listed): k_cdc_partial, and the grouped kernel (>= 24 cells, >= 8 listed)
GENES = [2, 129, 1025]                          # the lane vector, the wave vector, the second chunk
EDGE_GENES = [5, 129, 1025]                     # the same three, with enough genes in the first for r to depend on the roots


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def _oracle(e, d, ixs, psc):
    """(r, ratio, ratio_b) in long double from cells-major f64 e, d (C, G): the rule of speedboosted.pyx:372-378 on the f64 difference t,
    centred sums; ratio = sqrt(sum A^2 / sum (A - mean A)^2) per pair, ratio_b the same of d[c] per cell.  Zero variance: NaN."""
    C, nr = ixs.shape
    r = np.full((C, nr), np.nan, L)
    ratio = np.full((C, nr), np.nan, L)
    ratio_b = np.full((C, 1), np.nan, L)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(C):
            t = e[ixs[c]] - e[c][None, :]
            a = np.where(np.abs(t) < 1e-16, L(0), np.sign(t).astype(L) * np.sqrt(np.abs(t).astype(L) + L(psc)))
            b = d[c].astype(L)
            ac = a - a.mean(1, keepdims=True)
            bc = b - b.mean()
            va, vb = (ac * ac).sum(1), (bc * bc).sum()
            r[c] = (ac * bc[None, :]).sum(1) / np.sqrt(va * vb)
            ratio[c] = np.sqrt((a * a).sum(1) / va)
            ratio_b[c] = np.sqrt((b * b).sum() / vb)
    return r, ratio, ratio_b


def _pooled(rng, C, G, lam):
    """Count-like rows: Poisson counts x size factors averaged over four of 3 C cells - exact zeros where all four are empty."""
    f = rng.gamma(8.0, 0.125, 3 * C)
    return np.stack([(rng.poisson(lam, (3 * C, G)) * f[:, None])[rng.choice(3 * C, 4, replace=False)].mean(0) for _ in range(C)])


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def _same_bits(x, y):
    """Equal NaN pattern, equal bits everywhere else."""
    x, y = x.cpu().numpy(), y.cpu().numpy()
    nx, ny = np.isnan(x), np.isnan(y)
    return np.array_equal(nx, ny) and np.array_equal(x[~nx].view(np.int64), y[~ny].view(np.int64))


# --------------------------------------------------------------------------- the element through the grouped kernel
@pytest.mark.gpu
@pytest.mark.parametrize("psc", [PSC, 0.0])
def test_scaled_root_accuracy_through_the_kernel(ops, psc):
    """64 cells x 63 listed, G = 130: every pair differs in genes 5 and 77 only, by |t| over 2^-50 .. 2^61 (magnitudes on a log grid,
    random mantissas and signs), so r is a closed form of two roots.  |r - closed form| <= 2 ratio_A DELTA + the kernel's own rounding
    (module docstring) under RULES_PARTIAL, and the result differs somewhere from the two-correction root's (else the element is not what
    is being seen)."""
    rng = np.random.default_rng(20260)
    C, G, g1, g2, n = 64, 130, 5, 77, L(130)
    base = np.round(rng.gamma(2.0, 1.0, G) * 4) / 4                              # count-like, the same in every cell: t = 0 there
    e = np.tile(base, (C, 1))
    k = np.linspace(-50.0, 60.0, C)
    for g, kk in ((g1, k), (g2, rng.permutation(k))):
        e[:, g] = np.sign(rng.normal(size=C)) * rng.uniform(1.0, 1.4, C) * np.exp2(kk)       # (mantissas below 1.4: the largest difference stays under 2^61)
    d = rng.integers(-8, 9, (C, G)).astype(np.float64)
    ixs = np.stack([np.delete(np.arange(C), c) for c in range(C)])
    t1, t2 = e[ixs, g1] - e[:, None, g1], e[ixs, g2] - e[:, None, g2]            # (C, 63) f64 differences, as the kernel forms them
    assert 2.0 ** -50 <= np.abs(np.stack([t1, t2])).min() and np.abs(np.stack([t1, t2])).max() <= 2.0 ** 61
    root = lambda t: np.sign(t).astype(L) * np.sqrt(np.abs(t).astype(L) + L(psc))
    a1, a2 = root(t1), root(t2)
    b = d.astype(L)
    bm = b.mean(1, keepdims=True)
    vb = ((b - bm) ** 2).sum(1, keepdims=True)
    cov = a1 * (b[:, g1:g1 + 1] - bm) + a2 * (b[:, g2:g2 + 1] - bm)
    va = a1 * a1 + a2 * a2 - (a1 + a2) ** 2 / n
    want = cov / np.sqrt(va * vb)
    ratio_a = np.sqrt((a1 * a1 + a2 * a2) / va)
    ratio_b = np.sqrt((b * b).sum(1, keepdims=True) / vb)
    own = 16 * np.maximum(ratio_a, ratio_b) ** 2 * L(2.0 ** -53)
    E, Dm = ops.CellMatrix.from_cells_major(e, "float64"), ops.CellMatrix.from_cells_major(d, "float64")
    got = ops.coldeltacor_partial(E, Dm, ixs, ops.SQRT, ops.RULES_PARTIAL, psc).cpu().numpy()
    err = np.abs(got.astype(L) - want)
    bound = 2 * ratio_a * L(DELTA) + own
    print(f"psc {psc:g}: DELTA 2^{np.log2(DELTA):.2f}, max |r - closed form| {float(err.max()):.3g}, max err / bound {float((err / bound).max()):.3g}, "
          f"bound {float(bound.min()):.3g} .. {float(bound.max()):.3g}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (float(err.max()), float((err / bound).max()))
    diff = np.abs(got - ops.coldeltacor_partial(E, Dm, ixs, ops.SQRT, ops.RULES_PARTIAL_ROOT2, psc).cpu().numpy())
    print(f"psc {psc:g}: max |r_1 - r_3| {diff.max():.3g}, pairs that differ {int((diff > 0).sum())} of {diff.size}")
    assert diff.max() > 0


# --------------------------------------------------------------------------- homogeneity
@pytest.mark.gpu
@pytest.mark.parametrize("G", GENES)
@pytest.mark.parametrize("C,nr", SHAPES)
def test_four_times_the_data_gives_the_same_bits(ops, C, nr, G):
    """e and psc times 4: the correlations of the plain entry and of both outputs of the dual entry are the unscaled call's, bit for bit,
    under both rules values.  Pooled count rows: |t| is an exact 0 or at least 1e-6 (asserted here), so the 1e-16 threshold - which does not
    scale - separates the same elements in both calls."""
    rng = np.random.default_rng(77 * C + G)
    e = _pooled(rng, C, G, 0.3)
    d, d2 = rng.normal(size=(C, G)), rng.normal(size=(C, G))
    ixs = np.stack([rng.choice(C, nr, replace=False) for _ in range(C)])
    t = np.abs(e[ixs] - e[:, None, :])
    assert ((t == 0) | (t >= 1e-6)).all() and (t == 0).any() and (t > 0).any()
    assert np.array_equal(4.0 * e / 4.0, e) and 4.0 * PSC / 4.0 == PSC
    E, E4, Dm, D2 = (ops.CellMatrix.from_cells_major(a, "float64") for a in (e, 4.0 * e, d, d2))
    for rules in (ops.RULES_PARTIAL, ops.RULES_PARTIAL_ROOT2):
        one = lambda M, p: (ops.coldeltacor_partial(M, Dm, ixs, ops.SQRT, rules, p), *ops.coldeltacor_partial_dual(M, Dm, D2, ixs, ops.SQRT, rules, p))
        r1, r4 = one(E, PSC), one(E4, 4.0 * PSC)
        assert bool(torch.isfinite(r1[0]).any())
        for x, y, what in zip(r1, r4, ("plain", "dual", "dual control")):
            assert _same_bits(x, y), (rules, what, float(torch.nan_to_num(x - y).abs().max()))


# --------------------------------------------------------------------------- edges of the domain
_edge_cache = {}


def _edge_problem(ops, C, nr, G, plant):
    """Made once per case and never written.  Pooled count rows (exact zeros, so t is exactly 0 in many genes) with one plant:
      tiny  rows 2 and 3 differ in gene 0 only, by |t| = 1.2e-16 (kept, just above the rule's 1e-16); run at psc = 0
      wide  1e-30 against 1e30 in the last gene
      huge  |t| = 3e38 in the last gene (-1.5e38 against 1.5e38: beyond what ops.check_f64_sqrt_domain admits, inside what the element takes)
      same  rows 0 and 1 identical; rows 2 and 3 differ in gene 0 only, by |t| = 2^-54 (discarded): zero variance twice; cell 0 lists itself"""
    key = (C, nr, G, plant)
    if key in _edge_cache:
        return _edge_cache[key]
    rng = np.random.default_rng(1000 * C + G)
    s = _pooled(rng, C, G, 0.3)
    d = rng.integers(-8, 9, (C, G)).astype(np.float64)          # small integers: the sums of d are exact, what is seen is the element and sum A
    ixs = np.stack([rng.choice(C, nr, replace=False) for _ in range(C)])
    psc = PSC
    if plant == "tiny":
        s[3] = s[2]
        s[2, 0], s[3, 0], psc = 1e-3, 1e-3 + 1.2e-16, 0.0
        assert 1.1e-16 < s[3, 0] - s[2, 0] < 1.3e-16
    elif plant == "wide":
        s[2, G - 1], s[3, G - 1] = 1e-30, 1e30
    elif plant == "huge":
        s[2, G - 1], s[3, G - 1] = -1.5e38, 1.5e38
    else:
        s[1] = s[0]
        s[3] = s[2]
        s[2, 0], s[3, 0] = 0.25, 0.25 + 2.0 ** -54
        ixs[0, 0], ixs[1, 0] = 0, 0
    ixs[2, 0], ixs[3, 0] = 3, 2                                  # the planted pair, from both sides
    want, ratio, rb = _oracle(s, d, ixs, psc)
    ok = ~np.isnan(want.astype(np.float64))
    # the 1e-10 bar is ten times what rounding can do on this data: a G-term raw-moment sum and the 16 operations after it, amplified by the
    # cancellation ratios (a two-gene pair, r = +-1 whatever the roots, can have any ratio: the smallest G here is 5)
    assert ((16 + G) * np.maximum(ratio, rb)[ok] ** 2 * L(2.0 ** -53) <= 1e-11).all()
    p = dict(S=ops.CellMatrix.from_cells_major(s, "float64"), D=ops.CellMatrix.from_cells_major(d, "float64"), ixs=ixs, psc=psc, want=want)
    _edge_cache[key] = p
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("plant", ["tiny", "wide", "huge", "same"])
@pytest.mark.parametrize("G", EDGE_GENES)
@pytest.mark.parametrize("C,nr", SHAPES)
def test_domain_edges_through_the_scaled_element(ops, C, nr, G, plant):
    """The planted pairs are finite (tiny, wide, huge) or NaN (same: exactly where the restatement has zero variance), every entry meets
    the 1e-10 bar against the long-double restatement and has its NaN pattern."""
    p = _edge_problem(ops, C, nr, G, plant)
    want = p["want"]
    nan = np.isnan(want.astype(np.float64))
    if plant == "same":
        assert nan[0, 0] and nan[1, 0] and nan[2, 0] and nan[3, 0] and not nan.all()
    else:
        assert not nan[2, 0] and not nan[3, 0]
    got = ops.coldeltacor_partial(p["S"], p["D"], p["ixs"], ops.SQRT, ops.RULES_PARTIAL, p["psc"], validate=False).cpu().numpy()
    assert np.array_equal(np.isnan(got), nan)
    assert np.isfinite(got[~nan]).all()
    err = np.abs(got[~nan].astype(L) - want[~nan])
    print(f"C {C} nr {nr} G {G} {plant}: planted pair {got[2, 0]!r} / {got[3, 0]!r}, max |r - restatement| {float(err.max()):.3g}, NaN {int(nan.sum())} of {nan.size}")
    assert err.max() <= 1e-10, float(err.max())


# --------------------------------------------------------------------------- fused / dual consistency
@pytest.mark.gpu
def test_fused_and_dual_entries_share_the_scaled_element(ops):
    """RULES_PARTIAL on 26 cells x 9 listed, G = 1025 (grouped kernels, a second chunk of one gene): fused == plain and fused dual == dual
    bit for bit; the dual entry's first output against the single launch within the rounding of the d-moments, the one thing the two
    launches do not sum in the same order (two waves stage a member in the single launch, four in the dual one): sum b and sum b^2 carry
    at most g = G 2^-53 each, which moves r by at most 1.5 g ratio_b^2 |r| through vb and g ratio_A ratio_b through cov."""
    C, nr, G = 26, 9, 1025
    rng = np.random.default_rng(1000 * C + G)
    s, u = _pooled(rng, C, G, 0.3), _pooled(rng, C, G, 0.15)
    ixs = np.stack([rng.choice(C, nr, replace=False) for _ in range(C)])
    ixs[0, 0] = 0                                                 # a cell that lists itself: NaN
    gam = torch.as_tensor(rng.gamma(2.0, 0.3, G).astype(np.float32))
    q = torch.as_tensor(rng.gamma(1.0, 0.05, G).astype(np.float32))
    d2 = rng.normal(size=(C, G))
    Sx, Ux, D2 = (ops.CellMatrix.from_cells_major(a, "float64") for a in (s, u, d2))
    dmat = ops.velocity_chain(Sx, Ux, gam, q, want=("dmat",), transform=ops.SQRT, psc=PSC)["dmat"]
    want, ratio, rb = _oracle(s, dmat.t[:, :G].cpu().numpy(), ixs, PSC)
    rules = ops.RULES_PARTIAL
    a = ops.coldeltacor_partial(Sx, dmat, ixs, ops.SQRT, rules, PSC)
    fu = ops.coldeltacor_partial_fused(Sx, Ux, gam, q, ixs, ops.SQRT, rules, PSC)
    du, du2 = ops.coldeltacor_partial_dual(Sx, dmat, D2, ixs, ops.SQRT, rules, PSC)
    fd, fd2 = ops.coldeltacor_partial_fused_dual(Sx, Ux, gam, q, D2, ixs, ops.SQRT, rules, PSC)
    assert np.array_equal(_bits(fu), _bits(a)) and np.array_equal(_bits(fd), _bits(du)) and np.array_equal(_bits(fd2), _bits(du2))
    x, y = du.cpu().numpy(), a.cpu().numpy()
    ok = ~np.isnan(want.astype(np.float64))
    assert not ok[0, 0] and ok.any()
    assert np.array_equal(np.isnan(x), ~ok) and np.array_equal(np.isnan(y), ~ok)
    dd = np.abs(x - y)[ok].astype(L)
    bound = (L(G) * L(2.0 ** -53) * (1.5 * rb ** 2 + ratio * rb))[ok]
    err = np.abs(y[ok].astype(L) - want[ok])
    print(f"max |dual - single| {float(dd.max()):.3g}, max over its bound {float((dd / bound).max()):.3g}; max |single - restatement| {float(err.max()):.3g}")
    assert (dd <= bound).all(), float((dd / bound).max())
    assert err.max() <= 1e-10, float(err.max())
