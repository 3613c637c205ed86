"""The zero rule of the f64 partial-sqrt stage D (`|t| < 1e-16 -> A = 0`, speedboosted.pyx:372-378) where it is an execution mask: in
k_cdc_partial_grouped<double, SQRT, RULES_PARTIAL | RULES_PARTIAL_ROOT2> (csrc/coldeltacor.hip) the compare switches a discarded element's
lane off for the root and the three moment updates, and the sums of a pair start at zero instead of at the pair's first element.  Discarded
elements are planted where that can go wrong, and the single, dual, fused and fused-dual entries are compared with a long-double
restatement of the rule (the one of tests/test_gpu_cdc_root.py) at the project's f64 bar, 1e-10 absolute with equal NaN patterns, for
rules 1 and 3 and psc 1e-10 and 1.0.

Shapes: 12 cells x 6 listed (the one-cell-per-workgroup kernel, which keeps the select form: the same data must give the same answers) and
26 x 9 (the grouped kernels - they need >= 24 cells, dual >= 16, and >= 8 listed - where the mask is), each at G in {1, 2, 3, 127, 128,
129, 1024, 1025, 1153, 2049}: the lane vector (2 genes), the wave vector (128), the chunk (1024) and short last chunks.

Layout of an f64 chunk: lane l holds genes 2 (l + 64 u) + k of vector u = 0..7, element k = 0, 1.  Planted genes P (those below G; on G <= 3
one gene stays unplanted so that no pair has the same non-zero A in every gene - raw moments and centred sums disagree about such a pair,
with or without a mask):
    0     vector 0, element 0: the first element of a pair          1     element 1 of a vector
    896   first gene of the last vector                             1023  last gene of the last vector (end of a whole chunk)
    1024  first gene of the second chunk                            G - 1 end of the short last chunk
Rows (every cell is a member with its own list; the planted lists come first):
    0, 1, 2       0.25, 0.25 + 1 ulp, 0.25 + 2 ulps at every gene of P (1 ulp = 2^-54 = 5.6e-17: discarded; 2 ulps = 1.1e-16: kept)
    6 + j         0.25 + 1 ulp at P[j] alone: (0, 6 + j) has 0 < t < 1e-16 there, (1, 6 + j) has t == 0 there, nothing else discarded by design
    2 -> 0, 1     t = -2 ulps (kept: the threshold side) and t = -1 ulp (discarded) at every gene of P
    4, 5 == 7     identical rows: the pairs (4, 7), (5, 7) are discarded whole (NaN), between the ordinary pairs of row 7 with members 0, 1, 3
                  and 6 of the same workgroup (6-cell groups 0..5 | 6..11, dual 4-cell groups 0..3 | 4..7) - stale sums would show
    3 -> 9        row 9 equals row 3 in genes 0..127: vector 0 of the pair is discarded whole (no lane left: the skip branch)
    5 -> 10       row 10 equals row 5 in genes 384..511: vector 3, mid-chunk (G >= 512)
The base data is continuous (gamma) with half the entries exactly zero, so exact-zero differences are everywhere besides.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

L = np.longdouble
Q, U1 = 0.25, 2.0 ** -54
G_ALL = [1, 2, 3, 127, 128, 129, 1024, 1025, 1153, 2049]
SHAPES = [(12, 6), (26, 9)]
PSCS = [1e-10, 1.0]
BAR = 1e-10
RATIO_MAX = 100.0


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def _oracle(e, ds, ixs, psc):
    """Long-double r (C, nr) for each d of `ds` from cells-major f64 e, d (C, G): the rule of speedboosted.pyx:372-378 on the f64 difference t,
    centred sums.  Zero variance, or anything non-finite in A or d[c]: NaN."""
    C, nr = ixs.shape
    out = [np.full((C, nr), np.nan, L) for _ in ds]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(C):
            t = e[ixs[c]] - e[c][None, :]
            a = np.where(np.abs(t) < 1e-16, L(0), np.sign(t).astype(L) * np.sqrt(np.abs(t).astype(L) + L(psc)))
            ac = a - a.mean(1, keepdims=True)
            va = (ac * ac).sum(1)
            for o, d in zip(out, ds):
                b = d[c].astype(L)
                bc = b - b.mean()
                o[c] = (ac * bc[None, :]).sum(1) / np.sqrt(va * (bc * bc).sum())
    return out


def _positions(G):
    P = sorted({p for p in (0, 1, 896, 1023, 1024, G - 1) if p < G})
    while len(P) > max(1, G - 1):
        P.pop()
    return P


_cache = {}


def _ratio(e, ixs, psc):
    """Largest sqrt(sum A^2 / sum (A - mean A)^2) over the pairs of non-zero variance, in long double."""
    worst = L(0)
    for c in range(ixs.shape[0]):
        t = e[ixs[c]] - e[c][None, :]
        a = np.where(np.abs(t) < 1e-16, L(0), np.sign(t).astype(L) * np.sqrt(np.abs(t).astype(L) + L(psc)))
        ac = a - a.mean(1, keepdims=True)
        va, aa = (ac * ac).sum(1), (a * a).sum(1)
        if (va > 0).any():
            worst = max(worst, np.sqrt(aa[va > 0] / va[va > 0]).max())
    return float(worst)


def _problem(C, nr, G):
    """The planted matrices and lists of one shape (host arrays, made once, never written).  The data is well conditioned by construction:
    a relative error delta of the roots moves r by up to 2 delta sqrt(sum A^2 / sum (A - mean A)^2) (tests/test_gpu_cdc_root.py), and
    RULES_PARTIAL's root is good to delta = 2^-43.5 (include/velocyto_hip.h) - the 1e-10 bar can be asked of it only where that ratio
    stays small.  On two or three genes a random pair can have nearly the same A in every gene (any ratio); the draw is repeated, seed
    after seed, until every pair's ratio is at most RATIO_MAX = 100 at both pseudocounts (root: 1.6e-11; the kernel's own f64 rounding,
    16 ratio^2 2^-53: 1.8e-11).  Decided on the long-double oracle alone, never on what a kernel returns."""
    key = (C, nr, G)
    if key in _cache:
        return _cache[key]
    for attempt in range(200):
        h = _draw(C, nr, G, 88000 + 100 * C + G + 1000000 * attempt)
        if max(_ratio(h["s"], h["ixs"], psc) for psc in PSCS) <= RATIO_MAX:
            break
    else:
        raise AssertionError("no well-conditioned draw")
    _cache[key] = h
    return h


def _draw(C, nr, G, seed):
    rng = np.random.default_rng(seed)
    s = rng.gamma(2.0, 1.0, (C, G)) * (rng.random((C, G)) < 0.5)
    u = rng.gamma(1.0, 1.0, (C, G)) * (rng.random((C, G)) < 0.5)
    d2 = rng.normal(size=(C, G))
    P = _positions(G)
    s[0, P], s[1, P], s[2, P] = Q, Q + U1, Q + 2 * U1
    for j, p in enumerate(P):
        s[6 + j, p] = Q + U1
    s[4] = s[7]
    s[5] = s[7]
    s[9, :128] = s[3, :128]
    if G >= 512:
        s[10, 384:512] = s[5, 384:512]
    rows_p = [6 + j for j in range(len(P))]
    forced = {0: rows_p + [7], 1: rows_p + [7], 2: [0, 1], 3: [7, 9], 4: [7], 5: [7, 10], 6: [7]}
    ixs = np.empty((C, nr), np.int64)
    for m in range(C):
        f = list(dict.fromkeys(forced.get(m, [])))
        free = [r for r in range(3, C) if r != m and r not in f]        # rows 0..2 are listed by member 2 alone
        ixs[m] = f + list(rng.choice(free, nr - len(f), replace=False))
    gam = rng.gamma(2.0, 0.3, G).astype(np.float32)
    q = rng.gamma(1.0, 0.05, G).astype(np.float32)
    # the planted differences are what the docstring says they are
    for j, p in enumerate(P):
        assert 0 < s[6 + j, p] - s[0, p] < 1e-16 and s[6 + j, p] - s[1, p] == 0 and ixs[0, j] == 6 + j and ixs[1, j] == 6 + j
    assert 1e-16 < s[2, 0] - s[0, 0] < 1.2e-16 and 0 < s[2, 0] - s[1, 0] < 1e-16 and list(ixs[2, :2]) == [0, 1]
    assert 7 in ixs[0] and 7 in ixs[1] and ixs[3, 0] == 7 and ixs[4, 0] == 7 and ixs[5, 0] == 7 and ixs[6, 0] == 7 and ixs[3, 1] == 9 and ixs[5, 1] == 10
    assert np.array_equal(s[4], s[7]) and np.array_equal(s[5], s[7]) and np.array_equal(s[9, :128], s[3, :128])
    return dict(s=s, u=u, d2=d2, ixs=ixs, gam=gam, q=q, P=P)


_dev_cache = {}


def _on_device(ops, tag, s, u, d2, gam, q, ixs, psc):
    """Device matrices, the materialised dmat of the velocity chain and the oracle's r for (d, d2), made once per (tag, psc)."""
    key = (tag, psc)
    if key in _dev_cache:
        return _dev_cache[key]
    Sx, Ux, D2 = (ops.CellMatrix.from_cells_major(a, "float64") for a in (s, u, d2))
    tg, tq = torch.as_tensor(gam), torch.as_tensor(q)
    dmat = ops.velocity_chain(Sx, Ux, tg, tq, want=("dmat",), transform=ops.SQRT, psc=psc)["dmat"]
    d = dmat.t[:, :s.shape[1]].cpu().numpy()
    want, want2 = _oracle(s, (d, d2), ixs, psc)
    _dev_cache[key] = dict(Sx=Sx, Ux=Ux, D2=D2, dmat=dmat, d=d, gam=tg, q=tq, want=want, want2=want2)
    return _dev_cache[key]


def _entries(ops, p, ixs, rules, psc, validate=True):
    """[(entry, result, oracle)] of the four entries."""
    a = ops.coldeltacor_partial(p["Sx"], p["dmat"], ixs, ops.SQRT, rules, psc, validate=validate)
    du, du2 = ops.coldeltacor_partial_dual(p["Sx"], p["dmat"], p["D2"], ixs, ops.SQRT, rules, psc, validate=validate)
    fu = ops.coldeltacor_partial_fused(p["Sx"], p["Ux"], p["gam"], p["q"], ixs, ops.SQRT, rules, psc, validate=validate)
    fd, fd2 = ops.coldeltacor_partial_fused_dual(p["Sx"], p["Ux"], p["gam"], p["q"], p["D2"], ixs, ops.SQRT, rules, psc, validate=validate)
    return [("single", a, p["want"]), ("dual", du, p["want"]), ("dual control", du2, p["want2"]), ("fused", fu, p["want"]),
            ("fused dual", fd, p["want"]), ("fused dual control", fd2, p["want2"])]


def _check(name, got, want, what):
    got = got.cpu().numpy()
    ok = ~np.isnan(want.astype(np.float64))
    assert np.array_equal(np.isnan(got), ~ok), (what, name, np.argwhere(np.isnan(got) != ~ok)[:8].tolist())
    err = float(np.abs(got[ok].astype(L) - want[ok]).max()) if ok.any() else 0.0
    print(f"{what} {name}: max |r - oracle| {err:.3g} over {int(ok.sum())} pairs, {int((~ok).sum())} NaN")
    assert err <= BAR, (what, name, err)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("G", G_ALL)
@pytest.mark.parametrize("C,nr", SHAPES)
def test_discarded_elements_at_sensitive_positions(ops, C, nr, G):
    """Exact zeros and 0 < |t| < 1e-16 at the first element of a pair, element 1 of a vector, the last vector, the first gene of the second
    chunk and the end of the short last chunk; |t| = 2 ulps kept; whole vectors discarded (vector 0 and mid-chunk); whole pairs discarded
    between ordinary pairs of the same neighbour row: every entry, rules 1 and 3, psc 1e-10 and 1.0, against the oracle."""
    h = _problem(C, nr, G)
    for psc in PSCS:
        p = _on_device(ops, ("main", C, nr, G), h["s"], h["u"], h["d2"], h["gam"], h["q"], h["ixs"], psc)
        nan = np.isnan(p["want"].astype(np.float64))
        assert nan[4, 0] and nan[5, 0]                                    # the whole pairs (4, 7), (5, 7)
        if G >= 127:
            assert not nan[0].any() and not nan[1].any() and not nan[2, :2].any() and not nan[3, 0] and not nan[6, 0]
            assert nan[3, 1] or G > 128                                  # row 9 equals row 3 in genes 0..127
        for rules in (ops.RULES_PARTIAL, ops.RULES_PARTIAL_ROOT2):
            for name, got, want in _entries(ops, p, h["ixs"], rules, psc):
                _check(name, got, want, f"C {C} nr {nr} G {G} psc {psc:g} rules {rules}")


@pytest.mark.gpu
@pytest.mark.parametrize("G", G_ALL)
@pytest.mark.parametrize("C,nr", SHAPES)
def test_discard_invariance(ops, C, nr, G):
    """Every 0.25 + 1 ulp becomes 0.25: for member 0 (0.25 in the planted genes, its own row and hence its d unchanged) every difference that
    changes goes from 0 < |t| < 1e-16 to exactly 0 - its correlations keep their bits in every entry."""
    h = _problem(C, nr, G)
    s, ixs, P = h["s"], h["ixs"], h["P"]
    s0 = s.copy()
    cols = s0[:, P]
    cols[cols == Q + U1] = Q
    s0[:, P] = cols
    t, t0 = s[ixs[0]] - s[0][None, :], s0[ixs[0]] - s0[0][None, :]
    ch = t != t0
    assert ch.sum() >= len(P) and ((np.abs(t[ch]) < 1e-16) & (t[ch] != 0) & (t0[ch] == 0)).all() and np.array_equal(s0[0], s[0])
    for psc in PSCS:
        p = _on_device(ops, ("main", C, nr, G), s, h["u"], h["d2"], h["gam"], h["q"], ixs, psc)
        p0 = dict(p, Sx=ops.CellMatrix.from_cells_major(s0, "float64"))     # the same dmat: the plain entries see only e change
        for rules in (ops.RULES_PARTIAL, ops.RULES_PARTIAL_ROOT2):
            for (name, a, _), (_, b, _) in zip(_entries(ops, p, ixs, rules, psc), _entries(ops, p0, ixs, rules, psc)):
                a, b = a[0].cpu().numpy(), b[0].cpu().numpy()
                assert np.array_equal(a.view(np.int64), b.view(np.int64)), (name, rules, psc, a, b)
                assert np.isfinite(a).all() or G < 127


@pytest.mark.gpu
@pytest.mark.parametrize("G", G_ALL)
@pytest.mark.parametrize("C,nr", SHAPES)
def test_nan_and_inf_in_e(ops, C, nr, G):
    """NaN in a neighbour row (8), +inf in a member row (3) and in one of its neighbours at the same gene (9: t = inf - inf), -inf in the last
    row: a NaN t is a KEPT element (`!(|t| < 1e-16)`), an infinite one gives an infinite A - the NaN pattern is the oracle's, the rest holds
    the bar.  (validate=False: the f64 sqrt-domain check refuses a matrix that holds an infinity.)"""
    h = _problem(C, nr, G)
    s = h["s"].copy()
    ga, gb = min(G - 1, 5), min(G - 1, 70)
    s[8, ga] = np.nan
    s[3, gb] = s[9, gb] = np.inf
    s[C - 1, ga] = -np.inf
    for psc in PSCS:
        p = _on_device(ops, ("nonfinite e", C, nr, G), s, h["u"], h["d2"], h["gam"], h["q"], h["ixs"], psc)
        nan = np.isnan(p["want"].astype(np.float64))
        assert nan[8].all() and nan[3].all() and nan[C - 1].all() and nan[h["ixs"] == 8].all() and nan[h["ixs"] == 3].all()
        for rules in (ops.RULES_PARTIAL, ops.RULES_PARTIAL_ROOT2):
            for name, got, want in _entries(ops, p, h["ixs"], rules, psc, validate=False):
                _check(name, got, want, f"non-finite e: C {C} nr {nr} G {G} psc {psc:g} rules {rules}")


@pytest.mark.gpu
@pytest.mark.parametrize("G", G_ALL)
@pytest.mark.parametrize("C,nr", SHAPES)
def test_nan_and_inf_in_d_at_a_discarded_gene(ops, C, nr, G):
    """d[c] is NaN or inf at a gene where the element is discarded (member 1 at gene 0, t == 0 against row 6; member 0's control at gene 0,
    0 < t < 1e-16; member 4, whose pair with row 7 is discarded whole; member 5's control likewise): the product A b is never formed there,
    and the result is NaN all the same, through sum b - for every pair of that member, like the oracle's."""
    h = _problem(C, nr, G)
    u, d2 = h["u"].copy(), h["d2"].copy()
    g = min(G - 1, 5)
    u[1, 0], u[4, g] = np.nan, np.inf
    d2[0, 0], d2[5, g] = np.inf, np.nan
    for psc in PSCS:
        p = _on_device(ops, ("nonfinite d", C, nr, G), h["s"], u, d2, h["gam"], h["q"], h["ixs"], psc)
        assert not np.isfinite(p["d"][1, 0]) and not np.isfinite(p["d"][4, g])
        nan, nan2 = np.isnan(p["want"].astype(np.float64)), np.isnan(p["want2"].astype(np.float64))
        assert nan[1].all() and nan[4].all() and nan2[0].all() and nan2[5].all()
        assert G < 127 or (not nan[0].any() and not nan2[1].any())
        for rules in (ops.RULES_PARTIAL, ops.RULES_PARTIAL_ROOT2):
            for name, got, want in _entries(ops, p, h["ixs"], rules, psc):
                _check(name, got, want, f"non-finite d: C {C} nr {nr} G {G} psc {psc:g} rules {rules}")
