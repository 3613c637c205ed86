"""The two roots of the f64 partial-sqrt rule of stage D (csrc/coldeltacor.hip): RULES_PARTIAL forms sqrt(|t| + psc) with ONE Newton
correction on an f32 seed (relative error of A at most 2^-43.5, include/velocyto_hip.h), RULES_PARTIAL_ROOT2 with two (correctly
rounded except near ties).  Everything goes through the C ABI on cuda:0 and is compared with long-double restatements made here.

Bounds (none is taken from what the kernels return):
  * element test: a pair whose cells differ in two genes only has A = (a1, a2, 0, ..., 0); r is a closed form of the two roots.  A
    relative error delta on each root moves r by at most 2 delta sqrt(sum A^2 / sum (A - mean A)^2) = C delta (Cauchy-Schwarz on the
    centred, normalised vectors, as in ops.partial_rules_for); delta = 2^-43.5 + 2^-53 for the one-correction root (the second term:
    the rounding of |t| + psc, half of which reaches the root, and the final rounding), 2^-52 for the two-correction one (half an ulp,
    one ulp near ties, plus the same rounding of the argument).  The kernel's own f64 arithmetic between the roots and r is at most 16
    rounded operations (three moment updates of two terms, the products, quotients and differences of pearson_from_moments, one
    square root), each amplified by at most the product of the two cancellation ratios sqrt(sum A^2 / sum (A - mean A)^2) and
    sqrt(sum b^2 / sum (b - mean b)^2): 16 max(ratio_A, ratio_b)^2 2^-53.  d holds small integers, so its own sums are exact.
  * edge tests: the project's f64 bar against the oracle (1e-10 absolute), equal NaN patterns, and the a-priori distance of the two
    roots |r_1 - r_3| <= 2 2^-43.5 sqrt(sum A^2 / sum (A - mean A)^2) with the ratio from the long-double oracle.
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

L = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D1 = 2.0 ** -43.5
PSC = 1e-10


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def test_rules_values_agree_with_the_header():
    """ops.RULES_* are the enumerators of include/velocyto_hip.h, each with a name (no GPU needed)."""
    import velocyto_amd
    from velocyto_amd import ops as _ops
    text = open(os.path.join(ROOT, "include", "velocyto_hip.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(VCY_RULES_[A-Z0-9_]+) = (\d+)", text))
    assert enum == {"VCY_RULES_FULL": _ops.RULES_FULL, "VCY_RULES_PARTIAL": _ops.RULES_PARTIAL, "VCY_RULES_PARTIAL_NOPSC": _ops.RULES_PARTIAL_NOPSC,
                    "VCY_RULES_PARTIAL_ROOT2": _ops.RULES_PARTIAL_ROOT2}
    assert _ops.RULES_PARTIAL_ROOT2 == 3 and set(_ops.RULE_NAMES) == set(enum.values())


# --------------------------------------------------------------------------- long-double restatement
def _oracle(e, d, ixs, psc):
    """(r, ratio, ratio_b) in long double from cells-major f64 e, d (C, G): the rule of speedboosted.pyx:372-378 on the f64 difference t
    (the reference and the kernels both form t in f64), centred sums; ratio = sqrt(sum A^2 / sum (A - mean A)^2) per pair, ratio_b the same
    of d[c] per cell.  Zero variance: NaN."""
    C, nr = ixs.shape
    r = np.full((C, nr), np.nan, L)
    ratio = np.full((C, nr), np.nan, L)
    ratio_b = np.full((C, 1), np.nan, L)
    with np.errstate(invalid="ignore", divide="ignore"):
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


# --------------------------------------------------------------------------- the element through the grouped kernel
@pytest.mark.gpu
@pytest.mark.parametrize("psc", [PSC, 0.0])
def test_root_accuracy_through_the_kernel(ops, psc):
    """64 cells x 63 neighbours, G = 130: every pair differs in genes 5 and 77 only, by |t| over 2^-50 .. 2^61 (magnitudes on a log
    grid, random mantissas and signs), so r is a closed form of two roots.  |r - closed form| <= C delta + the kernel's own rounding
    (module docstring) for each rules value, and the two values differ somewhere (else the element is not what is being seen)."""
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
    got = {}
    for rules, delta in ((ops.RULES_PARTIAL, D1 + 2.0 ** -53), (ops.RULES_PARTIAL_ROOT2, 2.0 ** -52)):
        got[rules] = ops.coldeltacor_partial(E, Dm, ixs, ops.SQRT, rules, psc).cpu().numpy()
        err = np.abs(got[rules].astype(L) - want)
        bound = 2 * ratio_a * L(delta) + own
        print(f"psc {psc:g} rules {rules}: max |r - closed form| {float(err.max()):.3g}, max err / bound {float((err / bound).max()):.3g}, "
              f"bound {float(bound.min()):.3g} .. {float(bound.max()):.3g}")
        assert np.isfinite(got[rules]).all()
        assert (err <= bound).all(), (rules, float(err.max()), float((err / bound).max()))
    diff = np.abs(got[ops.RULES_PARTIAL] - got[ops.RULES_PARTIAL_ROOT2])
    print(f"psc {psc:g}: max |r_1 - r_3| {diff.max():.3g}, pairs that differ {int((diff > 0).sum())} of {diff.size}")
    assert diff.max() > 0


# --------------------------------------------------------------------------- edges
EDGE_G = [2, 3, 127, 128, 129, 1023, 1024, 1025, 2049]
EDGE_SHAPES = [(7, 5), (13, 7), (26, 9)]       # (cells, list): the one-cell-per-workgroup kernel twice, and the grouped kernel (>= 24 cells, >= 8 listed)
_edge_cache = {}


def _edge_problem(ops, C, nr, G):
    """Made once per shape and never written.  Count-like pooled rows (Poisson counts x size factors averaged over four cells: exact
    zeros where all four are empty, so t is exactly 0 in many genes) with planted entries: rows 0 and 1 identical (zero variance),
    0.25 against 0.25 + one and two ulps (|t| = 5.6e-17: discarded; 1.1e-16: kept) in the first gene, 1e-30 and 1e30 in the last."""
    key = (C, nr, G)
    if key in _edge_cache:
        return _edge_cache[key]
    rng = np.random.default_rng(1000 * C + G)
    f = rng.gamma(8.0, 0.125, 3 * C)
    pool = lambda lam: np.stack([(rng.poisson(lam, (3 * C, G)) * f[:, None])[rng.choice(3 * C, 4, replace=False)].mean(0) for _ in range(C)])
    s, u = pool(0.3), pool(0.15)
    s[1] = s[0]
    s[2, 0], s[3, 0], s[4, 0] = 0.25, 0.25 + 2.0 ** -54, 0.25 + 2.0 ** -53
    s[5, G - 1], s[6, G - 1] = 1e-30, 1e30
    ixs = np.stack([rng.choice(C, nr, replace=False) for _ in range(C)])
    ixs[1, 0], ixs[2, 0], ixs[2, 1], ixs[3, 0], ixs[4, 0], ixs[5, 0], ixs[0, 0] = 0, 3, 4, 2, 2, 6, 0   # the planted pairs; cell 0 lists itself
    gam = rng.gamma(2.0, 0.3, G).astype(np.float32)
    q = rng.gamma(1.0, 0.05, G).astype(np.float32)
    d2 = rng.normal(size=(C, G))
    Sx, Ux, D2 = (ops.CellMatrix.from_cells_major(a, "float64") for a in (s, u, d2))
    tg, tq = torch.as_tensor(gam), torch.as_tensor(q)
    dmat = ops.velocity_chain(Sx, Ux, tg, tq, want=("dmat",), transform=ops.SQRT, psc=PSC)["dmat"]
    d = dmat.t[:, :G].cpu().numpy()
    want, ratio, rb = _oracle(s, d, ixs, PSC)
    want2, _, rb2 = _oracle(s, d2, ixs, PSC)
    _edge_cache[key] = dict(Sx=Sx, Ux=Ux, D2=D2, dmat=dmat, gam=tg, q=tq, ixs=ixs, want=want, want2=want2, ratio=ratio, rb=rb, rb2=rb2)
    return _edge_cache[key]


def _bits(t):
    return t.cpu().numpy().view(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("G", EDGE_G)
@pytest.mark.parametrize("C,nr", EDGE_SHAPES)
def test_edges_plain_fused_dual_both_roots(ops, C, nr, G):
    """Plain, fused, dual and fused-dual entries with both rules values at the lane vector (2 genes), the wave vector (128) and the
    f64 chunk (1024) with short last chunks: the 1e-10 bar against the long-double oracle, its NaN pattern, the a-priori distance of
    the two roots, and for each rules value fused == plain and fused dual == dual bit for bit, and dual == single: bit for bit where the
    dual entry runs the single kernel once per control (the first two shapes: fewer than 8 listed or 24 cells), and on the grouped
    kernels (third shape) up to the rounding of the d-moments, the one thing the two launches do not sum in the same order - sum b and
    sum b^2 of a member are added up by the waves that stage it, two per member in the single launch (6 cells) and four in the dual one
    (4 cells), so from 257 genes on their partial sums split differently (include/velocyto_hip.h says so of VCY_F64).  Both are sums of
    G terms, relative error at most g = G 2^-53 each; through vb = sum b^2 - (sum b)^2 / n that moves r by at most 1.5 g ratio_b^2 |r|,
    through cov = sum A b - sum A sum b / n by at most g ratio_A ratio_b (|sum A| <= sqrt(n) ||A||), the ratios from the oracle."""
    p = _edge_problem(ops, C, nr, G)
    Sx, Ux, D2, dmat, gam, q, ixs = (p[k] for k in ("Sx", "Ux", "D2", "dmat", "gam", "q", "ixs"))
    nan = np.isnan(p["want"].astype(np.float64))
    assert nan[0, 0] and nan[1, 0] and not nan.all()                 # the self pair and the identical rows, and not everything
    plain = {}
    for rules in (ops.RULES_PARTIAL, ops.RULES_PARTIAL_ROOT2):
        a = ops.coldeltacor_partial(Sx, dmat, ixs, ops.SQRT, rules, PSC)
        a2 = ops.coldeltacor_partial(Sx, D2, ixs, ops.SQRT, rules, PSC)
        fu = ops.coldeltacor_partial_fused(Sx, Ux, gam, q, ixs, ops.SQRT, rules, PSC)
        du, du2 = ops.coldeltacor_partial_dual(Sx, dmat, D2, ixs, ops.SQRT, rules, PSC)
        fd, fd2 = ops.coldeltacor_partial_fused_dual(Sx, Ux, gam, q, D2, ixs, ops.SQRT, rules, PSC)
        assert np.array_equal(_bits(fu), _bits(a)) and np.array_equal(_bits(fd), _bits(du)) and np.array_equal(_bits(fd2), _bits(du2)), rules
        for x, y, rb in ((du, a, p["rb"]), (du2, a2, p["rb2"])):
            if C < 24 or nr < 8:
                assert np.array_equal(_bits(x), _bits(y)), rules
                continue
            x, y = x.cpu().numpy(), y.cpu().numpy()
            assert np.array_equal(np.isnan(x), np.isnan(y)), rules
            ok = ~np.isnan(y)
            dd = np.abs(x - y)[ok].astype(L)
            bound = (L(G) * L(2.0 ** -53) * (1.5 * rb ** 2 + p["ratio"] * rb))[ok]
            print(f"C {C} nr {nr} G {G} rules {rules}: max |dual - single| {float(dd.max()):.3g}, max over its bound {float((dd / bound).max()):.3g}")
            assert (dd <= bound).all(), (rules, float((dd / bound).max()))
        for got, want in ((a, p["want"]), (a2, p["want2"])):
            got = got.cpu().numpy()
            ok = ~np.isnan(want.astype(np.float64))
            assert np.array_equal(np.isnan(got), ~ok), rules
            err = np.abs(got[ok].astype(L) - want[ok])
            print(f"C {C} nr {nr} G {G} rules {rules}: max |r - oracle| {float(err.max()):.3g}")
            assert err.max() <= 1e-10, (rules, float(err.max()))
        plain[rules] = a.cpu().numpy()
    ok = ~nan
    diff = np.abs(plain[ops.RULES_PARTIAL][ok] - plain[ops.RULES_PARTIAL_ROOT2][ok]).astype(L)
    bound = 2 * L(D1) * p["ratio"][ok]
    print(f"C {C} nr {nr} G {G}: max |r_1 - r_3| {float(diff.max()):.3g}, max over its bound {float((diff / bound).max()):.3g}")
    assert (diff <= bound).all(), float((diff / bound).max())


# --------------------------------------------------------------------------- where value 3 is value 1
@pytest.mark.gpu
@pytest.mark.parametrize("C,nr,G", [(13, 7, 1025), (40, 9, 1600)])
def test_root2_is_the_partial_rule_elsewhere(ops, C, nr, G):
    """RULES_PARTIAL_ROOT2 names another root for sqrt on f64 only: on an f32 matrix (every entry; small-problem and grouped kernels)
    and with the other transforms on f64 it returns what RULES_PARTIAL returns, bit for bit."""
    rng = np.random.default_rng(C + G)
    s = rng.gamma(2.0, 1.0, (C, G)) * (rng.random((C, G)) < 0.5)
    u = rng.gamma(1.0, 1.0, (C, G)) * (rng.random((C, G)) < 0.5)
    d, d2 = rng.normal(size=(C, G)), rng.normal(size=(C, G))
    ixs = np.stack([rng.choice(C, nr, replace=False) for _ in range(C)])
    gam = torch.as_tensor(rng.gamma(2.0, 0.3, G), dtype=torch.float32)
    same = lambda x, y: torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0))
    for dtype, transforms in (("float32", (ops.SQRT, ops.LOG10, ops.LINEAR)), ("float64", (ops.LOG10, ops.LINEAR))):
        Sx, Ux, Dm, D2 = (ops.CellMatrix.from_cells_major(a, dtype) for a in (s, u, d, d2))
        for tr in transforms:
            psc = 0.0 if tr == ops.LINEAR else PSC
            one = lambda rules: (ops.coldeltacor_partial(Sx, Dm, ixs, tr, rules, psc), ops.coldeltacor_partial_fused(Sx, Ux, gam, None, ixs, tr, rules, psc),
                                 *ops.coldeltacor_partial_dual(Sx, Dm, D2, ixs, tr, rules, psc),
                                 *ops.coldeltacor_partial_fused_dual(Sx, Ux, gam, None, D2, ixs, tr, rules, psc))
            r1, r3 = one(ops.RULES_PARTIAL), one(ops.RULES_PARTIAL_ROOT2)
            assert all(bool(torch.isfinite(x).any()) for x in r1)
            assert all(same(x, y) for x, y in zip(r1, r3)), (dtype, tr)


@pytest.mark.gpu
def test_partial_rules_for_picks_the_root(ops, monkeypatch):
    """f64 + sqrt: RULES_PARTIAL by default, RULES_PARTIAL_ROOT2 under literal=True or VELOCYTO_AMD_LITERAL_RULE=1; the other
    transforms and the f32 decision are what they were."""
    monkeypatch.delenv("VELOCYTO_AMD_LITERAL_RULE", raising=False)
    a = np.random.default_rng(3).gamma(2.0, 1.0, (9, 70))
    E64, E32 = ops.CellMatrix.from_cells_major(a, "float64"), ops.CellMatrix.from_cells_major(a, "float32")
    assert ops.partial_rules_for(E64, ops.SQRT, PSC) == ops.RULES_PARTIAL
    assert ops.partial_rules_for(E64, ops.SQRT, PSC, literal=True) == ops.RULES_PARTIAL_ROOT2
    assert ops.partial_rules_for(E64, ops.LOG10, PSC, literal=True) == ops.RULES_PARTIAL
    assert ops.partial_rules_for(E32, ops.SQRT, PSC) == ops.RULES_PARTIAL_NOPSC
    assert ops.partial_rules_for(E32, ops.SQRT, PSC, literal=True) == ops.RULES_PARTIAL
    monkeypatch.setenv("VELOCYTO_AMD_LITERAL_RULE", "1")
    assert ops.partial_rules_for(E64, ops.SQRT, PSC) == ops.RULES_PARTIAL_ROOT2
    assert ops.partial_rules_for(E64, ops.LINEAR, 0.0) == ops.RULES_PARTIAL
    assert ops.partial_rules_for(E32, ops.SQRT, PSC) == ops.RULES_PARTIAL
