"""The kernels between pooling and stage D at the C ABI, at their edges: vcy_fit_weighted (+ _moments / _from_moments),
vcy_gamma_weights, vcy_lincomb, vcy_scale_log, vcy_delta_transform, vcy_velocity_chain.

The fit is held to oracle.fit_box_reference / fit_kkt / r2_reference (long double, centred data, active set by enumeration; pinned
on the CPU by test_fit_oracle.py), never to box_wls2, which shares the kernel's raw-moment formula and candidate order - except
where the issue is the selection among tied candidates, which only the same formula fed the kernel's own moments can decide.

Bounds.  Outputs are float32: a gene whose f64 error bound is below half a float32 ulp must land within 1 float32 ulp of the
reference rounded to float32, and its bound variables exactly on their bounds.  The f64 error bound is K C eps kappa, with
kappa = Swxx Sw / det for m and q (times the sizes sum w|xy| / sum w x^2 and sum w|y| / sum w of the two quotients) and
kappa = Syy / sstot for R2; K is measured on the CPU (fit_cases.FIT_K = 0.0075, FIT_K_R2 = 135, see
test_the_k_of_the_conditioning_bound_is_what_the_cpu_measures) and the kernel gets 4 K.  Moments: C eps of the sum of the absolute
terms.  Element-wise stages: bit-equal to numpy wherever the arithmetic is + - * / in the storage type, 1-2 ulps through
sqrt / log / pow."""
import math

import numpy as np
import pytest

import fit_cases as fc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DTYPES = ["float64", "float32"]
NP_T = {"float64": np.float64, "float32": np.float32}
SENTINEL = 7777.0
EPS = fc.EPS


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


# ----------------------------------------------------------------------------- helpers: inputs with NaN padding, outputs pre-filled
def _cm(ops, a, dtype):
    """(G, C) array -> device cells-major matrix of `dtype` whose padding columns hold NaN: they must never reach an output."""
    m = ops.CellMatrix.from_genes_major(np.ascontiguousarray(a, dtype=np.float64), dtype)
    if m.ld > m.G:
        m.t[:, m.G:] = float("nan")
    return m


def _filled(ops, like, value=float("nan")):
    return ops.CellMatrix(torch.full_like(like.t, value), like.G)


def _vec(v, dtype=torch.float64):
    return None if v is None else torch.as_tensor(np.ascontiguousarray(v)).to(device="cuda", dtype=dtype).contiguous()


def _ptr(t):
    """Device address of a tensor or of a CellMatrix's storage (a tensor has a method named t: tell them apart by type)."""
    return None if t is None else (t.data_ptr() if isinstance(t, torch.Tensor) else t.t.data_ptr())


def _fit(ops, Y, X, wmode, W=None, M=None, M2=None, sa=None, sb=None, down=None, up=None, fit_offset=1, box_q=1, lo=1e-8,
         up_default=20.0, up_gamma=None, q_fixed=None):
    """vcy_fit_weighted with its three outputs pre-filled: -> (gamma, q, R2) float32 numpy."""
    G = Y.G
    outs = [torch.full((G,), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(3)]
    ws = ops._fit_workspace(G, Y.t.device)
    ws.fill_(255)                                       # every partial a NaN until the kernel writes it
    keep = [_vec(v) for v in (sa, sb, down, up, up_gamma, q_fixed)]
    ops._lib.check(ops._lib.lib().vcy_fit_weighted(Y.t.data_ptr(), X.t.data_ptr(), wmode, _ptr(W), _ptr(M), _ptr(M2), *[_ptr(k) for k in keep[:4]],
                                                   int(fit_offset), int(box_q), float(lo), float(up_default), _ptr(keep[4]), _ptr(keep[5]),
                                                   outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(), Y.C, G, Y.ld,
                                                   Y.code, ops._stream()), "fit_weighted")
    return tuple(o.cpu().numpy() for o in outs)


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


def _ulps(got, ref, np_t):
    """|got - ref| in units of ref's spacing in np_t (NaN where both are NaN or equal infinities -> 0)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    same = (np.isnan(got) & np.isnan(ref)) | (got == ref)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - ref) / np.spacing(np.abs(ref.astype(np_t))).astype(np.float64)
    return np.where(same, 0.0, np.where(np.isfinite(d), d, np.inf))


def _bits_equal(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    nan = np.isnan(got) & np.isnan(ref)
    return bool(np.all((got.view(u) == ref.view(u)) | nan))


# ----------------------------------------------------------------------------- (a) every region of the box
REGION_G = (1, 63, 65, 255, 257, 513)


@pytest.mark.parametrize("wmode", [0, 2])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [33, 131])
@pytest.mark.parametrize("G", REGION_G)
def test_fit_weighted_in_every_region_of_the_box(ops, oracle, G, C, dtype, wmode):
    """Constructed genes (fit_cases.py) in the interior, on the four edges and in the four corners of [lo_gamma, up_gamma] x
    [0, 2 sum(wy)/sum(w)], three launches per case (lo_gamma = -1, 0.5, 1e-8), up_gamma per gene.  From the reference alone: no
    gene is degenerate, each of the nine regions holds >= 8 genes over the six gene counts of this (C, dtype, weight mode) - and
    in this case alone when it has >= 255 genes - and the f64 bound of the conditioning sweep is below half a float32 ulp of every
    free parameter.  Then, per gene and without skipping one: gamma and q within 1 float32 ulp of the reference rounded to
    float32; a parameter the reference puts on a bound is that bound's float32 exactly; the scaled KKT violation of the kernel's
    float32 (m, q) is at most that of the reference's rounded (m, q) plus twice the relative f64 bound (the gradient is linear in
    the parameters)."""
    launches = fc.region_launches(G, C, dtype, wmode)
    family = fc.census([L for g in REGION_G for L in fc.region_launches(g, C, dtype, wmode)])
    assert family["degenerate"] == 0 and min(family[r] for r in oracle.FIT_REGIONS) >= 8, family
    own = fc.census(launches)
    assert own["degenerate"] == 0
    if G >= 255:
        assert min(own[r] for r in oracle.FIT_REGIONS) >= 8, own
    worst_ulp = worst_kkt = 0.0
    for L in launches:
        X, Y, W = L["X"], L["Y"], L["W"]
        rel = np.empty(G)                               # 4 K C eps kappa, and it times the size of each parameter
        bm, bq = np.empty(G), np.empty(G)
        for g in range(G):
            kf, _, sm, sq = oracle.fit_condition(X[g], Y[g], W[g])
            rel[g] = 4 * fc.FIT_K * C * EPS * kf
            bm[g], bq[g] = rel[g] * sm, rel[g] * sq
        m_free = np.array([r[2:4] == "in" for r in L["region"]])
        q_free = np.array([r[7:9] == "in" for r in L["region"]])
        assert np.all(bm[m_free] < 0.5 * _ulp32(L["m"][m_free])) and np.all(bq[q_free] < 0.5 * _ulp32(L["q"][q_free]))
        # ---- the kernel
        Yd, Xd = _cm(ops, Y, dtype), _cm(ops, X, dtype)
        Wd = _cm(ops, W, dtype) if wmode == 0 else None
        m32, q32, r2 = _fit(ops, Yd, Xd, wmode, W=Wd, lo=L["lo"], up_gamma=L["up"])
        assert not np.any(m32 == SENTINEL) and not np.any(q32 == SENTINEL) and not np.any(r2 == SENTINEL)
        lo32, hiq32 = float(np.float32(L["lo"])), np.float32(L["hi_q"]).astype(np.float64)
        for g in range(G):
            region, what = L["region"][g], (L["lo"], g, L["region"][g], float(m32[g]), float(q32[g]), L["m"][g], L["q"][g])
            um = abs(float(m32[g]) - float(np.float32(L["m"][g]))) / _ulp32(L["m"][g])
            uq = abs(float(q32[g]) - float(np.float32(L["q"][g]))) / max(_ulp32(L["q"][g]), 1e-45)
            assert um <= 1 and uq <= 1, what
            worst_ulp = max(worst_ulp, um, uq)
            if region[2:4] == "lo":
                assert m32[g] == np.float32(L["lo"]), what
            if region[2:4] == "hi":
                assert m32[g] == np.float32(L["up"][g]), what
            if region[7:9] == "lo":
                assert q32[g] == 0.0, what
            if region[7:9] == "hi":
                assert q32[g] == np.float32(L["hi_q"][g]), what
            box = (lo32, L["up"][g], 0.0, hiq32[g])
            k_ref = oracle.fit_kkt(X[g], Y[g], W[g], float(np.float32(L["m"][g])), float(np.float32(L["q"][g])), *box)
            k_got = oracle.fit_kkt(X[g], Y[g], W[g], float(m32[g]), float(q32[g]), *box)
            assert k_got <= k_ref + 2 * rel[g], what + (k_got, k_ref)
            worst_kkt = max(worst_kkt, k_got - k_ref)
        if L["lo"] == -1.0:     # the two-step form of the cell-sharded fits gives the same bits
            mom = ops.fit_weighted_moments(Yd, Xd, wmode, W=Wd)
            m2, q2, r22 = ops.fit_weighted_from_moments(mom, C, lo_gamma=L["lo"], up_gamma=_vec(L["up"]))
            assert _bits_equal(m2.cpu().numpy(), m32) and _bits_equal(q2.cpu().numpy(), q32) and _bits_equal(r22.cpu().numpy(), r2)
    print(f"G={G} C={C} {dtype} wmode={wmode}: largest distance {worst_ulp} float32 ulp, largest KKT excess {worst_kkt:.3g}")


# ----------------------------------------------------------------------------- (b) degenerate genes
def _degenerate_problem():
    """(names, X, Y, W) of ten genes x nine cells.  `line` genes have a minimiser that is a line or the whole box."""
    rng = np.random.default_rng(3)
    C = 9
    base_x, base_y = rng.uniform(0.5, 3.0, C), rng.uniform(0.5, 3.0, C)
    rows = []

    def add(name, x, y, w, line):
        rows.append((name, np.array(x, float), np.array(y, float), np.array(w, float), line))

    add("Sw == 0", base_x, base_y, np.zeros(C), True)
    add("one weighted cell", base_x, base_y, np.eye(C)[4], True)
    w = np.array([1, 0, 2, 0, 1, 0, 0.5, 0, 1.0])
    add("weighted x all equal", np.where(w > 0, 1.5, base_x), base_y, w, True)
    add("weighted Sxx == 0, unweighted > 0", np.where(w > 0, 0.0, base_x), base_y, w, True)
    add("sum w y == 0", base_x, np.where(w > 0, 0.0, base_y), w, False)
    add("x == 0", np.zeros(C), base_y, w, False)
    add("y == 0", base_x, np.zeros(C), w, False)
    add("x == 0 and y == 0", np.zeros(C), np.zeros(C), w, False)
    add("ordinary", base_x, 0.8 * base_x + 0.4 + rng.normal(0, 0.1, C), w, False)
    add("ordinary, w = 1", base_x, np.abs(1.2 * (base_x - 1.0)), np.ones(C), False)
    names, X, Y, W, line = zip(*rows)
    return names, np.array(X), np.array(Y), np.array(W), np.array(line)


def _objective_slack(oracle, x, y, w, m, q, f_ref):
    """f(m32, q32) <= f* + 2 sqrt(f* E) + E, E = sum w (|x| ulp32(m) + ulp32(q))^2: a float32 rounding of a minimiser."""
    e = np.abs(x) * float(_ulp32(m)) + float(_ulp32(q))
    E = float(np.sum(w * e * e))
    return f_ref + 2 * math.sqrt(max(f_ref, 0.0) * E) + E + 1e-28


@pytest.mark.parametrize("dtype", DTYPES)
def test_fit_weighted_degenerate_genes(ops, oracle, dtype):
    """Sw == 0 (the upper q bound is 0/0), one weighted cell, all weighted x equal, weighted Sxx == 0 with unweighted Sxx > 0,
    sum w y == 0 (the q box is the point 0), x == 0 -> NaN, y == 0 -> 0, in the box fit, the unconstrained fit (box_q = 0) and the
    gamma-only fit with q_fixed given and NULL; C = 1 apart.  Every output is written (pre-filled with a sentinel).  Where the
    minimiser is a point the parameters are those of box_wls2_moments fed the kernel's own moments (1 float32 ulp) and of the
    reference; where it is a line the candidates tie in exact arithmetic and rounding picks one, so only feasibility and the
    objective are compared, against fit_box_reference's minimum plus what a float32 rounding of (m, q) can add."""
    names, X, Y, W, line = _degenerate_problem()
    X, Y, W = (fc.stored(a, dtype) for a in (X, Y, W))
    G, C = X.shape
    Yd, Xd, Wd = _cm(ops, Y, dtype), _cm(ops, X, dtype), _cm(ops, W, dtype)
    mom = ops.fit_weighted_moments(Yd, Xd, 0, W=Wd).cpu().numpy()
    assert np.isfinite(mom).all()
    lo, hi = 1e-8, 20.0
    lo32, hi32 = float(np.float32(lo)), 20.0
    m32, q32, r2 = _fit(ops, Yd, Xd, 0, W=Wd)
    for out in (m32, q32, r2):
        assert not np.any(out == SENTINEL)
    for g, name in enumerate(names):
        x, y, w = X[g], Y[g], W[g]
        if not x.any():
            assert np.isnan(m32[g]) and q32[g] == 0 and r2[g] == np.float32(-1e16), name
            continue
        if not y.any():
            assert m32[g] == 0 and q32[g] == 0 and r2[g] == np.float32(-1e16), name        # sstot == 0
            continue
        sw = mom[5, g]
        with np.errstate(all="ignore"):
            hi_q = 2.0 * mom[7, g] / sw
            me, qe = oracle.box_wls2_moments(sw, mom[6, g], mom[7, g], mom[8, g], mom[9, g], lo, hi, 0.0, hi_q)
        assert lo32 <= m32[g] <= hi32 and q32[g] >= 0, name
        if sw > 0:
            assert q32[g] <= np.float32(hi_q), name
        if not line[g]:
            assert _ulps(m32[g], np.float32(me), np.float32) <= 1 and _ulps(q32[g], np.float32(qe), np.float32) <= 1, (name, m32[g], q32[g], me, qe)
            mr, qr, region = oracle.fit_box_reference(x, y, w, lo, hi, 0.0, hi_q)
            assert region != "degenerate", name
            assert _ulps(m32[g], np.float32(mr), np.float32) <= 1 and _ulps(q32[g], np.float32(qr), np.float32) <= 1, (name, m32[g], q32[g], mr, qr)
        if sw > 0:
            mr, qr, region = oracle.fit_box_reference(x, y, w, lo, hi, 0.0, hi_q)
            assert (region == "degenerate") == bool(line[g]), name
            f_ref, f_got = oracle.fit_objective(x, y, w, mr, qr), oracle.fit_objective(x, y, w, float(m32[g]), float(q32[g]))
            assert f_got <= _objective_slack(oracle, x, y, w, m32[g], q32[g], f_ref), (name, f_got, f_ref)
        # R2 is evaluated at the kernel's f64 (m, q): the reference at the float32 pair, plus what their rounding moves
        ref = oracle.r2_reference(float(m32[g]), float(q32[g]), x, y)
        e = np.abs(x) * float(_ulp32(m32[g])) + float(_ulp32(q32[g]))
        ssres, sstot = (1.0 - ref) * np.sum((y - y.mean()) ** 2), np.sum((y - y.mean()) ** 2)
        tol = (2 * math.sqrt(ssres * np.sum(e * e)) + np.sum(e * e)) / sstot + float(_ulp32(ref)) + 4 * fc.FIT_K_R2 * C * EPS * np.sum(y * y) / sstot
        assert abs(float(r2[g]) - ref) <= tol, (name, r2[g], ref, tol)

    # gamma only (fit_offset = 0): q fixed to an array, and to 0 when the pointer is NULL; sum w x^2 == 0 -> lo_gamma
    qf = np.linspace(0.0, 0.9, G)
    for q_fixed in (qf, None):
        qv = np.zeros(G) if q_fixed is None else qf
        m32, q32, r2 = _fit(ops, Yd, Xd, 0, W=Wd, fit_offset=0, lo=0.25, up_gamma=np.full(G, 3.0), q_fixed=q_fixed)
        for out in (m32, q32, r2):
            assert not np.any(out == SENTINEL)
        for g, name in enumerate(names):
            x, y, w = (np.longdouble(a) for a in (X[g], Y[g], W[g]))
            if not X[g].any():
                assert np.isnan(m32[g]) and q32[g] == 0, name
            elif not Y[g].any():
                assert m32[g] == 0 and q32[g] == 0, name
            else:
                sxx = (w * x * x).sum()
                want = float(np.clip((w * x * (y - qv[g])).sum() / sxx, 0.25, 3.0)) if sxx > 0 else 0.25
                assert _ulps(m32[g], np.float32(want), np.float32) <= 1 and q32[g] == np.float32(qv[g]), (name, m32[g], want)
                if want in (0.25, 3.0):
                    assert m32[g] == np.float32(want), name

    # unconstrained with intercept (box_q = 0): ordinary least squares where det > 0, non-finite where it is 0 (as 0/0 is)
    m32, q32, r2 = _fit(ops, Yd, Xd, 0, W=Wd, box_q=0)
    for out in (m32, q32, r2):
        assert not np.any(out == SENTINEL)
    for g, name in enumerate(names):
        if not X[g].any() or not Y[g].any():
            continue
        if line[g]:
            continue                                     # det is 0 or a rounding residue: 0/0, nothing to pin but that it was written
        mr, qr, _ = oracle.fit_box_reference(X[g], Y[g], W[g], -np.inf, np.inf, -np.inf, np.inf)
        assert _ulps(m32[g], np.float32(mr), np.float32) <= 1 and _ulps(q32[g], np.float32(qr), np.float32) <= 1, (name, m32[g], q32[g], mr, qr)

    # C = 1: sstot == 0 -> R2 = -1e16, one cell is a line
    x1, y1 = np.array([[1.5], [0.0], [2.0], [0.0]]), np.array([[2.0], [3.0], [0.0], [0.0]])
    Y1, X1 = _cm(ops, y1, dtype), _cm(ops, x1, dtype)
    m32, q32, r2 = _fit(ops, Y1, X1, 2)
    assert np.all(r2 == np.float32(-1e16))
    assert np.isnan(m32[1]) and np.isnan(m32[3]) and m32[2] == 0 and np.all(q32[1:] == 0)
    assert lo32 <= m32[0] <= 20 and 0 <= q32[0] <= 4 and abs(float(m32[0]) * 1.5 + float(q32[0]) - 2.0) <= 1.5 * float(_ulp32(m32[0])) + float(_ulp32(q32[0]))


# ----------------------------------------------------------------------------- (c) conditioning sweep
@pytest.mark.parametrize("dtype", DTYPES)
def test_fit_weighted_conditioning_sweep(ops, oracle, dtype):
    """x = r + N(0, 1), r = 1, 10, ..., 1e5, C = 257, 40 genes per ratio, planted lines inside the default box.  Per gene
    |m - m_ref|, |q - q_ref| <= 4 K C eps kappa (kappa = Swxx Sw / det, times the size of each quotient), |R2 - R2_ref| <=
    4 K_R2 C eps Syy / sstot, each floored at 1 float32 ulp of the reference's value; the error is measured against
    fit_box_reference / r2_reference.  K = 0.0074 (m, q) and 131 (R2) are the oracle's own f64 expansion against the same
    reference over this sweep (CPU, test_fit_oracle.py); rounded up to 0.0075 and 135 in fit_cases.py."""
    s = fc.sweep(dtype)
    assert set(s["region"]) == {"m_in/q_in"}
    Yd, Xd, Wd = (_cm(ops, s[k], dtype) for k in ("Y", "X", "W"))
    m32, q32, r2 = _fit(ops, Yd, Xd, 0, W=Wd)
    got = np.stack([m32, q32, r2], 1).astype(np.float64)
    bounds = np.stack(fc.sweep_bounds(s, 4 * fc.FIT_K, 4 * fc.FIT_K_R2), 1)
    tol = np.maximum(bounds, _ulp32(s["ref"]))
    err = np.abs(got - s["ref"])
    for r in fc.SWEEP_RATIOS:
        k = s["ratio"] == r
        print(f"{dtype} mean/std {r:g}: err/tol m {np.max(err[k, 0] / tol[k, 0]):.3g} q {np.max(err[k, 1] / tol[k, 1]):.3g} R2 {np.max(err[k, 2] / tol[k, 2]):.3g};"
              f" bound / float32 ulp m {np.max(bounds[k, 0] / _ulp32(s['ref'][k, 0])):.3g} R2 {np.max(bounds[k, 2] / _ulp32(s['ref'][k, 2])):.3g}")
    assert np.all(err <= tol), np.argwhere(err > tol)[:5]


# ----------------------------------------------------------------------------- (d) the weighted-moments kernel
def _ld_moments(X, Y, W):
    L = np.longdouble
    x, y, w = L(X), L(Y), L(W)
    terms = (x, y, x * x, x * y, y * y, w, w * x, w * y, w * x * x, w * x * y)
    return np.stack([t.sum(1) for t in terms]), np.stack([np.abs(t).sum(1) for t in terms])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G", [1, 64, 257])
@pytest.mark.parametrize("C", [1, 2, 31, 32, 33, 65, 1025])
def test_weighted_moments_against_long_double_sums(ops, C, G, dtype):
    """The (10, G) f64 moments of vcy_fit_weighted_moments in the three weight modes against long-double sums of the stored
    values, |got - ref| <= C eps sum|term|.  C < 32 and C = 65 leave trailing cell blocks empty, 1025 gives a short last one;
    the padding columns of every input hold NaN; the workspace is NaN-filled before the launch."""
    rng = np.random.default_rng(100 * C + G)
    X = rng.gamma(2.0, 1.0, (G, C)) * (rng.random((G, C)) < 0.8)
    Y = rng.gamma(1.0, 1.0, (G, C)) * (rng.random((G, C)) < 0.7)
    W = rng.choice([0.0, 0.5, 1.0, 2.0], (G, C))
    Xd, Yd, Wd = _cm(ops, X, dtype), _cm(ops, Y, dtype), _cm(ops, W, dtype)
    Xs, Ys, Ws = fc.stored(X, dtype), fc.stored(Y, dtype), fc.stored(W, dtype)
    down, up = np.percentile(Xs, [2, 98], axis=1)
    w1 = ((Xs <= down[:, None]) | (Xs >= up[:, None])).astype(np.float64)
    for wmode, w in ((0, Ws), (1, w1), (2, np.ones((G, C)))):
        ops._fit_workspace(G, Xd.t.device).fill_(255)       # all-ones bytes: NaN in every partial
        mom = ops.fit_weighted_moments(Yd, Xd, wmode, W=Wd if wmode == 0 else None, M=Xd if wmode == 1 else None,
                                       down=_vec(down) if wmode == 1 else None, up=_vec(up) if wmode == 1 else None).cpu().numpy()
        ref, mag = _ld_moments(Xs, Ys, w)
        assert np.all(np.abs(mom - ref) <= C * EPS * mag), (wmode, np.max(np.abs(mom - ref) / np.maximum(C * EPS * mag, 1e-300)))
        if wmode != 0:
            assert np.array_equal(mom[5], w.sum(1))          # a count


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_weighted_moments_mode1_ties_at_the_thresholds(ops, dtype, two):
    """Weight mode 1 with thresholds that are data values: C = 101 puts the 2nd and 98th percentiles on order statistics 2 and 98
    (taken from ops.gene_quantiles), so z == down and z == up decide weights; integer-valued data repeat them.  With and without
    M2 / scales (Z = M / a + M2 / b evaluated in the storage type, as numpy does here).  Sw is the numpy count exactly."""
    rng = np.random.default_rng(11 + two)
    G, C = 70, 101
    t = NP_T[dtype]
    S = rng.integers(0, 6, (G, C)).astype(np.float64)
    U = rng.integers(0, 4, (G, C)).astype(np.float64)
    S[0] = 0
    S[1, 1:] = 0
    X, Y = rng.gamma(2.0, 1.0, (G, C)), rng.gamma(1.0, 1.0, (G, C))
    Sd, Ud, Xd, Yd = (_cm(ops, a, dtype) for a in (S, U, X, Y))
    sa, sb = np.where(np.arange(G) % 2, 4.0, rng.uniform(0.5, 3.0, G)), np.where(np.arange(G) % 3, 2.0, rng.uniform(0.5, 3.0, G))
    if two:
        Z = (S.astype(t) / sa.astype(t)[:, None] + U.astype(t) / sb.astype(t)[:, None]).astype(np.float64)
        qs = ops.gene_quantiles(Sd, [2, 98], M2=Ud, scale_a=_vec(sa), scale_b=_vec(sb))
    else:
        Z = S
        qs = ops.gene_quantiles(Sd, [2, 98])
    down, up = qs.cpu().numpy()
    srt = np.sort(Z, axis=1)
    assert np.array_equal(down, srt[:, 2]) and np.array_equal(up, srt[:, 98])           # thresholds ARE data values
    w = ((Z <= down[:, None]) | (Z >= up[:, None])).astype(np.float64)
    assert (w.sum(1) > 6).mean() > 0.5                                                 # ... and tied ones: more than the 3 + 3 cells outside
    mom = ops.fit_weighted_moments(Yd, Xd, 1, M=Sd, M2=Ud if two else None, scale_a=_vec(sa) if two else None,
                                   scale_b=_vec(sb) if two else None, down=qs[0].contiguous(), up=qs[1].contiguous()).cpu().numpy()
    assert np.array_equal(mom[5], w.sum(1))
    ref, mag = _ld_moments(fc.stored(X, dtype), fc.stored(Y, dtype), w)
    assert np.all(np.abs(mom - ref) <= C * EPS * mag)


# ----------------------------------------------------------------------------- (e) vcy_gamma_weights
def _gamma_weights(ops, S, U, mode, pa, pb, pc=None, pd=None, sa=None, sb=None, power=15.0):
    W = _filled(ops, S)
    keep = [_vec(v) for v in (pa, pb, pc, pd, sa, sb)]
    ops._lib.check(ops._lib.lib().vcy_gamma_weights(S.t.data_ptr(), _ptr(U), W.t.data_ptr(), *[_ptr(k) for k in keep], S.C, S.G, S.ld, int(mode),
                                                    float(power), S.code, ops._stream()), "gamma_weights")
    if S.ld > S.G:
        assert float(W.t[:, S.G:].abs().max()) == 0.0          # padding columns are written, as 0 (NaN would fail this)
    return W.to_genes_major()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [7, 300])
@pytest.mark.parametrize("G", [5, 64, 130])
def test_gamma_weights_against_the_oracle(ops, oracle, G, C, dtype):
    """Modes 0-3 (sum, prod, maxmin_weighted, maxmin_double) against oracle.gamma_weights on the stored values, thresholds by
    np.percentile as the oracle takes them.  Small-integer data put ties on every threshold of modes 2 and 3; gene 0 is all
    zero and gene 1 has one non-zero cell (> 98 % zeros at C = 300), so their 2nd and 98th percentiles coincide: the reference's
    0/0 row of NaN must be NaN here.  f64: rtol 1e-14; f32: 2 float32 ulps of the f64 value; the indicator weights of mode 3
    exactly (f32: Z evaluated in float32, as the quantile kernel sees it)."""
    rng = np.random.default_rng(G * 1000 + C)
    t = NP_T[dtype]
    S = rng.integers(0, 5, (G, C)).astype(np.float64) * 0.75
    U = rng.integers(0, 4, (G, C)).astype(np.float64) * 0.5
    S[0] = 0
    S[1] = 0
    S[1, C // 2] = 3.0
    Sd, Ud = _cm(ops, S, dtype), _cm(ops, U, dtype)
    Ss, Us = fc.stored(S, dtype), fc.stored(U, dtype)

    def check(got, ref):
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        if dtype == "float64":
            with np.errstate(invalid="ignore"):
                bad = ~(np.isnan(ref) | (got == ref) | (np.abs(got - ref) <= 1e-14 * np.abs(ref)))
            assert not bad.any(), (got[bad][:4], ref[bad][:4])
        else:
            assert np.all(_ulps(got, ref, np.float32) <= 2), np.max(_ulps(got, ref, np.float32))

    with np.errstate(all="ignore"):
        p99S, p99U = np.percentile(Ss, 99, 1), np.percentile(Us, 99, 1)
        check(_gamma_weights(ops, Sd, Ud, 0, p99S, p99U), oracle.gamma_weights(Ss, Us, Ss, Us, "sum"))
        check(_gamma_weights(ops, Sd, Ud, 1, p99S, p99U), oracle.gamma_weights(Ss, Us, Ss, Us, "prod"))
        down, up = np.percentile(Ss, [2, 98], 1)
        assert down[0] == up[0] and np.any(Ss == down[:, None]) and np.any(Ss == up[:, None])
        ref = oracle.gamma_weights(Ss, Us, Ss, Us, "maxmin_weighted")
        assert np.isnan(ref[0]).all() and (C < 300 or (down[1] == up[1] and np.isnan(ref[1]).all()))
        check(_gamma_weights(ops, Sd, None, 2, down, up), ref)
        # mode 3: Z = S / dS + U / dU with the oracle's denominators; thresholds of Z and of S
        dS, dU = np.percentile(Ss, 99.9, 1), np.percentile(Us, 99.9, 1)
        dS[dS == 0] = np.maximum(Ss[dS == 0].max(1), 0.001)
        dU[dU == 0] = np.maximum(Us[dU == 0].max(1), 0.001)
        Z = (Ss.astype(t) / dS.astype(t)[:, None] + Us.astype(t) / dU.astype(t)[:, None]).astype(np.float64)
        zd, zu = np.percentile(Z, [2, 98], 1)
        ref = ((Z <= zd[:, None]) | (Z >= zu[:, None])).astype(float) + ((Ss <= down[:, None]) | (Ss >= up[:, None])).astype(float)
        if dtype == "float64":
            assert np.array_equal(ref, oracle.gamma_weights(Ss, Us, Ss, Us, "maxmin_double"))
        assert np.any(Z == zd[:, None]) and np.any(Z == zu[:, None])
        got = _gamma_weights(ops, Sd, Ud, 3, zd, zu, down, up, dS, dU)
        assert np.array_equal(got, ref)


# ----------------------------------------------------------------------------- (f) element-wise chain stages
ELEMENT_SHAPES = [(1, 1), (3, 2), (65, 9), (257, 70)]


def _lincomb(ops, x, y, a, b, zero_below=None, clip=False):
    out = _filled(ops, x)
    zb = _vec(zero_below)
    ops._lib.check(ops._lib.lib().vcy_lincomb(x.t.data_ptr(), _ptr(y), out.t.data_ptr(), float(a), float(b), _ptr(zb), int(clip), x.C, x.G, x.ld,
                                              x.code, ops._stream()), "lincomb")
    if x.ld > x.G:
        assert float(out.t[:, x.G:].abs().max()) == 0.0
    return out.to_genes_major(NP_T[str(x.dtype).split(".")[1]])


@pytest.mark.parametrize("dtype", DTYPES)
def test_lincomb_rounds_both_products(ops, dtype):
    """a x + b y with a = -1, x = 1 + 2^-29, b = y = 1 + 2^-30 (f32: 2^-12, 2^-13): b y rounds to x, the sum is exactly 0; a
    contracted fma keeps the 2^-60 (2^-26).  The mirrored operands catch a contraction of the other product."""
    e = 2.0 ** -29 if dtype == "float64" else 2.0 ** -12
    G, C = 65, 9
    big, small = np.full((G, C), 1 + e), np.full((G, C), 1 + e / 2)
    assert NP_T[dtype](1 + e / 2) * NP_T[dtype](1 + e / 2) == NP_T[dtype](1 + e)
    assert np.all(_lincomb(ops, _cm(ops, big, dtype), _cm(ops, small, dtype), -1.0, 1 + e / 2) == 0)
    assert np.all(_lincomb(ops, _cm(ops, small, dtype), _cm(ops, big, dtype), 1 + e / 2, -1.0) == 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,C", ELEMENT_SHAPES)
def test_lincomb_against_numpy_bit_for_bit(ops, G, C, dtype):
    """y given and NULL, the strict `<` of zero_below (an entry whose |out| equals the threshold is kept, the next double above
    zeroes it), clip: the same bits as numpy's two-rounding evaluation in the storage type."""
    rng = np.random.default_rng(G + C)
    t = NP_T[dtype]
    x, y = rng.normal(size=(G, C)), rng.normal(size=(G, C))
    xd, yd = _cm(ops, x, dtype), _cm(ops, y, dtype)
    xs, ys = x.astype(t), y.astype(t)
    a, b = 0.7, -1.3
    plain = t(a) * xs + t(b) * ys
    assert _bits_equal(_lincomb(ops, xd, yd, a, b), plain)
    assert _bits_equal(_lincomb(ops, xd, None, a, 0.0), t(a) * xs)
    assert _bits_equal(_lincomb(ops, xd, yd, a, b, clip=True), np.maximum(plain, t(0)) + t(0))
    thr = np.abs(plain[:, C // 2]).astype(np.float64)                  # |out| of one entry per gene: a tie
    thr[1::2] = np.nextafter(thr[1::2], np.inf)
    for clip in (False, True):
        ref = plain.copy()
        ref[np.abs(ref).astype(np.float64) < thr[:, None]] = 0
        assert np.all(ref[0::2, C // 2] == plain[0::2, C // 2]) and np.all(ref[1::2, C // 2] == 0)
        if clip:
            ref = np.maximum(ref, t(0)) + t(0)
        assert _bits_equal(_lincomb(ops, xd, yd, a, b, zero_below=thr, clip=clip) + t(0), ref + t(0))


def _scale_log(ops, M, factor, want_sz, want_norm, pcount, fix):
    sz, nm = (_filled(ops, M) if want_sz else None), (_filled(ops, M) if want_norm else None)
    f = _vec(factor)
    ops._lib.check(ops._lib.lib().vcy_scale_log(M.t.data_ptr(), _ptr(f), _ptr(sz), _ptr(nm), M.C, M.G, M.ld, float(pcount), int(fix), M.code,
                                                ops._stream()), "scale_log")
    for o in (sz, nm):
        if o is not None and M.ld > M.G:
            assert float(o.t[:, M.G:].abs().max()) == 0.0
    return (None if sz is None else sz.to_genes_major()), (None if nm is None else nm.to_genes_major())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,C", ELEMENT_SHAPES)
def test_scale_log(ops, G, C, dtype):
    """factor[c] * M and log2(factor[c] * M + pcount): factor = inf on a cell of zeros (0 * inf = NaN -> 0 with fix_nonfinite,
    NaN without), factor = inf on counts, factor NULL, each output alone.  The scaled value is the product rounded once to the
    storage type; log2 within 2 ulps in f64, 1 float32 ulp of the f64 value in f32."""
    rng = np.random.default_rng(G * 7 + C)
    t = NP_T[dtype]
    M = rng.gamma(2.0, 1.0, (G, C)) * (rng.random((G, C)) < 0.7)
    M[:, 0] = 0
    factor = rng.gamma(8.0, 0.125, C)
    factor[0] = np.inf
    if C > 1:
        factor[C - 1] = np.inf
        M[0, C - 1] = 1.0
    Md = _cm(ops, M, dtype)
    Ms = fc.stored(M, dtype)
    for fac in (factor, None):
        for fix in (False, True):
            with np.errstate(all="ignore"):
                x = Ms * (1.0 if fac is None else fac[None, :])
                if fix:
                    x[~np.isfinite(x)] = 0
                want_sz, want_nm = x.astype(t).astype(np.float64), np.log2(x + 1.0)
            if fac is not None:
                assert np.all(want_sz[:, 0] == 0) if fix else np.isnan(want_sz[:, 0]).all()
            for ws, wn in ((True, True), (True, False), (False, True)):
                sz, nm = _scale_log(ops, Md, fac, ws, wn, 1.0, fix)
                if ws:
                    assert np.array_equal(sz, want_sz, equal_nan=True)
                if wn:
                    assert np.all(_ulps(nm, want_nm, t) <= (2 if dtype == "float64" else 1)), np.max(_ulps(nm, want_nm, t))


def _delta_transform(ops, hi, dS, dt, mode, psc):
    dm = _filled(ops, hi)
    eo = _filled(ops, hi) if mode == 3 else None
    ops._lib.check(ops._lib.lib().vcy_delta_transform(hi.t.data_ptr(), dS.t.data_ptr(), dm.t.data_ptr(), _ptr(eo), hi.C, hi.G, hi.ld, float(dt),
                                                      int(mode), float(psc), hi.code, ops._stream()), "delta_transform")
    for o in (dm, eo):
        if o is not None and hi.ld > hi.G:
            assert float(o.t[:, hi.G:].abs().max()) == 0.0
    return dm.to_genes_major(), (None if eo is None else eo.to_genes_major())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,C", ELEMENT_SHAPES)
def test_delta_transform(ops, oracle, G, C, dtype):
    """All four modes against oracle.delta_transform, D = (hi + dt dS) - hi formed in the storage type (numpy's + - * are the kernel's), with
    delta_S of both signs, exact zeros (D == 0) and entries with hi + dt dS < 0.  dt = 1 and 0.5 make dt * dS exact, so D is
    numpy's bit for bit whether or not the compiler fuses hi + dt * dS: linear exact; sqrt / log10 of that D, evaluated in f64,
    within 2 ulps (f64) or 1 float32 ulp (f32), and NaN exactly where numpy's sign(0) * log10(0) is (psc = 0).  dt = 0.7, linear:
    a fused multiply-add may move hi_t by one rounding, so |D - D_numpy| <= 1 ulp of hi_t + 1 ulp of D.  logratio (numpy in the storage type): e within 2 ulps, dmat within 2 ulps of each of its two
    logarithms plus one of itself."""
    rng = np.random.default_rng(G * 3 + C)
    t = NP_T[dtype]
    hi = (rng.gamma(2.0, 1.0, (G, C)) * (rng.random((G, C)) < 0.8)).astype(t)
    dS = (rng.normal(0, 1.5, (G, C)) * (rng.random((G, C)) < 0.8)).astype(t)
    hd, dd = _cm(ops, hi, dtype), _cm(ops, dS, dtype)
    neg = 0
    with np.errstate(all="ignore"):
        for dt in (1.0, 0.5):
            hi_t = hi + t(dt) * dS
            neg += int((hi_t < 0).sum())
            assert hi_t.dtype == t
            D = (hi_t - hi).astype(np.float64)              # numpy's D in the storage type; the transform of it in f64
            for mode, name, psc in ((0, "linear", 0.0), (1, "sqrt", 1e-10), (1, "sqrt", 0.0), (2, "log", 1.0), (2, "log", 0.0)):
                ref = oracle.delta_transform(np.zeros_like(D), D, name, float(t(psc)))
                got, _ = _delta_transform(ops, hd, dd, dt, mode, psc)
                assert np.array_equal(np.isnan(got), np.isnan(ref)), (dt, name, psc)
                assert np.all(_ulps(got, ref, t) <= (0 if mode == 0 else (2 if dtype == "float64" else 1))), (dt, name, psc, np.max(_ulps(got, ref, t)))
                if mode == 2 and psc == 0.0:
                    assert np.isnan(ref[D == 0]).all() and ((D == 0).any() or G * C < 100)
            l1, l2 = np.log2(np.abs(hi_t) + t(0.5)), np.log2(hi + t(0.5))
            got, e = _delta_transform(ops, hd, dd, dt, 3, 0.5)
            assert np.all(_ulps(e, l2, t) <= 2)
            sp = lambda v: np.spacing(np.abs(v)).astype(np.float64)
            assert np.all(np.abs(got - (l1 - l2).astype(np.float64)) <= 2 * (sp(l1) + sp(l2)) + sp(l1 - l2))
        hi_t = hi + t(0.7) * dS
        got, _ = _delta_transform(ops, hd, dd, 0.7, 0, 0.0)
        assert np.all(np.abs(got - (hi_t - hi).astype(np.float64)) <= (np.spacing(np.abs(hi_t)) + np.spacing(np.abs(hi_t - hi))).astype(np.float64))
    if G * C > 100:
        assert neg > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,C", ELEMENT_SHAPES)
def test_velocity_chain_edges(ops, oracle, G, C, dtype):
    """Dyadic inputs (eighths, gamma and q powers of two) make every product of the chain exact, so the kernel must give numpy's
    bits however it fuses: eps_thr with |velocity| exactly on the threshold (kept: strict <) and one double above it (zeroed),
    clip on and off, q NULL.  assumption = 1 with gamma == 0 on random data: non-finite exactly where numpy's is."""
    rng = np.random.default_rng(G * 5 + C)
    t = NP_T[dtype]
    S = rng.integers(0, 64, (G, C)) / 8.0
    U = rng.integers(0, 64, (G, C)) / 8.0
    gam = rng.choice([0.25, 0.5, 1.0, 2.0], G).astype(np.float32)
    q = rng.choice([0.0, 0.125, 0.5], G).astype(np.float32)
    Sd, Ud = _cm(ops, S, dtype), _cm(ops, U, dtype)
    names = ("Upred", "velocity", "delta_S", "Sx_sz_t", "dmat")
    for qq in (q, None):
        Upred = gam[:, None] * S + (0 if qq is None else qq[:, None])
        vel0 = U - Upred
        thr = np.abs(vel0[:, C // 2]).astype(np.float64)
        thr[1::2] = np.nextafter(thr[1::2], np.inf)
        for clip in (True, False):
            vel = vel0.copy()
            vel[np.abs(vel) < thr[:, None]] = 0
            dSr = 0.5 * vel
            St = S + 2.0 * dSr
            if clip:
                St = np.clip(St, 0, None)
            out = ops.velocity_chain(Sd, Ud, torch.from_numpy(gam), None if qq is None else torch.from_numpy(qq), want=names, eps_thr=_vec(thr),
                                     dt_shift=0.5, dt_extrap=2.0, used_dt=1.0, clip=clip, transform=ops.LINEAR, psc=0.0)
            for name, ref in zip(names, (Upred, vel, dSr, St, dSr)):
                got = out[name].to_genes_major()
                assert np.array_equal(got, ref.astype(t).astype(np.float64)), (name, clip, qq is None)
                assert np.array_equal(ref.astype(t).astype(np.float64), ref)                   # ... which are exact in the storage type
            got = out["velocity"].to_genes_major()
            assert np.all(got[0::2, C // 2] == vel0[0::2, C // 2]) and np.all(got[1::2, C // 2] == 0)
            if not clip and G * C > 100:
                assert (out["Sx_sz_t"].to_genes_major() < 0).any()
    # constant_unspliced with gamma == 0
    S = rng.gamma(2.0, 1.0, (G, C)) * (rng.random((G, C)) < 0.8)
    U = rng.gamma(1.0, 1.0, (G, C)) * (rng.random((G, C)) < 0.7)
    gam = rng.uniform(0.05, 2.0, G).astype(np.float32)
    gam[0::3] = 0
    Sd, Ud = _cm(ops, S, dtype), _cm(ops, U, dtype)
    out = ops.velocity_chain(Sd, Ud, torch.from_numpy(gam), torch.from_numpy(q), want=("delta_S",), dt_shift=0.7, assumption=1)
    _, _, ref, _ = oracle.velocity_chain(fc.stored(S, dtype), fc.stored(U, dtype), gam, q, delta_t_shift=0.7, assumption="constant_unspliced")
    got = out["delta_S"].to_genes_major()
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)) and not np.isfinite(ref[0]).any()
    ok = np.isfinite(ref)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-5 if dtype == "float64" else 2e-4, atol=1e-5 if dtype == "float64" else 1e-4)
