"""AtlasPath(fit="maxmin_diag", weighted=, weights=, maxmin_perc=, maxmin_weighted_pow=): every fit_gammas weight mode on the atlas path.

Bars (those of tests/test_gpu_atlas_fit_options.py, restated here).  One block: thresholds, moments, gamma, q, R2 BIT-IDENTICAL to
streamed_fit.StreamedFit fed the path's resident matrices as one block (which tests/test_gpu_streamed_fit.py ties to the resident
recipe and to VelocytoLoom.fit_gammas), corr to the fused stage C + D launch on them.  block_cells 500 and 401 against one block:
every percentile bit-identical; moments within 2 n 2^-53 relative where finite, non-finite in the same places; gamma, q, R2 within
the larger of one float32 ulp and the gene's 4 K n eps kappa (oracle.fit_condition on the gene's data and its actual weights);
corr finite in the same places and within 2e-6 (f32) / 1e-12 (f64)."""
import numpy as np
import pytest

import fit_cases as fc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C, G, K, NN = 1200, 200, 10, 60
NP_T = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = (torch.float32, torch.float64)
MODES = {"sum": dict(weights="sum"), "prod": dict(weights="prod", limit_gamma=True), "maxmin": dict(weights="maxmin", maxmin_perc=(5, 90)),
         "maxmin_weighted": dict(weights="maxmin_weighted", maxmin_weighted_pow=2.5), "maxmin_double": dict(weights="maxmin_double"),
         "maxmin_diag, other percentiles": dict(maxmin_perc=(10, 95)),
         "unweighted": dict(weighted=False), "unweighted, fixperc_q": dict(weighted=False, fit_offset=False, fixperc_q=True),
         "unweighted, no offset": dict(weighted=False, fit_offset=False)}


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


@pytest.fixture(scope="module")
def data(ops):
    from velocyto_amd import atlas
    dev = ops.require_gpu()
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(C, G, K, dev, density=0.08)
    fS, fU = atlas.size_factors(totS, totU, C)
    return cS, cU, fS, fU, pcs, emb


def _path(data, **kw):
    from velocyto_amd import atlas
    return atlas.AtlasPath(*data, k=K, n_neighbors=NN, sampled_fraction=0.5, **kw)


def _snapshot(p, corr):
    return dict(th={n: v.clone() for n, v in p.fit_thresholds.items()}, gamma=p.gamma.clone(), q=p.q.clone(), R2=p.R2.clone(), mom=p.fit_moments.clone(),
                corr=corr.clone(), neigh=p.neigh.clone(), n=p.n_fit_cells, rules=p.rules, state=p.select_state_bytes)


@pytest.fixture(scope="module")
def one(ops, data):
    """The one-block runs of every mode, both dtypes, and the pooled matrices: computed once, never modified."""
    out = {}
    for dt in DTYPES:
        for name, kw in (("default", {}), *MODES.items()):
            p = _path(data, block_cells=0, dtype=dt, fit="maxmin_diag", **kw)
            out[dt, name] = _snapshot(p, p.run())
        e_buf, u_buf = p._resident
        out[dt, "Sx"], out[dt, "Ux"] = ops.CellMatrix(e_buf.t[:C].clone(), G), ops.CellMatrix(u_buf.t[:C].clone(), G)
    return out


def _bits(t):
    t = t.contiguous()
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _same(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    eq = _bits(a) == _bits(b)
    return bool((eq | (torch.isnan(a) & torch.isnan(b)) if a.is_floating_point() else eq).all())


def _streamed(ops, Sx, Ux, kw):
    from velocyto_amd.streamed_fit import StreamedFit
    fit = StreamedFit(G, C, Sx.dtype, Sx.t.device, **kw)
    for _ in range(fit.n_walks):
        fit.add_block(Sx, Ux)
        fit.end_walk()
    return fit, fit.result()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(MODES))
def test_one_block_equals_streamed_fit_on_the_resident_matrices(ops, one, dt, name):
    o, Sx, Ux = one[dt, name], one[dt, "Sx"], one[dt, "Ux"]
    fit, (g, q, R2) = _streamed(ops, Sx, Ux, MODES[name])
    assert set(o["th"]) == set(fit.thresholds)
    for n, v in fit.thresholds.items():
        assert _same(o["th"][n], v), n
    for n, ref in (("gamma", g), ("q", q), ("R2", R2), ("mom", fit.moments)):
        assert _same(o[n], ref), n
    assert o["state"] == fit.state_bytes and o["n"] == C
    corr = ops.coldeltacor_partial_fused(Sx, Ux, g, q, o["neigh"], ops.SQRT, o["rules"], 1e-10, validate=False)
    assert torch.equal(torch.nan_to_num(o["corr"], nan=7.0), torch.nan_to_num(corr, nan=7.0))
    d = one[dt, "default"]
    assert not _same(o["gamma"], d["gamma"]), "the mode is not a no-op on this data"
    expect = {"sum": {"p99_S", "p99_U"}, "prod": {"p99_S", "p99_U", "med_S", "p90_S", "med_U", "U_p10_above", "S_med_above", "n_above", "up_gamma"},
              "maxmin": {"down_S", "up_S"}, "maxmin_weighted": {"down_S", "up_S"},
              "maxmin_double": {"denom_S", "denom_U", "down", "up", "down_S", "up_S"}, "maxmin_diag, other percentiles": {"denom_S", "denom_U", "down", "up"},
              "unweighted": set(), "unweighted, fixperc_q": {"p1_S", "n_below", "q_fixed"}, "unweighted, no offset": set()}
    assert set(o["th"]) == expect[name]


def test_the_default_keywords_are_the_default_run(ops, data, one):
    """weighted=True, weights="maxmin_diag", maxmin_perc=(2, 98), maxmin_weighted_pow=15 spelled out: today's bits."""
    for dt in DTYPES:
        p = _path(data, block_cells=0, dtype=dt, fit="default", weighted=True, weights="maxmin_diag", maxmin_perc=[2, 98], maxmin_weighted_pow=15)
        got, o = _snapshot(p, p.run()), one[dt, "default"]
        assert set(got["th"]) == set(o["th"]) == {"denom_S", "denom_U", "down", "up"}
        for n in got["th"]:
            assert _same(got["th"][n], o["th"][n]), n
        for n in ("gamma", "q", "R2", "mom", "corr"):
            assert _same(got[n], o[n]), n
        assert got["state"] == o["state"]
    _path(data, block_cells=0, fit="slope", weighted=True, weights="maxmin_diag", maxmin_perc=(2, 98), maxmin_weighted_pow=15)      # the defaults are fine


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


def _weights_of(ops, Sx, Ux, th, kw):
    """The (C, G) weights the mode gives every element, from the run's own thresholds (float64 numpy)."""
    if not kw.get("weighted", True):
        return np.ones((C, G))
    w = kw.get("weights", "maxmin_diag")
    if w in ("sum", "prod"):
        return ops.gamma_weights(Sx, Ux, 0 if w == "sum" else 1, th["p99_S"], th["p99_U"]).t[:, :G].double().cpu().numpy()
    if w == "maxmin_weighted":
        return ops.gamma_weights(Sx, None, 2, th["down_S"], th["up_S"], power=kw.get("maxmin_weighted_pow", 15)).t[:, :G].double().cpu().numpy()
    if w == "maxmin_double":
        return ops.gamma_weights(Sx, Ux, 3, th["down"], th["up"], th["down_S"], th["up_S"], th["denom_S"], th["denom_U"]).t[:, :G].double().cpu().numpy()
    t = NP_T[Sx.dtype]
    S, U = Sx.t[:, :G].cpu().numpy(), Ux.t[:, :G].cpu().numpy()
    with np.errstate(all="ignore"):
        if w == "maxmin":
            Z, dn, up = S.astype(np.float64), th["down_S"], th["up_S"]
        else:
            Z = (S / th["denom_S"].cpu().numpy().astype(t)[None, :] + U / th["denom_U"].cpu().numpy().astype(t)[None, :]).astype(np.float64)
            dn, up = th["down"], th["up"]
        return ((Z <= dn.cpu().numpy()[None, :]) | (Z >= up.cpu().numpy()[None, :])).astype(np.float64)


@pytest.fixture(scope="module")
def bounds(ops, oracle, one):
    out = {}
    for dt in DTYPES:
        Sx, Ux = one[dt, "Sx"], one[dt, "Ux"]
        Sn, Un = Sx.to_cells_major(NP_T[dt]), Ux.to_cells_major(NP_T[dt])
        for name, kw in MODES.items():
            W = _weights_of(ops, Sx, Ux, one[dt, name]["th"], kw)
            with np.errstate(all="ignore"):
                cond = np.array([oracle.fit_condition(Sn[:, g], Un[:, g], W[:, g]) for g in range(G)])
            kf, kr, sm, sq = cond.T
            u = 4 * C * fc.EPS
            out[dt, name] = fc.FIT_K * u * kf * sm, fc.FIT_K * u * kf * sq, fc.FIT_K_R2 * u * kr
    return out


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(MODES))
@pytest.mark.parametrize("block_cells", [500, 401])
def test_blocked_runs_equal_the_one_block_run(ops, data, one, bounds, dt, name, block_cells):
    p = _path(data, block_cells=block_cells, dtype=dt, fit="maxmin_diag", **MODES[name])
    assert len(p.blocks()) == 3 and p.blocks()[-1][1] == C
    got, o = _snapshot(p, p.run()), one[dt, name]
    what = f"{name}, blocks of {block_cells}, {dt}"
    assert set(got["th"]) == set(o["th"]) and got["n"] == o["n"] and got["state"] == o["state"]
    for n, v in o["th"].items():
        assert _same(got["th"][n], v), f"{what}: {n} differs from the one-block run"
    m1, m2 = o["mom"].cpu().numpy(), got["mom"].cpu().numpy()
    fin = np.isfinite(m1)
    assert np.array_equal(np.isfinite(m2), fin) and np.array_equal(np.isnan(m2), np.isnan(m1))
    assert (m1[fin] >= 0).all() and (m2[fin] >= 0).all()
    rel = np.abs(m2[fin] - m1[fin]) / np.where(m1[fin] > 0, m1[fin], 1.0)
    print(f"{what}: largest relative difference of a moment {rel.max():.3g} (bar {2 * C * 2.0 ** -53:.3g})")
    assert rel.max() <= 2 * C * 2.0 ** -53
    for n, b in zip(("gamma", "q", "R2"), bounds[dt, name]):
        a1, a2 = o[n].cpu().numpy().astype(np.float64), got[n].cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isfinite(a1), np.isfinite(a2))
        tol = np.fmax(_ulp32(a1), np.where(np.isnan(b), 0.0, b))
        same = (a1 == a2) | (np.isnan(a1) & np.isnan(a2))
        err = np.where(same, 0.0, np.abs(a2 - a1))
        worst = int(np.argmax(err / tol))
        print(f"{what}: {n}: {int((~same).sum())} genes differ, worst {err[worst]:.3g} against {tol[worst]:.3g} (gene {worst})")
        assert np.all(err <= tol), (what, n, worst, a1[worst], a2[worst], tol[worst])
    c1, c2 = o["corr"].cpu().numpy(), got["corr"].cpu().numpy()
    fin = np.isfinite(c1)
    assert np.array_equal(np.isfinite(c2), fin)
    d = float(np.abs(c2[fin] - c1[fin]).max())
    print(f"{what}: max |dcorr| {d:.3g}")
    assert d <= (2e-6 if dt == torch.float32 else 1e-12)


def test_bad_arguments_are_refused(ops, data):
    for kw in (dict(weighted=False), dict(weights="sum"), dict(maxmin_perc=(5, 95)), dict(maxmin_weighted_pow=2)):
        for fit in ({}, dict(fit="slope")):
            with pytest.raises(ValueError, match="belong to fit=\"maxmin_diag\""):
                _path(data, block_cells=0, **fit, **kw)
    for bad in ("maxmin_diagonal", "slope", None):
        with pytest.raises(ValueError, match="is not supported"):
            _path(data, block_cells=0, fit="maxmin_diag", weights=bad)
    with pytest.raises(ValueError, match="never sees a whole"):
        _path(data, block_cells=0, fit="maxmin_diag", weights=np.ones((G, C)))
    for fit in ("maxmin", "sum", "maxmin_double"):                        # the weight mode never travels in fit=
        with pytest.raises(ValueError, match="unknown fit"):
            _path(data, block_cells=0, fit=fit)
