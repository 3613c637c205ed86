"""streamed_fit.StreamedFit on the pooled matrices of the synthetic atlas: every fit_gammas weight mode and option.

Bars (those of tests/test_gpu_atlas_fit_options.py, restated here).  One block: thresholds, moments, gamma, q, R2 BIT-IDENTICAL to
the resident recipe - ops.gene_quantiles / ops.gamma_weights / ops.fit_weighted called with VelocytoLoom.fit_gammas' arguments on
the same matrices, the steady-state rows gathered as the facade gathers them - and to VelocytoLoom.fit_gammas itself.  (Every other
cell of 1200 as the steady state: the masked fold's 32 cell blocks of 38 cells keep 19 each, the gathered matrix's 32 blocks hold
those same 19, so the two sums run in the same order and the bits agree.)  Several blocks against one block: every percentile and
population bit-identical (integer counts); the (10, G) moments within 2 n 2^-53 relative where finite (non-negative terms, two
summation orders, n cells), non-finite in the same places; gamma, q, R2 within the larger of one float32 ulp and the gene's bound
4 K n eps kappa (oracle.fit_condition on the gene's data and its actual weights).  The sparse "prod" weights leave a few genes with
kappa_fit = inf (singular weighted normal equations: no bound for gamma and q, while R2, evaluated at them, keeps its own); the test
prints how many."""
import numpy as np
import pytest

import fit_cases as fc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C, G, K, NN = 1200, 200, 10, 60
NP_T = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = (torch.float32, torch.float64)
WEIGHTS = ("sum", "prod", "maxmin", "maxmin_weighted", "maxmin_diag", "maxmin_double", None)          # None: weighted=False
BRANCHES = {"box": dict(), "fixperc_q": dict(fit_offset=False, fixperc_q=True), "no offset": dict(fit_offset=False)}
HALF = np.arange(C) % 2 == 0
PERC, POWER = (2, 98), 15


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


@pytest.fixture(scope="module")
def pooled(ops):
    """The pooled matrices (Sx, Ux) of the synthetic atlas in both dtypes, from a resident AtlasPath run; never modified."""
    from velocyto_amd import atlas
    dev = ops.require_gpu()
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(C, G, K, dev, density=0.08)
    fS, fU = atlas.size_factors(totS, totU, C)
    out = {}
    for dt in DTYPES:
        p = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, k=K, n_neighbors=NN, sampled_fraction=0.5, block_cells=0, dtype=dt)
        p.run()
        e_buf, u_buf = p._resident
        out[dt] = ops.CellMatrix(e_buf.t[:C].clone(), G), ops.CellMatrix(u_buf.t[:C].clone(), G)
    return out


def _kw(weights, branch, limit):
    kw = dict(BRANCHES[branch], limit_gamma=limit, maxmin_perc=PERC, maxmin_weighted_pow=POWER)
    return dict(kw, weighted=False) if weights is None else dict(kw, weights=weights)


def _run(sf, Sx, Ux, kw, steady=None, cuts=(0, C)):
    """StreamedFit over the row blocks cuts[i]..cuts[i+1] of the pooled matrices."""
    ss = None if steady is None else torch.from_numpy(steady.astype(np.uint8)).cuda()
    fit = sf.StreamedFit(G, C, Sx.dtype, Sx.t.device, n_fit_cells=C if steady is None else int(steady.sum()), **kw)
    for w in range(fit.n_walks):
        order = range(len(cuts) - 1) if w % 2 == 0 else range(len(cuts) - 2, -1, -1)
        for i in order:
            a, b = cuts[i], cuts[i + 1]
            fit.add_block(Sx.rows(a, b), Ux.rows(a, b), cell_mask=None if ss is None else ss[a:b])
        fit.end_walk()
    g, q, R2 = fit.result()
    return dict(th=dict(fit.thresholds), mom=fit.moments, gamma=g, q=q, R2=R2, n=fit.n_fit_cells, state_bytes=fit.state_bytes, walks=fit.n_walks)


def _recipe(ops, Sx, Ux, kw, rows=None):
    """VelocytoLoom.fit_gammas(**kw) on the pooled matrices, call by call (analysis.py of the package): the thresholds and the dense
    weights over all cells, then the rows of the steady-state cells gathered, then the branch's solve.  -> thresholds, moments,
    gamma, q, R2, and the weights of the fitted cells (None = unweighted)."""
    from velocyto_amd import estimation as est
    weighted, weights = kw.get("weighted", True), kw.get("weights", "maxmin_diag")
    fit_offset, fixperc_q, limit = kw.get("fit_offset", True), kw.get("fixperc_q", False), kw.get("limit_gamma", False)
    perc = [float(p) for p in kw["maxmin_perc"]]
    th, wmode, wargs = {}, 2, {}
    if weighted:
        if weights in ("sum", "prod"):
            th["p99_S"], th["p99_U"] = ops.gene_quantiles(Sx, [99])[0], ops.gene_quantiles(Ux, [99])[0]
            wmode, wargs = 0, dict(W=ops.gamma_weights(Sx, Ux, 0 if weights == "sum" else 1, th["p99_S"], th["p99_U"]))
        elif weights in ("maxmin", "maxmin_weighted"):
            q = ops.gene_quantiles(Sx, perc)
            th["down_S"], th["up_S"] = q[0], q[1]
            if weights == "maxmin":
                wmode, wargs = 1, dict(M=Sx, down=q[0], up=q[1])
            else:
                wmode, wargs = 0, dict(W=ops.gamma_weights(Sx, None, 2, q[0], q[1], power=kw["maxmin_weighted_pow"]))
        else:
            den = lambda M: (lambda q: torch.where(q[0] == 0, torch.clamp(q[1], min=0.001), q[0]))(ops.gene_quantiles(M, [99.9, 100]))
            dS, dU = den(Sx), den(Ux)
            q = ops.gene_quantiles(Sx, perc, M2=Ux, scale_a=dS, scale_b=dU)
            th.update(denom_S=dS, denom_U=dU, down=q[0], up=q[1])
            if weights == "maxmin_diag":
                wmode, wargs = 1, dict(M=Sx, M2=Ux, scale_a=dS, scale_b=dU, down=q[0], up=q[1])
            else:
                q2 = ops.gene_quantiles(Sx, perc)
                th["down_S"], th["up_S"] = q2[0], q2[1]
                wmode, wargs = 0, dict(W=ops.gamma_weights(Sx, Ux, 3, q[0], q[1], q2[0], q2[1], dS, dU))
    if rows is not None:
        take = lambda m: ops.CellMatrix(m.t.index_select(0, rows).contiguous(), m.G)
        Sx, Ux = take(Sx), take(Ux)
        wargs = {k: (take(v) if isinstance(v, ops.CellMatrix) else v) for k, v in wargs.items()}
    need_up = weighted and limit and (fit_offset or not fixperc_q)
    need_qf = fixperc_q and not fit_offset
    if need_up:
        th["up_gamma"] = est._median_and_up_gamma(Ux, Sx)
        qx = ops.gene_quantiles(Sx, [50, 90])
        th.update(med_S=qx[0], p90_S=qx[1], med_U=ops.gene_quantiles(Ux, [50])[0], n_above=(Sx.t[:, :G].double() > qx[1][None, :]).sum(0))
        th["U_p10_above"] = ops.gene_quantiles(Ux, [10], mask_src=Sx, mask_thr=qx[1], mask_mode=1)[0]
        th["S_med_above"] = ops.gene_quantiles(Sx, [50], mask_src=Sx, mask_thr=qx[1], mask_mode=1)[0]
    if need_qf:
        th["q_fixed"] = est._fixperc_q(Ux, Sx)
        th["p1_S"] = ops.gene_quantiles(Sx, [1])[0]
        th["n_below"] = (Sx.t[:, :G].double() <= th["p1_S"][None, :]).sum(0)
    mom = ops.fit_weighted_moments(Ux, Sx, wmode, **wargs)
    if fit_offset:
        if weighted:
            g, q, R2 = ops.fit_weighted(Ux, Sx, wmode, fit_offset=True, box_q=True, lo_gamma=1e-8, up_gamma_default=20.0, up_gamma=th.get("up_gamma"), **wargs)
        else:
            g, q, R2 = ops.fit_weighted(Ux, Sx, 2, fit_offset=True, box_q=False)
    elif fixperc_q:
        g, q, R2 = ops.fit_weighted(Ux, Sx, wmode, fit_offset=False, lo_gamma=0.0, up_gamma_default=20.0, q_fixed=th["q_fixed"], **wargs)
    elif weighted:
        if limit:
            g, q, R2 = ops.fit_weighted(Ux, Sx, wmode, fit_offset=False, lo_gamma=1e-8, up_gamma=th["up_gamma"], **wargs)
        else:
            g, q, R2 = ops.fit_weighted(Ux, Sx, wmode, fit_offset=False, lo_gamma=0.0, up_gamma_default=20.0, **wargs)
    else:
        g = ops.fit_slope(Ux, Sx)                                        # the facade's call; it returns no q and no R2
        q, R2 = torch.zeros_like(g), None
    W = None
    if wmode == 0:
        W = wargs["W"].t[:, :G].double().cpu().numpy()
    elif wmode == 1:
        W = _binary(Sx, Ux, wargs)
    return dict(th=th, mom=mom, gamma=torch.where(torch.isfinite(g), g, torch.zeros_like(g)), q=q, R2=R2, W=W)


def _binary(Sx, Ux, w):
    """The weights of weight_mode 1 in numpy: Z formed in the storage type, compared in double."""
    t = NP_T[Sx.dtype]
    S = Sx.t[:, :G].cpu().numpy()
    with np.errstate(all="ignore"):
        if "M2" in w:
            Z = (S / w["scale_a"].cpu().numpy().astype(t)[None, :] + Ux.t[:, :G].cpu().numpy() / w["scale_b"].cpu().numpy().astype(t)[None, :])
        else:
            Z = S
        Z = Z.astype(np.float64)
        return ((Z <= w["down"].cpu().numpy()[None, :]) | (Z >= w["up"].cpu().numpy()[None, :])).astype(np.float64)


def _bits(t):
    t = t.contiguous()
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _same(a, b):
    """Bit-identical, NaN payloads aside."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (torch.isnan(a) & torch.isnan(b)) if a.is_floating_point()
                                                                  else _bits(a) == _bits(b)).all())


def _assert_bit_identical(got, ref, what):
    assert set(got["th"]) == set(ref["th"]), (what, set(got["th"]) ^ set(ref["th"]))
    for n, v in ref["th"].items():
        assert _same(got["th"][n], v), (what, n)
    for n in ("mom", "gamma", "q", "R2"):
        if ref[n] is not None:
            assert _same(got[n], ref[n]), (what, n)


@pytest.fixture(scope="module")
def sf():
    from velocyto_amd import streamed_fit
    return streamed_fit


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("weights", WEIGHTS)
def test_one_block_equals_the_resident_recipe(ops, sf, pooled, dt, weights):
    """{box, fixperc_q, no offset} x limit_gamma on / off x steady state {none, every other cell}."""
    Sx, Ux = pooled[dt]
    rows_half = torch.from_numpy(np.flatnonzero(HALF)).cuda()
    P = 4 if dt == torch.float32 else 8
    seen = set()
    for branch in BRANCHES:
        for limit in (False, True):
            kw = _kw(weights, branch, limit)
            for steady, rows in ((None, None), (HALF, rows_half)):
                what = (weights, branch, limit, steady is not None, dt)
                got = _run(sf, Sx, Ux, kw, steady)
                ref = _recipe(ops, Sx, Ux, kw, rows)
                _assert_bit_identical(got, ref, what)
                assert got["n"] == (C if steady is None else C // 2)
                assert got["walks"] in (1, P + 1, 2 * P + 1)
                # O(genes): at most 16 select targets ride on one walk (maxmin_double with limit_gamma), a histogram and 12 bytes each,
                # and five per-gene vectors of the masked selects
                assert (got["state_bytes"] > 0) == (got["walks"] > 1) and got["state_bytes"] <= 16 * G * (256 * 4 + 12) + 5 * G * 8 * 4
                seen.add(got["walks"])
                assert bool(torch.isfinite(got["gamma"]).all())
                if branch == "no offset":
                    assert bool((got["q"] == 0).all())
    print(f"{weights}, {dt}: walk counts {sorted(seen)}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("weights", WEIGHTS)
def test_one_block_equals_the_facade(ops, sf, pooled, dt, weights):
    """VelocytoLoom.fit_gammas on the same pooled matrices, end to end: the default branch, and fixperc_q with limit_gamma over every
    other cell."""
    from velocyto_amd.analysis import VelocytoLoom
    Sx, Ux = pooled[dt]
    rng = np.random.default_rng(0)
    vlm = VelocytoLoom.from_arrays(rng.poisson(1.0, (G, C)).astype(np.float64), rng.poisson(1.0, (G, C)).astype(np.float64), dtype=dt)
    for n, m in (("Sx", Sx), ("Ux", Ux), ("Sx_sz", Sx), ("Ux_sz", Ux)):
        vlm._set_dev(n, m)
    for branch, limit, steady in (("box", False, None), ("box", True, None), ("fixperc_q", True, HALF), ("no offset", True, HALF)):
        kw = _kw(weights, branch, limit)
        got = _run(sf, Sx, Ux, kw, steady)
        vlm.R2 = None
        vlm.fit_gammas(steady_state_bool=steady, **kw)
        assert _same(got["gamma"], vlm._gammas_dev) and _same(got["q"], vlm._q_dev), (weights, branch, limit)
        if vlm.R2 is not None:
            assert _same(got["R2"].cpu(), torch.from_numpy(vlm.R2)), (weights, branch, limit)


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


def _bounds(oracle, Sx, Ux, W, n):
    """(bm, bq, br): the bound of every gene for gamma, q and R2 from the data and weights of the n fitted cells."""
    with np.errstate(all="ignore"):
        cond = np.array([oracle.fit_condition(Sx[:, g], Ux[:, g], W[:, g]) for g in range(G)])
    kf, kr, sm, sq = cond.T
    u = 4 * n * fc.EPS
    return fc.FIT_K * u * kf * sm, fc.FIT_K * u * kf * sq, fc.FIT_K_R2 * u * kr


def _check_blocked(got, one, bnd, n, what):
    assert set(got["th"]) == set(one["th"])
    for name, v in one["th"].items():
        assert _same(got["th"][name], v), f"{what}: {name} differs from the one-block run"
    m1, m2 = one["mom"].cpu().numpy(), got["mom"].cpu().numpy()
    fin = np.isfinite(m1)
    assert np.array_equal(np.isfinite(m2), fin) and np.array_equal(np.isnan(m2), np.isnan(m1))
    assert (m1[fin] >= 0).all() and (m2[fin] >= 0).all()
    rel = np.abs(m2[fin] - m1[fin]) / np.where(m1[fin] > 0, m1[fin], 1.0)
    print(f"{what}: largest relative difference of a moment {rel.max():.3g} (bar {2 * n * 2.0 ** -53:.3g})")
    assert rel.max() <= 2 * n * 2.0 ** -53
    singular = np.isposinf(bnd[0]) | np.isposinf(bnd[1])
    print(f"{what}: {int(singular.sum())} genes whose weighted normal equations are singular (kappa_fit = inf)")
    for name, b in zip(("gamma", "q", "R2"), bnd):
        a1, a2 = one[name].cpu().numpy().astype(np.float64), got[name].cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isfinite(a1), np.isfinite(a2))
        tol = np.fmax(_ulp32(a1), np.where(np.isnan(b), 0.0, b))               # the larger of one float32 ulp and the gene's bound
        same = (a1 == a2) | (np.isnan(a1) & np.isnan(a2))
        err = np.where(same, 0.0, np.abs(a2 - a1))
        worst = int(np.argmax(err / tol))
        print(f"{what}: {name}: {int((~same).sum())} genes differ, worst {err[worst]:.3g} against {tol[worst]:.3g} (gene {worst})")
        assert np.all(err <= tol), (what, name, worst, a1[worst], a2[worst], tol[worst])


BLOCKINGS = {"3 uneven blocks, one a single cell": (0, 700, 701, C), "7 blocks": tuple(range(0, C, 172))[:7] + (C,)}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("weights", WEIGHTS)
def test_blockings_equal_one_block(ops, sf, oracle, pooled, dt, weights):
    """Box fit with limit_gamma over all cells, and fixperc_q over every other cell, in 3 uneven blocks and in 7."""
    Sx, Ux = pooled[dt]
    t = NP_T[dt]
    Sn, Un = Sx.to_cells_major(t), Ux.to_cells_major(t)
    rows_half = torch.from_numpy(np.flatnonzero(HALF)).cuda()
    for branch, limit, steady, rows in (("box", True, None, None), ("fixperc_q", False, HALF, rows_half)):
        kw = _kw(weights, branch, limit)
        one = _run(sf, Sx, Ux, kw, steady)
        W = _recipe(ops, Sx, Ux, kw, rows)["W"]
        keep = slice(None) if steady is None else steady
        n = C if steady is None else int(steady.sum())
        bnd = _bounds(oracle, Sn[keep], Un[keep], np.ones((n, G)) if W is None else W, n)
        for name, cuts in BLOCKINGS.items():
            assert cuts[0] == 0 and cuts[-1] == C and all(b > a for a, b in zip(cuts, cuts[1:]))
            _check_blocked(_run(sf, Sx, Ux, kw, steady, cuts), one, bnd, n, f"{weights}, {branch}, {name}, {dt}")


def test_misuse_is_refused(ops, sf, pooled):
    Sx, Ux = pooled[torch.float32]
    fit = sf.StreamedFit(G, C, torch.float32, Sx.t.device, weights="sum")
    with pytest.raises(ValueError, match="for a fit over"):
        fit.add_block(pooled[torch.float64][0], pooled[torch.float64][1])
    fit.add_block(Sx.rows(0, 600), Ux.rows(0, 600))
    with pytest.raises(ValueError, match="n_total"):                      # half the cells: the select notices at the end of the walk
        fit.end_walk()
    with pytest.raises(RuntimeError, match="walks done"):
        fit.result()
