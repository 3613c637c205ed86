"""AtlasPath(fit="maxmin_diag") with fit_gammas' options fit_offset, fixperc_q, limit_gamma and steady_state_bool: the conditional
per-gene percentiles from the masked streamed select, the moments over the steady-state cells.

Bars (those of tests/test_gpu_atlas_fit.py).  One block: up_gamma, q_fixed, the populations, gamma, q, R2 and corr BIT-IDENTICAL to
the resident recipe on the pooled matrices - estimation._median_and_up_gamma / _fixperc_q (whole-matrix ops.gene_quantiles with its
masks) and ops.fit_weighted with the arguments VelocytoLoom.fit_gammas passes.  Several blocks / ranks: every percentile and
population still bit-identical (integer counts); the (10, G) moments within 2 n 2^-53 relative (non-negative terms, two summation
orders, n cells); gamma, q, R2 within the larger of one float32 ulp and DESIGN section 11's bound of the gene, 4 K n eps kappa
(oracle.fit_condition on the gene's data and weights); corr with finite entries in the same places and within 2e-6 (f32) / 1e-12
(f64).  A steady-state mask: the same recipe on the gathered rows (thresholds over all cells), percentiles bit-identical, moments
and fit within the bars above with n = the masked cells."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fit_cases as fc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, G, K, NN = 1200, 200, 10, 60
NP_T = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = (torch.float32, torch.float64)
# the option rows of AtlasPath's docstring
OPTIONS = {"box, limit_gamma": dict(limit_gamma=True),
           "fixperc_q": dict(fit_offset=False, fixperc_q=True),
           "no offset, limit_gamma": dict(fit_offset=False, limit_gamma=True),
           "no offset": dict(fit_offset=False)}
PERCENTILES = ("denom_S", "denom_U", "down", "up", "med_S", "p90_S", "med_U", "U_p10_above", "S_med_above", "n_above", "up_gamma", "p1_S",
               "n_below", "q_fixed")


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
    th = {n: v.clone() for n, v in p.fit_thresholds.items()}
    return dict(th=th, gamma=p.gamma.clone(), q=p.q.clone(), R2=p.R2.clone(), mom=p.fit_moments.clone(), corr=corr.clone(), neigh=p.neigh.clone(),
                n=p.n_fit_cells)


@pytest.fixture(scope="module")
def one(ops, data):
    """The one-block runs (resident mode) of every option row and of the default, both dtypes: computed once, never modified."""
    out = {}
    for dt in DTYPES:
        for name, opt in (("default", {}), *OPTIONS.items()):
            p = _path(data, block_cells=0, dtype=dt, fit="maxmin_diag", **opt)
            corr = p.run()
            out[dt, name] = dict(_snapshot(p, corr), rules=p.rules)
        e_buf, u_buf = p._resident
        out[dt, "Sx"], out[dt, "Ux"] = ops.CellMatrix(e_buf.t[:C].clone(), G), ops.CellMatrix(u_buf.t[:C].clone(), G)
    return out


def _weights(Sx, Ux, th, t):
    with np.errstate(all="ignore"):
        Z = (Sx / th["denom_S"].astype(t)[None, :] + Ux / th["denom_U"].astype(t)[None, :]).astype(np.float64)
        return ((Z <= th["down"][None, :]) | (Z >= th["up"][None, :])).astype(np.float64)


def _bounds(oracle, Sx, Ux, W, n):
    """(bm, bq, br): DESIGN section 11's bound of every gene for gamma, q and R2 from the data and weights of the n fitted cells."""
    with np.errstate(all="ignore"):
        cond = np.array([oracle.fit_condition(Sx[:, g], Ux[:, g], W[:, g]) for g in range(G)])
    kf, kr, sm, sq = cond.T
    u = 4 * n * fc.EPS
    return fc.FIT_K * u * kf * sm, fc.FIT_K * u * kf * sq, fc.FIT_K_R2 * u * kr


@pytest.fixture(scope="module")
def bounds(oracle, one):
    out = {}
    for dt in DTYPES:
        t = NP_T[dt]
        Sx, Ux = one[dt, "Sx"].to_cells_major(t), one[dt, "Ux"].to_cells_major(t)
        th = {n: v.cpu().numpy() for n, v in one[dt, "default"]["th"].items()}
        W = _weights(Sx, Ux, th, t)
        half = np.arange(C) % 2 == 0
        out[dt] = _bounds(oracle, Sx, Ux, W, C)
        out[dt, "half"] = _bounds(oracle, Sx[half], Ux[half], W[half], int(half.sum()))
    return out


def _bits(t):
    t = t.contiguous()
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


def _check_moments_and_fit(got, ref, bnd, n, dt, what, corr=True):
    """got / ref: dicts of numpy arrays mom, gamma, q, R2 (and corr): the bars of several blocks / ranks against one block."""
    m1, m2 = ref["mom"], got["mom"]
    assert (m1 >= 0).all() and (m2 >= 0).all()
    rel = np.abs(m2 - m1) / np.where(m1 > 0, m1, 1.0)
    print(f"{what}: largest relative difference of a moment {rel.max():.3g} (bar {2 * n * 2.0 ** -53:.3g})")
    assert rel.max() <= 2 * n * 2.0 ** -53
    assert np.array_equal(m2[5], m1[5]), "Sw is a count"
    for name, b in zip(("gamma", "q", "R2"), bnd):
        a1, a2 = ref[name].astype(np.float64), got[name].astype(np.float64)
        tol = np.fmax(_ulp32(a1), np.where(np.isnan(b), 0.0, b))               # the larger of one float32 ulp and the gene's bound
        same = (a1 == a2) | (np.isnan(a1) & np.isnan(a2))
        err = np.where(same, 0.0, np.abs(a2 - a1))
        worst = int(np.argmax(err / tol))
        print(f"{what}: {name}: {int((~same).sum())} genes differ, worst {err[worst]:.3g} against {tol[worst]:.3g} (gene {worst})")
        assert np.all(err <= tol), (what, name, worst, a1[worst], a2[worst], tol[worst])
    if corr:
        fin = np.isfinite(ref["corr"])
        assert np.array_equal(np.isfinite(got["corr"]), fin)
        d = float(np.abs(got["corr"][fin] - ref["corr"][fin]).max())
        print(f"{what}: max |dcorr| {d:.3g}")
        assert d <= (2e-6 if dt == torch.float32 else 1e-12)


def _np(o):
    return {n: o[n].cpu().numpy() for n in ("mom", "gamma", "q", "R2", "corr")}


def _check_blocked_against_one(got, o, bnd, dt, what):
    assert set(got["th"]) == set(o["th"])
    for n in got["th"]:
        assert n in PERCENTILES and got["th"][n].dtype == o["th"][n].dtype
        assert torch.equal(_bits(got["th"][n]), _bits(o["th"][n])), f"{what}: {n} differs from the one-block run"
    assert got["n"] == o["n"]
    _check_moments_and_fit(_np(got), _np(o), bnd, o["n"], dt, what)


def _recipe(ops, Sx, Ux, th, opt, rows=None):
    """The resident recipe of VelocytoLoom.fit_gammas(weighted=True, weights="maxmin_diag", **opt) on the pooled matrices, the
    thresholds th over all cells; rows: the steady-state cells, gathered as the facade gathers them.  Returns (extras, gamma, q, R2)."""
    from velocyto_amd import estimation as est
    if rows is not None:
        Sx, Ux = (ops.CellMatrix(m.t.index_select(0, rows).contiguous(), m.G) for m in (Sx, Ux))
    w = dict(M=Sx, M2=Ux, scale_a=th["denom_S"], scale_b=th["denom_U"], down=th["down"], up=th["up"])
    fit_offset, fixperc_q, limit = opt.get("fit_offset", True), opt.get("fixperc_q", False), opt.get("limit_gamma", False)
    extras = {}
    if limit and (fit_offset or not fixperc_q):
        extras["up_gamma"] = est._median_and_up_gamma(Ux, Sx)
        qx = ops.gene_quantiles(Sx, [50, 90])
        extras.update(med_S=qx[0], p90_S=qx[1], med_U=ops.gene_quantiles(Ux, [50])[0],
                      n_above=(Sx.t[:, :G].double() > qx[1][None, :]).sum(0))
        extras["U_p10_above"] = ops.gene_quantiles(Ux, [10], mask_src=Sx, mask_thr=qx[1], mask_mode=1)[0]
        extras["S_med_above"] = ops.gene_quantiles(Sx, [50], mask_src=Sx, mask_thr=qx[1], mask_mode=1)[0]
    if fixperc_q and not fit_offset:
        extras["q_fixed"] = est._fixperc_q(Ux, Sx)
        extras["p1_S"] = ops.gene_quantiles(Sx, [1])[0]
        extras["n_below"] = (Sx.t[:, :G].double() <= extras["p1_S"][None, :]).sum(0)
    if fit_offset:
        g, q, R2 = ops.fit_weighted(Ux, Sx, 1, fit_offset=True, box_q=True, lo_gamma=1e-8, up_gamma_default=20.0, up_gamma=extras.get("up_gamma"), **w)
    elif fixperc_q:
        g, q, R2 = ops.fit_weighted(Ux, Sx, 1, fit_offset=False, lo_gamma=0.0, up_gamma_default=20.0, q_fixed=extras["q_fixed"], **w)
    elif limit:
        g, q, R2 = ops.fit_weighted(Ux, Sx, 1, fit_offset=False, lo_gamma=1e-8, up_gamma=extras["up_gamma"], **w)
    else:
        g, q, R2 = ops.fit_weighted(Ux, Sx, 1, fit_offset=False, lo_gamma=0.0, up_gamma_default=20.0, **w)
    return extras, torch.where(torch.isfinite(g), g, torch.zeros_like(g)), q, R2


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(OPTIONS))
def test_one_block_equals_the_resident_recipe(ops, one, dt, name):
    o, d = one[dt, name], one[dt, "default"]
    Sx, Ux = one[dt, "Sx"], one[dt, "Ux"]
    for n in ("denom_S", "denom_U", "down", "up"):                        # the weights' thresholds do not depend on the options
        assert torch.equal(_bits(o["th"][n]), _bits(d["th"][n])), n
    extras, g, q, R2 = _recipe(ops, Sx, Ux, d["th"], OPTIONS[name])
    assert set(o["th"]) == {"denom_S", "denom_U", "down", "up", *extras}
    for n, ref in extras.items():
        assert o["th"][n].dtype == ref.dtype and torch.equal(_bits(o["th"][n]), _bits(ref)), n
    for n, ref in (("gamma", g), ("q", q), ("R2", R2)):
        assert torch.equal(_bits(o[n]), _bits(ref)), n
    corr = ops.coldeltacor_partial_fused(Sx, Ux, g, q, o["neigh"], ops.SQRT, o["rules"], 1e-10, validate=False)
    assert torch.equal(torch.nan_to_num(o["corr"], nan=7.0), torch.nan_to_num(corr, nan=7.0))
    assert o["n"] == C
    # the option is not a no-op on this data: the masks kept a real subset of the cells, the box holds, a fit without offset moved
    for n in ("n_above", "n_below"):
        if n in extras:
            assert 0 < int(extras[n].max()) <= C and int(extras[n].min()) < C // 2
    if "up_gamma" in extras:
        ug = extras["up_gamma"]
        print(f"{name}, {dt}: up_gamma > 1.5 for {int((ug > 1.5).sum())} genes, NaN for {int(torch.isnan(ug).sum())}; "
              f"{int((o['gamma'] != d['gamma']).sum())} gammas differ from the default fit's")
        ok = ~torch.isnan(ug)
        assert bool((o["gamma"].double()[ok] <= ug[ok].float().double() * (1 + 2.0 ** -23)).all())
    if not OPTIONS[name].get("fit_offset", True):
        assert not torch.equal(_bits(o["gamma"]), _bits(d["gamma"]))
        if "q_fixed" not in extras:
            assert bool((o["q"] == 0).all())
        else:
            print(f"{name}, {dt}: q_fixed != 0 for {int((extras['q_fixed'] != 0).sum())} genes")


@pytest.mark.parametrize("name", ["box, limit_gamma", "no offset, limit_gamma"])
def test_limit_gamma_where_the_percentiles_decide_the_box(ops, oracle, name):
    """On the sparse synthetic atlas of this file up_gamma is 1.5 for every gene: median(U) never exceeds median(S), and the 10th
    percentile of U over the cells of high S is 0.  A denser atlas (density 0.6) whose unspliced size factors are 20 times larger
    has median(U) > median(S) and a positive conditional percentile for most genes, so y10 / xm decides their box: one block
    against the resident recipe bit for bit, three blocks against one block under the bars of this file."""
    from velocyto_amd import atlas
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(C, G, K, ops.require_gpu(), density=0.6)
    fS, fU = atlas.size_factors(totS, totU, C)
    swapped = (cS, cU, fS, fU * 20, pcs, emb)
    dt = torch.float32
    p = _path(swapped, block_cells=0, dtype=dt, fit="maxmin_diag", **OPTIONS[name])
    o = dict(_snapshot(p, p.run()), rules=p.rules)
    e_buf, u_buf = p._resident
    Sx, Ux = ops.CellMatrix(e_buf.t[:C].clone(), G), ops.CellMatrix(u_buf.t[:C].clone(), G)
    base = {n: o["th"][n] for n in ("denom_S", "denom_U", "down", "up")}
    extras, g, q, R2 = _recipe(ops, Sx, Ux, base, OPTIONS[name])
    for n, ref in extras.items():
        assert torch.equal(_bits(o["th"][n]), _bits(ref)), n
    for n, ref in (("gamma", g), ("q", q), ("R2", R2)):
        assert torch.equal(_bits(o[n]), _bits(ref)), n
    ug = extras["up_gamma"]
    at_box = (o["gamma"] == ug.float()) & (ug > 1.5)
    print(f"dense atlas, {name}: up_gamma > 1.5 for {int((ug > 1.5).sum())} genes, gamma on that bound for {int(at_box.sum())}")
    assert int((ug > 1.5).sum()) > 0
    t = NP_T[dt]
    Sx_n, Ux_n = Sx.to_cells_major(t), Ux.to_cells_major(t)
    bnd = _bounds(oracle, Sx_n, Ux_n, _weights(Sx_n, Ux_n, {n: v.cpu().numpy() for n, v in base.items()}, t), C)
    b = _path(swapped, block_cells=400, dtype=dt, fit="maxmin_diag", **OPTIONS[name])
    _check_blocked_against_one(_snapshot(b, b.run()), o, bnd, dt, f"dense atlas, {name}, 3 blocks")


def test_ignored_combinations_and_defaults(ops, data, one):
    """fixperc_q is ignored with fit_offset=True, limit_gamma with fixperc_q; the defaults spelled out are the default run, bit for bit."""
    dt = torch.float32
    for opt, same_as in ((dict(fit_offset=True, fixperc_q=False, limit_gamma=False, steady_state_bool=None), "default"),
                         (dict(fixperc_q=True), "default"), (dict(fit_offset=False, fixperc_q=True, limit_gamma=True), "fixperc_q")):
        p = _path(data, block_cells=0, dtype=dt, fit="maxmin_diag", **opt)
        got, o = _snapshot(p, p.run()), one[dt, same_as]
        assert set(got["th"]) == set(o["th"])
        for n in got["th"]:
            assert torch.equal(_bits(got["th"][n]), _bits(o["th"][n])), n
        for n in ("gamma", "q", "R2", "mom", "corr"):
            assert torch.equal(torch.nan_to_num(got[n], nan=7.0), torch.nan_to_num(o[n], nan=7.0)), (opt, n)
    assert set(one[dt, "default"]["th"]) == {"denom_S", "denom_U", "down", "up"}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(OPTIONS))
@pytest.mark.parametrize("block_cells,nblocks", [(C, 1), (400, 3), (500, 3)])
def test_blocked_runs_equal_the_one_block_run(ops, data, one, bounds, dt, name, block_cells, nblocks):
    p = _path(data, block_cells=block_cells, dtype=dt, fit="maxmin_diag", **OPTIONS[name])
    assert len(p.blocks()) == nblocks and (block_cells != 500 or p.blocks()[-1] == (1000, 1200))     # 500: uneven blocks
    got = _snapshot(p, p.run())
    per_target = 256 * 4 + 12
    assert 0 < p.select_state_bytes <= 6 * G * per_target + G * (6 * per_target + 3 * 8 + 2 * 8)
    _check_blocked_against_one(got, one[dt, name], bounds[dt], dt, f"{name}, {nblocks} blocks of {block_cells}, {dt}")


def _run_worker(world, out, cfg, port):
    env = dict(os.environ, VCY_SINGLE_DEVICE="1", VCY_DIST_BACKEND="gloo", MASTER_PORT=str(port), MASTER_ADDR="127.0.0.1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "atlas_fit_options_worker.py"), out, json.dumps(cfg)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = dict(np.load(out))
    per = {str(n): z["per_gene_every_rank"][:, i] for i, n in enumerate(z["names"])}
    return z, per


@pytest.mark.parametrize("name,dt,steady", [("box, limit_gamma", torch.float32, None), ("fixperc_q", torch.float64, None),
                                            ("no offset, limit_gamma", torch.float32, "half")])
def test_two_ranks_equal_one_rank(ops, data, one, bounds, tmp_path, name, dt, steady):
    cfg = dict(C=C, G=G, k=K, n_neighbors=NN, block_cells=350, dtype=str(dt).split(".")[1], options=OPTIONS[name], steady=steady)
    z, per = _run_worker(2, str(tmp_path / "o.npz"), cfg, 29641 + list(OPTIONS).index(name))
    if steady is None:
        o, bnd = one[dt, name], bounds[dt]
    else:
        p = _path(data, block_cells=0, dtype=dt, fit="maxmin_diag", steady_state_bool=np.arange(C) % 2 == 0, **OPTIONS[name])
        o, bnd = _snapshot(p, p.run()), bounds[dt, "half"]
    assert int(z["n_fit_cells"]) == o["n"] and set(per) == set(o["th"]) | {"gamma", "q", "R2"}
    for n, ref in o["th"].items():
        for r in range(2):
            assert np.array_equal(per[n][r].view(np.int64), ref.double().cpu().numpy().view(np.int64)), (n, r)
    for n in ("gamma", "q", "R2"):
        assert np.array_equal(per[n][0].view(np.int64), per[n][1].view(np.int64)), n                # every rank solved the same moments
    got = dict(mom=z["moments"], corr=z["corr"], **{n: per[n][0].astype(np.float32) for n in ("gamma", "q", "R2")})
    _check_moments_and_fit(got, _np(o), bnd, o["n"], dt, f"2 ranks, {name}, {dt}, steady {steady}")


@pytest.mark.parametrize("dt", DTYPES)
def test_all_true_steady_state_is_none(ops, data, one, dt):
    name = "box, limit_gamma"
    for mask in (np.ones(C, dtype=bool), torch.ones(C, dtype=torch.bool)):
        p = _path(data, block_cells=0, dtype=dt, fit="maxmin_diag", steady_state_bool=mask, **OPTIONS[name])
        assert p._ss is None
        got, o = _snapshot(p, p.run()), one[dt, name]
        for n in got["th"]:
            assert torch.equal(_bits(got["th"][n]), _bits(o["th"][n])), n
        for n in ("gamma", "q", "R2", "mom", "corr"):
            assert torch.equal(torch.nan_to_num(got[n], nan=7.0), torch.nan_to_num(o[n], nan=7.0)), n


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["default", *OPTIONS])
@pytest.mark.parametrize("block_cells", [0, 400])
def test_half_steady_state_equals_the_recipe_on_the_gathered_rows(ops, data, one, bounds, dt, name, block_cells):
    half = np.arange(C) % 2 == 0
    n = int(half.sum())
    opt = OPTIONS.get(name, {})
    p = _path(data, block_cells=block_cells, dtype=dt, fit="maxmin_diag", steady_state_bool=half, **opt)
    got = _snapshot(p, p.run())
    assert got["n"] == n and p._ss is not None
    d = one[dt, "default"]
    for nm in ("denom_S", "denom_U", "down", "up"):                       # the thresholds are taken over ALL cells
        assert torch.equal(_bits(got["th"][nm]), _bits(d["th"][nm])), nm
    Sx, Ux = one[dt, "Sx"], one[dt, "Ux"]
    rows = torch.from_numpy(np.flatnonzero(half)).cuda()
    extras, g, q, R2 = _recipe(ops, Sx, Ux, d["th"], opt, rows=rows)
    assert set(got["th"]) == {"denom_S", "denom_U", "down", "up", *extras}
    for nm, ref in extras.items():
        if nm != "up_gamma":
            assert torch.equal(_bits(got["th"][nm]), _bits(ref)), nm
    if "up_gamma" in extras:                                              # built from bit-identical percentiles by the same torch calls
        assert torch.equal(_bits(got["th"]["up_gamma"]), _bits(extras["up_gamma"]))
    take = lambda m: ops.CellMatrix(m.t.index_select(0, rows).contiguous(), m.G)
    w = dict(M=take(Sx), M2=take(Ux), scale_a=d["th"]["denom_S"], scale_b=d["th"]["denom_U"], down=d["th"]["down"], up=d["th"]["up"])
    ref = dict(mom=ops.fit_weighted_moments(take(Ux), take(Sx), 1, **w).cpu().numpy(), gamma=g.cpu().numpy(), q=q.cpu().numpy(), R2=R2.cpu().numpy())
    _check_moments_and_fit(_np(got), ref, bounds[dt, "half"], n, dt, f"half steady state, {name}, block_cells {block_cells}, {dt}", corr=False)
    assert not torch.equal(_bits(got["gamma"]), _bits(one[dt, name]["gamma"]))


def test_bad_arguments_are_refused(ops, data):
    for opt in (dict(fit_offset=False), dict(fixperc_q=True), dict(limit_gamma=True), dict(steady_state_bool=np.ones(C, dtype=bool))):
        for fit in ({}, dict(fit="slope")):
            with pytest.raises(ValueError, match="belong to fit=\"maxmin_diag\""):
                _path(data, block_cells=0, **fit, **opt)
    for bad in (np.ones(C - 1, dtype=bool), np.ones(C, dtype=np.int64), np.ones((C, 1), dtype=bool)):
        with pytest.raises(ValueError, match="1-d bool mask"):
            _path(data, block_cells=0, fit="maxmin_diag", steady_state_bool=bad)
    with pytest.raises(ValueError, match="selects no cell"):
        _path(data, block_cells=0, fit="maxmin_diag", steady_state_bool=np.zeros(C, dtype=bool))
    with pytest.raises(ValueError, match="unknown fit"):
        _path(data, block_cells=0, fit="maxmin", limit_gamma=True)
