"""AtlasPath(fit="maxmin_diag"): velocyto's default weighted fit_gammas on the streamed atlas path, the per-gene percentiles taken by
the streamed exact select.

Bars.  One block: thresholds, gamma, q, R2 and corr BIT-IDENTICAL to the resident dense recipe on the pooled matrices (exact
selections, the same kernels in the same order).  Several blocks / ranks: thresholds still bit-identical (integer counts);
the (10, G) moments within 2 C 2^-53 relative (non-negative terms, two summation orders); gamma, q, R2 within the larger of one
float32 ulp (the bar of test_gpu_sharded.py for this two-step fit) and DESIGN section 11's bound of the gene, 4 K C eps kappa
(oracle.fit_condition on the gene's data and weights, as tests/fit_cases.py states it) - every gene, none excluded; corr with
finite entries in the same places and within the tolerance of test_gpu_atlas.py's multi-block runs (f32 2e-6, f64 1e-12).
fit="slope" stays what it was, to the bit."""
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
C, G, K, NN = 3000, 1500, 12, 100
NP_T = {torch.float32: np.float32, torch.float64: np.float64}


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
    """What a run leaves, detached from the path's buffers."""
    th = {n: v.clone() for n, v in p.fit_thresholds.items()}
    return dict(th=th, gamma=p.gamma.clone(), q=p.q.clone(), R2=p.R2.clone(), mom=p.fit_moments.clone(), corr=corr.clone(), neigh=p.neigh.clone())


@pytest.fixture(scope="module")
def one(ops, data):
    """The one-block runs (resident mode) both dtypes' blocked runs are compared with: computed once, never modified."""
    out = {}
    for dt in (torch.float32, torch.float64):
        p = _path(data, block_cells=0, dtype=dt, fit="maxmin_diag")
        corr = p.run()
        e_buf, u_buf = p._resident
        out[dt] = dict(_snapshot(p, corr), Sx=ops.CellMatrix(e_buf.t[:C].clone(), G), Ux=ops.CellMatrix(u_buf.t[:C].clone(), G), rules=p.rules)
    return out


@pytest.fixture(scope="module")
def bounds(oracle, one):
    """Per dtype (bm, bq, br): DESIGN section 11's bound of every gene for gamma, q and R2 from the one-block run's data and weights."""
    out = {}
    for dt, o in one.items():
        t = NP_T[dt]
        Sx, Ux = o["Sx"].to_cells_major(t), o["Ux"].to_cells_major(t)
        th = {n: v.cpu().numpy() for n, v in o["th"].items()}
        with np.errstate(all="ignore"):
            Z = (Sx / th["denom_S"].astype(t)[None, :] + Ux / th["denom_U"].astype(t)[None, :]).astype(np.float64)
            W = ((Z <= th["down"][None, :]) | (Z >= th["up"][None, :])).astype(np.float64)
            cond = np.array([oracle.fit_condition(Sx[:, g], Ux[:, g], W[:, g]) for g in range(G)])
        kf, kr, sm, sq = cond.T
        u = 4 * C * fc.EPS
        out[dt] = (fc.FIT_K * u * kf * sm, fc.FIT_K * u * kf * sq, fc.FIT_K_R2 * u * kr, W.sum(0))
    return out


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


def _check_blocked_against_one(got, o, bnd, dt, what):
    for n in ("denom_S", "denom_U", "down", "up"):
        assert torch.equal(_bits(got["th"][n]), _bits(o["th"][n])), f"{what}: threshold {n} differs from the one-block run"
    # the moments: non-negative terms, two summation orders
    m1, m2 = o["mom"].cpu().numpy(), got["mom"].cpu().numpy()
    assert (m1 >= 0).all() and (m2 >= 0).all()
    rel = np.abs(m2 - m1) / np.where(m1 > 0, m1, 1.0)
    print(f"{what}: largest relative difference of a moment {rel.max():.3g} (bar {2 * C * 2.0 ** -53:.3g})")
    assert rel.max() <= 2 * C * 2.0 ** -53
    assert np.array_equal(m2[5], m1[5]), "Sw is a count"
    bm, bq, br, _ = bnd
    for n, b in (("gamma", bm), ("q", bq), ("R2", br)):
        a1, a2 = o[n].cpu().numpy().astype(np.float64), got[n].cpu().numpy().astype(np.float64)
        tol = np.fmax(_ulp32(a1), np.where(np.isnan(b), 0.0, b))               # the larger of one float32 ulp and the gene's bound
        same = (a1 == a2) | (np.isnan(a1) & np.isnan(a2))
        err = np.where(same, 0.0, np.abs(a2 - a1))
        worst = int(np.argmax(err / tol))
        print(f"{what}: {n}: {int((~same).sum())} genes differ, worst {err[worst]:.3g} against {tol[worst]:.3g} (gene {worst})")
        assert np.all(err <= tol), (what, n, worst, a1[worst], a2[worst], tol[worst])
    fin = torch.isfinite(o["corr"])
    assert torch.equal(torch.isfinite(got["corr"]), fin)
    d = float((got["corr"][fin] - o["corr"][fin]).abs().max())
    print(f"{what}: max |dcorr| {d:.3g}")
    assert d <= (2e-6 if dt == torch.float32 else 1e-12)


def test_one_block_equals_the_resident_dense_recipe(ops, data, one):
    """fit_thresholds, gamma, q, R2 and corr of the one-block run, bit for bit: _maxnorm_denominator's rule via ops.gene_quantiles,
    ops.fit_weighted_moments over all cells, fit_weighted_from_moments, coldeltacor_partial_fused(..., gamma, q, ...)."""
    o = one[torch.float32]
    Sx, Ux = o["Sx"], o["Ux"]
    qS, qU = ops.gene_quantiles(Sx, [99.9, 100]), ops.gene_quantiles(Ux, [99.9, 100])
    dS, dU = (torch.where(x[0] == 0, torch.clamp(x[1], min=0.001), x[0]) for x in (qS, qU))
    thr = ops.gene_quantiles(Sx, [2, 98], M2=Ux, scale_a=dS, scale_b=dU)
    for n, ref in (("denom_S", dS), ("denom_U", dU), ("down", thr[0]), ("up", thr[1])):
        assert o["th"][n].dtype == torch.float64 and torch.equal(_bits(o["th"][n]), _bits(ref)), n
    n0 = int((thr[1] == 0).sum())
    assert 0 < n0 < G // 2                                              # genes whose down = up = 0 (every cell weighted) among genes with real thresholds
    mom = ops.fit_weighted_moments(Ux, Sx, 1, M=Sx, M2=Ux, scale_a=dS, scale_b=dU, down=thr[0], up=thr[1])
    assert torch.equal(_bits(o["mom"]), _bits(mom))
    g, q, R2 = ops.fit_weighted_from_moments(mom, C, fit_offset=True, box_q=True, lo_gamma=1e-8, up_gamma_default=20.0)
    g = torch.where(torch.isfinite(g), g, torch.zeros_like(g))
    assert torch.equal(_bits(o["gamma"]), _bits(g)) and torch.equal(_bits(o["q"]), _bits(q)) and torch.equal(_bits(o["R2"]), _bits(R2))
    corr = ops.coldeltacor_partial_fused(Sx, Ux, g, q, o["neigh"], ops.SQRT, ops.partial_rules_for(Sx, ops.SQRT, 1e-10), 1e-10, validate=False)
    assert torch.equal(torch.nan_to_num(o["corr"], nan=7.0), torch.nan_to_num(corr, nan=7.0))
    assert bool(torch.isfinite(corr).float().mean() > 0.99)


def test_one_block_equals_the_facade_fit(ops, data, one):
    """VelocytoLoom.from_arrays(...).fit_gammas() (its defaults) on the densified layers.  The facade builds its kNN graph from its own
    PCA of its own normalisation, so it cannot be handed the atlas path's graph; it is handed what that graph produced instead - the
    pooled matrices, as Sx / Ux and Sx_sz / Ux_sz (the atlas path pools size-normalised counts: the two pairs coincide) - and from
    there its whole fit_gammas runs.  It keeps no thresholds; gamma, q and R2 are its outputs."""
    import velocyto_amd
    cS, cU = data[0], data[1]
    o = one[torch.float32]
    vlm = velocyto_amd.analysis.VelocytoLoom.from_arrays(cS.to_dense().as_int32().cpu().numpy().T.astype(np.float64),
                                                         cU.to_dense().as_int32().cpu().numpy().T.astype(np.float64), dtype="float32")
    for n, m in (("Sx", o["Sx"]), ("Sx_sz", o["Sx"]), ("Ux", o["Ux"]), ("Ux_sz", o["Ux"])):
        vlm._set_dev(n, m)
    vlm.fit_gammas()
    for n, ref in (("gamma", vlm.gammas), ("q", vlm.q), ("R2", vlm.R2)):
        assert np.array_equal(o[n].cpu().numpy().view(np.int32), np.asarray(ref, dtype=np.float32).view(np.int32)), n


@pytest.mark.parametrize("dt,block_cells,nblocks", [(torch.float32, 700, 5), (torch.float64, 450, 7)])
def test_blocked_runs_equal_the_one_block_run(ops, data, one, bounds, dt, block_cells, nblocks):
    p = _path(data, block_cells=block_cells, dtype=dt, fit="maxmin_diag")
    assert len(p.blocks()) == nblocks
    got = _snapshot(p, p.run())
    assert p.rules == one[dt]["rules"] and 0 < p.select_state_bytes <= 6 * G * (256 * 4 + 12)
    _check_blocked_against_one(got, one[dt], bounds[dt], dt, f"{nblocks} blocks, {dt}")
    # a second run of the same object walks the same passes again (the select's state is per run)
    again = _snapshot(p, p.run())
    for n in ("gamma", "q", "R2", "corr"):
        assert torch.equal(torch.nan_to_num(again[n], nan=7.0), torch.nan_to_num(got[n], nan=7.0)), n
    if dt == torch.float64:
        # the staging buffers holding what a caching allocator may hand out: no data pass reads a row it has not pooled
        g = _path(data, block_cells=block_cells, dtype=dt, fit="maxmin_diag")
        g._plan_blocks()
        g._ebuf.t[:, :G] = 1e308
        g._ebuf.t[::7, :G] = float("nan")
        g._ubuf.t[:, :G] = float("inf")
        garbage = _snapshot(g, g.run())
        for n in ("gamma", "q", "R2", "corr", "mom"):
            assert torch.equal(torch.nan_to_num(garbage[n], nan=7.0), torch.nan_to_num(got[n], nan=7.0)), n
        for n in garbage["th"]:
            assert torch.equal(_bits(garbage["th"][n]), _bits(got["th"][n])), n


def _dense_reference(ops, atlas, cS, cU, fS, fU, pcs, emb, k, n_neighbors, frac):
    """The resident dense path on the same data: knn_pool_counts -> fit_slope -> fused stage D with a full-height e."""
    C = cS.C
    idx, dist = ops.knn_search(pcs, k, include_self=False)
    conn = (dist > 0).float()
    w = torch.cat([torch.ones((C, 1), device=idx.device), conn], 1)
    w = w / w.sum(1, keepdim=True)
    ind = torch.cat([torch.arange(C, device=idx.device, dtype=torch.int32)[:, None], idx], 1)
    ind, w = ops.canonical_graph_rows(ind, w)                # rows by cell number: the order every device-built graph pools in
    ptr = torch.arange(0, (C + 1) * (k + 1), k + 1, device=idx.device, dtype=torch.int64)
    Sx, Ux = ops.knn_pool_counts(cS.to_dense(), cU.to_dense(), fS, fU, ptr, ind, w, dtype=torch.float32, validate=False)
    gamma = ops.fit_slope_from_moments(ops.fit_slope_moments(Ux, Sx))
    gamma[~torch.isfinite(gamma)] = 0.0                      # analysis.py:1260
    neigh = atlas.sample_neighbors(emb.double(), 0, C, n_neighbors, frac)
    corr = ops.coldeltacor_partial_fused(Sx, Ux, gamma, None, neigh, ops.SQRT, ops.partial_rules_for(Sx, ops.SQRT, 1e-10), 1e-10, validate=False)
    return Sx, Ux, gamma, neigh, corr


def test_default_path_is_untouched_and_the_two_fits_differ(ops, data, one):
    from velocyto_amd import atlas
    Sx, Ux, gamma, neigh, corr = _dense_reference(ops, atlas, *data, K, NN, 0.5)
    a, b = _path(data, block_cells=0), _path(data, block_cells=0, fit="slope")
    ca, cb = a.run().clone(), b.run().clone()
    assert a.fit == b.fit == "slope" and a.q is None and a.fit_thresholds is None
    assert torch.equal(_bits(a.gamma), _bits(b.gamma)) and torch.equal(torch.nan_to_num(ca, nan=7.0), torch.nan_to_num(cb, nan=7.0))
    assert torch.equal(_bits(a.gamma), _bits(gamma)) and torch.equal(torch.nan_to_num(ca, nan=7.0), torch.nan_to_num(corr, nan=7.0))
    assert torch.equal(Sx.t, one[torch.float32]["Sx"].t)      # both fits saw the same pooled matrix ...
    o = one[torch.float32]
    moved = (o["gamma"] != gamma)
    assert float(moved.float().mean()) > 0.5 and int((o["q"] != 0).sum()) > 0       # ... and give other numbers: the new path is taken
    assert _path(data, block_cells=0, fit="default").fit == "maxmin_diag"
    with pytest.raises(ValueError, match="unknown fit"):
        _path(data, block_cells=0, fit="maxmin")


def _run_worker(world, out, cfg, port):
    env = dict(os.environ, VCY_SINGLE_DEVICE="1", VCY_DIST_BACKEND="gloo", MASTER_PORT=str(port), MASTER_ADDR="127.0.0.1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "atlas_fit_worker.py"), out, json.dumps(cfg)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


@pytest.mark.parametrize("world,block_cells", [(2, 0), (3, 0), (2, 400)])
def test_sharded_ranks_equal_one_rank(ops, one, bounds, tmp_path, world, block_cells):
    """2 and 3 ranks on one GPU (gloo transport), once with several blocks per rank: the integer histograms summed over the ranks give
    every rank the one-rank thresholds bit for bit; the all-reduced moments, the fit and the gathered correlation rows meet the
    multi-block bars."""
    many = _run_worker(world, str(tmp_path / "many.npz"), dict(C=C, G=G, k=K, n_neighbors=NN, block_cells=block_cells), port=29891 + 2 * world + (block_cells > 0))
    assert int(many["world"]) == world and (int(many["blocks"]) >= 3 if block_cells else int(many["blocks"]) == 1)
    per = many["per_gene_every_rank"]
    assert per.shape == (world, 7, G)
    for rk in range(1, world):
        assert np.array_equal(per[rk].view(np.int64), per[0].view(np.int64)), f"rank {rk} holds other thresholds or another fit than rank 0"
    dev = one[torch.float32]["gamma"].device
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=dev)
    got = dict(th={n: t(per[0, i]) for i, n in enumerate(("denom_S", "denom_U", "down", "up"))}, gamma=t(per[0, 4], torch.float32), q=t(per[0, 5], torch.float32),
               R2=t(per[0, 6], torch.float32), mom=t(many["moments"]), corr=t(many["corr"], torch.float32))
    _check_blocked_against_one(got, one[torch.float32], bounds[torch.float32], torch.float32, f"{world} ranks, block_cells={block_cells}")
