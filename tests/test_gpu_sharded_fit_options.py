"""ShardedLoom.fit_gammas beyond its bare default: every argument combination goes through streamed_fit.StreamedFit with the rank's
shard as its one block.  Worlds 1 and 2 on one GPU (gloo), the tests/golden/pipeline.npz inputs in f64, against
VelocytoLoom.fit_gammas with the same arguments.

Bars.  Thresholds (percentiles, denominators, populations) bit-equal to the facade's own calls (ops.gene_quantiles on its pooled
matrices; estimation._median_and_up_gamma / _fixperc_q on the gathered steady-state rows), and world 2's to world 1's.  gammas, q, R2
within the larger of one float32 ulp and the gene's 4 K n eps kappa (oracle.fit_condition on the gene's data and its actual
weights): the ranks' f64 moments are summed in another order than the facade's.  World 1 with _route="select": thresholds, gammas,
q, R2 bit-identical to the gene-slice route's."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
PIPE = dict(k=12, n_pca_dims=10, dtype="float64")
# fit 0: the bare default (gene slices); fit 1: the same through the select; then one per new argument
FITS = [dict(), dict(_route="select"),
        dict(weights="sum"), dict(weights="prod"), dict(weights="maxmin"), dict(weights="maxmin_weighted", maxmin_weighted_pow=2.5),
        dict(weights="maxmin_double", maxmin_perc=[5, 95]), dict(limit_gamma=True), dict(fit_offset=False, fixperc_q=True), dict(weighted=False),
        dict(steady="half"), dict(weights="maxmin_weighted", fit_offset=False, limit_gamma=True, steady="half")]


@pytest.fixture(scope="module")
def vcy():
    import velocyto_amd
    velocyto_amd.ops.require_gpu()
    return velocyto_amd


def _launch(inp, out, world, port):
    env = dict(os.environ, VCY_SINGLE_DEVICE="1", VCY_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "sharded_fit_worker.py"), inp, out, json.dumps(dict(PIPE, fits=FITS))]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Worlds 1 and 2, one after the other (at most two worker processes at a time): every configuration in one launch each."""
    d = tmp_path_factory.mktemp("sharded_fit")
    g = np.load(os.path.join(GOLDEN, "pipeline.npz"))
    inp = str(d / "in.npz")
    np.savez(inp, S=g["S"], U=g["U"], pcs=g["pcs"], ts=g["ts"])
    return {w: _launch(inp, str(d / f"out{w}.npz"), w, 29811 + w) for w in (1, 2)}, dict(np.load(inp))


@pytest.fixture(scope="module")
def facade(vcy, runs):
    d = runs[1]
    vlm = vcy.analysis.VelocytoLoom.from_arrays(d["S"], d["U"], dtype=PIPE["dtype"])
    vlm.normalize("both", size=True, log=True)
    vlm.pcs, vlm.ts = d["pcs"], d["ts"]
    vlm.knn_imputation(k=PIPE["k"], n_pca_dims=PIPE["n_pca_dims"], n_jobs=1)
    return vlm


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = np.uint32 if a.dtype.itemsize == 4 else np.uint64
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


def _thr(run, i):
    pre = f"{i}_thr_"
    return {k[len(pre):]: v for k, v in run.items() if k.startswith(pre)}


def test_world_one_select_route_is_the_gene_slice_route_bit_for_bit(runs):
    r = runs[0][1]
    assert int(r["world"]) == 1
    a, b = _thr(r, 0), _thr(r, 1)
    assert set(a) == set(b) == {"denom_S", "denom_U", "down", "up"}
    for n in a:
        assert _bits_equal(a[n], b[n]), n
    for n in ("gammas", "q", "R2"):
        assert _bits_equal(r[f"0_{n}"], r[f"1_{n}"]), n


def test_exchange_bytes(runs):
    """The default route moves both pooled matrices through the gene-slice all-to-all; the select all-reduces histograms and moments."""
    r1, r2 = runs[0][1], runs[0][2]
    assert int(r2["world"]) == 2
    G, C = runs[1]["S"].shape
    assert r1["0_bytes"][1] == -1 and tuple(r1["1_bytes"]) == (-1, 0)                    # one rank: the select all-reduces nothing
    sl, _ = r2["0_bytes"]
    _, sel = r2["1_bytes"]
    assert sl > 0 and r2["0_bytes"][1] == -1 and r2["1_bytes"][0] == -1
    # 8 passes in f64.  Per select and pass: the cell count (8 bytes) and its histograms - one for all targets in pass 0, one per target
    # (a distinct rank, ops.percentile_targets) afterwards; three selects ([99.9, 100] of Sx and of Ux, [2, 98] of Z); then 10 G moments
    from velocyto_amd import ops
    hist, P = G * 256 * 4, 8
    expect = 10 * G * 8
    for qs in ([99.9, 100], [99.9, 100], [2, 98]):
        nt = len(ops.percentile_targets(qs, C)[0])
        expect += P * 8 + hist * (1 + (P - 1) * nt)
    assert sel == expect, (sel, expect)
    # ... and that is what went through the all-reduces: the worker counted every tensor handed to distributed.all_reduce_sum while the
    # fit ran
    assert int(r2["1_wire"]) == sel
    for i in range(2, len(FITS)):
        assert int(r2[f"{i}_wire"]) == r2[f"{i}_bytes"][1] > 0, i
        assert int(r1[f"{i}_wire"]) == 0
    print(f"world 2, {C} cells x {G} genes: gene slices {sl} bytes, select {sel} bytes")


def _facade_thresholds(vcy, vlm, kw, rows):
    """What the facade's fit_gammas derives on the way, by the calls it makes (analysis.py, estimation.py of the package)."""
    from velocyto_amd import ops, estimation as est
    Sx, Ux = vlm.dev("Sx_sz"), vlm.dev("Ux_sz")
    G = Sx.G
    perc = [float(p) for p in kw.get("maxmin_perc", [2, 98])]
    w, th, W = kw.get("weights", "maxmin_diag"), {}, None
    dense = lambda m: m.t[:, :G].double().cpu().numpy()
    if not kw.get("weighted", True):
        W = np.ones((Sx.C, G))
    elif w in ("sum", "prod"):
        th["p99_S"], th["p99_U"] = ops.gene_quantiles(Sx, [99])[0], ops.gene_quantiles(Ux, [99])[0]
        W = dense(ops.gamma_weights(Sx, Ux, 0 if w == "sum" else 1, th["p99_S"], th["p99_U"]))
    elif w in ("maxmin", "maxmin_weighted"):
        q = ops.gene_quantiles(Sx, perc)
        th["down_S"], th["up_S"] = q[0], q[1]
        if w == "maxmin":
            S = dense(Sx)
            W = ((S <= q[0].cpu().numpy()[None, :]) | (S >= q[1].cpu().numpy()[None, :])).astype(np.float64)
        else:
            W = dense(ops.gamma_weights(Sx, None, 2, q[0], q[1], power=kw.get("maxmin_weighted_pow", 15)))
    else:
        dS, dU = vlm._maxnorm_denominator(Sx), vlm._maxnorm_denominator(Ux)
        q = ops.gene_quantiles(Sx, perc, M2=Ux, scale_a=dS, scale_b=dU)
        th.update(denom_S=dS, denom_U=dU, down=q[0], up=q[1])
        if w == "maxmin_double":
            q2 = ops.gene_quantiles(Sx, perc)
            th["down_S"], th["up_S"] = q2[0], q2[1]
            W = dense(ops.gamma_weights(Sx, Ux, 3, q[0], q[1], q2[0], q2[1], dS, dU))
        else:
            with np.errstate(all="ignore"):
                Z = dense(Sx) / dS.cpu().numpy()[None, :] + dense(Ux) / dU.cpu().numpy()[None, :]        # f64 storage
            W = ((Z <= q[0].cpu().numpy()[None, :]) | (Z >= q[1].cpu().numpy()[None, :])).astype(np.float64)
    if rows is not None:
        take = lambda m: ops.CellMatrix(m.t.index_select(0, torch.from_numpy(rows).cuda()).contiguous(), m.G)
        Sx, Ux, W = take(Sx), take(Ux), W[rows]
    fit_offset, fixperc_q, limit = kw.get("fit_offset", True), kw.get("fixperc_q", False), kw.get("limit_gamma", False)
    if kw.get("weighted", True) and limit and (fit_offset or not fixperc_q):
        th["up_gamma"] = est._median_and_up_gamma(Ux, Sx)
        qx = ops.gene_quantiles(Sx, [50, 90])
        th.update(med_S=qx[0], p90_S=qx[1], med_U=ops.gene_quantiles(Ux, [50])[0], n_above=(Sx.t[:, :G].double() > qx[1][None, :]).sum(0))
        th["U_p10_above"] = ops.gene_quantiles(Ux, [10], mask_src=Sx, mask_thr=qx[1], mask_mode=1)[0]
        th["S_med_above"] = ops.gene_quantiles(Sx, [50], mask_src=Sx, mask_thr=qx[1], mask_mode=1)[0]
    if fixperc_q and not fit_offset:
        th["q_fixed"] = est._fixperc_q(Ux, Sx)
        th["p1_S"] = ops.gene_quantiles(Sx, [1])[0]
        th["n_below"] = (Sx.t[:, :G].double() <= th["p1_S"][None, :]).sum(0)
    return {k: v.cpu().numpy() for k, v in th.items()}, dense(Sx), dense(Ux), W


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


@pytest.mark.parametrize("i", range(2, len(FITS)))
def test_every_new_argument_against_the_facade(vcy, oracle, runs, facade, i):
    kw = dict(FITS[i])
    C = runs[1]["S"].shape[1]
    steady = np.arange(C) % 2 == 0 if kw.pop("steady", None) == "half" else None
    facade.R2 = None
    facade.fit_gammas(steady_state_bool=steady, **kw)
    th, Sn, Un, W = _facade_thresholds(vcy, facade, kw, None if steady is None else np.flatnonzero(steady))
    n, G = Sn.shape
    with np.errstate(all="ignore"):
        cond = np.array([oracle.fit_condition(Sn[:, g], Un[:, g], W[:, g]) for g in range(G)])
    kf, kr, sm, sq = cond.T
    u = 4 * n * fc.EPS
    bnd = dict(gammas=fc.FIT_K * u * kf * sm, q=fc.FIT_K * u * kf * sq, R2=fc.FIT_K_R2 * u * kr)
    for world in (1, 2):
        r = runs[0][world]
        got = _thr(r, i)
        assert set(got) == set(th), (world, set(got) ^ set(th))
        for name, v in th.items():
            assert _bits_equal(got[name], v), (world, name)
            assert _bits_equal(got[name], _thr(runs[0][1], i)[name]), (name, "world 2 against world 1")
        assert tuple(r[f"{i}_bytes"])[0] == -1 and (r[f"{i}_bytes"][1] > 0) == (world > 1)
        for name in ("gammas", "q", "R2"):
            ref = getattr(facade, name)
            if ref is None:                                 # the facade keeps no R2 on this branch
                continue
            a1, a2 = np.asarray(ref, dtype=np.float64), r[f"{i}_{name}"].astype(np.float64)
            assert np.array_equal(np.isfinite(a1), np.isfinite(a2)), (world, name)
            tol = np.fmax(_ulp32(a1), np.where(np.isnan(bnd[name]), 0.0, bnd[name]))
            same = (a1 == a2) | (np.isnan(a1) & np.isnan(a2))
            err = np.where(same, 0.0, np.abs(a2 - a1))
            worst = int(np.argmax(err / tol))
            print(f"{FITS[i]}, world {world}: {name}: {int((~same).sum())} genes differ, worst {err[worst]:.3g} against {tol[worst]:.3g}")
            assert np.all(err <= tol), (world, name, worst, a1[worst], a2[worst], tol[worst])


def test_unsupported_arguments_still_raise(runs):
    for world in (1, 2):
        assert runs[0][world]["refused"].tolist() == [1, 1, 1, 1, 1]
