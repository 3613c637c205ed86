"""Cell-sharded VelocytoLoom (velocyto_amd.sharded.ShardedLoom) and the pieces under it.

Kernels and exchanges in one process: the transposing pack / unpack of the gene-slice exchange (vcy_gene_slices_pack / _unpack)
with the all-to-all of three ranks emulated on one device, per-gene percentiles on gene slices against np.percentile, the
gene-offset shuffle of the randomised control (vcy_permute_rows_nsign_genes) against the whole matrix's, the two-step weighted
fit (vcy_fit_weighted_moments + vcy_fit_weighted_from_moments) against vcy_fit_weighted.

The whole chain at 1, 2 and 3 ranks (`python -m torch.distributed.run`, every rank on cuda:0, gloo) against the one-process
VelocytoLoom on the same input, and at 2 ranks against the reference's goldens.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def vcy():
    import velocyto_amd
    velocyto_amd.build()
    from velocyto_amd import ops
    ops.require_gpu()
    return velocyto_amd


def _bounds(sizes):
    b = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(b[i]), int(b[i + 1])) for i in range(len(sizes))]


def _emulated_exchange(ops, M_user, user_row, cell_sizes, gene_sizes, dtype):
    """The GeneSlices exchange of len(cell_sizes) ranks on one device, the all-to-alls done by slicing: returns (the slices each
    rank receives, the shards each rank gets back)."""
    dev = torch.device("cuda")
    C, G = M_user.shape[1], M_user.shape[0]
    cells, genes = _bounds(cell_sizes), _bounds(gene_sizes)
    run = M_user[:, user_row]                                           # (G, C) in the run's order
    shards = [ops.CellMatrix.from_genes_major(np.ascontiguousarray(run[:, a:b]), dtype) for a, b in cells]
    seg_cells = torch.tensor([0] + [b for _, b in cells], dtype=torch.int64, device=dev)
    urow = torch.from_numpy(user_row.astype(np.int64)).to(dev)
    sends = []
    for (a, b), sh in zip(cells, shards):
        seg = torch.tensor([0, b - a], dtype=torch.int64, device=dev)
        sends.append(ops.gene_slices_pack(sh, seg))
    slices = []
    for g0, g1 in genes:
        recv = torch.cat([buf[g0 * (b - a):g1 * (b - a)] for buf, (a, b) in zip(sends, cells)])
        slices.append(ops.gene_slices_unpack(recv, seg_cells, ops.CellMatrix.empty(C, g1 - g0, dtype), row_map=urow))
    backs = []
    packed = [ops.gene_slices_pack(sl, seg_cells, row_map=urow) for sl in slices]
    for a, b in cells:
        recv = torch.cat([buf[(g1 - g0) * a:(g1 - g0) * b] for buf, (g0, g1) in zip(packed, genes)])
        seg = torch.tensor([0, b - a], dtype=torch.int64, device=dev)
        backs.append(ops.gene_slices_unpack(recv, seg, ops.CellMatrix.empty(b - a, G, dtype)))
    return slices, backs, shards


def _awkward_matrix(rng, G, C):
    """Ties, all-zero genes, constant genes, signed zeros, a few large values."""
    M = rng.gamma(0.7, 2.0, (G, C)) * (rng.random((G, C)) < 0.4)
    M[3] = 0.0
    M[4] = 2.5
    M[5] = np.where(rng.random(C) < 0.5, -0.0, 0.0)
    M[6] = np.round(M[6])
    M[7, : C // 2] = -M[7, : C // 2]
    M[8, ::7] = 1e6
    return M


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_gene_slices_round_trip_and_percentiles(vcy, dtype):
    from velocyto_amd import ops
    rng = np.random.default_rng(7)
    G, C = 203, 517
    M = _awkward_matrix(rng, G, C)
    if dtype == "float32":
        M = M.astype(np.float32).astype(np.float64)
    user_row = rng.permutation(C)
    cell_sizes, gene_sizes = (1, 300, C - 301), (70, 1, G - 71)          # a rank with one cell, a slice of one gene
    slices, backs, shards = _emulated_exchange(ops, M, user_row, cell_sizes, gene_sizes, dtype)
    qs = [2, 98, 99.9, 100]
    whole = ops.gene_quantiles(ops.CellMatrix.from_genes_major(M, dtype), qs).cpu().numpy()
    for (g0, g1), sl in zip(_bounds(gene_sizes), slices):
        assert np.array_equal(sl.to_genes_major(), M[g0:g1]), "slice differs from the user-order genes"
        assert not torch.any(sl.t[:, sl.G:]), "padding columns of a slice are not zero"
        got = ops.gene_quantiles(sl, qs).cpu().numpy()
        # what fit_gammas relies on: the slice's percentiles are the whole matrix's, bit for bit (signed zeros included)
        assert np.array_equal(got.view(np.int64), whole[:, g0:g1].view(np.int64)), "percentiles on a gene slice differ from the whole matrix's"
        # and numpy's (its virtual index (n - 1) * (q / 100) may round differently from (n - 1) * q / 100 in the last bit)
        want = np.percentile(M[g0:g1].astype(np.float32 if dtype == "float32" else np.float64), qs, axis=1)
        # (numpy interpolates float32 data in float32, the kernel in float64)
        np.testing.assert_allclose(got, want, rtol=1e-13 if dtype == "float64" else 1e-7, atol=0)
    for sh, back in zip(shards, backs):
        assert torch.equal(sh.t[:, : sh.G], back.t[:, : back.G]), "round trip is not bit-equal"


@pytest.mark.parametrize("gene_major", [False, True])
def test_permute_on_gene_slices_equals_whole_matrix(vcy, gene_major):
    from velocyto_amd import ops
    rng = np.random.default_rng(11)
    G, C = 157, 1203
    M = rng.normal(size=(G, C))
    whole = ops.permute_rows_nsign(ops.CellMatrix.from_genes_major(M, "float64"), 15071990, gene_major=gene_major).to_genes_major()
    for g0, g1 in _bounds((40, 1, 116)):
        sl = ops.CellMatrix.from_genes_major(np.ascontiguousarray(M[g0:g1]), "float64")
        got = ops.permute_rows_nsign(sl, 15071990, gene_major=gene_major, gene0=g0).to_genes_major()
        assert np.array_equal(got, whole[g0:g1])


def _ulps32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    return np.where(same, 0, np.abs(ia - ib))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_weighted_fit_from_moments_of_three_blocks(vcy, dtype):
    from velocyto_amd import ops
    rng = np.random.default_rng(3)
    G, C = 300, 2001
    X = rng.gamma(1.2, 1.5, (G, C)) * (rng.random((G, C)) < 0.6)
    Y = 0.4 * X * rng.gamma(4.0, 0.25, (1, C)) + rng.gamma(0.8, 0.3, (G, C))
    X[0], Y[1] = 0.0, 0.0
    Xd, Yd = ops.CellMatrix.from_genes_major(X, dtype), ops.CellMatrix.from_genes_major(Y, dtype)
    dS = ops.gene_quantiles(Xd, [99.9])[0].clamp(min=1e-3)
    dU = ops.gene_quantiles(Yd, [99.9])[0].clamp(min=1e-3)
    q = ops.gene_quantiles(Xd, [2, 98], M2=Yd, scale_a=dS, scale_b=dU)
    w = dict(M=Xd, M2=Yd, scale_a=dS, scale_b=dU, down=q[0], up=q[1])
    g_ref, q_ref, r_ref = ops.fit_weighted(Yd, Xd, 1, fit_offset=True, box_q=True, lo_gamma=1e-8, up_gamma_default=20.0, **w)
    whole = ops.fit_weighted_moments(Yd, Xd, 1, **w)
    g1, q1, r1 = ops.fit_weighted_from_moments(whole, C)
    # one block: the composition IS vcy_fit_weighted
    bits = lambda t: t.cpu().numpy().view(np.int32)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in ((g1, g_ref), (q1, q_ref), (r1, r_ref)))
    mom = torch.zeros_like(whole)
    for a, b in _bounds((700, 1, C - 701)):
        blk = lambda m: ops.CellMatrix(m.t[a:b].contiguous(), m.G)
        mom += ops.fit_weighted_moments(blk(Yd), blk(Xd), 1, M=blk(Xd), M2=blk(Yd), scale_a=dS, scale_b=dU, down=q[0], up=q[1])
    np.testing.assert_allclose(mom.cpu().numpy(), whole.cpu().numpy(), rtol=1e-13, atol=1e-300)
    g3, q3, r3 = ops.fit_weighted_from_moments(mom, C)
    for got, ref in ((g3, g_ref), (q3, q_ref), (r3, r_ref)):
        assert _ulps32(got.cpu().numpy(), ref.cpu().numpy()).max() <= 1


@pytest.mark.parametrize("cull", [False, True])
def test_markov_step_of_three_target_ranges_equals_one_step(vcy, cull):
    """vcy_diffuse_step_factored_rows over three target ranges, assembled, is the full factored step bit for bit (two steps: the
    second full step starts from its fold, the ranged one from the state), with the culled transform and without."""
    from velocyto_amd import ops
    rng = np.random.default_rng(13)
    n, k = 5000, 30
    emb = rng.normal(size=(n, 2)) * np.array([40.0, 25.0])
    ixs = np.stack([rng.choice(n, k, replace=False) for _ in range(n)]).astype(np.int64)
    tp = rng.random((n, k))
    tp /= tp.sum(1, keepdims=True)
    indptr = np.arange(0, n * k + 1, k)
    # (sigma_D wide against the embedding: random neighbour lists keep non-zero rows; sigma_W narrow: the culled transform skips)
    tr = ops.prepare_markov_factored(indptr, ixs.ravel(), tp.ravel(), emb, 500.0, 4.0, compute_dtype=torch.float64, cull=cull)
    assert (tr.cull is not None) == cull
    x0 = rng.random(n)
    x0 /= x0.sum()
    xf, accf = ops.diffuse(x0, tr, 2, accumulate=True)
    assert bool(torch.isfinite(xf).all()) and bool(torch.isfinite(accf).all())
    x = torch.from_numpy(x0).cuda()
    acc = torch.zeros(n, dtype=torch.float64, device="cuda")
    cells = tr.target_order()
    for _ in range(2):
        y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        for t0, t1 in _bounds((1700, 1, n - 1701)):
            ops.diffuse_step_rows(tr, x, y, t0, t1, accum=acc)
        assert not torch.isnan(y[cells]).any()
        x = y
    assert np.array_equal(x.cpu().numpy().view(np.int64), xf.cpu().numpy().view(np.int64))
    assert np.array_equal(acc.cpu().numpy().view(np.int64), accf.cpu().numpy().view(np.int64))


def test_loom_constructor_equals_from_arrays(vcy, tmp_path):
    """ShardedLoom(loom_path, pcs, ts) reads the rank's cells from the file: the same layers as from_arrays (one rank, no process group)."""
    from velocyto_amd import loom_io
    from velocyto_amd.sharded import ShardedLoom
    g = np.load(os.path.join(GOLDEN, "pipeline.npz"))
    path = str(tmp_path / "p.loom")
    loom_io.write_loom(path, {"spliced": g["S"], "unspliced": g["U"]})
    a = ShardedLoom.from_arrays(g["S"], g["U"], g["pcs"], g["ts"], dtype="float64")
    b = ShardedLoom(path, g["pcs"], g["ts"], dtype="float64")
    for name in ("S", "U"):
        assert np.array_equal(a.gather(name), g[name]) and np.array_equal(b.gather(name), g[name])


def test_gene_slices_one_rank(vcy):
    """GeneSlices without a process group: the slice is the whole matrix in the user's order, and back."""
    from velocyto_amd import ops, distributed
    rng = np.random.default_rng(5)
    G, C = 77, 301
    M = rng.normal(size=(G, C))
    user = rng.permutation(C)
    run = ops.CellMatrix.from_genes_major(np.ascontiguousarray(M[:, user]), "float64")
    gs = distributed.GeneSlices(C, G, torch.from_numpy(user).cuda())
    sl = gs.to_slices(run)
    assert np.array_equal(sl.to_genes_major(), M)
    assert torch.equal(gs.from_slices(sl).t[:, :G], run.t[:, :G])


# ---------------------------------------------------------------------------------------------------------- the whole chain
PIPE = dict(k=12, n_pca_dims=10, n_neighbors=40, sampled_fraction=0.5)
SYNTH = dict(k=20, n_pca_dims=10, n_neighbors=150, sampled_fraction=0.3)


def synthetic(path, C=3001, G=1500, seed=2024):
    rng = np.random.default_rng(seed)
    lat = np.concatenate([rng.normal(c, 0.6, (n, 2)) for c, n in zip(((0, 0), (4, 1), (1, 5)), (C // 3, C // 3, C - 2 * (C // 3)))])
    pcs = np.concatenate([lat, 0.3 * rng.normal(size=(C, 10))], 1) @ rng.normal(size=(12, 12))
    a, b = rng.normal(-0.5, 1.0, (G, 1)), rng.normal(0.0, 0.6, (G, 2))
    rate = np.exp(np.clip(a + b @ lat.T, -6, 4))
    S = rng.poisson(rate).astype(np.uint16)
    U = rng.poisson(0.4 * rate * np.exp(0.3 * lat[:, :1].T)).astype(np.uint16)
    np.savez(path, S=S, U=U, pcs=pcs, ts=lat + 1e-3 * rng.normal(size=(C, 2)))


def run_chain(inp, out, world, cfg, port):
    env = dict(os.environ, VCY_SINGLE_DEVICE="1", VCY_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "sharded_chain_worker.py"), inp, out, json.dumps(cfg)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


def facade_chain(vcy, d, cfg, fit=None):
    from velocyto_amd import ops
    vlm = vcy.analysis.VelocytoLoom.from_arrays(d["S"], d["U"], dtype=cfg["dtype"])
    vlm.normalize("both", size=True, log=True)
    vlm.pcs, vlm.ts = d["pcs"], d["ts"]
    vlm.knn_imputation(k=cfg["k"], n_pca_dims=cfg["n_pca_dims"], n_jobs=1)
    vlm.fit_gammas()
    Sx, Ux = vlm.dev("Sx"), vlm.dev("Ux")
    q = ops.gene_quantiles(Sx, [99.9, 100]), ops.gene_quantiles(Ux, [99.9, 100])
    dS, dU = (torch.where(x[0] == 0, torch.clamp(x[1], min=0.001), x[0]) for x in q)
    thr = ops.gene_quantiles(Sx, [2, 98], M2=Ux, scale_a=dS, scale_b=dU)
    own_fit = {n: getattr(vlm, n).copy() for n in ("gammas", "q", "R2")}
    if fit is not None:
        # downstream of the fit both chains start from the SAME gammas / q (the sharded fit may differ by one float32 ulp: its f64
        # moments are summed in another order), so that every later difference is the later stages' own
        vlm.gammas, vlm.q = fit["gammas"], fit["q"]
    vlm.predict_U()
    vlm.calculate_velocity()
    vlm.calculate_shift()
    vlm.extrapolate_cell_at_t()
    vlm.estimate_transition_prob(hidim="Sx_sz", embed="ts", transform="sqrt", n_neighbors=cfg["n_neighbors"], knn_random=True,
                                 sampled_fraction=cfg["sampled_fraction"])
    vlm.calculate_embedding_shift(sigma_corr=0.05)
    st = vlm.__dict__
    res = {n: getattr(vlm, n) for n in ("S_sz", "U_sz", "Sx_sz", "Ux_sz", "Upred", "velocity", "delta_S", "delta_S_rndm", "Sx_sz_t",
                                       "sampling_ixs", "delta_embedding", "scaling")}
    res.update(own_fit)
    res["knn_indices"] = st["_graph_lazy"]["idx_s"].cpu().numpy()
    res["embedding_knn_indices"] = st["_neigh"].cpu().numpy()
    res["corrcoef"], res["corrcoef_random"] = st["_corr"].double().cpu().numpy(), st["_corr_random"].double().cpu().numpy()
    res["transition_prob"] = st["_tp"].double().cpu().numpy()
    res.update(thr_denom_S=dS.cpu().numpy(), thr_denom_U=dU.cpu().numpy(), thr_down=thr[0].cpu().numpy(), thr_up=thr[1].cpu().numpy())
    vlm.prepare_markov(sigma_D=2.0, sigma_W=4.0)
    vlm.run_markov(n_steps=50)
    res["diffused"] = vlm.diffused
    return res


def compare(sh, fa):
    for n in ("knn_indices", "embedding_knn_indices", "sampling_ixs", "S_sz", "U_sz", "Sx_sz", "Ux_sz",
              "thr_denom_S", "thr_denom_U", "thr_down", "thr_up"):
        assert np.array_equal(np.asarray(sh[n]), np.asarray(fa[n])), n
    for n in ("gammas", "q", "R2"):
        assert _ulps32(sh[n], fa[n]).max() <= 1, n
    for n in ("Upred", "velocity", "delta_S", "delta_S_rndm", "Sx_sz_t"):            # row-local from the same gammas: bit-equal
        assert np.array_equal(sh[n], fa[n]), n
    for n in ("corrcoef", "corrcoef_random"):
        np.testing.assert_allclose(sh[n], fa[n], atol=1e-9, err_msg=n)
    np.testing.assert_allclose(sh["transition_prob"], fa["transition_prob"], rtol=1e-8, atol=1e-13)
    np.testing.assert_allclose(sh["delta_embedding"], fa["delta_embedding"], rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(sh["scaling"], fa["scaling"], rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(sh["diffused"], fa["diffused"], rtol=1e-13, atol=0)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sharded")
    g = np.load(os.path.join(GOLDEN, "pipeline.npz"))
    pipe = str(d / "pipeline_in.npz")
    np.savez(pipe, S=g["S"], U=g["U"], pcs=g["pcs"], ts=g["ts"])
    syn = str(d / "synthetic_in.npz")
    synthetic(syn)
    return {"pipeline": (pipe, PIPE), "synthetic": (syn, SYNTH)}


@pytest.mark.parametrize("which,world", [("pipeline", 1), ("pipeline", 2), ("pipeline", 3), ("synthetic", 2), ("synthetic", 3)])
def test_sharded_chain_equals_facade(vcy, inputs, tmp_path, which, world):
    inp, cfg = inputs[which]
    cfg = dict(cfg, dtype="float64")
    sh = run_chain(inp, str(tmp_path / "out.npz"), world, cfg, port=29711 + 7 * world + (0 if which == "pipeline" else 3))
    assert int(sh["world"]) == world
    compare(sh, facade_chain(vcy, dict(np.load(inp)), cfg, fit=sh))


def test_sharded_chain_meets_the_goldens(vcy, inputs, tmp_path):
    inp, cfg = inputs["pipeline"]
    sh = run_chain(inp, str(tmp_path / "out.npz"), 2, dict(cfg, dtype="float64"), port=29771)
    g = np.load(os.path.join(GOLDEN, "pipeline.npz"))
    np.testing.assert_allclose(sh["S_sz"], g["S_sz"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(sh["Sx_sz"], g["Sx"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(sh["Ux_sz"], g["Ux"], rtol=1e-11, atol=1e-11)
    assert np.array_equal(sh["knn_indices"], np.sort(g["knn_indices"], 1))
    assert np.array_equal(sh["sampling_ixs"], g["sampling_ixs"])
    assert np.array_equal(sh["embedding_knn_indices"], g["neigh_ixs"])
    # the default fit is the exact box-constrained minimum, the reference's L-BFGS-B stops near it (tests/test_gpu_facade.py)
    ok = np.isclose(sh["gammas"], g["gammas"], rtol=1e-3, atol=1e-5)
    assert ok.mean() >= 0.95
