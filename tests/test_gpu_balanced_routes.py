"""Balanced kNN pooling on the two routes built for scale: ShardedLoom.knn_imputation(balanced=True) against the facade's, and
AtlasPath(balanced=True) against rows built from the host BalancedKNN result - on one rank in this process and on two ranks
(`python -m torch.distributed.run`, every rank on cuda:0, gloo) through tests/balanced_routes_worker.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import balanced_routes_worker as worker

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHARDED = dict(k=12, n_pca_dims=10, b_sight=48, b_maxl=20, dtype="float64")
ATLAS = dict(C=701, G=300, P=10, k=12, b_sight=48, b_maxl=20, n_neighbors=100)


@pytest.fixture(scope="module")
def vcy():
    import velocyto_amd
    velocyto_amd.build()
    from velocyto_amd import ops
    ops.require_gpu()
    return velocyto_amd


def run_worker(mode, world, out, cfg, port):
    env = dict(os.environ, VCY_SINGLE_DEVICE="1", VCY_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "balanced_routes_worker.py"), mode, out, json.dumps(cfg)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = dict(np.load(out))
    assert int(res["world"]) == world
    return res


# ---------------------------------------------------------------------------------------------------------------- ShardedLoom
def write_input(name, path):
    """An input tests/test_gpu_sharded.py builds ("pipeline": the golden pipeline; "synthetic": its 3001 x 1500 counts) plus three groups
    dealt at random: a sight of 48 then holds about 16 cells of a cell's own group, so part of the constrained rows run out of sight and
    are padded."""
    if name == "pipeline":
        g = np.load(os.path.join(GOLDEN, "pipeline.npz"))
        data = dict(S=g["S"], U=g["U"], pcs=g["pcs"], ts=g["ts"])
    else:
        from test_gpu_sharded import synthetic
        synthetic(path)
        data = dict(np.load(path))
    data["groups"] = np.random.default_rng(48).integers(0, 3, data["pcs"].shape[0])
    np.savez(path, **data)
    return data


@pytest.fixture(scope="module", params=["pipeline", "synthetic"])
def sharded_input(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("balanced") / f"{request.param}_in.npz")
    return path, write_input(request.param, path)


@pytest.fixture(scope="module")
def facade(vcy, sharded_input):
    """The facade's knn_imputation with the same arguments, and the host BalancedKNN graph it pools over."""
    from velocyto_amd.neighbors import BalancedKNN
    _, d = sharded_input
    res = {}
    for tag, constraint in (("free", None), ("grouped", d["groups"])):
        vlm = vcy.analysis.VelocytoLoom.from_arrays(d["S"], d["U"], dtype=SHARDED["dtype"])
        vlm.normalize("both", size=True, log=True)
        vlm.pcs, vlm.ts = d["pcs"], d["ts"]
        vlm.knn_imputation(k=12, n_pca_dims=10, balanced=True, b_sight=48, b_maxl=20, group_constraint=constraint, n_jobs=1)
        res[f"{tag}_Sx_sz"], res[f"{tag}_Ux_sz"] = np.array(vlm.Sx_sz), np.array(vlm.Ux_sz)
        _, dsi_new, _ = BalancedKNN(k=12, sight_k=48, maxl=20, constraint=constraint).fit(d["pcs"][:, :10]).kneighbors()
        res[f"{tag}_knn_indices"] = np.sort(dsi_new[:, 1:], 1)
        res[f"{tag}_padded"] = (dsi_new[:, 1:] == np.arange(dsi_new.shape[0])[:, None]).any(1)
    return res


def check_sharded(sh, fa):
    assert not fa["free_padded"].any() and fa["grouped_padded"].any() and not fa["grouped_padded"].all()     # both kinds of row are met
    for tag in ("free", "grouped"):
        assert not bool(sh[f"{tag}_fell_back"]) and int(sh[f"{tag}_rounds"]) >= 2
        for name in ("knn_indices", "Sx_sz", "Ux_sz"):
            assert np.array_equal(np.asarray(sh[f"{tag}_{name}"]), fa[f"{tag}_{name}"]), (tag, name)
    assert not np.array_equal(sh["free_Sx_sz"], sh["grouped_Sx_sz"])


def test_sharded_balanced_one_rank_equals_facade(vcy, sharded_input, facade):
    _, d = sharded_input
    check_sharded(worker.sharded_results(d, SHARDED), facade)


def test_sharded_balanced_two_ranks_equal_facade(vcy, sharded_input, facade, tmp_path):
    path, _ = sharded_input
    port = 29931 if path.endswith("pipeline_in.npz") else 29933
    check_sharded(run_worker("sharded", 2, str(tmp_path / "out.npz"), dict(SHARDED, input=path), port=port), facade)


def test_sharded_balanced_arguments(vcy, tmp_path):
    from velocyto_amd.sharded import ShardedLoom
    d = write_input("pipeline", str(tmp_path / "in.npz"))
    sl = ShardedLoom.from_arrays(d["S"], d["U"], d["pcs"], d["ts"], dtype="float64")
    sl.normalize("both", size=True, log=True)
    with pytest.raises(NotImplementedError):
        sl.knn_imputation(k=12, n_pca_dims=10, group_constraint=d["groups"])           # a constraint needs balanced=True
    sl.cluster_ix = d["groups"]
    sl.knn_imputation(k=12, n_pca_dims=10, balanced=True, b_sight=48, b_maxl=20, group_constraint="clusters")
    by_name = sl.gather("knn_indices")
    sl.knn_imputation(k=12, n_pca_dims=10, balanced=True, b_sight=48, b_maxl=20, group_constraint=d["groups"])
    assert np.array_equal(by_name, sl.gather("knn_indices"))
    # the facade's defaults: sight and cap of the whole dataset - the cap never binds, the graph is the plain one, two rounds
    sl.knn_imputation(k=12, n_pca_dims=10, balanced=True)
    balanced = sl.gather("knn_indices")
    assert sl.knn_stats == {"rounds": 2, "fell_back": False}
    sl.knn_imputation(k=12, n_pca_dims=10)
    assert np.array_equal(balanced, sl.gather("knn_indices"))


# ------------------------------------------------------------------------------------------------------------------ AtlasPath
@pytest.fixture(scope="module")
def atlas_one(vcy):
    return worker.atlas_results(ATLAS, 0, ATLAS["C"])


def test_atlas_balanced_rows_equal_host_balanced_knn(vcy, atlas_one):
    from velocyto_amd import ops
    from velocyto_amd.neighbors import BalancedKNN
    path, rows, Sx = atlas_one
    C, k, dev = ATLAS["C"], ATLAS["k"], path.dev
    dist_new, dsi_new, _ = BalancedKNN(k=k, sight_k=ATLAS["b_sight"], maxl=ATLAS["b_maxl"]).fit(path._pcs_full.cpu().numpy()).kneighbors()
    assert np.array_equal(dsi_new[:, 0], np.arange(C))
    conn = torch.from_numpy(dist_new[:, 1:] > 0).to(dev, path.dtype)
    w = torch.cat([torch.ones((C, 1), device=dev, dtype=path.dtype), conn], 1)
    w = w / w.sum(1, keepdim=True)
    ind, w = ops.canonical_graph_rows(torch.from_numpy(dsi_new).to(dev, torch.int32), w)
    assert rows.dtype == torch.int64 and torch.equal(rows, ind.long()) and torch.equal(path.g_idx.long(), ind.long())
    assert torch.equal(path.g_w.view(torch.int32), w.view(torch.int32))
    assert not path.knn_stats["balance_fell_back"] and path.knn_stats["balance_rounds"] >= 3          # the cap of 20 binds on this data
    # one pooled block against dense pooling over those rows
    ptr = torch.arange(0, (C + 1) * (k + 1), k + 1, device=dev, dtype=torch.int64)
    ref, _ = ops.knn_pool_counts(path.cS.to_dense(), path.cU.to_dense(), path.fS, path.fU, ptr, ind, w, dtype=path.dtype, validate=False)
    assert torch.equal(Sx.t, ref.t)
    path.run()
    assert torch.equal(path._resident[0].t[:C], ref.t)


def test_atlas_unbalanced_is_unchanged_and_differs(vcy, atlas_one):
    from velocyto_amd import atlas, ops
    dev = ops.require_gpu()
    C, G = ATLAS["C"], ATLAS["G"]
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(C, G, ATLAS["P"], dev, density=0.08)
    fS, fU = atlas.size_factors(totS, totU, C)
    kw = dict(k=ATLAS["k"], n_neighbors=ATLAS["n_neighbors"], sampled_fraction=0.5, block_cells=0)
    plain = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, **kw)
    off = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, balanced=False, **kw)
    assert torch.equal(plain.g_idx, off.g_idx) and torch.equal(plain.g_w.view(torch.int32), off.g_w.view(torch.int32))
    assert torch.equal(torch.nan_to_num(plain.run(), nan=7.0), torch.nan_to_num(off.run(), nan=7.0))
    assert off.knn_stats == plain.knn_stats == {}
    assert not torch.equal(plain.g_idx, atlas_one[0].g_idx)
    with pytest.raises(ValueError):
        atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, group_constraint=np.zeros(C), **kw)
    # the sight lists through the pruned search (the route from PRUNE_FROM cells on, self column prepended): the same graph
    pruned = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, knn="pruned", balanced=True, b_sight=48, b_maxl=20, **kw)
    assert torch.equal(pruned.g_idx, atlas_one[0].g_idx) and torch.equal(pruned.g_w.view(torch.int32), atlas_one[0].g_w.view(torch.int32))
    assert pruned.knn_stats["balance_rounds"] == atlas_one[0].knn_stats["balance_rounds"] and "distance_evaluations" in pruned.knn_stats
    # a constraint: picks stay inside the group
    groups = torch.arange(C, device=dev) % 2
    con = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, balanced=True, b_sight=48, b_maxl=20, group_constraint=groups, **kw)
    used = con.g_w > 0
    assert bool((groups[con.g_idx.long()] == groups[:, None])[used].all()) and int(used.sum(1).min()) >= 2
    plan = atlas.memory_plan(1_000_000, 30_000, 2400, 8, 0, b_sight=240)
    assert plan["balanced_sight_lists_GB"] == pytest.approx(1_000_000 * 241 * 4 / 1e9)
    assert plan["total_GB"] == pytest.approx(atlas.memory_plan(1_000_000, 30_000, 2400, 8, 0)["total_GB"] + plan["balanced_sight_lists_GB"])


def test_atlas_balanced_two_ranks_equal_one_rank(vcy, atlas_one, tmp_path):
    path, rows, Sx = atlas_one
    two = run_worker("atlas", 2, str(tmp_path / "out.npz"), ATLAS, port=29937)
    assert np.array_equal(two["rows"], rows.cpu().numpy())
    assert np.array_equal(two["weights"].view(np.int32), path.g_w.cpu().numpy().view(np.int32))
    assert np.array_equal(two["Sx"], Sx.t[:, :path.G].cpu().numpy())
    assert int(two["rounds"]) == path.knn_stats["balance_rounds"]
