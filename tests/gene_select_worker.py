"""One rank of tests/test_gpu_csr_select.py's sharded gene selection (launched by `python -m torch.distributed.run`): the atlas
route's score_* functions and default_gene_filter on the rank's own cells of the fixed dataset; every rank's masks, scores and kept
list gathered and written by rank 0 to an .npz.  Every rank runs on cuda:0 when VCY_SINGLE_DEVICE=1; the backend is
VCY_DIST_BACKEND (gloo in the tests).

Also the home of the dataset (`make_dataset`) and of the route itself (`atlas_route`), which the test module imports so that the
one-rank run and the ranks run the same calls on the same counts."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (30, 200, 370)          # cells per cluster: the first is under size_limit = 40
N_CV = 300
DETECTION = dict(min_expr_counts=30, min_cells_express=15)


def make_dataset():
    """(S, U, cluster_ix): Poisson counts, (cells, genes) = (600, 2500) int64, with all-zero genes, genes expressed in one or two cells
    and cluster-specific genes.  Cells are ordered so that the LAST third holds no cell of cluster 0 or 1 (a shard of a 3-rank run
    without any cell of a cluster) while clusters 0 and 1 interleave in front."""
    rng = np.random.Generator(np.random.PCG64(20180815))
    C, G = sum(SIZES), 2500
    ix = np.concatenate([rng.permutation(np.repeat([0, 1, 2], [SIZES[0], SIZES[1], 170])), np.full(200, 2)])
    assert ix.size == C and tuple(np.bincount(ix)) == SIZES and set(ix[400:]) == {2}
    rate = np.exp(rng.normal(-1.2, 1.1, G))
    fold = np.exp(0.8 * rng.normal(size=(3, G)) * (rng.random((3, G)) < 0.3))
    size = np.exp(0.25 * rng.normal(size=C))
    lam = rate[None, :] * fold[ix] * size[:, None]
    S = rng.poisson(lam)
    U = rng.poisson(0.35 * lam)
    S[:, :40] = 0                                            # never seen
    U[:, :40] = 0
    U[:, 40:60] = 0                                          # spliced only
    for g in range(60, 100):                                 # expressed in one or two cells
        S[:, g] = 0
        S[rng.choice(C, 1 + g % 2, replace=False), g] = rng.integers(1, 60)
    S[:, 100:110] = rng.poisson(55.0, (C, 10))               # house-keeping-like: above max_expr_avg = 40
    return S.astype(np.int64), U.astype(np.int64), ix.astype(np.int64)


def atlas_route(atlas, cS, cU, ix, n_clusters):
    """Every function of the route once, in the facade's order; returns a dict of numpy arrays."""
    out = {}
    det = atlas.score_detection_levels(cS, cU, **DETECTION)
    out["detection"] = det
    dS, dU = atlas.select_genes(det, cS, cU)
    out["cv_score"], out["cv_selected"] = atlas.score_cv_vs_mean(dS, N=N_CV, max_expr_avg=40)
    out["U_avgs"], out["S_avgs"], out["clu_selected"] = atlas.score_cluster_expression(dS, dU, ix, n_clusters)
    fS, fU, kept = atlas.default_gene_filter(cS, cU, ix, n_clusters, N=N_CV, **DETECTION)
    out["kept"] = kept
    out["kept_row_sums"] = np.stack([fS.row_sums().cpu().numpy(), fU.row_sums().cpu().numpy()])
    assert fS.G == fU.G == kept.size and kept.dtype == np.int64
    return out


def main():
    out, cfg = sys.argv[1], json.loads(sys.argv[2])
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0 if os.environ.get("VCY_SINGLE_DEVICE", "0") == "1" else int(os.environ.get("LOCAL_RANK", "0")))
    dist.init_process_group(os.environ.get("VCY_DIST_BACKEND", "gloo"), rank=rank, world_size=world)
    import scipy.sparse as sp
    import velocyto_amd  # noqa: F401
    from velocyto_amd import atlas, ops
    from velocyto_amd import distributed as D
    S, U, ix = make_dataset()
    c0, c1 = D.shard_bounds(S.shape[0], world, rank)
    if cfg.get("expect_missing_cluster") and rank == world - 1:
        assert 0 not in set(ix[c0:c1]), "the last shard was meant to hold no cell of cluster 0"
    cS = ops.CsrCounts.from_scipy(sp.csr_matrix(S[c0:c1]), G=S.shape[1])
    cU = ops.CsrCounts.from_scipy(sp.csr_matrix(U[c0:c1]), G=U.shape[1])
    res = atlas_route(atlas, cS, cU, ix[c0:c1], 3)
    rows = D.all_gather_rows(torch.as_tensor(res.pop("kept_row_sums").T.copy(), device=cS.indptr.device), S.shape[0])
    gathered = {}
    for name, v in res.items():                              # every rank's copy, to be compared with the one-rank run and with each other
        t = torch.as_tensor(np.ascontiguousarray(v).astype(np.float64) if v.dtype == bool else np.ascontiguousarray(v))
        every = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(every, t)
        gathered[name] = torch.stack(every).numpy()
    if rank == 0:
        np.savez(out, world=np.array(world), kept_row_sums=rows.cpu().numpy().T, **gathered)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
