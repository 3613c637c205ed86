"""One rank of tests/test_gpu_balanced_routes.py's multi-rank runs (launched by `python -m torch.distributed.run`).

mode "sharded": ShardedLoom.knn_imputation(balanced=True) on an .npz input (S, U, pcs, ts, groups), once without and once with the
group constraint; rank 0 writes the gathered graph and pooled layers of both.
mode "atlas": AtlasPath(balanced=True) on the rank's own cells of the synthetic atlas; rank 0 writes the gathered graph rows (global
cell numbers), their weights and the pooled rows of the own cells.
Every rank runs on cuda:0 when VCY_SINGLE_DEVICE=1; the backend is VCY_DIST_BACKEND (gloo in the tests)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sharded_results(d, cfg):
    """{name: array} of both variants (every rank must call it).  Also what the test runs in-process for one rank."""
    from velocyto_amd.sharded import ShardedLoom
    sl = ShardedLoom.from_arrays(d["S"], d["U"], d["pcs"], d["ts"], dtype=cfg["dtype"])
    sl.normalize("both", size=True, log=True)
    res = {}
    for tag, constraint in (("free", None), ("grouped", d["groups"])):
        sl.knn_imputation(k=cfg["k"], n_pca_dims=cfg["n_pca_dims"], balanced=True, b_sight=cfg["b_sight"], b_maxl=cfg["b_maxl"],
                          group_constraint=constraint, n_jobs=1)
        for name in ("knn_indices", "Sx_sz", "Ux_sz"):
            res[f"{tag}_{name}"] = sl.gather(name)
        res[f"{tag}_rounds"] = np.array(sl.knn_stats["rounds"])
        res[f"{tag}_fell_back"] = np.array(sl.knn_stats["fell_back"])
    return res


def atlas_results(cfg, c0, c1):
    """(path, global graph rows (nloc, k + 1), pooled Sx rows of the own cells) of AtlasPath(balanced=True) on cells c0 .. c1 - 1."""
    import torch
    from velocyto_amd import atlas, ops
    dev = ops.require_gpu()
    C, G = cfg["C"], cfg["G"]
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(C, G, cfg["P"], dev, density=0.08, c0=c0, c1=c1)
    fS, fU = atlas.size_factors(totS, totU, C)
    path = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, c0=c0, C_total=C, k=cfg["k"], n_neighbors=cfg["n_neighbors"], sampled_fraction=0.5,
                           block_cells=0, balanced=True, b_sight=cfg["b_sight"], b_maxl=cfg["b_maxl"])
    local = path.g_idx[:path.nloc].long()                                   # numbering of the local count CSR: [own | k_out]
    rows = torch.cat([torch.arange(c0, c1, device=dev), path.k_out.long()])[local]
    Sx = ops.CellMatrix.empty(path.nloc, G, path.dtype)
    path._pool(path.cS, path.fS, slice(0, path.nloc), Sx)
    return path, rows, Sx


def main():
    mode, out, cfg = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0 if os.environ.get("VCY_SINGLE_DEVICE", "0") == "1" else int(os.environ.get("LOCAL_RANK", "0")))
    dist.init_process_group(os.environ.get("VCY_DIST_BACKEND", "gloo"), rank=rank, world_size=world)
    import velocyto_amd  # noqa: F401
    from velocyto_amd import distributed as D
    if mode == "sharded":
        res = sharded_results(dict(np.load(cfg["input"])), cfg)
    else:
        C = cfg["C"]
        c0, c1 = D.shard_bounds(C, world, rank)
        path, rows, Sx = atlas_results(cfg, c0, c1)
        res = {"rows": D.all_gather_rows(rows.contiguous(), C).cpu().numpy(),
               "weights": D.all_gather_rows(path.g_w[:path.nloc].contiguous(), C).cpu().numpy(),
               "Sx": D.all_gather_rows(Sx.t[:, :path.G].contiguous(), C).cpu().numpy(),
               "rounds": np.array(path.knn_stats["balance_rounds"])}
    res["world"] = np.array(world)
    if rank == 0:
        np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
