"""One rank of tests/test_gpu_atlas_fit_options.py's sharded runs (launched by `python -m torch.distributed.run`):
AtlasPath(fit="maxmin_diag", **options) on the rank's own cells of the synthetic atlas; rank 0 writes every rank's thresholds and fit
and the gathered correlation rows to an .npz.  cfg["steady"] = "half" masks every second cell (a mask over ALL cells, which each rank
cuts to its own).  Every rank runs on cuda:0 when VCY_SINGLE_DEVICE=1; the backend is VCY_DIST_BACKEND (gloo in the tests)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    out, cfg = sys.argv[1], json.loads(sys.argv[2])
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0 if os.environ.get("VCY_SINGLE_DEVICE", "0") == "1" else int(os.environ.get("LOCAL_RANK", "0")))
    dist.init_process_group(os.environ.get("VCY_DIST_BACKEND", "gloo"), rank=rank, world_size=world)
    import velocyto_amd  # noqa: F401
    from velocyto_amd import atlas, ops
    from velocyto_amd import distributed as D
    dev = ops.require_gpu()
    C, G = cfg["C"], cfg["G"]
    c0, c1 = D.shard_bounds(C, world, rank)
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(C, G, cfg["k"], dev, density=0.08, c0=c0, c1=c1)
    fS, fU = atlas.size_factors(totS, totU, C)
    steady = (np.arange(C) % 2 == 0) if cfg.get("steady") == "half" else None
    path = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, c0=c0, C_total=C, k=cfg["k"], n_neighbors=cfg["n_neighbors"], sampled_fraction=0.5,
                           block_cells=cfg["block_cells"], fit="maxmin_diag", dtype=getattr(torch, cfg["dtype"]), steady_state_bool=steady,
                           **cfg["options"])
    path.run()
    corr = path.gathered_corr()
    names = sorted(path.fit_thresholds)
    mine = torch.stack([*(path.fit_thresholds[n].double() for n in names), path.gamma.double(), path.q.double(), path.R2.double()]).cpu()
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    if rank == 0:
        np.savez(out, per_gene_every_rank=torch.stack(every).numpy(), names=np.array(names + ["gamma", "q", "R2"]), corr=corr.cpu().numpy(),
                 moments=path.fit_moments.cpu().numpy(), n_fit_cells=np.array(path.n_fit_cells))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
