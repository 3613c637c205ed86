"""One rank of tests/test_gpu_atlas_shift.py's sharded runs (launched by `python -m torch.distributed.run`): AtlasPath(shift=True) on the
rank's own cells of the synthetic atlas; rank 0 writes the gathered correlation rows, fit, neighbour lists and stage-E results to an
.npz.  Every rank runs on cuda:0 when VCY_SINGLE_DEVICE=1; the backend is VCY_DIST_BACKEND (gloo in the tests)."""
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
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(C, G, cfg["P"], dev, density=0.08, c0=c0, c1=c1)
    fS, fU = atlas.size_factors(totS, totU, C)
    path = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, c0=c0, C_total=C, k=cfg["k"], n_neighbors=cfg["n_neighbors"], sampled_fraction=0.5,
                           block_cells=cfg["block_cells"], dtype=getattr(torch, cfg["dtype"]), fit=cfg["fit"], shift=True, sigma_corr=cfg["sigma_corr"])
    path.run()
    de, scaling = path.gathered_shift()
    every = dict(corr=path.gathered_corr(), neigh=D.all_gather_rows(path.neigh, C), tp=D.all_gather_rows(path.tp, C), delta_embedding=de, scaling=scaling,
                 delta_embedding_unscaled=D.all_gather_rows(path.delta_embedding_unscaled, C))
    if rank == 0:
        np.savez(out, gamma=path.gamma.cpu().numpy(), q=(path.q if path.q is not None else torch.zeros(0)).cpu().numpy(),
                 blocks=np.array(len(path.blocks())), world=np.array(world), **{n: v.cpu().numpy() for n, v in every.items()})
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
