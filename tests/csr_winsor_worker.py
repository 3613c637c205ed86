"""One rank of tests/test_gpu_csr_winsor.py's sharded run (launched by `python -m torch.distributed.run`): the winsorised gene
selection of the atlas route on the rank's own cells of tests/csr_winsor_cases.selection_dataset; every rank's arrays gathered and
written by rank 0 to an .npz.  Every rank runs on cuda:0 when VCY_SINGLE_DEVICE=1; the backend is VCY_DIST_BACKEND (gloo in the tests).

Also the home of the route itself (`winsor_route`), which the test module imports so that the one-rank run and the ranks run the
same calls on the same counts."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csr_winsor_cases as cases  # noqa: E402

PERC = (1, 99.5)


def winsor_route(atlas, cS, mask):
    """Every new function of the route once; returns a dict of float64 / bool numpy arrays."""
    out = {}
    out["percentiles"] = atlas.gene_percentiles(cS, cases.Q16)
    out["percentiles_masked"] = atlas.gene_percentiles(cS, PERC, mask)
    out["moments"], out["bounds"] = atlas.winsorized_gene_stats(cS, PERC)
    out["moments_masked"], out["bounds_masked"] = atlas.winsorized_gene_stats(cS, (2.5, 97.25), mask)
    out["cv_score"], out["cv_selected"] = atlas.score_cv_vs_mean(cS, N=cases.N_CV, max_expr_avg=40, winsor_perc=PERC)
    return out


def cell_mask(C):
    return np.arange(C) % 7 != 3


def main():
    out = sys.argv[1]
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0 if os.environ.get("VCY_SINGLE_DEVICE", "0") == "1" else int(os.environ.get("LOCAL_RANK", "0")))
    dist.init_process_group(os.environ.get("VCY_DIST_BACKEND", "gloo"), rank=rank, world_size=world)
    import scipy.sparse as sp
    import velocyto_amd  # noqa: F401
    from velocyto_amd import atlas, ops
    from velocyto_amd import distributed as D
    S, _ = cases.selection_dataset()
    c0, c1 = D.shard_bounds(S.shape[0], world, rank)
    cS = ops.CsrCounts.from_scipy(sp.csr_matrix(S[c0:c1]), G=S.shape[1])
    assert (cS.code == ops.U16) == (rank == 0), "only the first shard was meant to hold a count above 255"
    res = winsor_route(atlas, cS, cell_mask(S.shape[0])[c0:c1])
    gathered = {}
    for name, v in res.items():                              # every rank's copy, to be compared with the one-rank run and with each other
        t = torch.as_tensor(np.ascontiguousarray(v).astype(np.float64))
        every = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(every, t)
        gathered[name] = torch.stack(every).numpy()
    if rank == 0:
        np.savez(out, world=np.array(world), **gathered)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
