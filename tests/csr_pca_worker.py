"""One rank of tests/test_gpu_csr_pca.py's sharded fits (launched by `python -m torch.distributed.run`): DevicePCA.fit_transform_csr on
the rank's own cells of the fixed synthetic input, the gathered scores and every rank's components written by rank 0 to an .npz.
Every rank runs on cuda:0 when VCY_SINGLE_DEVICE=1; the backend is VCY_DIST_BACKEND (gloo in the tests).

Also the home of the input generator (`make_input`), which the test module imports so that both sides draw the same matrix."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_input(C: int, G: int, r: int):
    """Counts with a low-rank log-rate (a gap behind the r-th component) and per-cell sizes; returns (S (C, G) int64, f (C,) float64)."""
    rng = np.random.Generator(np.random.PCG64(20180813))
    L = rng.normal(size=(C, r)) * np.linspace(2.0, 0.8, r)
    W = rng.normal(size=(r, G))
    base = rng.normal(-2.6, 1.0, size=G)
    size = np.exp(0.3 * rng.normal(size=C))
    S = rng.poisson(np.exp(base + 0.6 * L @ W) * size[:, None])
    # the log-normal rates have a tail: 19 of the 1.35 M entries at (1500, 900) and 10 at (700, 1200) come out above 65535, the largest count
    # a layer holds (uint16, as in a loom file; atlas.synth_atlas clamps likewise).  Clamped BEFORE the totals, so that every route -
    # the device's, the dense one and scikit-learn's - sees the same counts and the same size factors
    S = np.minimum(S, 65535)
    total = S.sum(1)
    f = total.mean() / np.maximum(total, 1)
    return S, f


def main():
    out, cfg = sys.argv[1], json.loads(sys.argv[2])
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0 if os.environ.get("VCY_SINGLE_DEVICE", "0") == "1" else int(os.environ.get("LOCAL_RANK", "0")))
    dist.init_process_group(os.environ.get("VCY_DIST_BACKEND", "gloo"), rank=rank, world_size=world)
    import scipy.sparse as sp
    import velocyto_amd  # noqa: F401
    from velocyto_amd import distributed as D
    from velocyto_amd import ops
    from velocyto_amd.preprocess import DevicePCA
    S, f = make_input(cfg["C"], cfg["G"], cfg["r"])
    c0, c1 = D.shard_bounds(cfg["C"], world, rank)
    counts = ops.CsrCounts.from_scipy(sp.csr_matrix(S[c0:c1]), G=cfg["G"])
    pca = DevicePCA(n_components=cfg["k"])
    pcs = pca.fit_transform_csr(counts, f[c0:c1], pcount=cfg["pcount"])
    assert pcs.shape == (c1 - c0, cfg["k"]) and pca.n_samples_ == cfg["C"]
    pcs_all = D.all_gather_rows(pcs.contiguous(), cfg["C"])
    comps = torch.as_tensor(pca.components_)
    every = [torch.empty_like(comps) for _ in range(world)]
    dist.all_gather(every, comps)
    if rank == 0:
        np.savez(out, pcs=pcs_all.cpu().numpy(), components_every_rank=torch.stack(every).numpy(), explained_variance=pca.explained_variance_,
                 explained_variance_ratio=pca.explained_variance_ratio_, mean=pca.mean_, n_iter=np.array(pca.n_iter_), world=np.array(world))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
