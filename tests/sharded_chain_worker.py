"""One rank of tests/test_gpu_sharded.py's chain runs (launched by `python -m torch.distributed.run`): the whole ShardedLoom chain on
an .npz input (S, U, pcs, ts), every gathered result written by rank 0 to the output .npz.  Every rank runs on cuda:0 when
VCY_SINGLE_DEVICE=1; the backend is VCY_DIST_BACKEND (gloo in the tests)."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    inp, out, cfg = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0 if os.environ.get("VCY_SINGLE_DEVICE", "0") == "1" else int(os.environ.get("LOCAL_RANK", "0")))
    dist.init_process_group(os.environ.get("VCY_DIST_BACKEND", "gloo"), rank=rank, world_size=world)
    import velocyto_amd  # noqa: F401
    from velocyto_amd.sharded import ShardedLoom
    d = np.load(inp)
    sl = ShardedLoom.from_arrays(d["S"], d["U"], d["pcs"], d["ts"], dtype=cfg["dtype"])
    sl.normalize("both", size=True, log=True)
    sl.knn_imputation(k=cfg["k"], n_pca_dims=cfg["n_pca_dims"], n_jobs=1)
    sl.fit_gammas()
    sl.predict_U()
    sl.calculate_velocity()
    sl.calculate_shift()
    sl.extrapolate_cell_at_t()
    sl.estimate_transition_prob(hidim="Sx_sz", embed="ts", transform="sqrt", n_neighbors=cfg["n_neighbors"], knn_random=True,
                                sampled_fraction=cfg["sampled_fraction"])
    sl.calculate_embedding_shift(sigma_corr=0.05)
    sl.prepare_markov(sigma_D=2.0, sigma_W=4.0)
    sl.run_markov(n_steps=50)
    res = {}
    for name in ("S_sz", "U_sz", "Sx_sz", "Ux_sz", "Upred", "velocity", "delta_S", "delta_S_rndm", "Sx_sz_t", "gammas", "q", "R2",
                 "knn_indices", "embedding_knn_indices", "sampling_ixs", "delta_embedding", "scaling", "diffused"):
        res[name] = sl.gather(name)
    for name in ("corrcoef", "corrcoef_random", "transition_prob"):
        res[name], _ = sl.gather(name)
    for k, v in sl.gather("fit_thresholds").items():
        res["thr_" + k] = v
    res["world"] = np.array(sl.world)
    if rank == 0:
        np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
