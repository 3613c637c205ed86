"""One rank of tests/test_gpu_sharded_fit_options.py (launched by `python -m torch.distributed.run`): ShardedLoom up to knn_imputation on
an .npz input (S, U, pcs, ts), then fit_gammas once per configuration of the JSON list; rank 0 writes gammas, q, R2, the thresholds
and the exchange bytes of every configuration, and which of the unsupported calls raised NotImplementedError.  Every rank runs on
cuda:0 when VCY_SINGLE_DEVICE=1; the backend is VCY_DIST_BACKEND (gloo in the tests)."""
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
    res = {"world": np.array(sl.world), "C": np.array(sl.C)}
    # what the fit really hands to its all-reduces: every tensor that goes through distributed.all_reduce_sum while fit_gammas runs
    from velocyto_amd import distributed as D
    wire, plain_sum = [0], D.all_reduce_sum

    def counting_sum(t, group=None):
        if D.active():
            wire[0] += t.numel() * t.element_size()
        return plain_sum(t, group)
    D.all_reduce_sum = counting_sum
    for i, kw in enumerate(cfg["fits"]):
        kw = dict(kw)
        if kw.pop("steady", None) == "half":
            kw["steady_state_bool"] = np.arange(sl.C) % 2 == 0
        sl.exchange_bytes.pop("fit_select", None)
        sl.exchange_bytes.pop("gene_slices_fit", None)
        wire[0] = 0
        sl.fit_gammas(**kw)
        res[f"{i}_wire"] = np.array(wire[0])
        assert sl.steady_state.dtype == np.bool_ and sl.steady_state.shape == (sl.C,) and sl.steady_state.sum() == (sl.C if "steady_state_bool" not in kw else (sl.C + 1) // 2)
        for name in ("gammas", "q", "R2"):
            res[f"{i}_{name}"] = sl.gather(name)
        for k, v in sl.gather("fit_thresholds").items():
            res[f"{i}_thr_{k}"] = v
        res[f"{i}_bytes"] = np.array([sl.exchange_bytes.get("gene_slices_fit", -1), sl.exchange_bytes.get("fit_select", -1)])
    D.all_reduce_sum = plain_sum
    refused = []
    for kw in (dict(use_imputed_data=False), dict(use_size_norm=False), dict(weights=np.ones((sl.G, sl.C))),
               dict(steady_state_bool=np.arange(0, sl.C, 2)), dict(weights="sum", use_size_norm=False)):
        try:
            sl.fit_gammas(**kw)
            refused.append(0)
        except NotImplementedError:
            refused.append(1)
    res["refused"] = np.array(refused)
    if rank == 0:
        np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
