"""One rank of tests/test_gpu_masked_select.py's sharded run (launched by `python -m torch.distributed.run`): the masked streamed
select over the rank's own cells, in two blocks, under a value mask and a cell mask; rank 0 writes every rank's result and
populations to an .npz.  Every rank runs on cuda:0 when VCY_SINGLE_DEVICE=1; the backend is VCY_DIST_BACKEND (gloo in the tests)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_data(cfg):
    """(values, mask source, thresholds, cell mask) of all cells: the same on every rank and in the test."""
    rng = np.random.default_rng(cfg["seed"])
    C, G = cfg["C"], cfg["G"]
    B = np.asarray(rng.gamma(1.0, 1.0, (C, G)) * (rng.random((C, G)) < 0.7), dtype=np.float32)
    S = np.asarray(np.round(rng.gamma(1.0, 2.0, (C, G)) * (rng.random((C, G)) < 0.5), 1), dtype=np.float32)
    thr = np.percentile(S.astype(np.float64), 90, axis=0)
    thr[::7] = 1e30                                                   # genes without a kept cell
    return B, S, thr, rng.random(C) < 0.6


def main():
    out, cfg = sys.argv[1], json.loads(sys.argv[2])
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0 if os.environ.get("VCY_SINGLE_DEVICE", "0") == "1" else int(os.environ.get("LOCAL_RANK", "0")))
    dist.init_process_group(os.environ.get("VCY_DIST_BACKEND", "gloo"), rank=rank, world_size=world)
    import velocyto_amd  # noqa: F401
    from velocyto_amd import ops
    from velocyto_amd import distributed as D
    ops.require_gpu()
    B_np, S_np, thr_np, cells_np = make_data(cfg)
    c0, c1 = D.shard_bounds(cfg["C"], world, rank)
    B, S = ops.CellMatrix.from_cells_major(B_np[c0:c1], "float32"), ops.CellMatrix.from_cells_major(S_np[c0:c1], "float32")
    thr, cells = torch.from_numpy(thr_np).cuda(), torch.from_numpy(cells_np[c0:c1]).cuda()
    sel = ops.StreamedMaskedGeneQuantiles(cfg["G"], cfg["qs"], "float32")
    n, cut = c1 - c0, (c1 - c0) // 3
    while not sel.done:
        for (a, b) in ((cut, n), (0, cut)):
            sel.add_block(B.rows(a, b), S.rows(a, b), thr, cfg["mode"], cells[a:b])
        sel.advance()
    mine, cnt = sel.result().cpu(), sel.counts().cpu()
    every, every_n = [torch.empty_like(mine) for _ in range(world)], [torch.empty_like(cnt) for _ in range(world)]
    dist.all_gather(every, mine)
    dist.all_gather(every_n, cnt)
    if rank == 0:
        np.savez(out, result=torch.stack(every).numpy(), counts=torch.stack(every_n).numpy())
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
