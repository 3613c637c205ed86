#!/usr/bin/env python3
"""Device t-SNE (DeviceTSNE, csrc/tsne.hip) and perform_TSNE's scikit-learn backend on 12 N(0, 1) blobs in 30 dimensions,
perplexity 30, 1000 iterations: fit wall time, the affinity stage alone, ms per iteration of the descent, and the repulsion's
issue bound per iteration from the kernel's own ISA (k_tsne_repulsion<2>: the compiler packs x / y, so a lane's pair is 5.5 plain
VALU instructions + 1 v_rcp_f32 = 5.5 x 4 + 8 = 30 cycles per 64 pairs per SIMD, 1024 SIMDs; the s_nop hazard padding, 1.4 per
pair, is not counted - see profiles/tsne_repulsion_isa.txt).
One JSON line per measurement.
usage: tools/bench_tsne.py [--sizes 10000 50000 100000] [--sklearn-sizes 10000 50000] [--ghz 2.4] [--out FILE]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats` with `--sklearn-sizes` (none)."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def blobs(n, seed=0, d=30, centers=12):
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 4.0, (centers, d))
    return c[rng.integers(0, centers, n)] + rng.normal(size=(n, d))


def issue_bound_ms(N, ghz, cycles_per_64_pairs=30.0, simds=1024):
    return N * (N - 1) / 64.0 * cycles_per_64_pairs / (simds * ghz * 1e9) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[10000, 50000, 100000])
    ap.add_argument("--sklearn-sizes", type=int, nargs="*", default=[10000, 50000])
    ap.add_argument("--ghz", type=float, default=2.4, help="shader clock assumed by the issue bound")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import velocyto_amd  # noqa: F401
    from velocyto_amd.preprocess import PreprocessMixin
    from velocyto_amd.tsne import DeviceTSNE
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    for N in a.sizes:
        Xd = torch.from_numpy(blobs(N)).cuda()
        DeviceTSNE(random_state=0, max_iter=250).fit_transform(Xd)          # warm-up at this size: code objects, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aff = DeviceTSNE(random_state=0)._affinities(Xd)
        torch.cuda.synchronize()
        t_aff = time.perf_counter() - t0
        nnz = int(aff["indices"].numel())
        del aff
        t = DeviceTSNE(random_state=0)
        t0 = time.perf_counter()
        t.fit_transform(Xd)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        iters = t.n_iter_ + 1
        emit(dict(what="DeviceTSNE.fit_transform", n=N, dims=30, perplexity=30, nnz_P=nnz, wall_s=round(wall, 4), affinities_s=round(t_aff, 4),
                  iterations=iters, ms_per_iter=round((wall - t_aff) * 1e3 / iters, 4), kl=t.kl_divergence_,
                  repulsion_issue_bound_ms=round(issue_bound_ms(N, a.ghz), 4), assumed_ghz=a.ghz))
    for N in a.sklearn_sizes:
        ns = types.SimpleNamespace(pcs=blobs(N))
        np.random.seed(0)
        t0 = time.perf_counter()
        PreprocessMixin.perform_TSNE(ns, backend="sklearn")
        emit(dict(what="perform_TSNE(backend='sklearn')", n=N, dims=30, perplexity=30, wall_s=round(time.perf_counter() - t0, 3),
                  omp_threads=os.environ.get("OMP_NUM_THREADS")))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
