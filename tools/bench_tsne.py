#!/usr/bin/env python3
"""Device t-SNE (DeviceTSNE, csrc/tsne.hip) and perform_TSNE's scikit-learn backend on 12 N(0, 1) blobs in 30 dimensions,
perplexity 30, 1000 iterations: fit wall time, the affinity stage alone, ms per iteration of the descent, and the repulsion's
issue bound per iteration from the kernel's own ISA (k_tsne_repulsion<2>: the compiler packs x / y, so a lane's pair is 5.5 plain
VALU instructions + 1 v_rcp_f32 = 5.5 x 4 + 8 = 30 cycles per 64 pairs per SIMD, 1024 SIMDs; the s_nop hazard padding, 1.4 per
pair, is not counted - see profiles/tsne_repulsion_isa.txt).
One JSON line per measurement.
--repulsion tree runs the fits with the Barnes-Hut tree repulsion (--angle, --depth).  --step-sizes N .. times single iterations
instead of fits: on the embedding of iteration 300 of a tree fit, ten iterations of the tree step (keys + sort + step, at the
automatic depth and one either side) and ten of the exact step, alternating in blocks of five; the parts of a tree iteration
(keys, sort, build + traversal, all with a synchronise after each), and the accepted nodes and direct pairs per target.
usage: tools/bench_tsne.py [--sizes 10000 50000 100000] [--sklearn-sizes 10000 50000] [--ghz 2.4] [--out FILE]
                           [--repulsion exact|tree] [--angle 0.5] [--depth D] [--step-sizes 50000 1000000] [--step-depths 8 9] [--no-exact-above N]
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


def step_bench(N, a, emit):
    """Single iterations at N points on the embedding of iteration 300 of a tree fit (see the module docstring)."""
    import torch
    from velocyto_amd import _lib, ops
    from velocyto_amd.tsne import DeviceTSNE
    sync = torch.cuda.synchronize
    X = torch.from_numpy(blobs(N)).cuda()
    t = DeviceTSNE(random_state=0, repulsion="tree", angle=a.angle, tree_depth=a.depth)
    t._check_params(tuple(X.shape))
    t.learning_rate_ = max(N / t.early_exaggeration / 4, 50)
    t0 = time.perf_counter()
    aff = t._affinities(X)
    sync()
    t_aff = time.perf_counter() - t0
    indptr, indices, P = aff["indptr"], aff["indices"], aff["P"]
    del aff, X
    Y = torch.from_numpy(t._initial_embedding(N)).cuda()
    t0 = time.perf_counter()
    Y, _, it = t._gradient_descent(Y, (indptr, indices, (P * t.early_exaggeration).to(torch.float32)), 0, 250, 0.5, 250)
    pval = P.to(torch.float32)
    del P
    Y, kl, it = t._gradient_descent(Y, (indptr, indices, pval), it + 1, 300, 0.8, 300)
    sync()
    emit(dict(what="tree fit to iteration 300", n=N, angle=a.angle, affinities_s=round(t_aff, 3), descent_s=round(time.perf_counter() - t0, 3),
              kl=kl, nnz_P=int(indices.numel())))
    Y300 = Y.clone()
    auto = ops.tsne_tree_depth(N)
    depths = a.step_depths or [d for d in (auto - 1, auto, auto + 1) if 1 <= d <= 11]
    lr = float(t.learning_rate_)
    state = lambda: (torch.zeros((N, 2), dtype=torch.float64, device="cuda"), torch.ones((N, 2), device="cuda"),
                     torch.zeros(4, dtype=torch.float64, device="cuda"))
    with_exact = N <= a.no_exact_above
    ws_x = ops.tsne_workspace(N, 2) if with_exact else None

    def run(mode, n, Ya, Yb, st, depth=None, tws=None):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            if mode == "tree":
                _, order, skeys = ops.tsne_tree_keys(Ya, tws, depth)
                ops.tsne_tree_step(Ya, Yb, indptr, indices, pval, order, skeys, st[0], st[1], st[2], tws, depth, a.angle, 0.8, lr, 0.01, False)
            else:
                ops.tsne_step(Ya, Yb, indptr, indices, pval, st[0], st[1], st[2], ws_x, 0.8, lr, 0.01, False)
            Ya, Yb = Yb, Ya
        sync()
        return (time.perf_counter() - t0) * 1e3 / n, Ya, Yb

    for depth in depths:
        tws = ops.tsne_tree_workspace(N, depth)
        Ya, Yb, st = Y300.clone(), torch.empty_like(Y300), state()
        run("tree", 2, Ya.clone(), Yb, state(), depth, tws)                      # warm-up
        if with_exact:
            run("exact", 1, Ya.clone(), Yb, state())
        ms = {"tree": [], "exact": []}
        Yx, Yxb, stx = Y300.clone(), torch.empty_like(Y300), state()
        for _ in range(2):                                                       # alternating blocks of five iterations
            m, Ya, Yb = run("tree", 5, Ya, Yb, st, depth, tws)
            ms["tree"].append(m)
            if with_exact:
                m, Yx, Yxb = run("exact", 5, Yx, Yxb, stx)
                ms["exact"].append(m)
        # the parts, each followed by a synchronise (so their sum is above the pipelined iteration)
        Yc = Y300.clone()
        parts = {"keys": [], "sort": [], "build+traversal": []}

        def lap(name, t0):
            sync()
            parts[name].append((time.perf_counter() - t0) * 1e3)
            return time.perf_counter()

        keys = torch.empty(N, dtype=torch.int32, device="cuda")
        for _ in range(5):
            sync()
            t0 = time.perf_counter()
            _lib.check(_lib.lib().vcy_tsne_tree_keys(Yc.data_ptr(), keys.data_ptr(), tws.data_ptr(), N, depth, ops._stream()), "keys")
            t0 = lap("keys", t0)
            skeys, order = torch.sort(keys, stable=True)
            t0 = lap("sort", t0)
            rep, Z, vis = ops.tsne_tree_repulsion(Yc, order, skeys, tws, depth, a.angle, visits=True)
            lap("build+traversal", t0)
        v = vis.to(torch.float64).mean(0).tolist()
        leaf = torch.bincount(skeys.to(torch.int64), minlength=4 ** depth)
        emit(dict(what="iteration at the embedding of iteration 300", n=N, depth=depth, automatic_depth=auto, angle=a.angle,
                  tree_ms_per_iter=[round(x, 4) for x in ms["tree"]], exact_ms_per_iter=[round(x, 4) for x in ms["exact"]] or "not run",
                  parts_ms_min={k: round(min(x), 4) for k, x in parts.items()}, accepted_nodes_per_target=round(v[0], 2),
                  direct_pairs_per_target=round(v[1], 2), largest_leaf=int(leaf.max()), occupied_leaves=int((leaf > 0).sum()),
                  tree_workspace_mb=round(tws.numel() / 2 ** 20, 1)))
        del tws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[10000, 50000, 100000])
    ap.add_argument("--sklearn-sizes", type=int, nargs="*", default=[10000, 50000])
    ap.add_argument("--ghz", type=float, default=2.4, help="shader clock assumed by the issue bound")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repulsion", choices=["exact", "tree"], default="exact", help="DeviceTSNE(repulsion=...) of the timed fits")
    ap.add_argument("--angle", type=float, default=0.5)
    ap.add_argument("--depth", type=int, default=None, help="tree depth of the fits (default: automatic)")
    ap.add_argument("--step-sizes", type=int, nargs="*", default=[], help="time single iterations of both modes at these sizes")
    ap.add_argument("--step-depths", type=int, nargs="*", default=[], help="depths timed by --step-sizes (default: automatic and one either side)")
    ap.add_argument("--no-exact-above", type=int, default=10 ** 9, help="skip the exact step above this size")
    a = ap.parse_args()
    import torch
    import velocyto_amd  # noqa: F401
    from velocyto_amd.preprocess import PreprocessMixin
    from velocyto_amd.tsne import DeviceTSNE
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    mode = dict(repulsion=a.repulsion, angle=a.angle, tree_depth=a.depth)
    for N in a.step_sizes:
        step_bench(N, a, emit)
    for N in a.sizes:
        Xd = torch.from_numpy(blobs(N)).cuda()
        DeviceTSNE(random_state=0, max_iter=250, **mode).fit_transform(Xd)  # warm-up at this size: code objects, allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aff = DeviceTSNE(random_state=0)._affinities(Xd)
        torch.cuda.synchronize()
        t_aff = time.perf_counter() - t0
        nnz = int(aff["indices"].numel())
        del aff
        t = DeviceTSNE(random_state=0, **mode)
        t0 = time.perf_counter()
        t.fit_transform(Xd)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        iters = t.n_iter_ + 1
        emit(dict(what="DeviceTSNE.fit_transform", repulsion=a.repulsion, angle=a.angle if a.repulsion == "tree" else None, n=N, dims=30, perplexity=30, nnz_P=nnz, wall_s=round(wall, 4), affinities_s=round(t_aff, 4),
                  iterations=iters, ms_per_iter=round((wall - t_aff) * 1e3 / iters, 4), kl=t.kl_divergence_,
                  repulsion_issue_bound_ms=round(issue_bound_ms(N, a.ghz), 4) if a.repulsion == "exact" else None, assumed_ghz=a.ghz))
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
