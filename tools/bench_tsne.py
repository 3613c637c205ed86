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
--depth adaptive (with --leaf-size) selects the adaptive tree: the fits use it, and --step-sizes times it on the same embedding
beside the fixed tree at its automatic depth.  --trace-sizes N .. fits N points twice, with the fixed automatic depth and with the
adaptive tree, from the same affinities and start, and records per iteration (device events) the keys + sort and the build + walk
(one extra evaluation of the repulsion alone, for the first 300 iterations and the listed ones), the largest leaf met, the nodes
used against the workspace bound, and - on the adaptive fit's embeddings of iterations 100 and 300 - a sweep over leaf_size.
usage: tools/bench_tsne.py [--sizes 10000 50000 100000] [--sklearn-sizes 10000 50000] [--ghz 2.4] [--out FILE]
                           [--repulsion exact|tree] [--angle 0.5] [--depth D|adaptive] [--leaf-size 32] [--step-sizes 50000 1000000]
                           [--step-depths 8 9] [--no-exact-above N] [--trace-sizes 1000000] [--sweep-leaf-sizes 1 2 4 8 16 32]
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
    t = DeviceTSNE(random_state=0, repulsion="tree", angle=a.angle, tree_depth=a.depth, leaf_size=a.leaf_size)
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
    adaptive = a.depth == "adaptive"
    leaf = ops.TSNE_ATREE_LEAF_SIZE if a.leaf_size is None else a.leaf_size
    depths = a.step_depths or ([auto] if adaptive else [d for d in (auto - 1, auto, auto + 1) if 1 <= d <= 11])
    lr = float(t.learning_rate_)
    state = lambda: (torch.zeros((N, 2), dtype=torch.float64, device="cuda"), torch.ones((N, 2), device="cuda"),
                     torch.zeros(4, dtype=torch.float64, device="cuda"))
    with_exact = N <= a.no_exact_above
    ws_x = ops.tsne_workspace(N, 2) if with_exact else None

    def run(mode, n, Ya, Yb, st, depth=None, tws=None):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            if mode == "atree":
                _, order, skeys = ops.tsne_atree_keys(Ya, tws, leaf)
                ops.tsne_atree_step(Ya, Yb, indptr, indices, pval, order, skeys, st[0], st[1], st[2], tws, a.angle, 0.8, lr, 0.01, False, leaf_size=leaf)
            elif mode == "tree":
                _, order, skeys = ops.tsne_tree_keys(Ya, tws, depth)
                ops.tsne_tree_step(Ya, Yb, indptr, indices, pval, order, skeys, st[0], st[1], st[2], tws, depth, a.angle, 0.8, lr, 0.01, False)
            else:
                ops.tsne_step(Ya, Yb, indptr, indices, pval, st[0], st[1], st[2], ws_x, 0.8, lr, 0.01, False)
            Ya, Yb = Yb, Ya
        sync()
        return (time.perf_counter() - t0) * 1e3 / n, Ya, Yb

    for depth in depths + (["adaptive"] if adaptive else []):
        mode = "atree" if depth == "adaptive" else "tree"
        tws = ops.tsne_atree_workspace(N, leaf) if mode == "atree" else ops.tsne_tree_workspace(N, depth)
        Ya, Yb, st = Y300.clone(), torch.empty_like(Y300), state()
        run(mode, 2, Ya.clone(), Yb, state(), depth, tws)                        # warm-up
        if with_exact:
            run("exact", 1, Ya.clone(), Yb, state())
        ms = {"tree": [], "exact": []}
        Yx, Yxb, stx = Y300.clone(), torch.empty_like(Y300), state()
        for _ in range(2):                                                       # alternating blocks of five iterations
            m, Ya, Yb = run(mode, 5, Ya, Yb, st, depth, tws)
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

        keys = torch.empty(N, dtype=torch.int64 if mode == "atree" else torch.int32, device="cuda")
        for _ in range(5):
            sync()
            t0 = time.perf_counter()
            if mode == "atree":
                _lib.check(_lib.lib().vcy_tsne_atree_keys(Yc.data_ptr(), keys.data_ptr(), tws.data_ptr(), N, leaf, ops.TSNE_ATREE_MAX_DEPTH,
                                                          ops._stream()), "keys")
            else:
                _lib.check(_lib.lib().vcy_tsne_tree_keys(Yc.data_ptr(), keys.data_ptr(), tws.data_ptr(), N, depth, ops._stream()), "keys")
            t0 = lap("keys", t0)
            skeys, order = torch.sort(keys, stable=True)
            t0 = lap("sort", t0)
            if mode == "atree":
                rep, Z, vis = ops.tsne_atree_repulsion(Yc, order, skeys, tws, a.angle, leaf, visits=True)
            else:
                rep, Z, vis = ops.tsne_tree_repulsion(Yc, order, skeys, tws, depth, a.angle, visits=True)
            lap("build+traversal", t0)
        v = vis.to(torch.float64).mean(0).tolist()
        row = dict(what="iteration at the embedding of iteration 300", n=N, depth=depth, automatic_depth=auto, angle=a.angle,
                   tree_ms_per_iter=[round(x, 4) for x in ms["tree"]], exact_ms_per_iter=[round(x, 4) for x in ms["exact"]] or "not run",
                   parts_ms_min={k: round(min(x), 4) for k, x in parts.items()}, accepted_nodes_per_target=round(v[0], 2),
                   direct_pairs_per_target=round(v[1], 2), tree_workspace_mb=round(tws.numel() / 2 ** 20, 1))
        if mode == "atree":
            row.update(leaf_size=leaf, **atree_census(tws, N, leaf))
        else:
            cells = torch.bincount(skeys.to(torch.int64), minlength=4 ** depth)
            row.update(largest_leaf=int(cells.max()), occupied_leaves=int((cells > 0).sum()))
        emit(row)
        del tws


def atree_census(tws, N, leaf, max_depth=24):
    """Nodes used, their bound, the largest leaf and the deepest level of the adaptive tree last built in the workspace `tws`."""
    import torch
    nn = int(tws[132:136].view(torch.int32).item())
    off = 256 + 4096
    rec = tws[off:off + 32 * nn].view(torch.int32).view(nn, 8)
    leaves = rec[:, 6] == 1
    return dict(nodes=nn, node_bound=1 + 4 * max_depth * (N // (leaf + 1)), leaves=int(leaves.sum()), largest_leaf=int(rec[:, 1][leaves].max()),
                deepest_level=int(rec[:, 2].max()))


TRACE_AT = (50, 100, 150, 200, 250, 300, 500, 1000)


def trace_bench(N, a, emit):
    """One fit with the fixed tree at its automatic depth and one with the adaptive tree, the same affinities and start: per-iteration
    device times (see the module docstring).  The descent is DeviceTSNE's schedule without the stopping checks."""
    import torch
    from velocyto_amd import ops
    from velocyto_amd.tsne import DeviceTSNE
    sync = torch.cuda.synchronize
    leaf = ops.TSNE_ATREE_LEAF_SIZE if a.leaf_size is None else a.leaf_size
    X = torch.from_numpy(blobs(N)).cuda()
    t = DeviceTSNE(random_state=0, repulsion="tree", angle=a.angle)
    t._check_params(tuple(X.shape))
    sync()
    t0 = time.perf_counter()
    aff = t._affinities(X)
    sync()
    t_aff = time.perf_counter() - t0
    indptr, indices, P = aff["indptr"], aff["indices"], aff["P"]
    del aff, X
    p_ex, p_late = (P * t.early_exaggeration).to(torch.float32), P.to(torch.float32)
    del P
    lr = float(max(N / t.early_exaggeration / 4, 50))
    depth = ops.tsne_tree_depth(N)
    kept = {}

    def evaluate(mode, Y, tws):
        if mode == "adaptive":
            _, order, skeys = ops.tsne_atree_keys(Y, tws, leaf)
        else:
            _, order, skeys = ops.tsne_tree_keys(Y, tws, depth)
        return order, skeys

    def fit(mode, instrument):
        tws = ops.tsne_atree_workspace(N, leaf) if mode == "adaptive" else ops.tsne_tree_workspace(N, depth)
        Y = torch.from_numpy(t._initial_embedding(N)).cuda()
        Yn = torch.empty_like(Y)
        stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        ev, largest, census = [], 0, {}
        sync()
        w0 = time.perf_counter()
        for i in range(1000):
            if i in (0, 250):
                update, gains = torch.zeros((N, 2), dtype=torch.float64, device="cuda"), torch.ones((N, 2), device="cuda")
            pval, momentum = (p_ex, 0.5) if i < 250 else (p_late, 0.8)
            timed = instrument and (i < 300 or (i + 1) in TRACE_AT)
            if instrument and mode == "adaptive" and i in (100, 300):
                kept[i] = Y.clone()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            order, skeys = evaluate(mode, Y, tws)
            e[1].record()
            if timed:                                                    # the repulsion alone, once more: build + walk
                if mode == "adaptive":
                    ops.tsne_atree_repulsion(Y, order, skeys, tws, a.angle, leaf)
                else:
                    ops.tsne_tree_repulsion(Y, order, skeys, tws, depth, a.angle)
            e[2].record()
            if mode == "adaptive":
                ops.tsne_atree_step(Y, Yn, indptr, indices, pval, order, skeys, update, gains, stats, tws, a.angle, momentum, lr, 0.01,
                                    i == 999, leaf_size=leaf)
            else:
                ops.tsne_tree_step(Y, Yn, indptr, indices, pval, order, skeys, update, gains, stats, tws, depth, a.angle, momentum, lr, 0.01,
                                   i == 999)
            e[3].record()
            ev.append((timed, e))
            if timed and mode == "adaptive":
                c = atree_census(tws, N, leaf)
                largest = max(largest, c["largest_leaf"])
                if (i + 1) in TRACE_AT:
                    census[i + 1] = c
            elif timed and (i + 1) in TRACE_AT:
                census[i + 1] = dict(largest_leaf=int(torch.bincount(skeys.to(torch.int64), minlength=4 ** depth).max()))
            Y, Yn = Yn, Y
        sync()
        wall = time.perf_counter() - w0
        ks = [e[0].elapsed_time(e[1]) for _, e in ev]
        bw = [e[1].elapsed_time(e[2]) if timed else None for timed, e in ev]
        st = [e[2].elapsed_time(e[3]) for _, e in ev]
        row = dict(what="fit with per-iteration times" if instrument else "fit, plain loop", n=N, mode=mode, depth=depth if mode == "fixed" else "adaptive",
                   leaf_size=leaf if mode == "adaptive" else None, angle=a.angle, affinities_s=round(t_aff, 3), loop_wall_s=round(wall, 3),
                   kl=float(stats[1]), iteration_ms_sum_without_the_extra_evaluation=round(sum(ks) + sum(st), 1))
        if instrument:
            first = np.asarray(bw[:300])
            row.update(tree_ms_at={str(i): dict(keys_sort=round(ks[i - 1], 3), build_walk=round(bw[i - 1], 3), step_call=round(st[i - 1], 3),
                                                **census.get(i, {})) for i in TRACE_AT},
                       build_walk_ms_first_300=dict(max=round(float(first.max()), 3), median=round(float(np.median(first)), 3),
                                                    mean=round(float(first.mean()), 3), argmax=int(first.argmax())),
                       step_call_ms_first_300=dict(max=round(max(st[:300]), 3), median=round(float(np.median(st[:300])), 3)))
            if mode == "adaptive":
                row.update(largest_leaf_first_300_and_listed=largest)
        emit(row)
        del tws

    DeviceTSNE(random_state=0, max_iter=250, repulsion="tree", tree_depth="adaptive").fit_transform(torch.from_numpy(blobs(20000)).cuda())   # code objects
    fit("adaptive", True)
    fit("fixed", True)
    fit("adaptive", False)
    # leaf_size sweep on the two kept embeddings: keys + sort + build + walk, device events, minimum and median of 7
    for it, Y in sorted(kept.items()):
        for mode, ls in [("fixed", None)] + [("adaptive", l) for l in a.sweep_leaf_sizes]:
            tws = ops.tsne_atree_workspace(N, ls) if mode == "adaptive" else ops.tsne_tree_workspace(N, depth)
            ms = []
            for r in range(8):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if mode == "adaptive":
                    _, order, skeys = ops.tsne_atree_keys(Y, tws, ls)
                    ops.tsne_atree_repulsion(Y, order, skeys, tws, a.angle, ls)
                else:
                    _, order, skeys = ops.tsne_tree_keys(Y, tws, depth)
                    ops.tsne_tree_repulsion(Y, order, skeys, tws, depth, a.angle)
                e1.record()
                sync()
                if r:
                    ms.append(e0.elapsed_time(e1))
            row = dict(what="tree time on a kept embedding", n=N, iteration=it, mode=mode, leaf_size=ls, ms_min=round(min(ms), 3),
                       ms_median=round(float(np.median(ms)), 3), ms_max=round(max(ms), 3))
            if mode == "adaptive":
                row.update(atree_census(tws, N, ls))
            emit(row)
            del tws


def depth_arg(v):
    return v if v == "adaptive" else int(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[10000, 50000, 100000])
    ap.add_argument("--sklearn-sizes", type=int, nargs="*", default=[10000, 50000])
    ap.add_argument("--ghz", type=float, default=2.4, help="shader clock assumed by the issue bound")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repulsion", choices=["exact", "tree"], default="exact", help="DeviceTSNE(repulsion=...) of the timed fits")
    ap.add_argument("--angle", type=float, default=0.5)
    ap.add_argument("--depth", type=depth_arg, default=None, help="tree depth of the fits: 1 .. 11 or 'adaptive' (default: automatic)")
    ap.add_argument("--leaf-size", type=int, default=None, help="leaf_size of the adaptive tree (default: DeviceTSNE's)")
    ap.add_argument("--trace-sizes", type=int, nargs="*", default=[], help="fixed and adaptive fits with per-iteration times at these sizes")
    ap.add_argument("--sweep-leaf-sizes", type=int, nargs="*", default=[1, 2, 4, 8, 16, 32], help="leaf sizes swept by --trace-sizes")
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

    mode = dict(repulsion=a.repulsion, angle=a.angle, tree_depth=a.depth, leaf_size=a.leaf_size)
    for N in a.trace_sizes:
        trace_bench(N, a, emit)
        if a.out:                                                            # the long measurement first on disk
            with open(a.out, "w") as f:
                f.writelines(json.dumps(r) + "\n" for r in rows)
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
