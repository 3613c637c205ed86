"""What fit_gammas' other weight modes cost on the scaled routes.  Writes profiles/atlas_fit_weights.txt (or OUT=...).
usage: [PART=weights,fused,parent,sharded] [SIZE=200000x4] [G=30000] [STEPS=3] [FUSED_CELLS=100000] [SHARDED_CELLS=50000]
       [PARENT_TREE=dir] [PARENT_RUNS=3] python tools/bench_atlas_fit_weights.py

weights: stage B of AtlasPath.run(timed=True) per weight mode against the default fit, ONE object whose mode is switched between
         runs, alternating, at SIZE (cells x blocks).
fused:   each launch of vcy_fit_weighted_moments_fused against the two-step pair vcy_gamma_weights + vcy_fit_weighted_moments
         (weight_mode 0) on the same resident block of FUSED_CELLS cells, f32 and f64.  GB/s counts the bytes each route must move:
         fused reads S, U (not in mode 2), X = S and Y = U once; two-step reads S (U), writes W, then reads X, Y, W.
sharded: ShardedLoom.fit_gammas() (gene slices) against fit_gammas(_route="select") on SHARDED_CELLS cells, one device, with the
         exchange bytes each would put on the wire per rank at that size (one rank moves nothing; the figures are the routes' own
         accounting formulas at world sizes 2 and 8).
parent:  the default fit="maxmin_diag" stage B of this tree against the parent commit: tools/bench_atlas_fit.py PART=path at SIZE, one
         fresh process per run, from PARENT_TREE (a checkout of the parent commit with its library built, e.g.
         `git archive HEAD~1 | tar -x -C DIR` and velocyto_amd.build() there) and from this tree, alternating, PARENT_RUNS each;
         prints every run of both and whether this tree's median lies within the parent's own spread.  Skipped, and said so, when
         PARENT_TREE is not given."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import smi_sample
from velocyto_amd import _lib, atlas, ops

G = int(os.environ.get("G", 30000))
STEPS = int(os.environ.get("STEPS", 3))
PARTS = os.environ.get("PART", "weights,fused,parent,sharded").split(",")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = os.environ.get("SIZE", "200000x4")
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "atlas_fit_weights.txt"))
dev = ops.require_gpu()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
out_fh = open(OUT, "a" if os.environ.get("APPEND") == "1" else "w")


def say(s=""):
    print(s, flush=True)
    out_fh.write(s + "\n")
    out_fh.flush()


def timed(fn, n=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def part_weights():
    c, b = SIZE.split("x")
    C = int(c)
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(C, G, 30, dev, density=0.08)
    fS, fU = atlas.size_factors(totS, totU, C)
    path = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, k=30, n_neighbors=500, sampled_fraction=0.5, block_cells=C // int(b), fit="maxmin_diag")
    rows = {"default (maxmin_diag)": dict(), "sum": dict(weights="sum"), "prod": dict(weights="prod"), "maxmin": dict(weights="maxmin"),
            "maxmin_weighted": dict(weights="maxmin_weighted"), "maxmin_double": dict(weights="maxmin_double"),
            "weighted=False": dict(weighted=False), "weighted=False, fixperc_q": dict(weighted=False, fit_offset=False, fixperc_q=True),
            "sum, limit_gamma": dict(weights="sum", limit_gamma=True)}
    say(f"## (a) stage B of AtlasPath.run(timed=True) per weight mode, {C} cells x {G} genes, f32, {len(path.blocks())} block(s) of {path.block_cells} "
        f"cells; ONE object, modes switched between runs, alternating, {STEPS} timed runs each after one warm-up each")

    def set_row(o):
        path.weighted, path.weights = o.get("weighted", True), o.get("weights", "maxmin_diag")
        path.fit_offset, path.fixperc_q, path.limit_gamma = o.get("fit_offset", True), o.get("fixperc_q", False), o.get("limit_gamma", False)
    tb, peak = {n: [] for n in rows}, {}
    for o in rows.values():
        set_row(o)
        path.run(); torch.cuda.synchronize()
    for _ in range(STEPS):
        for n, o in rows.items():
            set_row(o)
            before = path.stage_ms.copy()
            path.run(timed=True)
            torch.cuda.synchronize()
            tb[n].append((path.stage_ms - before)[1])
            peak[n] = path.select_state_bytes
    base = float(np.median(tb["default (maxmin_diag)"]))
    for n in rows:
        m = float(np.median(tb[n]))
        say(f"{n:28s} stage B {m:8.1f} ms ({min(tb[n]):.1f} .. {max(tb[n]):.1f})  = default {m - base:+.1f} ms (x{m / base:.3f})   select state {peak[n] / 1e6:.0f} MB")
    say()
    del path, cS, cU
    torch.cuda.empty_cache()


def part_fused():
    C = int(os.environ.get("FUSED_CELLS", 100_000))
    say(f"## (b) vcy_fit_weighted_moments_fused against vcy_gamma_weights + vcy_fit_weighted_moments(weight_mode 0), resident block of {C} cells x {G} "
        "genes, X = S, Y = U as in the fit; median of 5 (min .. max); GB = the bytes the route must move")
    names = {0: "sum", 1: "prod", 2: "maxmin_weighted", 3: "maxmin_double"}
    for dt in (torch.float32, torch.float64):
        es = 4 if dt == torch.float32 else 8
        ld = ops.padded_ld(G)
        gen = torch.Generator(device=dev).manual_seed(1)
        mats = []
        for _ in range(2):
            t = torch.empty((C, ld), dtype=dt, device=dev)
            for a in range(0, C, 50_000):
                b = min(C, a + 50_000)
                t[a:b] = (torch.rand((b - a, ld), generator=gen, device=dev) ** 2 * 8 * (torch.rand((b - a, ld), generator=gen, device=dev) < 0.4)).to(dt)
            mats.append(ops.CellMatrix(t, G))
        S, U = mats
        blk = C * ld * es / 1e9
        p99S, p99U = ops.gene_quantiles(S, [99])[0], ops.gene_quantiles(U, [99])[0]
        qS = ops.gene_quantiles(S, [2, 98])
        den = lambda M: (lambda q: torch.where(q[0] == 0, torch.clamp(q[1], min=0.001), q[0]))(ops.gene_quantiles(M, [99.9, 100]))
        dS, dU = den(S), den(U)
        qZ = ops.gene_quantiles(S, [2, 98], M2=U, scale_a=dS, scale_b=dU)
        args = {0: (p99S, p99U), 1: (p99S, p99U), 2: (qS[0], qS[1]), 3: (qZ[0], qZ[1], qS[0], qS[1], dS, dU)}
        for mode in range(4):
            Um = None if mode == 2 else U
            fused = lambda: ops.fit_weighted_moments_fused(U, S, mode, S, Um, *args[mode])
            box = {}

            def weights():
                box["W"] = None
                box["W"] = ops.gamma_weights(S, Um, mode, *args[mode])
            two = lambda: (weights(), ops.fit_weighted_moments(U, S, 0, W=box["W"]))
            mf = fused()
            two()
            same = bool(torch.equal(torch.nan_to_num(mf, nan=7.0), torch.nan_to_num(ops.fit_weighted_moments(U, S, 0, W=box["W"]), nan=7.0)))
            f_med, f_lo, f_hi = timed(fused)
            t_med, t_lo, t_hi = timed(two)
            w_med, _, _ = timed(weights)
            gb_f = blk * 2                                        # S (= X) and U (= Y) once each: Y is read in every mode
            gb_t = blk * ((1 if mode == 2 else 2) + 1 + 3)       # weights: S (U) in, W out; moments: X, Y, W in
            say(f"{str(dt):14s} mode {mode} {names[mode]:16s} fused {f_med:7.3f} ms ({f_lo:.3f} .. {f_hi:.3f}) {gb_f:5.1f} GB -> {gb_f / f_med * 1e3:6.0f} GB/s | "
                f"two-step {t_med:7.3f} ms ({t_lo:.3f} .. {t_hi:.3f}; weights alone {w_med:.3f}) {gb_t:5.1f} GB -> {gb_t / t_med * 1e3:6.0f} GB/s | "
                f"fused = x{f_med / t_med:.2f} of two-step, block-sized buffers 0 against 1 ({blk:.1f} GB); moments bit-identical: {same}")
        del mats, S, U
        torch.cuda.empty_cache()
    say()


def part_parent():
    parent = os.environ.get("PARENT_TREE")
    runs = int(os.environ.get("PARENT_RUNS", 3))
    say(f"## (c) the default fit=\"maxmin_diag\": the parent commit against this tree, tools/bench_atlas_fit.py PART=path SIZES={SIZE} STEPS={STEPS}, one "
        f"process per run, alternating, {runs} runs each, in this one call")
    if not parent:
        say("not measured: PARENT_TREE was not given")
        say()
        return
    stage_b = {"parent": [], "new": []}
    for i in range(runs):
        for tag, tree in (("parent", parent), ("new", ROOT)):
            with tempfile.TemporaryDirectory() as tmp:
                env = dict(os.environ, PART="path", SIZES=SIZE, STEPS=str(STEPS), G=str(G), OUT=os.path.join(tmp, "o.txt"))
                r = subprocess.run([sys.executable, os.path.join("tools", "bench_atlas_fit.py")], cwd=tree, env=env, capture_output=True, text=True, timeout=600)
            line = next((l for l in r.stdout.splitlines() if l.startswith("fit=maxmin_diag")), None)
            if r.returncode != 0 or line is None:
                say(f"{tag} run {i + 1}: failed ({r.returncode}): {r.stderr[-500:]}")
                raise SystemExit(1)
            stage_b[tag].append(float(re.search(r"B fit ([0-9.]+)", line).group(1)))
            say(f"{tag:6s} run {i + 1}: {line}")
    p, n = stage_b["parent"], stage_b["new"]
    med = float(np.median(n))
    where = "lies within" if min(p) <= med <= max(p) else ("lies BELOW (faster than)" if med < min(p) else "lies ABOVE (slower than)")
    say(f"stage B, parent: median {np.median(p):.1f} ms ({min(p):.1f} .. {max(p):.1f});  this tree: median {np.median(n):.1f} ms ({min(n):.1f} .. {max(n):.1f});  "
        f"this tree's median {where} the parent's own spread ({np.median(n) - np.median(p):+.2f} ms between the medians)")
    say()


def part_sharded():
    from velocyto_amd.sharded import ShardedLoom
    C = int(os.environ.get("SHARDED_CELLS", 50_000))
    rng = np.random.default_rng(0)
    say(f"## (d) ShardedLoom.fit_gammas(): gene slices against _route=\"select\", {C} cells x {G} genes, f64, one device (world 1)")
    gen = torch.Generator(device=dev).manual_seed(3)
    draw = lambda lam: torch.poisson(torch.full((G, C), lam, device=dev), generator=gen).to(torch.int16).cpu().numpy().view(np.uint16)
    S, U = draw(0.3), draw(0.1)
    pcs, ts = rng.normal(size=(C, 10)), rng.normal(size=(C, 2))
    sl = ShardedLoom.from_arrays(S, U, pcs, ts, dtype="float64")
    del S, U
    sl.normalize("both", size=True, log=True)
    sl.knn_imputation(k=30, n_pca_dims=10, n_jobs=1)
    res = {}
    for route in (None, "select", None, "select", None, "select"):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        sl.fit_gammas(_route=route)
        torch.cuda.synchronize()
        res.setdefault(route, []).append((time.perf_counter() - t0) * 1e3)
        res[str(route) + " gammas"] = sl.gammas.copy()
    same = np.array_equal(res["None gammas"].view(np.int32), res["select gammas"].view(np.int32))
    es, P = 8, 8
    for route, label in ((None, "gene slices (default)"), ("select", "streamed select")):
        t = res[route][1:]
        say(f"{label:24s} {np.median(t):8.1f} ms ({min(t):.1f} .. {max(t):.1f}; first call {res[route][0]:.1f})")
    hist = G * 256 * 4
    sel = 10 * G * 8
    for qs in ([99.9, 100], [99.9, 100], [2, 98]):
        nt = len(ops.percentile_targets(qs, C)[0])
        sel += P * 8 + hist * (1 + (P - 1) * nt)
    for W in (2, 8):
        say(f"world {W}: gene slices move 2 x {C * G * es / 1e9:.1f} GB x (1 - 1/{W}) = {2 * C * G * es * (1 - 1 / W) / 1e9:.2f} GB over all ranks "
            f"({2 * C * G * es * (1 - 1 / W) / W / 1e9:.2f} GB per rank); the select all-reduces {sel / 1e9:.2f} GB per rank (int32 histograms of "
            f"{P} passes + 10 G f64 moments), whatever the number of cells")
    say(f"gammas bit-identical between the routes on one rank: {same}")
    say()


say(f"# tools/bench_atlas_fit_weights.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}")
say("smi before: " + json.dumps(smi_sample()))
if "weights" in PARTS:
    part_weights()
if "fused" in PARTS:
    part_fused()
if "parent" in PARTS:
    part_parent()
if "sharded" in PARTS:
    part_sharded()
say("smi after: " + json.dumps(smi_sample()))
out_fh.close()
