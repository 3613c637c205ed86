"""What AtlasPath(fit="maxmin_diag") costs over fit="slope", and how fast the streamed select's counting launch runs.
Writes profiles/atlas_fit.txt (or OUT=...).   usage: [PART=count,path] [SIZES=200000x4,resident,1000000xauto] [G=30000] [STEPS=2]
                                                     python tools/bench_atlas_fit.py

count: vcy_gene_select_count_block alone on a resident block of G genes, f32 and f64, at the largest cell count that fits beside
       nothing else (0.8 of the free HBM, capped at 1 000 000): the first pass (one histogram for all targets) and a later pass
       (four targets, prefixes from a real first pass, so the matching keys are as few as in a real run).  Bytes read = cells x ld x
       element size; the rate is held against STREAM_TBS, the read rate the project measured for its streaming stage B
       (profiles/r06_pool_levers.txt: 24 GB at 6.2 TB/s).
path:  AtlasPath.run(timed=True) with fit="maxmin_diag" and fit="slope" ALTERNATING in one process on the same data: wall time
       per run between device synchronisations and the stage times (stage B holds all the extra walks, re-pooling included).
Opt-in parts (not in the default PART):
mcount:  the masked counting launch (vcy_gene_mselect_count_block) against the unmasked one on a resident block of MC_CELLS (100 000)
         cells, per digit, f32 and f64, two targets each (percentile 10): no value mask, the mask's source = the matrix itself, and
         a second matrix; with and without a cell mask that keeps half of the rows.
options: stage B of AtlasPath.run(timed=True) with each of fit_gammas' options against the default fit, ONE object whose options are
         switched between runs, alternating, at the first of SIZES."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import smi_sample
from velocyto_amd import _lib, atlas, ops

STREAM_TBS = 6.2
G = int(os.environ.get("G", 30000))
STEPS = int(os.environ.get("STEPS", 2))
PARTS = os.environ.get("PART", "count,path").split(",")
SIZES = os.environ.get("SIZES", "200000x4,resident,1000000xauto").split(",")
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "atlas_fit.txt"))
dev = ops.require_gpu()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
out_fh = open(OUT, "w")


def say(s=""):
    print(s, flush=True)
    out_fh.write(s + "\n")
    out_fh.flush()


def clock_during(fn, ms):
    pr = ops.ClockProbe(interval_ms=1.0)
    torch.cuda.synchronize()
    pr.start(max(2.0, 0.8 * ms))
    fn()
    torch.cuda.synchronize()
    return pr.ghz()[0]


def timed(fn, n=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def part_count():
    say("## the counting launch alone (vcy_gene_select_count_block), resident block, median of 5 (min .. max)")
    for dt in (torch.float32, torch.float64):
        es = 4 if dt == torch.float32 else 8
        ld = ops.padded_ld(G)
        C = int(min(1_000_000, torch.cuda.mem_get_info(dev)[0] * 0.8 // (ld * es)))
        gen = torch.Generator(device=dev).manual_seed(1)
        t = torch.empty((C, ld), dtype=dt, device=dev)
        step = 50_000
        for a in range(0, C, step):      # expression-like: 60 % exact zeros, the rest spread over a few binades
            b = min(C, a + step)
            t[a:b] = (torch.rand((b - a, ld), generator=gen, device=dev) ** 2 * 8 * (torch.rand((b - a, ld), generator=gen, device=dev) < 0.4)).to(dt)
        M = ops.CellMatrix(t, G)
        sel = ops.StreamedGeneQuantiles(G, [2, 98], C, dt)
        L = _lib.lib()
        gb = C * ld * es / 1e9

        def launch():
            _lib.check(L.vcy_gene_select_count_block(M.t.data_ptr(), None, None, None, sel.state.data_ptr(), sel.hist.data_ptr(), sel.pass_no,
                                                     sel.nt, C, G, ld, sel.code, torch.cuda.current_stream().cuda_stream), "count_block")
        for name in ("first pass, 1 histogram", "second pass, 4 targets", "third pass, 4 targets"):
            med, lo, hi = timed(launch)
            ghz = clock_during(launch, med)
            say(f"{str(dt):14s} C={C} G={G}: {name:24s} {med:8.2f} ms ({lo:.2f} .. {hi:.2f})  reads {gb:.1f} GB -> {gb / med:.2f} TB/s = "
                f"{gb / med / STREAM_TBS:.2f} of the {STREAM_TBS} TB/s the streaming stage B reads at; shader clock {ghz:.2f} GHz")
            sel.hist.zero_()             # the timed launches all added to the histogram: count the pass once more, properly, and advance
            sel.add_block(M)
            sel.advance()
        del t, M, sel
        torch.cuda.empty_cache()
    say()


def part_path(spec):
    if spec == "resident":               # one block: what fits resident beside the CSR layers, the generator's temporaries and the kNN workspace
        C = int(os.environ.get("RESIDENT_CELLS", 0)) or int(min(1_000_000, 0.7 * torch.cuda.mem_get_info(dev)[0] // (2 * ops.padded_ld(G) * 4 + 40_000)) // 10_000 * 10_000)
        block = 0
    else:
        c, b = spec.split("x")
        C = int(c)
        block = -1 if b == "auto" else C // int(b)
    t0 = time.perf_counter()
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(C, G, 30, dev, density=0.08)
    fS, fU = atlas.size_factors(totS, totU, C)
    if block < 0:
        block = atlas.auto_block_cells(C, C, G, dev, 4)
    path = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, k=30, n_neighbors=500, sampled_fraction=0.5, block_cells=block)
    say(f"## AtlasPath.run(timed=True), {C} cells x {G} genes, f32, {len(path.blocks())} block(s) of {path.block_cells} cells (setup {time.perf_counter() - t0:.0f} s); "
        f"ONE object, its fit switched between runs: maxmin_diag and slope alternating, {STEPS} timed runs each after one warm-up each")
    fits = ("maxmin_diag", "slope")
    wall, stage = {f: [] for f in fits}, {f: np.zeros(4) for f in fits}
    for f in fits:
        path.fit = f
        path.run(); torch.cuda.synchronize()
    for _ in range(STEPS):
        for f in fits:
            path.fit = f
            before = path.stage_ms.copy()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            path.run(timed=True)
            torch.cuda.synchronize(); wall[f].append((time.perf_counter() - t0) * 1e3)
            stage[f] += path.stage_ms - before
    for f in fits:
        st = stage[f] / STEPS
        say(f"fit={f:12s} wall {np.median(wall[f]):9.1f} ms/run ({min(wall[f]):.1f} .. {max(wall[f]):.1f})   stage ms: A pooling {st[0]:.1f}  B fit {st[1]:.1f}  "
            f"A kNN search {st[2]:.1f}  D {st[3]:.1f}" + (f"   select state {path.select_state_bytes / 1e6:.0f} MB" if f != "slope" else ""))
    a, b = np.median(wall["maxmin_diag"]), np.median(wall["slope"])
    say(f"fit=maxmin_diag over fit=slope: +{a - b:.1f} ms per run = x{a / b:.2f}")
    say()
    del path, cS, cU
    torch.cuda.empty_cache()


def part_mcount():
    C = int(os.environ.get("MC_CELLS", 100_000))
    say(f"## the masked counting launch (vcy_gene_mselect_count_block) against the unmasked one, resident block of {C} cells, percentile 10 "
        "(two targets), median of 5 (min .. max); the value mask keeps x > 4.5, about a tenth of the entries")
    L = _lib.lib()
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
        M, S = mats
        thr = torch.full((G,), 4.5, dtype=torch.float64, device=dev)
        half = (torch.arange(C, device=dev) % 2 == 0).to(torch.uint8)
        gb = C * ld * es / 1e9
        plain = ops.StreamedGeneQuantiles(G, [10], C, dt)
        # (label, mask_src, mask_mode, cell mask, bytes read relative to the block)
        variants = [("masked, no value mask", None, 0, None, 1.0), ("masked, source = M", M, 1, None, 1.0), ("masked, second matrix", S, 1, None, 2.0),
                    ("no value mask, half the rows", None, 0, half, 0.5), ("second matrix, half the rows", S, 1, half, 1.0)]
        sels = [ops.StreamedMaskedGeneQuantiles(G, [10], dt) for _ in variants]
        st = lambda: torch.cuda.current_stream().cuda_stream
        for p_no in range(plain.passes):
            def unmasked():
                _lib.check(L.vcy_gene_select_count_block(M.t.data_ptr(), None, None, None, plain.state.data_ptr(), plain.hist.data_ptr(), plain.pass_no,
                                                         plain.nt, C, G, ld, plain.code, st()), "count_block")
            base, lo, hi = timed(unmasked)
            say(f"{str(dt):14s} digit {p_no}: unmasked{'':30s} {base:7.3f} ms ({lo:.3f} .. {hi:.3f})  reads {gb:.1f} GB -> {gb / base:.2f} TB/s")
            plain.hist.zero_(); plain.add_block(M); plain.advance()
            for (label, src, mode, cm, rel), sel in zip(variants, sels):
                def masked():
                    _lib.check(L.vcy_gene_mselect_count_block(M.t.data_ptr(), None if src is None else src.t.data_ptr(), thr.data_ptr() if mode else None,
                                                              mode, None if cm is None else cm.data_ptr(), sel.state.data_ptr(), sel.hist.data_ptr(),
                                                              sel.pass_no, sel.nq, C, G, ld, sel.code, st()), "mselect_count_block")
                med, lo, hi = timed(masked)
                say(f"{str(dt):14s} digit {p_no}: {label:38s} {med:7.3f} ms ({lo:.3f} .. {hi:.3f})  reads {gb * rel:.1f} GB -> {gb * rel / med:.2f} TB/s  "
                    f"= x{med / base:.2f} of the unmasked launch ({med - base:+.3f} ms)")
                sel.hist.zero_(); sel.add_block(M, src, thr if mode else None, mode, cm); sel.advance()
        del mats, M, S, sels, plain
        torch.cuda.empty_cache()
    say()


def part_options(spec):
    c, b = spec.split("x")
    C = int(c)
    block = C // int(b)
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(C, G, 30, dev, density=0.08)
    fS, fU = atlas.size_factors(totS, totU, C)
    path = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, k=30, n_neighbors=500, sampled_fraction=0.5, block_cells=block, fit="maxmin_diag")
    rows = {"default": dict(fit_offset=True, fixperc_q=False, limit_gamma=False, ss=False),
            "limit_gamma": dict(fit_offset=True, fixperc_q=False, limit_gamma=True, ss=False),
            "fit_offset=False, fixperc_q": dict(fit_offset=False, fixperc_q=True, limit_gamma=False, ss=False),
            "fit_offset=False, limit_gamma": dict(fit_offset=False, fixperc_q=False, limit_gamma=True, ss=False),
            "fit_offset=False": dict(fit_offset=False, fixperc_q=False, limit_gamma=False, ss=False),
            "steady state (half the cells)": dict(fit_offset=True, fixperc_q=False, limit_gamma=False, ss=True),
            "steady state, limit_gamma": dict(fit_offset=True, fixperc_q=False, limit_gamma=True, ss=True)}
    half = (torch.arange(C, device=dev) % 2 == 0).to(torch.uint8)
    say(f"## stage B of AtlasPath.run(timed=True) per fit option, {C} cells x {G} genes, f32, {len(path.blocks())} block(s) of {path.block_cells} cells; "
        f"ONE object, options switched between runs, alternating, {STEPS} timed runs each after one warm-up each")

    def set_row(o):
        path.fit_offset, path.fixperc_q, path.limit_gamma = o["fit_offset"], o["fixperc_q"], o["limit_gamma"]
        path._ss, path.n_fit_cells = (half, int(half.sum())) if o["ss"] else (None, C)
    tb, peak = {n: [] for n in rows}, {}
    for n, o in rows.items():
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
    base = float(np.median(tb["default"]))
    for n in rows:
        m = float(np.median(tb[n]))
        say(f"{n:32s} stage B {m:8.1f} ms ({min(tb[n]):.1f} .. {max(tb[n]):.1f})  = default {m - base:+.1f} ms (x{m / base:.3f})   select state {peak[n] / 1e6:.0f} MB")
    say()
    del path, cS, cU
    torch.cuda.empty_cache()


say(f"# tools/bench_atlas_fit.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  digit bits {_lib.lib().vcy_gene_select_digit_bits()}")
say("smi before: " + json.dumps(smi_sample()))
if "count" in PARTS:
    part_count()
if "path" in PARTS:
    for spec in SIZES:
        part_path(spec)
if "mcount" in PARTS:
    part_mcount()
if "options" in PARTS:
    part_options(SIZES[0])
say("smi after: " + json.dumps(smi_sample()))
out_fh.close()
