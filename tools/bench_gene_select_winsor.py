"""What the winsorised gene selection from CSR count layers costs, beside the plain statistics pass that reads the same bytes, measured
in the same call.  Writes profiles/gene_select_winsor.txt (or OUT=...).
usage: [C=1000000] [G=30000] [REPS=5] [DENSIFY=1] [WALK_ONLY=0] python tools/bench_gene_select_winsor.py
(WALK_ONLY=1 DENSIFY=0: the statistics pass and the counting walks alone - for a library built with other VCY_QH_SHORT / VCY_QH_CELLS.)

On atlas.synth_atlas layers at 8 % density, as uint8 and as uint16 counts (the same counts widened): ops.csr_gene_stats (the yardstick:
one read of the layer), each counting walk of ops.CsrGeneQuantiles on its own (vcy_csr_quantiles_count), the whole of
ops.csr_gene_quantiles((1, 99.5)), the clipped statistics (ops.csr_gene_stats(lo=, hi=)), atlas.score_cv_vs_mean with and without
winsor_perc, and - DENSIFY=1 - the route there was before: CsrCounts.transposed() + a per-gene reduction over the gene-major copy
(profiles/gene_select.txt).  Times are device events around the call after a warm-up call, median of REPS (min .. max)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from velocyto_amd import _lib, atlas, ops

C = int(os.environ.get("C", 1000000))
G = int(os.environ.get("G", 30000))
REPS = int(os.environ.get("REPS", 5))
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gene_select_winsor.txt"))
PERC = (1, 99.5)
dev = ops.require_gpu()
L = _lib.lib()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
out_fh = open(OUT, "w")


def say(s=""):
    print(s, flush=True)
    out_fh.write(s + "\n")
    out_fh.flush()


def timed(fn, n=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def fmt(t):
    return f"{t[0]:9.2f} ms ({t[1]:.2f} .. {t[2]:.2f})"


def layer(c, name):
    es = c.data.element_size()
    layer_b = c.nnz * (4 + es)
    say(f"## {name} counts: {c.nnz} stored elements ({100 * c.nnz / C / G:.2f} %), {layer_b / 1e9:.2f} GB of indices + counts")
    c.slabptr
    t_stats = timed(lambda: ops.csr_gene_stats(c))
    say(f"csr_gene_stats (the yardstick)          : {fmt(t_stats)}   {layer_b / t_stats[0] / 1e9:.3f} TB/s of the layer")
    wide = c.code == ops.U16
    sel = ops.CsrGeneQuantiles(G, PERC, C, wide, dev)
    say(f"select state: {sel.nt} distinct ranks, histograms {sel.hist.numel() * 4 / 1e6:.1f} MB + state {sel.state.numel() * 4 / 1e6:.1f} MB "
        f"= {sel.state_bytes / 1e6:.1f} MB (vcy_csr_quantiles_hist_bytes + _state_bytes); tiles of {L.vcy_csr_quantiles_block_cells()} cells")

    def walk(p):
        L.vcy_csr_quantiles_begin(sel.hist.data_ptr(), sel.nt, G, sel.code, ops._stream()) if p == 0 else sel.hist[1:].zero_()
        sel.pass_no = p
        sel.cells_in_pass = 0
        sel.add_block(c)
    for p in range(sel.passes):
        # the zeroing of the histograms is timed apart, and taken off: the walk's own time is what is compared with the statistics pass
        t_zero = timed(lambda: (L.vcy_csr_quantiles_begin(sel.hist.data_ptr(), sel.nt, G, sel.code, ops._stream()) if p == 0 else sel.hist[1:].zero_()))
        t_w = timed(lambda: walk(p))
        say(f"counting walk {p} (+ zeroing {t_zero[0]:.2f} ms)     : {fmt(t_w)}   walk alone {t_w[0] - t_zero[0]:.2f} ms = x{(t_w[0] - t_zero[0]) / t_stats[0]:.2f} the statistics pass")
        sel.advance()
    assert sel.done
    if os.environ.get("WALK_ONLY", "0") == "1":
        return t_stats, t_stats, t_stats
    t_q = timed(lambda: ops.csr_gene_quantiles(c, PERC))
    say(f"csr_gene_quantiles((1, 99.5)), whole    : {fmt(t_q)}   x{t_q[0] / t_stats[0]:.2f} the statistics pass")
    q = ops.csr_gene_quantiles(c, PERC)
    assert torch.equal(q, sel.result())
    t_c = timed(lambda: ops.csr_gene_stats(c, None, q[0], q[1]))
    ws = int(L.vcy_csr_gene_stats_parts_workspace_bytes(C, G))
    say(f"csr_gene_stats(lo=, hi=)                : {fmt(t_c)}   x{t_c[0] / t_stats[0]:.2f} the statistics pass; workspace {ws / 1e6:.0f} MB "
        f"({int(L.vcy_csr_gene_stats_workspace_bytes(C, G)) / 1e6:.0f} MB for the plain pass)")
    say(f"bounds: {float((q[0] > 0).double().mean()) * 100:.1f} % of the lower bounds positive, upper bound up to {float(q[1].max()):.0f}")
    # as the reference, the score takes log2 of the winsorised mean: a gene seen in fewer than 0.5 % of the cells has an upper bound of 0
    # and no finite score, so the detection asks for more cells than that here (in both calls)
    N, mec = min(3000, G // 4), int(0.0051 * C) + 2
    t_a = timed(lambda: atlas.score_cv_vs_mean(c, C, N=N, max_expr_avg=40, min_expr_cells=mec), 3)
    t_b = timed(lambda: atlas.score_cv_vs_mean(c, C, N=N, max_expr_avg=40, min_expr_cells=mec, winsor_perc=PERC), 3)
    say(f"atlas.score_cv_vs_mean (min_expr_cells={mec}): {fmt(t_a)}")
    say(f"atlas.score_cv_vs_mean(winsor_perc=)    : {fmt(t_b)}   + {t_b[0] - t_a[0]:.2f} ms")
    return t_stats, t_q, t_c


say(f"# winsorised gene selection from CSR layers: {C} cells x {G} genes, one {torch.cuda.get_device_name(0)}, median of {REPS} (min .. max)")
t0 = time.perf_counter()
cS, cU, *_ = atlas.synth_atlas(C, G, 4, dev, density=0.08)
del cU, _
torch.cuda.empty_cache()
say(f"[layers generated in {time.perf_counter() - t0:.1f} s; the largest count is {int(cS.data.max() if cS.code == ops.U8 else (cS.data.to(torch.int32) & 0xFFFF).max())}]")
if cS.code == ops.U8:
    narrow, wide = cS, ops.CsrCounts(cS.indptr, cS.indices, cS.data.to(torch.int16), G)
else:                                                                          # the uint8 layer: the same counts cut at 255
    narrow, wide = ops.CsrCounts(cS.indptr, cS.indices, (cS.data.to(torch.int32) & 0xFFFF).clamp(max=255).to(torch.uint8), G), cS
    say("[the uint8 layer holds the same counts cut at 255]")
res = {"uint8": layer(narrow, "uint8"), "uint16": layer(wide, "uint16")}
if os.environ.get("DENSIFY", "1") == "1":
    c = narrow if narrow is not None else wide
    t_T = timed(lambda: c.transposed(), 2)
    cT = c.transposed()
    ones = torch.ones(C, dtype=torch.float64, device=dev)
    t_m = timed(lambda: ops.csr_lognorm_stats(cT, ones), 3)
    say(f"## the route before: transposed() {fmt(t_T)} + a per-gene reduction over the gene-major copy {fmt(t_m)}, and {cT.nbytes / 1e9:.1f} GB for the copy")
    for name, (t_s, t_q, t_c) in res.items():
        say(f"{name}: percentiles + clipped statistics {t_q[0] + t_c[0]:.2f} ms straight from the layer against {t_T[0] + t_m[0]:.2f} ms for the copy alone")
out_fh.close()
