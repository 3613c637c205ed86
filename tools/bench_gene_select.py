"""What the gene selection from CSR count layers costs, each figure beside what it is to be compared with, measured in the same call.
Writes profiles/gene_select.txt (or OUT=...).   usage: [SIZES=200000,1000000] [G=30000] [REPS=5] python tools/bench_gene_select.py

stats:  ops.csr_gene_stats (vcy_csr_gene_stats) on atlas.synth_atlas layers, unmasked and with a cluster-like mask (a contiguous tenth
        and a random tenth of the cells), against
          - the route available before it: CsrCounts.transposed() + a per-gene reduction over the gene-major copy
            (ops.csr_lognorm_stats, the only per-gene CSR reduction the library had), time and extra memory;
          - the rate at which that kernel, the fastest streaming CSR kernel of profiles/csr_pca.txt, reads the SAME layer's gene-major
            copy: bytes/s of the layer (indices + counts) as the figure of merit for both.
        Bytes the stats pass needs: every stored element once (4 B index + 1 or 2 B count), the slab table ((nslab + 1) x 4 B per cell,
        each entry read by the slab's workgroup and its neighbour's) and the row starts (8 B per cell and slab).
select: CsrCounts.select_genes (vcy_csr_select_count + cumsum + vcy_csr_select_fill) keeping 3 000 of the genes (what
        score_cv_vs_mean leaves) and a random half, against the torch mask route (remap[indices] >= 0, nonzero, gather): time and
        the torch.cuda.max_memory_allocated delta of each, next to the size of the output and of the C- and G-sized temporaries.
Times are device events around the call after a warm-up call, median of REPS (min .. max).  A 1M-cell size is skipped when the layers
and the comparison routes do not fit the free memory."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import smi_sample
from velocyto_amd import _lib, atlas, ops

G = int(os.environ.get("G", 30000))
REPS = int(os.environ.get("REPS", 5))
SIZES = [int(s) for s in os.environ.get("SIZES", "200000,1000000").split(",")]
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gene_select.txt"))
dev = ops.require_gpu()
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


def peak_extra(fn):
    """(result, bytes): the most memory allocated during fn() above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    res = fn()
    torch.cuda.synchronize()
    return res, torch.cuda.max_memory_allocated(dev) - before


def fmt(t):
    return f"{t[0]:9.2f} ms ({t[1]:.2f} .. {t[2]:.2f})"


def torch_mask_route(c, remap):
    """The column subset as index plumbing: what a user would write without the kernels."""
    new = remap[c.indices.long()]
    keep = new >= 0
    pos = torch.nonzero(keep).squeeze(1)
    cs = torch.zeros(c.nnz + 1, dtype=torch.int64, device=dev)
    torch.cumsum(keep, 0, dtype=torch.int64, out=cs[1:])
    return ops.CsrCounts(cs[c.indptr], new[pos], c.data[pos], int(remap.max()) + 1)


def part(C):
    free = torch.cuda.mem_get_info(dev)[0]
    need = C * G * 0.085 * 6 * 2 * 3.5                       # both layers; the gene-major copy and the mask route's temporaries beside them
    if need > free:
        say(f"## {C} cells x {G} genes: skipped, about {need / 1e9:.0f} GB needed beside the rest, {free / 1e9:.0f} GB free")
        return
    t0 = time.perf_counter()
    cS, cU, *_ = atlas.synth_atlas(C, G, 4, dev, density=0.08)
    del cU, _
    torch.cuda.empty_cache()
    es = cS.data.element_size()
    nslab = (G + int(_lib.lib().vcy_csr_slab_genes()) - 1) // int(_lib.lib().vcy_csr_slab_genes())
    layer_b = cS.nnz * (4 + es)
    say(f"## {C} cells x {G} genes: {cS.nnz} stored elements ({100 * cS.nnz / C / G:.2f} %), {layer_b / 1e9:.2f} GB of indices + "
        f"{'uint8' if es == 1 else 'uint16'} counts   [generated in {time.perf_counter() - t0:.1f} s]")
    # ---------------------------------------------------------------- stats
    t_slab = timed(lambda: (setattr(cS, "_slabptr", None), cS.slabptr), 3)
    stats_b = layer_b + C * (nslab + 1) * 4 * 2 + C * nslab * 8
    ws_b = int(_lib.lib().vcy_csr_gene_stats_workspace_bytes(C, G))
    say(f"slab table (vcy_csr_slab_ptr, once per layer, shared with the pooling): {fmt(t_slab)}, {cS.slabptr.numel() * 4 / 1e6:.0f} MB")
    t = timed(lambda: ops.csr_gene_stats(cS))
    say(f"csr_gene_stats, all cells:              {fmt(t)}   needs {stats_b / 1e9:.2f} GB -> {stats_b / t[0] / 1e9:.3f} TB/s "
        f"({layer_b / t[0] / 1e9:.3f} TB/s of the layer); workspace {ws_b / 1e6:.0f} MB in "
        f"{(C + int(_lib.lib().vcy_csr_gene_stats_block_cells()) - 1) // int(_lib.lib().vcy_csr_gene_stats_block_cells())} tiles")
    st = ops.csr_gene_stats(cS)
    for name, mask in (("a contiguous tenth of the cells", torch.arange(C, device=dev) < C // 10),
                       ("a random tenth of the cells", torch.rand(C, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) < 0.1)):
        m8 = mask.to(torch.uint8)
        tm = timed(lambda: ops.csr_gene_stats(cS, m8))
        rows = mask.nonzero().squeeze(1)
        part_b = int((cS.indptr[rows + 1] - cS.indptr[rows]).sum()) * (4 + es)
        say(f"csr_gene_stats, {name:31s}: {fmt(tm)}   {part_b / 1e9:.2f} GB of elements in the selected rows -> {part_b / tm[0] / 1e9:.3f} TB/s of them; "
            f"x{t[0] / tm[0]:.1f} faster than the unmasked pass")
    # the route available before: gene-major copy + per-gene reduction over it
    ones = torch.ones(C, dtype=torch.float64, device=dev)
    cT, extra_T = peak_extra(lambda: cS.transposed())
    t_T = timed(lambda: cS.transposed(), 3)
    t_m = timed(lambda: ops.csr_lognorm_stats(cT, ones))
    say(f"before: transposed()                    {fmt(t_T)}   peak extra memory {extra_T / 1e9:.2f} GB (the copy itself {cT.nbytes / 1e9:.2f} GB)")
    say(f"before: csr_lognorm_stats on the copy   {fmt(t_m)}   {layer_b / t_m[0] / 1e9:.3f} TB/s of the layer - the streaming rate of the CSR kernels "
        f"of profiles/csr_pca.txt on this layer (sum and sum of squares of log2(c + 1) only: no detection count, no maximum, no mask)")
    say(f"csr_gene_stats against transposed() + reduction: {t[0]:.2f} ms against {t_T[0] + t_m[0]:.2f} ms = x{(t_T[0] + t_m[0]) / t[0]:.1f}; against the reduction "
        f"alone (copy already there): x{t_m[0] / t[0]:.2f}; rate of the layer {layer_b / t[0] / 1e9:.3f} TB/s against {layer_b / t_m[0] / 1e9:.3f} TB/s")
    # cross-check at the size timed: the unmasked sums against the gene-major copy's row lengths and torch's integer sums
    assert torch.equal(st[2], (cT.indptr[1:] - cT.indptr[:-1]).double()), "detection counts differ from the gene-major copy's row lengths"
    assert float(st[0].sum()) == float(cS.row_sums().sum()), "total of the per-gene sums differs from the total of the per-cell sums"
    del cT
    torch.cuda.empty_cache()
    # ---------------------------------------------------------------- select
    gen = np.random.default_rng(7)
    for name, keep in ((f"3000 of {G} genes", np.isin(np.arange(G), gen.choice(G, min(3000, G), replace=False))), ("a random half", gen.random(G) < 0.5)):
        remap_h, G_new = ops.gene_remap(keep, G)
        remap = torch.from_numpy(remap_h).to(dev)
        sub, extra = peak_extra(lambda: cS.select_genes(keep))
        out_b, small_b = sub.nbytes, G * 4 + C * 8
        ts = timed(lambda: cS.select_genes(keep))
        try:
            ref, extra_ref = peak_extra(lambda: torch_mask_route(cS, remap))
            tr = timed(lambda: torch_mask_route(cS, remap), 3)
        except RuntimeError as e:                            # what torch refuses at this size is part of the comparison
            ref = None
            torch.cuda.empty_cache()
            err = str(e).splitlines()[0][:160]
        assert ref is None or (torch.equal(sub.indptr, ref.indptr) and torch.equal(sub.indices, ref.indices) and torch.equal(sub.data, ref.data))
        say(f"select_genes, {name:19s}: {fmt(ts)}   peak extra memory {extra / 1e6:.1f} MB = output {out_b / 1e6:.1f} MB + {(extra - out_b) / 1e6:.1f} MB "
            f"(remap G x 4 B + row_len C x 8 B = {small_b / 1e6:.1f} MB; indptr_out is part of the output); reads {layer_b / 1e9:.2f} GB + {cS.nnz * 4 / 1e9:.2f} GB of "
            f"indices again -> {(layer_b + cS.nnz * 4 + out_b) / ts[0] / 1e9:.3f} TB/s")
        if ref is None:
            say(f"torch mask route, {name:15s}: failed at this size: {err}")
            del sub
            continue
        say(f"torch mask route, {name:15s}: {fmt(tr)}   peak extra memory {extra_ref / 1e6:.1f} MB = x{extra_ref / max(extra, 1):.1f} ({(extra_ref - out_b) / cS.nnz:.1f} B of "
            f"temporaries per stored element); time x{tr[0] / ts[0]:.1f}")
        del sub, ref
        torch.cuda.empty_cache()
    say()
    del cS
    torch.cuda.empty_cache()


say(f"# tools/bench_gene_select.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  "
    f"tile {_lib.lib().vcy_csr_gene_stats_block_cells()} cells x slab {_lib.lib().vcy_csr_slab_genes()} genes, median of {REPS} (min .. max)")
say("smi before: " + json.dumps(smi_sample()))
for C in SIZES:
    part(C)
say("smi after: " + json.dumps(smi_sample()))
out_fh.close()
