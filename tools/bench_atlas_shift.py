"""What AtlasPath(shift=True) adds to a pass, and the fused stage-E kernel against the materialised route it replaces.
Writes profiles/atlas_shift.txt (or OUT=...).   usage: [PART=kernel,path] [SIZES=200000x4,resident] [G=30000] [STEPS=2] [KERNEL_CELLS=100000]
                                                       python tools/bench_atlas_shift.py

kernel: on ONE resident block of KERNEL_CELLS cells (a one-block AtlasPath after a run, so Sx, Ux, gamma, the neighbour lists and the
        weights are a real pass's), f32 and f64: vcy_embedding_scaling_fused against velocity_chain(want=delta_S) + vcy_embedding_scaling
        on the materialised matrix (its two launches timed apart), median of 5 (min .. max), shader clock during the launch; and the
        other launches of stage E (corr copy + fix-up, vcy_transition_prob).  Checks that the two routes return the same bits.
path:   AtlasPath.run(timed=True) with shift=False (the pass as it was) and shift=True ALTERNATING in one process on one object:
        wall time per run between device synchronisations, the four stage times and stage_e_ms."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import smi_sample
from velocyto_amd import atlas, ops

G = int(os.environ.get("G", 30000))
STEPS = int(os.environ.get("STEPS", 2))
PARTS = os.environ.get("PART", "kernel,path").split(",")
SIZES = os.environ.get("SIZES", "200000x4,resident").split(",")
KERNEL_CELLS = int(os.environ.get("KERNEL_CELLS", 100000))
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "atlas_shift.txt"))
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


def part_kernel():
    C = KERNEL_CELLS
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(C, G, 30, dev, density=0.08)
    fS, fU = atlas.size_factors(totS, totU, C)
    for dt in (torch.float32, torch.float64):
        path = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, k=30, n_neighbors=500, sampled_fraction=0.5, block_cells=0, dtype=dt, shift=True)
        path.run()
        e_buf, Ux_b = path._resident
        ixs, gamma, n = path._plan[0][3], path.gamma, path.nrndm
        es = e_buf.t.element_size()
        say(f"## stage E on one resident block: {C} cells x {G} genes, lists of {n}, {dt}; median of 5 (min .. max)")
        fixed = path.corr.clone()
        ops.corr_fixup(fixed, path.neigh)
        _, wd, _ = ops.transition_prob(fixed, path.neigh, emb, path.sigma_corr)
        dS = ops.velocity_chain(e_buf, Ux_b, gamma, None, want=("delta_S",))["delta_S"]
        (a,) = ops.embedding_scaling(e_buf, dS, ixs, wd, validate=False)
        (b,) = ops.embedding_scaling_fused(e_buf, Ux_b, gamma, None, ixs, wd, validate=False)
        same = torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
        say(f"fused == materialised, bit for bit: {same}; scaling > 0 on {100 * float((b > 0).float().mean()):.0f} % of the cells, NaN on {int(torch.isnan(b).sum())}")
        del dS
        rows = {}
        for name, fn in (("vcy_embedding_scaling_fused", lambda: ops.embedding_scaling_fused(e_buf, Ux_b, gamma, None, ixs, wd, validate=False)),
                         ("vcy_velocity_chain(delta_S)", lambda: ops.velocity_chain(e_buf, Ux_b, gamma, None, want=("delta_S",))),
                         ("vcy_embedding_scaling", None),
                         ("corr copy + vcy_corr_fixup", lambda: ops.corr_fixup(path.corr.clone(), path.neigh)),
                         ("vcy_transition_prob", lambda: ops.transition_prob(fixed, path.neigh, emb, path.sigma_corr))):
            if fn is None:
                dS = ops.velocity_chain(e_buf, Ux_b, gamma, None, want=("delta_S",))["delta_S"]
                fn = lambda: ops.embedding_scaling(e_buf, dS, ixs, wd, validate=False)
            med, lo, hi = timed(fn)
            rows[name] = med
            say(f"{name:30s} {med:9.2f} ms ({lo:.2f} .. {hi:.2f})   shader clock {clock_during(fn, med):.2f} GHz")
        mat = rows["vcy_velocity_chain(delta_S)"] + rows["vcy_embedding_scaling"]
        say(f"materialised route {mat:.2f} ms and a third block-sized buffer of {C * e_buf.ld * es / 1e9:.1f} GB; fused {rows['vcy_embedding_scaling_fused']:.2f} ms "
            f"= x{rows['vcy_embedding_scaling_fused'] / mat:.3f} of it, x{rows['vcy_embedding_scaling_fused'] / rows['vcy_embedding_scaling']:.3f} of the unfused launch alone")
        say()
        del path, e_buf, Ux_b, dS, fixed, wd
        torch.cuda.empty_cache()


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
    path = atlas.AtlasPath(cS, cU, fS, fU, pcs, emb, k=30, n_neighbors=500, sampled_fraction=0.5, block_cells=block, shift=True)
    say(f"## AtlasPath.run(timed=True), {C} cells x {G} genes, f32, {len(path.blocks())} block(s) of {path.block_cells} cells (setup {time.perf_counter() - t0:.0f} s); "
        f"ONE object, its shift switched between runs: shift=False (the pass as it was) and shift=True alternating, {STEPS} timed runs each after one warm-up each")
    modes = (False, True)
    wall, stage, st_e = {m: [] for m in modes}, {m: np.zeros(4) for m in modes}, {m: 0.0 for m in modes}
    for m in modes:
        path.shift = m
        path.run(); torch.cuda.synchronize()
    for _ in range(STEPS):
        for m in modes:
            path.shift = m
            before, before_e = path.stage_ms.copy(), path.stage_e_ms
            torch.cuda.synchronize(); t0 = time.perf_counter()
            path.run(timed=True)
            torch.cuda.synchronize(); wall[m].append((time.perf_counter() - t0) * 1e3)
            stage[m] += path.stage_ms - before
            st_e[m] += path.stage_e_ms - before_e
    for m in modes:
        st = stage[m] / STEPS
        say(f"shift={str(m):5s} wall {np.median(wall[m]):9.1f} ms/run ({min(wall[m]):.1f} .. {max(wall[m]):.1f})   stage ms: A pooling {st[0]:.1f}  B fit {st[1]:.1f}  "
            f"A kNN search {st[2]:.1f}  D {st[3]:.1f}  E {st_e[m] / STEPS:.1f}")
    a, b = np.median(wall[True]), np.median(wall[False])
    say(f"shift=True over shift=False: +{a - b:.1f} ms per run = x{a / b:.3f}; scaling > 0 on {100 * float((path.scaling > 0).float().mean()):.0f} % of the cells")
    say()
    del path, cS, cU
    torch.cuda.empty_cache()


say(f"# tools/bench_atlas_shift.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}")
say("smi before: " + json.dumps(smi_sample()))
if "kernel" in PARTS:
    part_kernel()
if "path" in PARTS:
    for spec in SIZES:
        part_path(spec)
say("smi after: " + json.dumps(smi_sample()))
out_fh.close()
