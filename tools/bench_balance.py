"""What the balanced kNN selection costs on the device (ops.balance_knn_device, csrc/balance.hip) beside the route it stands next to
(ops.balance_knn_device_lists: int32 host copy of the sight lists + the sequential loop vcy_balance_knn_host32), in the same run on the
same lists.  Writes profiles/balance_knn.txt (or OUT=...).   usage: [INPUTS=cfg2,whole50k,synth1m,tight20k,hubs20k] [REPS=3] python tools/bench_balance.py

cfg2      the sight lists of BASELINE.json configs[1]: 10 000 cells of bench.synth_counts_survey(cfg=2), 30 PCs, k = 30, sight 240, maxl 120
whole50k  50 000 cells (12 Gaussian clusters in 10 dimensions), k = 30, knn_imputation's default: sight and maxl of the whole dataset
synth1m   1 000 000 x 241 synthetic clustered lists (clusters of 2 048 cells; a cell lists itself and 240 cells of its cluster drawn
          without replacement with log-normal node weights, so that some nodes are in far more lists than maxl = 120), k = 30
tight20k  20 000 cells of the same 12 clusters, sight 240, k = 30, maxl = 35: a cap barely above k, most nodes capped (the kind of input
          that takes the most rounds)
hubs20k   20 000 iid Gaussian points in 50 dimensions (hubs), sight 240, k = 30, maxl = 40
Per input: the rounds to the fixed point; milliseconds per round split into the walk (vcy_balance_select), the sort of the C * k keys
(torch.sort) and the thresholds (vcy_balance_thresholds), device events, median over the rounds of REPS runs; the whole call of both
routes, wall clock between device syncs, best of REPS; the bytes each route moves to or holds on the host.  Both routes' results are
compared before anything is reported."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from velocyto_amd import _lib, ops

REPS = int(os.environ.get("REPS", 3))
INPUTS = os.environ.get("INPUTS", "cfg2,whole50k,synth1m,tight20k,hubs20k").split(",")
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "balance_knn.txt"))
dev = ops.require_gpu()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
out_fh = open(OUT, "w")


def say(s=""):
    print(s, flush=True)
    out_fh.write(s + "\n")
    out_fh.flush()


def wall(fn):
    best, res = float("inf"), None
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, res


def clustered_space(C, P=10, clusters=12, seed=11):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 4.0, (clusters, P))
    return centres[rng.integers(0, clusters, C)] + rng.normal(size=(C, P))


def synthetic_lists(C, K, size=2048, seed=5):
    """(C, K) int32 lists: column 0 the cell, then K - 1 distinct cells of its cluster (contiguous blocks of `size` cells), drawn by
    Efraimidis-Spirakis keys u^(1 / w) with log-normal node weights w - a few nodes are wanted by most of their cluster."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((C, K), dtype=torch.int32, device=dev)
    for a in range(0, C, size):
        n = min(size, C - a)
        w = torch.exp(1.5 * torch.randn(n, device=dev, generator=gen))
        keys = torch.rand((n, n), device=dev, generator=gen).log() / w[None, :]
        keys.fill_diagonal_(float("inf"))                          # the cell itself first
        out[a:a + n] = (torch.topk(keys, K, dim=1).indices + a).to(torch.int32)
    return out


def rounds_timed(idx, maxl, k):
    """The round loop of ops.balance_knn_positions with device events around its three steps: (rounds, [(walk, sort, thresholds) ms])."""
    C, K = idx.shape
    L = _lib.lib()
    lsi = ops._balance_order(idx)
    rank = torch.empty(C, dtype=torch.int32, device=dev)
    rank[lsi] = torch.arange(C, dtype=torch.int32, device=dev)
    keys = torch.empty(C * k, dtype=torch.int64, device=dev)
    sel = [torch.empty(C * k, dtype=torch.int32, device=dev) for _ in range(2)]
    s, l = torch.empty(C, dtype=torch.int32, device=dev), torch.empty(C, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    st = torch.cuda.current_stream().cuda_stream
    rounds, prev, times = 0, None, []
    while True:
        cur = sel[rounds & 1]
        ev[0].record()
        _lib.check(L.vcy_balance_select(idx.data_ptr(), idx.stride(0), rank.data_ptr(), None if prev is None else s.data_ptr(), None,
                                        None if prev is None else prev.data_ptr(), cur.data_ptr(), keys.data_ptr(), flag.data_ptr(), C, K, k, st))
        ev[1].record()
        rounds += 1
        if not int(flag.item()) & 1:
            times.append((ev[0].elapsed_time(ev[1]), 0.0, 0.0))
            return rounds, times
        sk = torch.sort(keys).values
        ev[2].record()
        _lib.check(L.vcy_balance_thresholds(sk.data_ptr(), s.data_ptr(), l.data_ptr(), C, k, maxl, st))
        ev[3].record()
        torch.cuda.synchronize()
        times.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])))
        prev = cur


def part(name, idx, dist, maxl, k):
    C, K = idx.shape
    say(f"## {name}: {C} cells, sight lists (C, {K}) int32 = {C * K * 4 / 1e9:.2f} GB, k = {k}, maxl = {maxl}")
    stats = {}
    t_dev, got = wall(lambda: ops.balance_knn_device(idx, dist, maxl, k, stats=stats))
    t_host, want = wall(lambda: ops.balance_knn_device_lists(idx, dist, maxl, k))
    same = all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    assert same, "the two routes disagree"
    per = []
    for _ in range(REPS):
        rounds, times = rounds_timed(idx, maxl, k)
        assert rounds == stats["rounds"]
        per += times[:-1] if len(times) > 1 else times
    walk, srt, thr = (float(np.median([p[i] for p in per])) for i in range(3))
    say(f"rounds to the fixed point: {stats['rounds']} (the last one confirms), fell back: {stats['fell_back']}; results of both routes equal: {same}")
    say(f"per round, median of {len(per)}: walk {walk:.3f} ms, sort of {C * k} keys {srt:.3f} ms, thresholds {thr:.3f} ms")
    say(f"balance_knn_device       (device, whole call): {t_dev:10.2f} ms   host traffic: 4 bytes per round")
    say(f"balance_knn_device_lists (host loop, whole call): {t_host:10.2f} ms   host memory: {C * K * 4 / 1e9:.2f} GB copy of the lists + "
        f"{C * (k + 1) * 12 / 1e6:.1f} MB of results")
    verdict = f"x{t_host / t_dev:.2f} faster" if t_dev <= t_host else f"SLOWER than the host route on this input, x{t_dev / t_host:.2f}"
    say(f"device against host route: {verdict}")
    say()


say(f"# tools/bench_balance.py  {time.strftime('%Y-%m-%d %H:%M:%S')}  device {torch.cuda.get_device_name(0)}  whole calls: best of {REPS}, wall clock between syncs")
say("smi before: " + json.dumps(bench.smi_sample()))
if "cfg2" in INPUTS:
    pcs = bench.synth_counts_survey(10000, 20000, 30, dev, cfg=2)[4]
    torch.cuda.empty_cache()
    idx, dist = ops.knn_search(pcs, 241, include_self=True)
    part("cfg2 (sight 240)", idx, dist, 120, 30)
    del idx, dist, pcs
if "whole50k" in INPUTS:
    C = 50000
    idx, dist = ops.knn_search(clustered_space(C), C, include_self=True)
    part("50 000 cells, whole-dataset default", idx, dist, C - 1, 30)
    del idx, dist
    torch.cuda.empty_cache()
if "synth1m" in INPUTS:
    # (distances: the position in the list, one row broadcast - both routes only gather k + 1 of them per cell)
    part("synthetic clustered lists", synthetic_lists(1_000_000, 241), torch.arange(241, dtype=torch.float64, device=dev).expand(1_000_000, 241), 120, 30)
for name, space, maxl in (("tight20k", lambda: clustered_space(20000), 35),
                          ("hubs20k", lambda: np.random.default_rng(3).normal(size=(20000, 50)), 40)):
    if name in INPUTS:
        idx, dist = ops.knn_search(space(), 241, include_self=True)
        part(f"{name} (sight 240)", idx, dist, maxl, 30)
        del idx, dist
say("smi after: " + json.dumps(bench.smi_sample()))
out_fh.close()
