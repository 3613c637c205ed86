#!/usr/bin/env python3
"""Table of idle time in one grouped stage-D launch, from the stamps of the VCY_EXP=30 build (stage_d_idle_stamps.patch):
usage: VCY_CDC_STAMPS=<file> python bench.py --gpus 1 --steps 1 --warmup 1 --no-extra --no-cpu-baseline   (library built with -DVCY_EXP=30)
       python tools/experiments/stage_d_idle.py <file> [label]
Stamps are the 100 MHz real-time counter.  Per unit: XCD it ran on, start, end, rows, the list it was drawn from; per workgroup: the time
it found every list empty; per wave and chunk of every 16th unit of each list: after barrier 1, after barrier 2, first row arrived, last
row finished."""
import sys
import numpy as np

d = np.fromfile(sys.argv[1], dtype=np.uint64)
label = sys.argv[2] if len(sys.argv) > 2 else ""
nunits, W, SC, es = (int(x) for x in d[:4])
body = d[4:]
units = body[:nunits * 8].reshape(nunits, 8).astype(np.int64)
wg = body[nunits * 8:nunits * 8 + 1024].reshape(512, 2).astype(np.int64)
st = body[nunits * 8 + 1024:].reshape(-1, SC, 16, 4).astype(np.int64)
ran = units[:, 0] > 0
wg = wg[wg[:, 0] > 0]
us = 0.01                                                        # microseconds per tick
t0 = units[ran, 1].min()
end = wg[:, 1].max()
launch = (end - t0) * us
print(f"== {label}: {nunits} units ({int(ran.sum())} with a group), {len(wg)} workgroups, element {es} bytes; launch (first unit start -> last workgroup out) {launch / 1e3:.3f} ms")
xr, owner = units[:, 0] - 1, units[:, 5] - 1
stolen = ran & (xr != owner)
print(f"units evaluated on another XCD than the one that owns their list: {int(stolen.sum())} of {int(ran.sum())}")
rule = np.array([np.bincount((units[ran & (xr == x), 7] % 8), minlength=8).argmax() if (ran & (xr == x)).any() else -1 for x in range(8)])
share = np.mean([(units[ran & (xr == x), 7] % 8 == rule[x]).mean() for x in range(8) if rule[x] >= 0])
print(f"workgroup -> XCD: hardware id x runs blockIdx % 8 = {rule.tolist()} (share of units that follow it {share:.3f})")
print("per XCD (hardware id): units run, of them drawn from other lists, rows, last unit finished [ms], workgroups out first / mean / last [ms], idle CU-time after the workgroups left [CU-ms]")
idle_all = 0.0
for x in range(8):
    m = ran & (xr == x)
    w = wg[wg[:, 0] - 1 == x]
    out = (w[:, 1] - t0) * us / 1e3
    idle = float(((end - w[:, 1]) * us / 1e3).sum())
    idle_all += idle
    print(f"  xcd {x}: {int(m.sum()):5d} {int((m & stolen).sum()):4d} {int(units[m, 3].sum()):8d}   {(units[m, 2].max() - t0) * us / 1e3:8.3f}   {out.min():8.3f} {out.mean():8.3f} {out.max():8.3f}   {idle:7.2f}")
print(f"idle CU-time at the end of the launch: {idle_all:.1f} CU-ms = {100 * idle_all / (len(wg) * launch / 1e3):.2f} % of {len(wg)} CUs x launch")
gap = []
for b in np.unique(units[ran, 7]):
    u = units[ran & (units[:, 7] == b)]
    u = u[np.argsort(u[:, 1])]
    gap.append(((u[1:, 1] - u[:-1, 2]) * us).sum())
print(f"between units (end of one -> start of the next on the same workgroup, the draw included): {np.mean(gap) / 1e3:.3f} ms per workgroup = {100 * np.mean(gap) / launch:.2f} % of the launch")
# chunks of the sampled units
rows = []
for unit in np.nonzero(ran & (((np.arange(nunits) >> 3) & 15) == 0))[0]:
    s = st[(unit >> 7) * 8 + (unit & 7)]
    nch = int(units[unit, 4])
    if nch < 1 or (s[:nch + 1, :, 0] == 0).any():
        continue
    for c in range(nch):
        period = s[c + 1, :, 0].mean() - s[c, :, 0].mean()
        w1 = s[c + 1, :, 0] - s[c, :, 3]                       # last row finished -> through the barrier the rows end at
        stg = s[c, :, 1] - s[c, :, 0]                            # staging + barrier 2
        rst = s[c, :, 2] - s[c, :, 1]                            # barrier 2 -> first row's data in registers
        rws = s[c, :, 3] - s[c, :, 2]
        rows.append([period, w1.mean(), w1.max(), stg.mean(), stg.max(), rst.mean(), rst.max(), rws.mean(), int(units[unit, 3])])
r = np.array(rows, dtype=np.float64)
r[:, :8] *= us
print(f"chunks: {len(r)} of {len(np.unique(np.nonzero(ran & (((np.arange(nunits) >> 3) & 15) == 0))[0]))} sampled units; mean rows per unit {r[:, 8].mean():.0f}; times in microseconds, per wave, "
      "mean over chunks of (mean over the 16 waves | max over the 16 waves)")
P = r[:, 0].mean()
for name, a, b in (("wait at the chunk-end barrier (last row finished -> barrier passed)", 1, 2), ("member staging + barrier 2", 3, 4),
                   ("restart (barrier 2 -> first row's data arrived)", 5, 6)):
    print(f"  {name:70s} {r[:, a].mean():7.2f} | {r[:, b].mean():7.2f}   = {100 * r[:, a].mean() / P:5.2f} % | {100 * r[:, b].mean() / P:5.2f} % of the chunk period")
print(f"  {'rows (first row arrived -> last row finished)':70s} {r[:, 7].mean():7.2f}             = {100 * r[:, 7].mean() / P:5.2f} %")
print(f"  chunk period {P:.2f}")
