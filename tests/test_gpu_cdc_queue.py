"""The unit queue of the grouped stage-D launch (csrc/coldeltacor.hip, k_cdc_partial_grouped / launch_grouped): one persistent workgroup
per CU draws (group, column tile) units from eight per-XCD lists and steals from the other lists when its own is empty.

Who evaluates a pair must not show: every case compares a whole call BIT FOR BIT with the same entry point called one group at a time
(GC cells per call: 6 in f64, 8 in f32; the dual-control instances 4 and 6), and holds the Pearson values to the bars of the other stage-D
tests against the CPU oracle (1e-10 absolute in f64, 5e-5 in f32, the same NaN pattern).

One group per call, as a call of GC cells, is served by the one-cell-per-workgroup kernel (a grouped launch needs 4 GC cells and 8
neighbours), whose sums are ordered differently: no grouped result equals it in its last bits, before this queue or after.  Where the
whole call is a grouped launch the reference call therefore names the group under test FIRST and three more groups' worth of other
cells behind it, so that it is a grouped launch too, and only the rows of the group under test are taken from it.  A pair's sums do not
depend on the other members of its group, on its tile or on its place in the launch.  Where the whole call is not a grouped launch
(fewer than 4 GC cells, fewer than 8 neighbours) the reference is the plain GC-cell call.

Outputs start as a sentinel, so a unit that nobody drew shows as rows that were never written."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSC = 1e-10
BAR = {"float64": 1e-10, "float32": 5e-5}
SENTINEL = 7.0                                                   # no correlation
DTYPES = ["float64", "float32"]


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def _gc(dtype, entry):
    text = open(os.path.join(ROOT, "velocyto.py_amd", "csrc", "coldeltacor.hip")).read()
    c = dict((k, int(v)) for k, v in re.findall(r"\b(GRP_[A-Z0-9_]+) = (\d+)", text))
    if dtype == "float64":
        return c["GRP_GC_DUAL_F64"] if entry == "dual" else c["GRP_GC_F64"]
    return c["GRP_GC_DUAL"] if entry == "dual" else c["GRP_GC"]


_problems = {}


def _problem(ops, dtype, C, G, ixs, seed):
    """Made once per key and never written: count-like pooled rows (exact zeros), d, a control d2, and Ux / gamma / q for the fused entry;
    rounded to the storage type first, so that the oracle sees what the kernels see.  ixs: (C, nrndm), rows ascending."""
    key = (dtype, C, G, seed, ixs.shape[1])
    if key in _problems:
        return _problems[key]
    rng = np.random.default_rng(seed)
    npdt = np.dtype(dtype)
    e = (rng.gamma(2.0, 1.0, (C, G)) * (rng.random((C, G)) < 0.6)).astype(npdt).astype(np.float64)
    u = (rng.gamma(2.0, 0.5, (C, G)) * (rng.random((C, G)) < 0.5)).astype(npdt).astype(np.float64)
    d = rng.normal(size=(C, G)).astype(npdt).astype(np.float64)
    d2 = rng.normal(size=(C, G)).astype(npdt).astype(np.float64)
    ixs = np.sort(ixs, axis=1)
    p = dict(dtype=dtype, C=C, G=G, e=e, d=d, d2=d2, ixs=ixs, ix=torch.as_tensor(ixs.astype(np.int32)).cuda(),
             E=ops.CellMatrix.from_cells_major(e, dtype), D=ops.CellMatrix.from_cells_major(d, dtype),
             D2=ops.CellMatrix.from_cells_major(d2, dtype), U=ops.CellMatrix.from_cells_major(u, dtype),
             gam=torch.as_tensor(rng.gamma(2.0, 0.3, G).astype(np.float32)), q=torch.as_tensor(rng.gamma(1.0, 0.05, G).astype(np.float32)),
             want={}, ref={})
    _problems[key] = p
    return p


def _want(ops, oracle, p, entry):
    """Oracle values of an entry's outputs, computed once."""
    if entry not in p["want"]:
        eT = np.ascontiguousarray(p["e"].T)

        def corr(x):
            return oracle.coldeltacor_partial_compact(eT, np.ascontiguousarray(x.T), p["ixs"], "sqrt", PSC)
        if entry == "single":
            p["want"][entry] = (corr(p["d"]),)
        elif entry == "dual":
            p["want"][entry] = (corr(p["d"]), corr(p["d2"]))
        else:
            dm = ops.velocity_chain(p["E"], p["U"], p["gam"], p["q"], want=("dmat",), transform=ops.SQRT, psc=PSC)["dmat"]
            p["want"][entry] = (corr(dm.t[:, :p["G"]].double().cpu().numpy()),)     # the d the fused launch builds while staging, as stored
    return p["want"][entry]


def _outs(p, entry):
    return tuple(torch.full(tuple(p["ix"].shape), SENTINEL, dtype=getattr(torch, p["dtype"]), device="cuda") for _ in range(2 if entry == "dual" else 1))


def _call(ops, p, entry, order, outs):
    kw = dict(order=order, validate=False, presorted=True)
    if entry == "single":
        ops.coldeltacor_partial(p["E"], p["D"], p["ix"], ops.SQRT, ops.RULES_PARTIAL, PSC, out=outs[0], **kw)
    elif entry == "fused":
        ops.coldeltacor_partial_fused(p["E"], p["U"], p["gam"], p["q"], p["ix"], ops.SQRT, ops.RULES_PARTIAL, PSC, out=outs[0], **kw)
    else:
        ops.coldeltacor_partial_dual(p["E"], p["D"], p["D2"], p["ix"], ops.SQRT, ops.RULES_PARTIAL, PSC, out=outs[0], out_rndm=outs[1], **kw)
    return outs


def _by_groups(ops, p, entry, order):
    """The reference: the entry called one group of the schedule at a time (module docstring).  Computed once per (entry, schedule)."""
    order = np.arange(p["C"]) if order is None else np.asarray(order)
    key = (entry, order.tobytes())
    if key in p["ref"]:
        return p["ref"][key]
    GC = _gc(p["dtype"], entry)
    grouped = len(order) >= 4 * GC and p["ix"].shape[1] >= 8
    ref, tmp = _outs(p, entry), _outs(p, entry)
    for g0 in range(0, len(order), GC):
        mine = order[g0:g0 + GC]
        sched = mine
        if grouped:                                              # the group under test first, then other cells of the schedule
            others = np.concatenate([order[g0 + GC:], order[:g0]])[:4 * GC - len(mine)]
            sched = np.concatenate([mine, others])
        _call(ops, p, entry, torch.as_tensor(sched.astype(np.int32)), tmp)
        rows = torch.as_tensor(mine.astype(np.int64)).cuda()
        for r, t in zip(ref, tmp):
            r[rows] = t[rows]
    p["ref"][key] = ref
    return ref


def _same_bits(a, b):
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return torch.equal(a.view(it), b.view(it))


def _check(ops, oracle, p, entry, what, order=None, got=None):
    """A whole call (or `got`, the outputs of one) against the oracle and, bit for bit, against the calls group by group."""
    got = _call(ops, p, entry, None if order is None else torch.as_tensor(np.asarray(order, dtype=np.int32)), _outs(p, entry)) if got is None else got
    rows = np.arange(p["C"]) if order is None else np.asarray(order)
    for k, (g, w, r) in enumerate(zip(got, _want(ops, oracle, p, entry), _by_groups(ops, p, entry, order))):
        gn = g.double().cpu().numpy()
        rest = np.setdiff1d(np.arange(p["C"]), rows)
        assert (gn[rest] == SENTINEL).all(), (what, "rows outside the schedule were written")
        gn, w = gn[rows], w[rows]
        ok = ~np.isnan(w)
        err = float(np.abs(gn[ok] - w[ok]).max()) if ok.any() else 0.0
        print(f"{what} {entry}[{k}]: max |r - oracle| {err:.3g} over {int(ok.sum())} pairs, NaN in the oracle {int((~ok).sum())}, here {int(np.isnan(gn).sum())}")
        assert np.array_equal(np.isnan(gn), ~ok), what
        assert err <= BAR[p["dtype"]], (what, err)
        assert _same_bits(g, r), (what, entry, k, "differs from the calls group by group")
    return got


def _random_lists(C, nr, seed):
    rng = np.random.default_rng(seed)
    ixs = np.stack([rng.choice(C, nr, replace=False) for _ in range(C)]) if nr <= C else rng.integers(0, C, (C, nr))
    ixs[0, 0] = 0                                                # a cell that lists itself: zero variance in A, NaN
    return ixs


# --------------------------------------------------------------------------- how many units, against how many workgroups and lists
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [13, 32, "GC"])
def test_fewer_groups_than_lists(ops, oracle, dtype, C):
    """13 cells and exactly one group (both below the grouped launch: the one-cell kernel, unchanged), and 32 cells: 6 groups in f64,
    4 in f32 - fewer units than the eight lists, some lists empty from the start, every workgroup after the first few finds nothing."""
    C = _gc(dtype, "single") if C == "GC" else C
    p = _problem(ops, dtype, C, 130, _random_lists(C, 8, 1), 1)
    _check(ops, oracle, p, "single", f"{dtype} C {C}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nr", [4, 8])
def test_more_units_than_workgroups(ops, oracle, dtype, nr):
    """1 800 cells x 64 genes: 300 groups in f64, 225 in f32.  4 neighbours is the size the issue names (below the grouped launch's 8:
    the one-cell kernel); 8 neighbours is the same shape on the queue - more units than the 256 persistent workgroups in f64, so
    workgroups loop, and the groups beyond the full round are narrow tail units at the end of every list."""
    p = _problem(ops, dtype, 1800, 64, _random_lists(1800, nr, 2), 2)
    _check(ops, oracle, p, "single", f"{dtype} C 1800 nrndm {nr}")


# --------------------------------------------------------------------------- chunks and rows of a unit
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["single", "fused", "dual"])
@pytest.mark.parametrize("G", [130, 1025, 2049])
def test_chunks(ops, oracle, dtype, G, entry):
    """48 cells x 16 neighbours; in f64 (1024-gene chunks) 130, 1 025 and 2 049 genes are one chunk, two with a short last one, and three;
    through the single, the fused and the dual-control entry points."""
    p = _problem(ops, dtype, 48, G, _random_lists(48, 16, 3), 3)
    _check(ops, oracle, p, entry, f"{dtype} G {G}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("U", [8, 15, 16, 17, 64, 65, 67, 68, 72])
def test_row_counts(ops, oracle, dtype, U):
    """Every cell lists the same U neighbours, so every group has exactly U rows, each carrying all its members.  U < 16: waves without
    a row at the start of a chunk; 16, 17: one row per wave, one more; up to 64 rows all are tail tickets; 65 .. 67: still no quad;
    68: one quad; 72: two.  (U = 1 cannot be built: a grouped launch has at least 8 neighbours per cell and a neighbour listed twice by
    one member opens a row of its own.)  1 025 genes: two chunks, so the row counter starts twice."""
    C = 32
    p = _problem(ops, dtype, max(C, U), 1025, np.tile(np.arange(U), (max(C, U), 1)), 100 + U)
    _check(ops, oracle, p, "single", f"{dtype} U {U}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_hub(ops, oracle, dtype):
    """One neighbour with the highest index listed by every cell: the last row of every group carries all its members."""
    C = 48
    ixs = _random_lists(C - 1, 15, 4)
    ixs = np.concatenate([np.concatenate([ixs, ixs[:1]]), np.full((C, 1), C - 1)], axis=1)
    p = _problem(ops, dtype, C, 1025, ixs, 4)
    _check(ops, oracle, p, "single", f"{dtype} hub")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_lists_wider_than_a_tile(ops, oracle, dtype):
    """700 cells x 600 neighbours x 64 genes: several column tiles per group, fewer groups than one round, so every unit is a tail piece."""
    p = _problem(ops, dtype, 700, 64, _random_lists(700, 600, 5), 5)
    _check(ops, oracle, p, "single", f"{dtype} nrndm 600")


# --------------------------------------------------------------------------- schedules, streams, calls back to back
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["single", "fused", "dual"])
def test_subset_schedules(ops, oracle, dtype, entry):
    """A schedule that names a strict subset of the cells, in an order of its own; then the sharded overlap shape: two launches over
    complementary subsets, on two streams (each stream has its own list heads), into one output."""
    p = _problem(ops, dtype, 1800, 64, _random_lists(1800, 8, 2), 2)
    rng = np.random.default_rng(6)
    perm = rng.permutation(1800)
    a, b = perm[:1100], perm[1100:]
    _check(ops, oracle, p, entry, f"{dtype} subset", order=a)
    outs = _outs(p, entry)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        _call(ops, p, entry, torch.as_tensor(a.astype(np.int32)).cuda(), outs)
    with torch.cuda.stream(s2):
        _call(ops, p, entry, torch.as_tensor(b.astype(np.int32)).cuda(), outs)
    torch.cuda.synchronize()
    _check(ops, oracle, p, entry, f"{dtype} two launches", order=perm, got=outs)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_same_call_twice_without_synchronisation(ops, oracle, dtype):
    """Two calls back to back on one stream share the eight list heads: the second must find them zeroed, in stream order."""
    p = _problem(ops, dtype, 1800, 64, _random_lists(1800, 8, 2), 2)
    _by_groups(ops, p, "single", None)                           # (the reference first, so that nothing below waits)
    first, second = _outs(p, "single"), _outs(p, "single")
    _call(ops, p, "single", None, first)
    _call(ops, p, "single", None, second)
    _check(ops, oracle, p, "single", f"{dtype} first of two", got=first)
    _check(ops, oracle, p, "single", f"{dtype} second of two", got=second)
