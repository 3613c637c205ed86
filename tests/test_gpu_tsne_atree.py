"""The adaptive-tree repulsion of the device t-SNE (csrc/tsne.hip: k_atree_*, k_tsne_atree_repulsion; vcy_tsne_atree_*) against the
numpy restatement of tests/tsne_atree_cases.py, through the C ABI (ops.tsne_atree_*), and DeviceTSNE(tree_depth="adaptive").

Structure is compared bit for bit: the int64 keys, their order, the number of nodes, every node's level, range, skip, leaf flag and
com (read from the workspace, whose layout include/velocyto_hip.h states) and, per target, the number of accepted nodes and of
directly summed points - so every split and every accept / open decision is the specified one.

Sums.  The bounds of tests/test_gpu_tsne_tree.py, unchanged: with u = 2^-24, gamma = (256 + 16) u (a term costs at most 16 f32
roundings, at most 256 terms are added in f32 between two f64 carries) and A, W, Z the oracle's sums over the SAME interaction set,
    force |F - F_ref| <= gamma A       weight sum |W - W_ref| <= gamma W_ref       Z |Z - Z_ref| <= gamma Z_ref,
and at angle 0 against vcy_tsne_gradient's partials on the same points by the sum of the two kernels' bounds:
|F_tree - F_exact| <= gamma (A + A), |W_tree - W_exact| <= gamma (2 W + 1), |Z_tree - Z_exact| <= gamma (2 Z + N).
None of these is fitted to a run.  Coincident points, repeated calls and a NaN-filled workspace carry no tolerance.

The step is compared with vcy_tsne_step's at angle 0 on the decided components, and the fit with the exact mode's by the allowed
excess of tests/test_gpu_tsne_tree.py (2.5 x scikit-learn's own KL(angle 0.5) - KL(angle 0) at that seed).

Recorded on an MI355X (largest error / bound over all cases; a run with -s prints them per input kind, DESIGN.md section 9 has the
context): force 0.060 (clumps of radius 1e-3), W 0.048, Z 0.0093; at angle 0 against the exact kernel force 0.057, W 0.24
(heavy-tailed), Z 0.010; step against the exact step update 0.076, position 0.75, Z 0.00098, no undecided component; fit: exact KL
of the adaptive fit 1.39558 at the default leaf_size 32 against 1.40070 for the exact mode (excess -0.0051, allowed 0.0154; at
leaf_size 8 the same fit ends at 1.42249, above the allowance - profiles/tsne_atree.txt has seeds 0-2 and leaf sizes 1-32).
"""
import types

import numpy as np
import pytest

import tsne_atree_cases as ac

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
U, GAMMA = ac.U, ac.GAMMA
RECORD = {}
_dev_cache = {}

# scikit-learn 1.7.2's own spread on blobs() at seed 0 and the margin over it: the figures of tests/test_gpu_tsne_tree.py
FIT_SPREAD = 0.006173
FIT_MARGIN = 2.5


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd  # noqa: F401
    from velocyto_amd import ops
    ops.require_gpu()
    assert hasattr(ops, "tsne_atree_keys"), "this build has no adaptive tree repulsion"
    yield ops
    if RECORD:
        print("\nlargest error / bound, tests/test_gpu_tsne_atree.py:")
        for k in sorted(RECORD):
            print(f"  {k}: {RECORD[k]:.3g}")


def note(name, value):
    RECORD[name] = max(RECORD.get(name, 0.0), float(value))


def within(name, err, bound):
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    assert np.all(np.isfinite(err)), name
    zero = bound == 0
    assert not np.any(err[zero] != 0), (name, "error where the bound is 0")
    r = float(np.max(err[~zero] / bound[~zero], initial=0.0))
    note(name, r)
    assert r <= 1.0, (name, r)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)             # a copy: the cases' arrays are read only


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def align(b):
    return (b + 127) // 128 * 128


def read_nodes(ws, N, ls, D):
    """The node count (head, byte 132) and the records from the workspace: head 256 bytes, 256 box partials of 16 bytes, then
    1 + 4 D (N // (ls + 1)) records of 32 bytes {start, count, level, skip, com x, com y, leaf, 0}."""
    nn = int(ws[132:136].view(torch.int32).item())
    assert 1 <= nn <= ac.node_bound(N, ls, D)
    off = 256 + align(16 * 256)
    rec = ws[off:off + 32 * nn].view(torch.int32).view(nn, 8).cpu().numpy()
    return dict(start=rec[:, 0].copy(), count=rec[:, 1].copy(), level=rec[:, 2].copy(), skip=rec[:, 3].copy(),
                com=rec[:, 4:6].copy().view(np.float32), leaf=rec[:, 6].copy(), pad=rec[:, 7].copy())


def evaluate(ops, Y, ls, D, angle, ws=None):
    Yd = dev(Y)
    N = Y.shape[0]
    ws = ops.tsne_atree_workspace(N, ls, D) if ws is None else ws
    keys, order, skeys = ops.tsne_atree_keys(Yd, ws, ls, D)
    rep, Z, vis = ops.tsne_atree_repulsion(Yd, order, skeys, ws, angle, ls, D, visits=True)
    return dict(keys=keys, order=order, rep=rep, Z=Z, vis=vis, ws=ws)


def device_case(ops, kind, N, leaf_size, D, angle):
    k = (kind, N, leaf_size, D, angle)
    if k not in _dev_cache:
        Y, t, o = ac.case(kind, N, leaf_size, D, angle)
        _dev_cache[k] = evaluate(ops, Y, t["leaf_size"], D, angle)
    return _dev_cache[k]


def case_id(c):
    return f"{c[0]}-{c[1]}-leaf{'N' if c[2] is None else c[2]}-d{c[3]}"


def test_cases_cover_the_shapes(ops):
    assert {c[1] for c in ac.CASES} >= {2, 3, 63, 64, 65, 127, 129, 1000, 5000}
    assert {c[2] for c in ac.CASES} >= {1, 8, ac.DEFAULT_LEAF, 64, None} and {c[3] for c in ac.CASES} >= {1, 15, 16, 24}
    assert {a for c in ac.CASES for a in c[4]} == {0.0, 0.2, 0.5, 0.8, 1.0}
    assert {c[0] for c in ac.CASES} >= {"normal", "start", "five", "heavy", "clusters", "collinear", "dyadic", "duplicates", "lone", "clumps3", "clumps5"}
    assert ops.TSNE_ATREE_LEAF_SIZE == ac.DEFAULT_LEAF and ops.TSNE_ATREE_MAX_DEPTH == ac.MAX_DEPTH
    assert {(c[1], ac.leaf_of(c[1], c[2])) for c in ac.CASES} >= {(8, 8), (9, 8), (32, 32), (33, 32), (64, 64), (65, 64)}     # N = leaf_size, and the first split
    assert len(ac.case("normal", 8, 8, 24, 0.5)[1]["level"]) == 1 and len(ac.case("normal", 9, 8, 24, 0.5)[1]["level"]) > 1
    _, t, _ = ac.case("clusters", 5000, 8, 24, 0.5)                       # the cluster of 1500 points in a radius of 0.01 is split to the cap
    assert t["count"][t["leaf"]].max() <= 8 and t["level"].max() >= 16
    _, t, _ = ac.case("duplicates", 1000, 1, 24, 0.5)                     # copies chain down to a depth-24 leaf of two points
    assert t["count"][t["leaf"]].max() == 2 and t["level"][t["leaf"] & (t["count"] == 2)].min() == 24
    _, t, _ = ac.case("clumps5", 3000, 8, 24, 0.5)
    assert t["level"].max() == 24 and t["level"][t["leaf"]].min() <= 19
    _, t, o = ac.case("lone", 65, 8, 24, 0.5)
    assert (t["count"][t["leaf"]] == 1).any() and (o["visits"][:, 1] == 0).any()   # a target alone in its leaf sums no point directly
    Y, t, _ = ac.case("dyadic", 1000, 1, 24, 0.5)
    assert t["side"] == 4.0 and np.array_equal(Y * 8, np.round(Y * 8))
    assert ac.case("collinear", 129, 8, 24, 0.5)[1]["side"] > 0 and np.ptp(ac.embedding("collinear", 129)[:, 1]) == 0


# ---------------------------------------------------------------------------------------------- structure, bit for bit
@pytest.mark.parametrize("c", ac.CASES, ids=case_id)
def test_structure_bit_for_bit(ops, c):
    kind, N, leaf_size, D, angles = c
    for angle in angles:
        Y, t, o = ac.case(kind, N, leaf_size, D, angle)
        d = device_case(ops, kind, N, leaf_size, D, angle)
        assert d["keys"].dtype == torch.int64 and np.array_equal(d["keys"].cpu().numpy(), t["keys"])
        assert np.array_equal(d["order"].cpu().numpy(), t["order"])
        n = read_nodes(d["ws"], N, t["leaf_size"], D)
        assert len(n["level"]) == len(t["level"])
        for f in ("level", "start", "count", "skip"):
            assert np.array_equal(n[f], t[f]), f
        assert np.array_equal(n["leaf"], t["leaf"].astype(np.int32)) and not n["pad"].any()
        assert np.array_equal(n["com"].view(np.int32), t["com"].view(np.int32))
        assert np.array_equal(d["vis"].cpu().numpy(), o["visits"]), (kind, N, leaf_size, D, angle)
        if angle == 0.0:
            assert not o["visits"][:, 0].any() and np.all(o["visits"][:, 1] == N - 1)


# ---------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("c", ac.CASES, ids=case_id)
def test_sums_within_the_summation_bounds(ops, c):
    kind, N, leaf_size, D, angles = c
    for angle in angles:
        Y, t, o = ac.case(kind, N, leaf_size, D, angle)
        d = device_case(ops, kind, N, leaf_size, D, angle)
        rep, Z = d["rep"].cpu().numpy(), float(d["Z"])
        assert np.all(np.isfinite(rep)) and np.isfinite(Z)
        within(f"{kind}: force", np.abs(rep[:, :2] - o["rep"]), GAMMA * o["A"])
        within(f"{kind}: W", np.abs(rep[:, 2] - o["W"]), GAMMA * o["W"])
        within(f"{kind}: Z", abs(Z - o["Z"]), GAMMA * o["Z"])
        assert abs(rep[:, 2].sum() - Z) <= 1e-12 * Z                     # f64 sums of the kernel's own output, in another order


def exact_partials(ops, Y):
    """vcy_tsne_gradient's repulsion partials on Y (empty P): (F (N, 2), W (N), Z)."""
    N = Y.shape[0]
    tb = (N + 511) // 512
    S = max(1, min((2048 + tb - 1) // tb, (N + 1023) // 1024))
    per = ((N + S - 1) // S + 255) // 256 * 256
    S = (N + per - 1) // per
    ws = ops.tsne_workspace(N, 2)
    P = (dev(np.zeros(N + 1, np.int64)), dev(np.zeros(1, np.int32)), dev(np.zeros(1, np.float32)))
    _, stats = ops.tsne_gradient(dev(Y), *P, compute_error=False, ws=ws)
    part = ws.view(torch.float64)[:S * 3 * N].view(S, 3, N).sum(0).cpu().numpy()
    return part[:2].T, part[2], float(stats[0])


@pytest.mark.parametrize("c", [c for c in ac.CASES if 0.0 in c[4]], ids=case_id)
def test_angle_zero_against_the_exact_kernel(ops, c):
    kind, N, leaf_size, D, _ = c
    Y, t, o = ac.case(kind, N, leaf_size, D, 0.0)
    ex = ac.exact_case(kind, N)
    d = device_case(ops, kind, N, leaf_size, D, 0.0)
    rep, Z = d["rep"].cpu().numpy(), float(d["Z"])
    F, W, Zx = exact_partials(ops, Y)
    within(f"{kind}: angle 0, force against the exact kernel", np.abs(rep[:, :2] - F), GAMMA * (o["A"] + ex["A"]))
    within(f"{kind}: angle 0, W against the exact kernel", np.abs(rep[:, 2] - W), GAMMA * (o["W"] + ex["W"] + 1.0))
    within(f"{kind}: angle 0, Z against the exact kernel", abs(Z - Zx), GAMMA * (o["Z"] + ex["Z"] + N))


@pytest.mark.parametrize("N,leaf_size,D", ac.COINCIDENT)
@pytest.mark.parametrize("angle", [0.0, 0.5, 1.0])
def test_coincident_points_exactly(ops, N, leaf_size, D, angle):
    """Every point at one position: side == 0, every key 0; with N > leaf_size a chain of D internal nodes ends in one leaf of all
    N points; no node is ever accepted (0 < angle^2 0 is false), all N (N - 1) weights are exactly 1 and every force term exactly 0."""
    ls = ac.leaf_of(N, leaf_size)
    d = evaluate(ops, ac.embedding("coincident", N), ls, D, angle)
    assert not d["keys"].any()
    n = read_nodes(d["ws"], N, ls, D)
    chain = 1 if N <= ls else D + 1
    assert n["level"].tolist() == list(range(chain)) and np.all(n["count"] == N) and np.all(n["start"] == 0) and np.all(n["skip"] == chain)
    assert n["leaf"].tolist() == [0] * (chain - 1) + [1]
    assert np.array_equal(n["com"], np.tile(np.asarray([1.5, -2.25], np.float32), (chain, 1)))
    rep = d["rep"].cpu().numpy()
    assert not rep[:, :2].any() and np.array_equal(rep[:, 2], np.full(N, N - 1.0)) and float(d["Z"]) == N * (N - 1.0)
    vis = d["vis"].cpu().numpy()
    assert not vis[:, 0].any() and np.all(vis[:, 1] == N - 1)
    Yd = dev(ac.embedding("coincident", N))
    P = (dev(np.zeros(N + 1, np.int64)), dev(np.zeros(1, np.int32)), dev(np.zeros(1, np.float32)))
    ws = ops.tsne_atree_workspace(N, ls, D)
    _, order, skeys = ops.tsne_atree_keys(Yd, ws, ls, D)
    grad, stats = ops.tsne_atree_gradient(Yd, *P, order, skeys, ws, angle, ls, D, compute_error=True)
    assert float(stats[0]) == N * (N - 1.0) and not grad.view(torch.int32).any()
    assert float(stats[1]) == 0.0 and float(stats[2]) == 0.0


@pytest.mark.parametrize("c", [("normal", 129, 1, 24, 0.5), ("heavy", 1000, 8, 24, 0.2), ("clusters", 5000, 8, 24, 0.5), ("dyadic", 1000, 1, 24, 0.0),
                               ("clumps5", 3000, 8, 24, 0.5)], ids=lambda c: f"{c[0]}-{c[1]}")
def test_repeated_call_and_nan_workspace_give_the_same_bits(ops, c):
    kind, N, ls, D, angle = c
    Y, t, _ = ac.case(kind, N, ls, D, angle)
    a = device_case(ops, kind, N, ls, D, angle)
    b = evaluate(ops, Y, ls, D, angle)
    ws = ops.tsne_atree_workspace(N, ls, D)
    ws.fill_(0xFF)
    n = evaluate(ops, Y, ls, D, angle, ws=ws)
    for other in (b, n):
        assert all(same_bits(a[k], other[k]) for k in ("keys", "order", "rep", "Z", "vis"))
    na, nn = read_nodes(a["ws"], N, ls, D), read_nodes(n["ws"], N, ls, D)
    assert all(np.array_equal(na[f].view(np.int32), nn[f].view(np.int32)) for f in na)


# ---------------------------------------------------------------------------------------------- arguments
def test_arguments_are_validated(ops):
    from velocyto_amd import _lib
    L = _lib.lib()
    N, ls, D = 100, 8, 24
    Y = dev(ac.embedding("normal", N))
    ws = ops.tsne_atree_workspace(N, ls, D)
    _, order, skeys = ops.tsne_atree_keys(Y, ws, ls, D)
    assert skeys.dtype == torch.int64
    for angle in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="angle"):
            ops.tsne_atree_repulsion(Y, order, skeys, ws, angle, ls, D)
    keys = torch.empty(N, dtype=torch.int64, device=DEV)
    for leaf, depth, what in ((0, 24, "leaf_size"), (-3, 24, "leaf_size"), (8, 0, "max_depth"), (8, 25, "max_depth")):
        with pytest.raises(ValueError):
            ops.tsne_atree_workspace(N, leaf, depth)
        assert L.vcy_tsne_atree_workspace_bytes(N, leaf, depth) == 0
        with pytest.raises(ValueError, match=what):
            _lib.check(L.vcy_tsne_atree_keys(Y.data_ptr(), keys.data_ptr(), ws.data_ptr(), N, leaf, depth, ops._stream()), "tsne_atree_keys")
    assert L.vcy_tsne_atree_workspace_bytes(1, ls, D) == 0 and L.vcy_tsne_atree_workspace_bytes(N, ls, D) > 0
    assert L.vcy_tsne_atree_workspace_bytes(N, N, 1) > 0 and L.vcy_tsne_atree_workspace_bytes(2 ** 29, 1, 24) == 0    # node numbers are int32
    assert L.vcy_tsne_atree_workspace_bytes(N, ls, D) >= 256 + 4096 + 48 * ac.node_bound(N, ls, D) + 32 * N
    Y3 = torch.zeros((N, 3), device=DEV)
    P = (dev(np.zeros(N + 1, np.int64)), dev(np.zeros(1, np.int32)), dev(np.zeros(1, np.float32)))
    with pytest.raises(NotImplementedError, match="n_components"):
        ops.tsne_atree_gradient(Y3, *P, order, skeys, ws, 0.5, ls, D)
    update, gains = torch.zeros((N, 3), dtype=torch.float64, device=DEV), torch.ones((N, 3), device=DEV)
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    with pytest.raises(NotImplementedError, match="n_components"):
        ops.tsne_atree_step(Y3, torch.empty_like(Y3), *P, order, skeys, update, gains, stats, ws, 0.5, 0.5, 200.0, leaf_size=ls, max_depth=D)
    with pytest.raises(ValueError, match="int64"):
        ops.tsne_atree_repulsion(Y, order, skeys.to(torch.int32), ws, 0.5, ls, D)
    # the fixed tree's entry points keep their range
    assert L.vcy_tsne_tree_workspace_bytes(N, 12) == 0 and L.vcy_tsne_tree_workspace_bytes(N, 11) > 0


# ---------------------------------------------------------------------------------------------- one step
def attraction(N, seed=0):
    """A kNN-like CSR P: six entries per row, some rows empty, values of several magnitudes."""
    rng = np.random.default_rng([seed, N, 78])
    rows = [[] if (N > 3 and i % 7 == 3) else sorted(int(j) + (int(j) >= i) for j in rng.choice(N - 1, min(N - 1, 6), replace=False)) for i in range(N)]
    indptr = np.zeros(N + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.asarray([j for r in rows for j in r], np.int32)
    pval = rng.uniform(0.1, 1.0, len(indices)) / N
    pval[np.arange(len(indices)) % 13 == 5] = 3.0
    return indptr, indices, pval.astype(np.float32)


@pytest.mark.parametrize("state", ["first", "mixed"])
@pytest.mark.parametrize("N,ls,D", [(65, 1, 24), (257, 8, 24), (1025, 8, 24), (1025, 64, 15)])
def test_step_at_angle_zero_against_the_exact_step(ops, oracle, N, ls, D, state):
    lr, momentum, min_gain = 200.0, 0.8, 0.01
    Y = ac.embedding("normal", N, seed=1)
    P = attraction(N)
    o = oracle.tsne_objective(Y, *P, 2)
    Zr = o["Z"]
    bound = o["c"] * (GAMMA * o["A_rep"] / Zr + GAMMA * np.abs(o["rep"]) * (Zr + N) / Zr ** 2 + 8 * U * o["A_attr"]) + 2 * U * np.abs(o["grad"])
    decided = np.abs(o["grad"]) > 4 * bound
    share = 1.0 - decided.mean()
    assert share <= 0.01, share                             # a condition on the case, from the oracle alone
    note("step: undecided share", share)
    rng = np.random.default_rng(N)
    t = np.arange(2 * N).reshape(N, 2)
    gains0 = np.asarray([0.0125, 0.0101, min_gain, 1.0, 7.0], np.float32)[t % 5]
    if state == "first":
        update0 = np.zeros((N, 2))
    else:
        mag = lr * np.where(o["grad"] != 0, np.abs(o["grad"]), 1e-3) * rng.uniform(0.5, 2.0, (N, 2))
        update0 = np.asarray([1.0, -1.0, 0.0])[(t // 5) % 3] * np.where(o["grad"] < 0, -1.0, 1.0) * mag
    Yd, csr = dev(Y), (dev(P[0]), dev(P[1]), dev(P[2]))

    def fresh():
        return (torch.full_like(Yd, float("nan")), dev(update0), dev(gains0), torch.tensor([-1.0, -7.5, -9.25, -11.0], dtype=torch.float64, device=DEV))

    Yx, ux, gx, sx = fresh()
    ops.tsne_step(Yd, Yx, *csr, ux, gx, sx, ops.tsne_workspace(N, 2), momentum, lr, min_gain, True)
    Yt, ut, gt, st = fresh()
    ws = ops.tsne_atree_workspace(N, ls, D)
    _, order, skeys = ops.tsne_atree_keys(Yd, ws, ls, D)
    ops.tsne_atree_step(Yd, Yt, *csr, order, skeys, ut, gt, st, ws, 0.0, momentum, lr, min_gain, True, leaf_size=ls, max_depth=D)
    assert np.array_equal(Yd.cpu().numpy().view(np.int32), Y.view(np.int32))                       # Y is read only
    Yx, ux, gx, Yt, ut, gt = (a.cpu().numpy() for a in (Yx, ux, gx, Yt, ut, gt))
    assert all(np.all(np.isfinite(a)) for a in (Yt, ut, gt))
    assert np.array_equal(gt[decided], gx[decided])                                                # the same branch: bit-equal gains
    gg = np.abs(o["grad"]) * gx
    tol_u = 2 * lr * (gx.astype(np.float64) * bound + U * gg)                                      # either kernel is within half of it of the oracle
    within("step: update against the exact step", np.abs(ut - ux)[decided], tol_u[decided])
    within("step: position against the exact step", np.abs(Yt.astype(np.float64) - Yx)[decided], (tol_u + 2 * U * np.abs(Yx))[decided])
    sx, st = sx.cpu().numpy(), st.cpu().numpy()
    within("step: Z against the exact step", abs(st[0] - sx[0]), GAMMA * (2 * Zr + N))
    assert st[3] == -11.0 and np.isfinite(st[1]) and np.isfinite(st[2])
    # Y_out == Y is refused before any launch
    before = ut.copy()
    u2 = dev(before)
    with pytest.raises(ValueError, match="must not alias"):
        ops.tsne_atree_step(Yd, Yd, *csr, order, skeys, u2, dev(gt), dev(st), ws, 0.0, momentum, lr, min_gain, True, leaf_size=ls, max_depth=D)
    torch.cuda.synchronize()
    assert np.array_equal(u2.cpu().numpy(), before) and np.array_equal(Yd.cpu().numpy().view(np.int32), Y.view(np.int32))


# ---------------------------------------------------------------------------------------------- the fit
def test_fit_with_the_adaptive_tree(ops):
    from scipy import sparse
    from velocyto_amd.tsne import DeviceTSNE
    X, lab = ac.blobs()
    N = X.shape[0]
    t1 = DeviceTSNE(repulsion="tree", tree_depth="adaptive", angle=0.5, random_state=0)
    E1 = t1.fit_transform(X)
    t2 = DeviceTSNE(repulsion="tree", tree_depth="adaptive", angle=0.5, random_state=0)
    E2 = t2.fit_transform(X)
    assert np.array_equal(E1.view(np.int32), E2.view(np.int32)) and t1.kl_divergence_ == t2.kl_divergence_ and t1.n_iter_ == t2.n_iter_
    assert E1.shape == (N, 2) and E1.dtype == np.float32 and np.all(np.isfinite(E1)) and E1 is t1.embedding_
    assert 250 <= t1.n_iter_ <= 999 and t1.n_features_in_ == 10 and t1.learning_rate_ == max(N / 12.0 / 4.0, 50.0)
    assert np.isfinite(t1.kl_divergence_) and t1.kl_divergence_ > 0
    tx = DeviceTSNE(random_state=0)                                      # the exact mode, from the same start
    tx.fit_transform(X)
    aff = tx._affinities(torch.from_numpy(X).to(DEV))
    P = sparse.csr_matrix((aff["P"].cpu().numpy(), aff["indices"].cpu().numpy(), aff["indptr"].cpu().numpy()), shape=(N, N))
    kl_tree, _ = tx._objective(E1, P)                                    # the adaptive fit's positions under the EXACT objective
    kl_own, _ = tx._objective(E1, P, repulsion="tree", angle=0.5, tree_depth="adaptive")
    print(f"\nfit: KL exact mode {tx.kl_divergence_:.6f}, adaptive-tree fit under the exact objective {kl_tree:.6f} (its own {kl_own:.6f}, "
          f"reported {t1.kl_divergence_:.6f}); excess {kl_tree - tx.kl_divergence_:.3e}, allowed {FIT_MARGIN * FIT_SPREAD:.3e}")
    note("fit: KL excess / allowed", max(kl_tree - tx.kl_divergence_, 0.0) / (FIT_MARGIN * FIT_SPREAD))
    assert kl_tree - tx.kl_divergence_ <= FIT_MARGIN * FIT_SPREAD
    centres = np.stack([E1[lab == b].mean(0) for b in range(6)])
    nearest = np.argmin(((E1[:, None, :] - centres[None, :, :]) ** 2).sum(-1), 1)
    assert np.array_equal(nearest, lab)


def test_options_and_defaults(ops):
    from velocyto_amd.preprocess import PreprocessMixin
    from velocyto_amd.tsne import DeviceTSNE
    X, _ = ac.blobs(300)
    assert DeviceTSNE().tree_depth is None and DeviceTSNE().leaf_size is None and DeviceTSNE().repulsion == "exact"
    with pytest.raises(ValueError, match="tree_depth"):
        DeviceTSNE(repulsion="tree", tree_depth="deep").fit_transform(X)
    with pytest.raises(ValueError, match="tree_depth"):
        DeviceTSNE(repulsion="tree", tree_depth=12).fit_transform(X)
    for bad in (0, -1, 2.5, "8", True):
        with pytest.raises(ValueError, match="leaf_size"):
            DeviceTSNE(repulsion="tree", tree_depth="adaptive", leaf_size=bad).fit_transform(X)
    with pytest.raises(NotImplementedError, match="n_components == 2"):
        DeviceTSNE(n_components=3, repulsion="tree", tree_depth="adaptive").fit_transform(X)
    DeviceTSNE(repulsion="tree", leaf_size=0, max_iter=250, random_state=0).fit_transform(X)      # read in adaptive mode only
    np.random.seed(3)
    a = DeviceTSNE(repulsion="tree", tree_depth="adaptive", angle=0.3, max_iter=250).fit_transform(X)
    ns = types.SimpleNamespace(pcs=X)
    np.random.seed(3)
    PreprocessMixin.perform_TSNE(ns, theta=0.3, max_iter=250, backend="hip", repulsion="tree", tree_depth="adaptive")
    assert ns.ts.shape == (300, 2) and np.array_equal(ns.ts.view(np.int32), a.view(np.int32))
    np.random.seed(3)
    b = DeviceTSNE(repulsion="tree", angle=0.3, max_iter=250).fit_transform(X)
    np.random.seed(3)
    PreprocessMixin.perform_TSNE(ns, theta=0.3, max_iter=250, backend="hip", repulsion="tree")
    assert np.array_equal(ns.ts.view(np.int32), b.view(np.int32)) and not np.array_equal(a, b)
    np.random.seed(3)
    c = DeviceTSNE(repulsion="tree", tree_depth="adaptive", leaf_size=1, angle=0.3, max_iter=250).fit_transform(X)
    assert np.all(np.isfinite(c)) and not np.array_equal(a, c)
