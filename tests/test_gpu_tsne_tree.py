"""The tree repulsion of the device t-SNE (csrc/tsne.hip: k_tree_*, k_tsne_tree_repulsion; vcy_tsne_tree_*) against the numpy
restatement of tests/tsne_tree_cases.py, through the C ABI (ops.tsne_tree_*), and DeviceTSNE(repulsion="tree").

Structure is compared bit for bit: the keys, the pyramid's count and com (read from the workspace, whose layout
include/velocyto_hip.h states) and, per target, the number of accepted nodes and of directly summed points - so every accept / open
decision is the specified one.

Sums.  Write u = 2^-24.  A term (an accepted node: the difference, the fma chain, a 1-ulp v_rcp_f32, count -> f32, three products;
a direct pair: as in the exact kernel) costs at most 16 f32 roundings; at most 256 terms are added in f32 between two f64 carries;
everything else is f64.  With gamma = (256 + 16) u and A, W, Z the oracle's sums over the SAME interaction set:
    force |F - F_ref| <= gamma A       weight sum |W - W_ref| <= gamma W_ref       Z |Z - Z_ref| <= gamma Z_ref
(no "+ 1" and "+ N" as in the exact kernel's bounds: the self term is left out, not summed and subtracted).  At angle 0 the tree
result is also compared with vcy_tsne_gradient's partials on the same points: both are within their bound of the f64 all-pairs
sum, so |F_tree - F_exact| <= gamma (A + A), |W_tree - W_exact| <= gamma (2 W + 1), |Z_tree - Z_exact| <= gamma (2 Z + N).
None of these is fitted to a run.  Coincident points, repeated calls and a NaN-filled workspace carry no tolerance.

The step is compared with vcy_tsne_step's at angle 0 on the *decided* components of tests/test_gpu_tsne_kernels.py (|g_ref| > 4 bound
from the f64 oracle; at most 1 % undecided, asserted from the oracle alone): there both kernels take the same gain branch.

The fit.  scikit-learn 1.7.2 (method="barnes_hut", random start) on tsne_tree_cases.blobs(): see FIT_SPREAD below.

Recorded on an MI355X (largest error / bound over all cases; a run with -s prints them per input kind, DESIGN.md section 9 has the
table): force 0.048, W 0.053, Z 0.0074; at angle 0 against the exact kernel force 0.023, W 0.24 (heavy-tailed), Z 0.0040; step against
the exact step update 0.076, position 0.75, Z 0.0016, no undecided component; fit: exact KL of the tree fit 1.39713 against 1.40070
for the exact mode (excess -0.0036, allowed 0.0154).
"""
import types

import numpy as np
import pytest

import tsne_tree_cases as tc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
U, GAMMA = tc.U, tc.GAMMA
RECORD = {}
_dev_cache = {}

# scikit-learn 1.7.2's own spread on blobs(): TSNE(method="barnes_hut", init="random", random_state=s), kl_divergence_ at angle 0.5
# minus that at angle 0.0, measured on the CPU: s = 0: 1.404748 - 1.398575 = +0.006173; s = 1: +0.013899; s = 2: -0.000227.
# FIT_SPREAD is the figure of the seed this test uses (0).  The difference of two fits is one draw of a chaotic descent: over the
# three seeds it reaches 2.25 x the seed-0 figure, so FIT_MARGIN = 2.5 - a tree fit may end 0.0154 above the exact-mode fit.
FIT_SPREAD = 0.006173
FIT_MARGIN = 2.5


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd  # noqa: F401
    from velocyto_amd import ops
    ops.require_gpu()
    assert hasattr(ops, "tsne_tree_keys"), "this build has no tree repulsion"
    yield ops
    if RECORD:
        print("\nlargest error / bound, tests/test_gpu_tsne_tree.py:")
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


def read_pyramid(ws, L):
    """count (nodes) int32 and com (nodes, 2) f32 from the workspace: head 128 bytes, 256 box partials of 16 bytes, then the nodes."""
    nn = (4 ** (L + 1) - 1) // 3
    off = 128 + align(16 * 256)
    rec = ws[off:off + 16 * nn].view(torch.int32).view(nn, 4).cpu().numpy()
    return rec[:, 0].copy(), rec[:, 1:3].copy().view(np.float32)


def evaluate(ops, Y, L, angle, ws=None):
    Yd = dev(Y)
    N = Y.shape[0]
    ws = ops.tsne_tree_workspace(N, L) if ws is None else ws
    keys, order, skeys = ops.tsne_tree_keys(Yd, ws, L)
    rep, Z, vis = ops.tsne_tree_repulsion(Yd, order, skeys, ws, L, angle, visits=True)
    return dict(keys=keys, order=order, rep=rep, Z=Z, vis=vis, ws=ws)


def device_case(ops, kind, N, depth, angle):
    k = (kind, N, depth, angle)
    if k not in _dev_cache:
        Y, L, pyr, o = tc.case(kind, N, depth, angle)
        _dev_cache[k] = evaluate(ops, Y, L, angle)
    return _dev_cache[k]


def case_id(c):
    return f"{c[0]}-{c[1]}-{'auto' if c[2] is None else c[2]}"


def test_cases_cover_the_shapes(ops):
    assert {c[1] for c in tc.CASES} >= {2, 3, 63, 64, 65, 127, 129, 1000, 5000}
    assert {c[2] for c in tc.CASES} >= {1, 2, 5, 8, 11, None}
    assert {a for c in tc.CASES for a in c[3]} == {0.0, 0.2, 0.5, 0.8, 1.0}
    for N in (2, 4, 5, 16, 17, 1000, 4096, 4097, 10 ** 6, 4 ** 11, 4 ** 11 + 1, 2 ** 29):
        assert ops.tsne_tree_depth(N) == tc.auto_depth(N), N
    _, L, pyr, _ = tc.case("clusters", 5000, 5, 0.5)
    assert pyr["count"][L].max() > 1024                                  # one leaf holds more than 1024 points
    _, L, pyr, o = tc.case("lone", 65, 5, 0.5)
    assert (pyr["count"][L] == 1).any() and (o["visits"][:, 1] == 0).any()   # a target alone in its leaf sums no point directly
    Y, L, pyr, _ = tc.case("dyadic", 1000, 5, 0.5)
    assert pyr["side"] == 4.0 and np.array_equal(Y * 8, np.round(Y * 8))
    assert tc.case("collinear", 129, None, 0.5)[2]["side"] > 0 and np.ptp(tc.embedding("collinear", 129)[:, 1]) == 0


# ---------------------------------------------------------------------------------------------- structure, bit for bit
@pytest.mark.parametrize("c", tc.CASES, ids=case_id)
def test_structure_bit_for_bit(ops, c):
    kind, N, depth, angles = c
    for angle in angles:
        Y, L, pyr, o = tc.case(kind, N, depth, angle)
        d = device_case(ops, kind, N, depth, angle)
        assert np.array_equal(d["keys"].cpu().numpy(), pyr["keys"])
        assert np.array_equal(d["order"].cpu().numpy(), pyr["order"])
        cnt, com = read_pyramid(d["ws"], L)
        assert np.array_equal(cnt, np.concatenate(pyr["count"]))
        assert np.array_equal(com.view(np.int32), np.concatenate(pyr["com"]).view(np.int32))
        assert np.array_equal(d["vis"].cpu().numpy(), o["visits"]), (kind, N, L, angle)
        if angle == 0.0:
            assert not o["visits"][:, 0].any() and np.all(o["visits"][:, 1] == N - 1)


# ---------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("c", tc.CASES, ids=case_id)
def test_sums_within_the_summation_bounds(ops, c):
    kind, N, depth, angles = c
    for angle in angles:
        Y, L, pyr, o = tc.case(kind, N, depth, angle)
        d = device_case(ops, kind, N, depth, angle)
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


@pytest.mark.parametrize("c", [c for c in tc.CASES if 0.0 in c[3]], ids=case_id)
def test_angle_zero_against_the_exact_kernel(ops, c):
    kind, N, depth, _ = c
    Y, L, pyr, o = tc.case(kind, N, depth, 0.0)
    ex = tc.exact_case(kind, N)
    d = device_case(ops, kind, N, depth, 0.0)
    rep, Z = d["rep"].cpu().numpy(), float(d["Z"])
    F, W, Zx = exact_partials(ops, Y)
    within(f"{kind}: angle 0, force against the exact kernel", np.abs(rep[:, :2] - F), GAMMA * (o["A"] + ex["A"]))
    within(f"{kind}: angle 0, W against the exact kernel", np.abs(rep[:, 2] - W), GAMMA * (o["W"] + ex["W"] + 1.0))
    within(f"{kind}: angle 0, Z against the exact kernel", abs(Z - Zx), GAMMA * (o["Z"] + ex["Z"] + N))


@pytest.mark.parametrize("N,depth", tc.COINCIDENT)
@pytest.mark.parametrize("angle", [0.0, 0.5, 1.0])
def test_coincident_points_exactly(ops, N, depth, angle):
    """Every point at one position: side == 0, every key 0, no node is ever accepted (0 < angle^2 0 is false), all N (N - 1)
    weights are exactly 1 and every force term exactly 0."""
    L = tc.auto_depth(N) if depth is None else depth
    d = evaluate(ops, tc.embedding("coincident", N), L, angle)
    assert not d["keys"].any()
    rep = d["rep"].cpu().numpy()
    assert not rep[:, :2].any() and np.array_equal(rep[:, 2], np.full(N, N - 1.0)) and float(d["Z"]) == N * (N - 1.0)
    vis = d["vis"].cpu().numpy()
    assert not vis[:, 0].any() and np.all(vis[:, 1] == N - 1)
    Yd = dev(tc.embedding("coincident", N))
    P = (dev(np.zeros(N + 1, np.int64)), dev(np.zeros(1, np.int32)), dev(np.zeros(1, np.float32)))
    ws = ops.tsne_tree_workspace(N, L)
    _, order, skeys = ops.tsne_tree_keys(Yd, ws, L)
    grad, stats = ops.tsne_tree_gradient(Yd, *P, order, skeys, ws, L, angle, compute_error=True)
    assert float(stats[0]) == N * (N - 1.0) and not grad.view(torch.int32).any()
    assert float(stats[1]) == 0.0 and float(stats[2]) == 0.0


@pytest.mark.parametrize("c", [("normal", 129, 11, 0.5), ("heavy", 1000, None, 0.2), ("clusters", 5000, 5, 0.5), ("dyadic", 1000, 5, 0.0)],
                         ids=lambda c: f"{c[0]}-{c[1]}")
def test_repeated_call_and_nan_workspace_give_the_same_bits(ops, c):
    kind, N, depth, angle = c
    Y, L, _, _ = tc.case(kind, N, depth, angle)
    a = device_case(ops, kind, N, depth, angle)
    b = evaluate(ops, Y, L, angle)
    ws = ops.tsne_tree_workspace(N, L)
    ws.fill_(0xFF)
    n = evaluate(ops, Y, L, angle, ws=ws)
    for other in (b, n):
        assert all(same_bits(a[k], other[k]) for k in ("keys", "order", "rep", "Z", "vis"))


# ---------------------------------------------------------------------------------------------- arguments
def test_arguments_are_validated(ops):
    from velocyto_amd import _lib
    N, L = 100, 4
    Y = dev(tc.embedding("normal", N))
    ws = ops.tsne_tree_workspace(N, L)
    _, order, skeys = ops.tsne_tree_keys(Y, ws, L)
    for angle in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="angle"):
            ops.tsne_tree_repulsion(Y, order, skeys, ws, L, angle)
    for depth in (0, 12):
        with pytest.raises(ValueError):
            ops.tsne_tree_workspace(N, depth)
        keys = torch.empty(N, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError, match="depth"):
            _lib.check(_lib.lib().vcy_tsne_tree_keys(Y.data_ptr(), keys.data_ptr(), ws.data_ptr(), N, depth, ops._stream()), "tsne_tree_keys")
    assert _lib.lib().vcy_tsne_tree_workspace_bytes(1, 4) == 0 and _lib.lib().vcy_tsne_tree_workspace_bytes(N, 4) > 0
    Y3 = torch.zeros((N, 3), device=DEV)
    P = (dev(np.zeros(N + 1, np.int64)), dev(np.zeros(1, np.int32)), dev(np.zeros(1, np.float32)))
    with pytest.raises(NotImplementedError, match="n_components"):
        ops.tsne_tree_gradient(Y3, *P, order, skeys, ws, L, 0.5)
    update, gains = torch.zeros((N, 3), dtype=torch.float64, device=DEV), torch.ones((N, 3), device=DEV)
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    with pytest.raises(NotImplementedError, match="n_components"):
        ops.tsne_tree_step(Y3, torch.empty_like(Y3), *P, order, skeys, update, gains, stats, ws, L, 0.5, 0.5, 200.0)


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
@pytest.mark.parametrize("N,depth", [(65, 2), (257, None), (1025, None), (1025, 11)])
def test_step_at_angle_zero_against_the_exact_step(ops, oracle, N, depth, state):
    lr, momentum, min_gain = 200.0, 0.8, 0.01
    L = tc.auto_depth(N) if depth is None else depth
    Y = tc.embedding("normal", N, seed=1)
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
    ws = ops.tsne_tree_workspace(N, L)
    _, order, skeys = ops.tsne_tree_keys(Yd, ws, L)
    ops.tsne_tree_step(Yd, Yt, *csr, order, skeys, ut, gt, st, ws, L, 0.0, momentum, lr, min_gain, True)
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
        ops.tsne_tree_step(Yd, Yd, *csr, order, skeys, u2, dev(gt), dev(st), ws, L, 0.0, momentum, lr, min_gain, True)
    torch.cuda.synchronize()
    assert np.array_equal(u2.cpu().numpy(), before) and np.array_equal(Yd.cpu().numpy().view(np.int32), Y.view(np.int32))


# ---------------------------------------------------------------------------------------------- the fit
def test_fit_with_the_tree(ops):
    from scipy import sparse
    from velocyto_amd.tsne import DeviceTSNE
    X, lab = tc.blobs()
    N = X.shape[0]
    t1 = DeviceTSNE(repulsion="tree", angle=0.5, random_state=0)
    E1 = t1.fit_transform(X)
    t2 = DeviceTSNE(repulsion="tree", angle=0.5, random_state=0)
    E2 = t2.fit_transform(X)
    assert np.array_equal(E1.view(np.int32), E2.view(np.int32)) and t1.kl_divergence_ == t2.kl_divergence_ and t1.n_iter_ == t2.n_iter_
    assert E1.shape == (N, 2) and E1.dtype == np.float32 and np.all(np.isfinite(E1)) and E1 is t1.embedding_
    assert 250 <= t1.n_iter_ <= 999 and t1.n_features_in_ == 10 and t1.learning_rate_ == max(N / 12.0 / 4.0, 50.0)
    assert np.isfinite(t1.kl_divergence_) and t1.kl_divergence_ > 0
    tx = DeviceTSNE(random_state=0)                                      # the exact mode, from the same start
    tx.fit_transform(X)
    aff = tx._affinities(torch.from_numpy(X).to(DEV))
    P = sparse.csr_matrix((aff["P"].cpu().numpy(), aff["indices"].cpu().numpy(), aff["indptr"].cpu().numpy()), shape=(N, N))
    kl_tree, _ = tx._objective(E1, P)                                    # the tree fit's positions under the EXACT objective
    kl_same, _ = tx._objective(tx.embedding_, P)                         # kl_divergence_ is taken before the last update: close, not equal
    assert abs(kl_same - tx.kl_divergence_) <= 1e-3 * kl_same
    kl_tree_own, _ = tx._objective(E1, P, repulsion="tree", angle=0.5)
    print(f"\nfit: KL exact mode {tx.kl_divergence_:.6f}, tree fit under the exact objective {kl_tree:.6f} (its own {kl_tree_own:.6f}, "
          f"reported {t1.kl_divergence_:.6f}); excess {kl_tree - tx.kl_divergence_:.3e}, allowed {FIT_MARGIN * FIT_SPREAD:.3e}")
    note("fit: KL excess / allowed", max(kl_tree - tx.kl_divergence_, 0.0) / (FIT_MARGIN * FIT_SPREAD))
    assert kl_tree - tx.kl_divergence_ <= FIT_MARGIN * FIT_SPREAD
    centres = np.stack([E1[lab == b].mean(0) for b in range(6)])
    nearest = np.argmin(((E1[:, None, :] - centres[None, :, :]) ** 2).sum(-1), 1)
    assert np.array_equal(nearest, lab)


def test_options_and_defaults(ops):
    from velocyto_amd.preprocess import PreprocessMixin
    from velocyto_amd.tsne import DeviceTSNE
    X, _ = tc.blobs(300)
    with pytest.raises(NotImplementedError, match="n_components == 2"):
        DeviceTSNE(n_components=3, repulsion="tree").fit_transform(X)
    with pytest.raises(ValueError, match="repulsion"):
        DeviceTSNE(repulsion="grid").fit_transform(X)
    with pytest.raises(ValueError, match="angle"):
        DeviceTSNE(repulsion="tree", angle=1.5).fit_transform(X)
    assert DeviceTSNE().repulsion == "exact"
    DeviceTSNE(angle=7.0, max_iter=250, random_state=0).fit_transform(X)                          # exact mode: angle stays ignored
    np.random.seed(3)
    a = DeviceTSNE(repulsion="tree", angle=0.3, max_iter=250).fit_transform(X)
    ns = types.SimpleNamespace(pcs=X)
    np.random.seed(3)
    PreprocessMixin.perform_TSNE(ns, theta=0.3, max_iter=250, backend="hip", repulsion="tree")
    assert np.array_equal(ns.ts.view(np.int32), a.view(np.int32))
    np.random.seed(3)
    b = DeviceTSNE(max_iter=250).fit_transform(X)
    np.random.seed(3)
    PreprocessMixin.perform_TSNE(ns, theta=0.3, max_iter=250, backend="hip")
    assert np.array_equal(ns.ts.view(np.int32), b.view(np.int32)) and not np.array_equal(a, b)
