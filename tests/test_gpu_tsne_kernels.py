"""The t-SNE kernels (csrc/tsne.hip: k_tsne_perplexity, k_tsne_repulsion, k_tsne_step, k_tsne_stats) and tsne._symmetrize against
the f64 oracle (oracle/oracle.py: tsne_*), called directly through ops.tsne_perplexity / tsne_gradient / tsne_step /
tsne_workspace, at the sizes where the launch plan changes shape.  scikit-learn is not imported here: tests/test_tsne_oracle.py
pins the oracle on it (and on closed forms) on the CPU.

Tolerances.  Write u = 2^-24.  A repulsion term costs at most 16 f32 roundings (the difference, the fma chain, a 1-ulp v_rcp_f32,
the products, the sqrt at dof = 2); a tile adds 256 terms sequentially in f32; everything across tiles and splits is f64.  With
gamma = (256 + 16) u, and A_rep, A_attr, W the oracle's sums of the absolute terms:
    force      |F - F_ref|   <= gamma A_rep
    weight sum |W - W_ref|   <= gamma (W_ref + 1)            (the self term is summed, then subtracted)
    Z          |Z - Z_ref|   <= gamma (Z_ref + N)
    gradient   |g - g_ref|   <= c (gamma A_rep / Z + gamma |rep| (Z_ref + N) / Z^2 + 8 u A_attr) + 2 u |g_ref|
    KL         |KL - KL_ref| <= 4 u sum(p) + 1e-12 |KL_ref|
KL contains -sum(p) log Z, so the error of Z enters it in full, and the bound of Z above allows gamma (Z_ref + N) / Z_ref >= 272 u
relative: far more than 4 u.  The stated KL bound covers the terms at a given Z only.  So two things are asserted: against the
oracle's KL, the stated bound plus sum(p) (dz / (1 - dz) + 2 u / (1 - u)) with dz = gamma (Z_ref + N) / Z_ref (log(1 + d) and
the one f32 rounding of q / Z on either side); and, sharper, the stated bound itself against the oracle's KL evaluated at the
kernel's own Z (oracle.tsne_kl), Z being held to its own bound.  The ratio of the first distance to the stated bound is
recorded below: where the self term of a tile swallows distant sources (they are added to a partial sum of 1) it passes 1.
None of them is fitted to a run.  The exact cases (coincident points, two points at distance 1, repeated calls) carry no
tolerance at all.  Where an exact statement of the issue holds at dof = 1 only (two points at distance 1 give w = 1/2 and Z = 1;
at dof = 2 the weight is (2/3)^1.5) the dof = 2 case is held to the oracle by the bounds above instead.

A step's gain branches on the sign of update x gradient, so a component of the gradient is *decided* when |g_ref| > 4 bound;
undecided components may take either branch and are at most 1 % of every case (asserted from the oracle alone).  A row of the
bisection is an *edge row* when its margin (the smallest | |diff| - tol | over its steps) is below 1e-9 - device exp / log and the
k-term sums move diff by about 1e-14 - and edge rows are at most 0.1 % of every case (again from the oracle alone).

The update is compared with the oracle's; the new position with the oracle's float64(y) + update before its rounding to f32,
so that the stated bound (the update's, plus u |ref|) covers the one rounding the kernel makes.

Recorded on an MI355X (largest error / bound of each test over all its cases; every figure is printed at the end of a run with -s):
  test_objective_within_the_summation_bounds        normal    start     heavy     boundary
    force                                           0.053     0.049     0.48      0.097
    W                                               0.056     0.015     0.68      0.20
    Z                                               0.0044    0.0028    0.0035    0.059
    grad                                            0.69      0.40      0.67      0.67
    KL, bound with the Z term                       0.0051    0.0033    0.0035    0.059
    KL at the kernel's Z, stated bound              0.50      0.39      0.50      0.50
    |KL - KL_ref| / stated bound (not asserted)     19.5      0.23      207       244
  test_two_points_at_distance_one (dof 2)           Z 0.00079, grad 0.0029
  test_step_against_the_oracle                      update 0.56, position 0.95, Z 0.0022, |grad gain|^2 1.7e-9 (of 4 u relative),
                                                    KL with the Z term 0.0026, KL at the kernel's Z 0.50,
                                                    |KL - KL_ref| / stated bound 3.5 (not asserted); undecided share 0.016 % at most
  test_three_step_ping_pong_chain                   update 0.63, 0.63, 0.63 and position 0.71, 0.90, 0.67 at steps 1, 2, 3;
                                                    KL with the Z term 0.018, KL at the kernel's Z 0.028,
                                                    |KL - KL_ref| / stated bound 2.25 (not asserted); no component dropped as undecided
  test_perplexity_against_the_oracle                P error / tolerance 0.00076; edge share 0.1 % at most (one row of 1000), 0 in most cases
  test_symmetrize_against_the_oracle                values and normaliser bit-equal to the oracle's (error 0)
So the distance to the oracle's KL passes the stated 4 u sum(p) + 1e-12 |KL_ref| by up to 244 times (boundary embedding), all of it
the -sum(p) log Z term: with that term in the bound the same distance is 0.059 of it, the figure of Z's own bound.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U = 2.0 ** -24
GAMMA = (256 + 16) * U
TPB, TGT, TILE = 256, 512, 256                       # threads, targets per workgroup, sources per LDS tile (csrc/tsne.hip)
NS = [2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2049, 5000]
ZMIN = float(np.float32(np.finfo(np.float64).eps))
TOL = float(np.float32(1e-5))
RECORD = {}
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd  # noqa: F401
    from velocyto_amd import ops
    ops.require_gpu()
    yield ops
    if RECORD:
        print("\nlargest error / bound and realised shares, tests/test_gpu_tsne_kernels.py:")
        for k in sorted(RECORD):
            print(f"  {k}: {RECORD[k]:.3g}")


def note(name, value):
    RECORD[name] = max(RECORD.get(name, 0.0), float(value))


def within(name, err, bound):
    """max(err / bound) <= 1, recorded under ``name``; where the bound is 0 the error must be 0."""
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    assert np.all(np.isfinite(err)), name
    zero = bound == 0
    assert not np.any(err[zero] != 0), (name, "error where the bound is 0")
    r = float(np.max(err[~zero] / bound[~zero], initial=0.0))
    note(name, r)
    assert r <= 1.0, (name, r)
    return r


def plan(N):
    """tsne_plan of csrc/tsne.hip: (target blocks, source splits, sources per split)."""
    tb = (N + TGT - 1) // TGT
    S = max(1, min((2048 + tb - 1) // tb, (N + 1023) // 1024))
    per = ((N + S - 1) // S + TILE - 1) // TILE * TILE
    return tb, (N + per - 1) // per, per


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr_dev(P):
    """(indptr, indices, values) on the device; an empty P still gets one (unread) element so that no pointer is null."""
    indptr, indices, pval = P
    pad = lambda a, t: np.ascontiguousarray(a if len(a) else np.zeros(1), dtype=t)
    return dev(np.asarray(indptr, np.int64)), dev(pad(indices, np.int32)), dev(pad(pval, np.float32))


def empty_p(N):
    return np.zeros(N + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)


def special_sources(N):
    """The sources at which a boundary can go wrong: first, last, both ends of every split and of every 256-source tile."""
    _, S, per = plan(N)
    s = {0, N - 1}
    for i in range(S):
        s |= {i * per, i * per + per - 1}
    for m in range(0, N + TILE, TILE):
        s |= {m, m - 1}
    return np.asarray(sorted(i for i in s if 0 <= i < N))


def embedding(kind, N, D, seed=0):
    rng = np.random.default_rng([seed, N, D, len(kind)])
    if kind == "normal":
        Y = rng.normal(0.0, 5.0, (N, D))
    elif kind == "start":                              # scikit-learn's start: every w ~ 1, the cancellation in the force is maximal
        Y = 1e-4 * rng.standard_normal((N, D))
    elif kind == "heavy":
        Y = np.clip(2.0 * rng.standard_cauchy((N, D)), -1e5, 1e5)
    else:                                              # "boundary": about 40 apart, but the special sources in one small cluster
        Y = rng.normal(0.0, 1.0, (N, D))
        Y[:, 0] += 40.0 * np.arange(N)
        sp = special_sources(N)
        Y[sp] = rng.uniform(-0.35, 0.35, (len(sp), D))
        Y[sp, 0] -= 120.0
    return Y.astype(np.float32)


def attraction(N, seed=0):
    """A kNN-like CSR P with: empty rows, a row of one entry, a row longer than 256, an explicit self-loop, entries at index 0 and
    N - 1, a duplicated column, values below FLT_MIN and values of several units.  Returns (indptr, indices, values f32)."""
    rng = np.random.default_rng([seed, N, 77])
    others = lambda i, n: sorted(int(j) + (int(j) >= i) for j in rng.choice(N - 1, n, replace=False))
    rows = [[] if (N > 3 and i % 7 == 3) else others(i, min(N - 1, 6)) for i in range(N)]
    rows[0] = sorted(set(rows[0]) | {0, N - 1})                       # self-loop, first and last index
    rows[1] = [N - 1] if N > 2 else [0]                               # one entry
    if N > 2:
        rows[2] = [0, 1, 1, N - 1]                                    # a duplicated column
        rows[N - 1] = sorted(set(rows[N - 1]) | {0, 1})
    if N > 300:
        rows[5] = sorted(int(j) for j in rng.choice(N, 300, replace=False))
    indptr = np.zeros(N + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.asarray([j for r in rows for j in r], np.int32)
    nnz = len(indices)
    pval = rng.uniform(0.1, 1.0, nnz) / N
    e = np.arange(nnz)
    pval[e % 11 == 0] = 1e-40                                         # below FLT_MIN: the fmaxf(p, tiny) clamp
    pval[e % 11 == 6] = 1e-45
    pval[e % 13 == 5] = 3.0
    pval[e % 13 == 9] = 12.0
    return indptr, indices, pval.astype(np.float32)


def with_coincident_neighbour(Y):
    """Row 2 of attraction() stores column 1 (twice): put the two points at the same position."""
    if Y.shape[0] > 2:
        Y = Y.copy()
        Y[1] = Y[2]
    return Y


def grad_bound(o, N):
    Z = o["Z"]
    return o["c"] * (GAMMA * o["A_rep"] / Z + GAMMA * np.abs(o["rep"]) * (Z + N) / Z ** 2 + 8 * U * o["A_attr"]) + 2 * U * np.abs(o["grad"])


def kl_bound(o):
    """The bound of the KL terms at a given Z."""
    return 4 * U * o["sum_p"] + 1e-12 * abs(o["KL"])


def kl_bound_with_z(o, N):
    """kl_bound plus what the error of Z adds: every term holds -p log Z, Z_dev = Z_ref (1 + d) with |d| <= dz =
    gamma (Z_ref + N) / Z_ref, |log(1 + d)| <= dz / (1 - dz), and float32(q / Z) is rounded once on either side (2 u / (1 - u))."""
    dz = GAMMA * (o["Z"] + N) / o["Z"]
    assert dz < 0.5, dz                                     # a condition on the case, from the oracle alone: the series needs dz << 1
    return kl_bound(o) + o["sum_p"] * (dz / (1.0 - dz) + 2 * U / (1.0 - U))


def check_kl(name, oracle, Y, P, o, kl, Z):
    """KL against the oracle's KL within the bound that carries the error of Z, and - the sharper statement - against the
    oracle's KL at the normaliser the kernel used within the bound of the terms alone.  The ratio of the first distance to
    the bound of the terms alone is recorded."""
    N = Y.shape[0]
    note(name + " against the oracle's KL / bound without the Z term (recorded only)", abs(kl - o["KL"]) / kl_bound(o))
    within(name + " (bound with the Z term)", abs(kl - o["KL"]), kl_bound_with_z(o, N))
    within(name + " at the kernel's Z", abs(kl - oracle.tsne_kl(Y, *P, Z)), kl_bound(o))


def read_workspace(ws, N, D):
    """The repulsion's partials as k_tsne_repulsion leaves them: part (S, D + 1, N) f64 then zpart (S x target blocks).
    Returns (F (N, D), W (N), sum of zpart), each summed over the splits in f64."""
    tb, S, _ = plan(N)
    w = ws.view(torch.float64)
    n = S * (D + 1) * N
    part = w[:n].view(S, D + 1, N).sum(0).cpu().numpy()
    return part[:D].T, part[D], w[n:n + S * tb].cpu().numpy()


def raw_gradient(ops, Yd, csr, stats, ws, compute_error):
    """vcy_tsne_gradient with the caller's own stats buffer (ops.tsne_gradient allocates a zeroed one)."""
    from velocyto_amd import _lib
    N, D = Yd.shape
    grad = torch.empty_like(Yd)
    _lib.check(_lib.lib().vcy_tsne_gradient(Yd.data_ptr(), csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), grad.data_ptr(),
                                            stats.data_ptr(), ws.data_ptr(), N, D, int(compute_error), ops._stream()), "tsne_gradient")
    return grad


def raw_perplexity_without_steps(ops, d, P, perplexity):
    """vcy_tsne_perplexity with n_steps = NULL."""
    from velocyto_amd import _lib
    N, k = d.shape
    _lib.check(_lib.lib().vcy_tsne_perplexity(d.data_ptr(), P.data_ptr(), None, N, k, float(perplexity), ops._stream()), "tsne_perplexity")


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---------------------------------------------------------------------------------------------- the launch plan
def test_shapes_reach_every_edge_of_the_plan(ops):
    plans = {N: plan(N) for N in NS}
    assert any(S == 1 for _, S, _ in plans.values())
    assert any(S > 1 and (N - (S - 1) * per) % TILE != 0 for N, (_, S, per) in plans.items())      # last split ends in a partial tile
    assert plans[1025] == (3, 2, 768) and 1025 - 768 == TILE + 1                                   # ... whose last tile holds ONE source
    assert any(tb > 1 and N % TGT != 0 for N, (tb, _, _) in plans.items())                         # partly filled last target block
    assert {S for _, S, _ in plans.values()} >= {1, 2, 3, 5}
    for N, (tb, S, per) in plans.items():                                                          # the same plan as the library's
        for D in (1, 2, 3):
            assert ops.tsne_workspace(N, D).numel() == 8 * (S * (D + 1) * N + S * tb + 2 * ((N + TPB - 1) // TPB)), (N, D)


# ---------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("N", NS)
def test_coincident_points_exactly(ops, N, D):
    """Every point at one (non-zero) position, empty P: all N (N - 1) weights are exactly 1 (sums of ones are exact in f32 up to
    256 and in f64 beyond) and every force term is exactly 0.  One counted padding source, a self term subtracted in the wrong
    split or in none, a target or split visited twice, a dropped tail: each changes Z."""
    Y = dev(np.tile(np.asarray([1.5, -2.25, 3.0], np.float32)[:D], (N, 1)))
    ws = ops.tsne_workspace(N, D)
    grad, stats = ops.tsne_gradient(Y, *csr_dev(empty_p(N)), compute_error=True, ws=ws)
    assert float(stats[0]) == N * (N - 1.0)
    assert not grad.view(torch.int32).any()                                                        # +0.0 bit for bit
    F, W, zpart = read_workspace(ws, N, D)
    assert not F.any() and np.array_equal(W, np.full(N, N - 1.0)) and zpart.sum() == N * (N - 1.0)
    assert float(stats[1]) == 0.0 and float(stats[2]) == 0.0


@pytest.mark.parametrize("D", [1, 2, 3])
def test_two_points_at_distance_one(ops, oracle, D):
    Y = np.zeros((2, D), np.float32)
    Y[:, 0] = [3.0, 4.0]
    grad, stats = ops.tsne_gradient(dev(Y), *csr_dev(empty_p(2)), compute_error=False)
    grad, Z = grad.cpu().numpy(), float(stats[0])
    if D < 3:                                              # dof = 1: w = 1/2, Z = 1, force -+1/4, c = 4
        assert Z == 1.0
        want = np.zeros((2, D), np.float32)
        want[:, 0] = [4.0 * 0.25 / Z, -4.0 * 0.25 / Z]
        assert np.array_equal(grad, want)
    else:                                                  # dof = 2: w = (2/3)^1.5, not a closed binary value
        o = oracle.tsne_objective(Y, *empty_p(2), D)
        within("two points, dof 2: Z", abs(Z - o["Z"]), GAMMA * (o["Z"] + 2))
        within("two points, dof 2: grad", np.abs(grad - o["grad"]), grad_bound(o, 2))
        assert not grad[:, 1:].any() and grad[0, 0] == -grad[1, 0] and grad[0, 0] > 0


@pytest.mark.parametrize("D", [1, 2, 3])
def test_far_pair_stays_finite(ops, D):
    """Two points 1e20 apart: d^2 overflows f32.  Properties only."""
    Y = np.zeros((2, D), np.float32)
    Y[1, D - 1] = 1e20
    P = (np.asarray([0, 1, 2], np.int64), np.asarray([1, 0], np.int32), np.asarray([0.5, 0.5], np.float32))
    grad, stats = ops.tsne_gradient(dev(Y), *csr_dev(P), compute_error=True)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(stats).all())
    assert float(stats[0]) == ZMIN
    assert float(grad.abs().max()) <= 1e-15
    Yn, update, gains = torch.empty(2, D, device=DEV), torch.zeros(2, D, dtype=torch.float64, device=DEV), torch.ones(2, D, device=DEV)
    st = torch.zeros(4, dtype=torch.float64, device=DEV)
    ops.tsne_step(dev(Y), Yn, *csr_dev(P), update, gains, st, ops.tsne_workspace(2, D), 0.5, 200.0, 0.01, True)
    assert all(bool(torch.isfinite(t).all()) for t in (Yn, update, gains, st)) and float(st[0]) == ZMIN
    assert float(update.abs().max()) <= 200.0 * 1e-15


# ---------------------------------------------------------------------------------------------- the objective
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", ["normal", "start", "heavy", "boundary"])
def test_objective_within_the_summation_bounds(ops, oracle, kind, N, D):
    Y = with_coincident_neighbour(embedding(kind, N, D))
    P = attraction(N)
    o = oracle.tsne_objective(Y, *P, D)
    Yd, csr = dev(Y), csr_dev(P)
    ws = ops.tsne_workspace(N, D)
    grad, stats = ops.tsne_gradient(Yd, *csr, compute_error=True, ws=ws)
    F, W, zpart = read_workspace(ws, N, D)
    g, st = grad.cpu().numpy().astype(np.float64), stats.cpu().numpy()
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(st))
    tag = f"objective[{kind}]"
    within(tag + " force", np.abs(F - o["rep"]), GAMMA * o["A_rep"])
    within(tag + " W", np.abs(W - o["W"]), GAMMA * (o["W"] + 1.0))
    within(tag + " Z", abs(st[0] - o["Z"]), GAMMA * (o["Z"] + N))
    within(tag + " grad", np.abs(g - o["grad"]), grad_bound(o, N))
    check_kl(tag + " KL", oracle, Y, P, o, st[1], st[0])
    # f64 sums of the kernel's own outputs, in another order
    assert abs(zpart.sum() - st[0]) <= 1e-12 * st[0] and abs(W.sum() - st[0]) <= 1e-12 * st[0]
    assert abs(st[2] - float(np.sum(g * g))) <= 1e-12 * st[2]

    # the same call again, and with a workspace full of NaN bytes: the same bits
    grad2, stats2 = ops.tsne_gradient(Yd, *csr, compute_error=True)
    assert same_bits(grad, grad2) and same_bits(stats, stats2)
    ws3 = ops.tsne_workspace(N, D)
    ws3.fill_(0xFF)
    grad3, stats3 = ops.tsne_gradient(Yd, *csr, compute_error=True, ws=ws3)
    assert same_bits(grad, grad3) and same_bits(stats, stats3)
    # compute_error = 0: stats[1] and stats[2] are left alone, stats[0] is still Z, the gradient does not change
    sent = torch.tensor([-1.0, -7.5, -9.25, -11.0], dtype=torch.float64, device=DEV)
    grad4 = raw_gradient(ops, Yd, csr, sent, ws3, False)
    assert same_bits(grad, grad4) and same_bits(sent[:1], stats[:1]) and sent.tolist()[1:] == [-7.5, -9.25, -11.0]


# ---------------------------------------------------------------------------------------------- one step
_objective_cache = {}


def step_case(oracle, N, D):
    if (N, D) not in _objective_cache:
        Y = with_coincident_neighbour(embedding("normal", N, D, seed=1))
        P = attraction(N, seed=1)
        o = oracle.tsne_objective(Y, *P, D)
        _objective_cache[(N, D)] = (Y, P, o, grad_bound(o, N))
    return _objective_cache[(N, D)]


def prior_state(kind, g_ref, lr, min_gain, seed):
    """update and gains before the step, laid out so that every branch of the rule is taken: gains of 0.0125, 0.0101, exactly
    min_gain, 1 and 7, crossed ("mixed") with an update of the gradient's sign, of the other sign, and 0; "first" is the first
    iteration's update == 0 everywhere."""
    rng = np.random.default_rng([seed, g_ref.size])
    t = (np.arange(g_ref.size) + seed).reshape(g_ref.shape)
    gains = np.asarray([0.0125, 0.0101, min_gain, 1.0, 7.0], np.float32)[t % 5]
    if kind == "first":
        return np.zeros(g_ref.shape), gains
    mag = lr * np.where(g_ref != 0, np.abs(g_ref), 1e-3) * rng.uniform(0.5, 2.0, g_ref.shape)
    sign = np.asarray([1.0, -1.0, 0.0])[(t // 5) % 3] * np.where(g_ref < 0, -1.0, 1.0)
    return sign * mag, gains


def check_step(name, got, ref, decided, bound, g_ref, lr, Y_before):
    """got = (Y_out, update, gains) of the kernel, ref = oracle.tsne_step's result, on the components ``decided``."""
    Yo, up, ga = got
    Yr, ur, gr, ggr = ref
    assert np.array_equal(ga[decided], gr[decided])                                                # bit-equal f32 gains
    tol_u = lr * (gr.astype(np.float64) * bound + U * np.abs(ggr))
    within(name + " update", np.abs(up - ur)[decided], tol_u[decided])
    y_ref = Y_before.astype(np.float64) + ur
    within(name + " position", np.abs(Yo.astype(np.float64) - y_ref)[decided], (tol_u + U * np.abs(y_ref))[decided])


@pytest.mark.parametrize("compute_error", [False, True])
@pytest.mark.parametrize("min_gain", [0.01, 0.05])
@pytest.mark.parametrize("momentum", [0.5, 0.8])
@pytest.mark.parametrize("state", ["first", "mixed"])
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("N", [2, 257, 1025, 2049])
def test_step_against_the_oracle(ops, oracle, N, D, state, momentum, min_gain, compute_error):
    lr = 200.0
    Y, P, o, bound = step_case(oracle, N, D)
    g_ref = o["grad"]
    decided = np.abs(g_ref) > 4 * bound
    share = 1.0 - decided.mean()
    assert share <= 0.01, share                             # a condition on the case, from the oracle alone
    note("step: undecided share", share)
    update0, gains0 = prior_state(state, g_ref, lr, min_gain, seed=N + D)
    ref = oracle.tsne_step(Y, update0, gains0, g_ref, momentum, lr, min_gain)
    if state == "mixed" and g_ref.size >= 30:               # every branch is there
        f32 = np.float32
        inc = update0 * g_ref < 0
        assert inc.any() and (~inc & (update0 != 0)).any() and (update0 == 0).any()
        assert np.any(ref[2] == f32(min_gain)) and np.any(ref[2] == f32(7.0) + f32(0.2)) and np.any(ref[2] == f32(1.0) * f32(0.8))

    Yd, csr = dev(Y), csr_dev(P)
    Yn = torch.full_like(Yd, float("nan"))
    update, gains = dev(update0), dev(gains0)
    stats = torch.tensor([-1.0, -7.5, -9.25, -11.0], dtype=torch.float64, device=DEV)
    ops.tsne_step(Yd, Yn, *csr, update, gains, stats, ops.tsne_workspace(N, D), momentum, lr, min_gain, compute_error)
    assert np.array_equal(Yd.cpu().numpy().view(np.int32), Y.view(np.int32))                       # Y is read only
    got = (Yn.cpu().numpy(), update.cpu().numpy(), gains.cpu().numpy())
    assert all(np.all(np.isfinite(a)) for a in got)
    check_step("step", got, ref, decided, bound, g_ref, lr, Y)
    # an undecided component took one of the two branches
    f = np.float32
    either = (got[2] == np.maximum(gains0 + f(0.2), f(min_gain))) | (got[2] == np.maximum(gains0 * f(0.8), f(min_gain)))
    assert np.all(either)
    st = stats.cpu().numpy()
    within("step: Z", abs(st[0] - o["Z"]), GAMMA * (o["Z"] + N))
    if compute_error:
        check_kl("step: KL", oracle, Y, P, o, st[1], st[0])
        gg = (momentum * update0 - got[1]) / lr                                                    # g x gain as the kernel applied it
        within("step: |grad gain|^2", abs(st[2] - float(np.sum(gg * gg))), 4 * U * float(np.sum(gg * gg)))
    else:
        assert st[1] == -7.5 and st[2] == -9.25
    assert st[3] == -11.0


def test_step_refuses_aliased_output(ops):
    N, D = 257, 2
    Y = dev(embedding("normal", N, D))
    csr = csr_dev(attraction(N))
    update = torch.full((N, D), 0.25, dtype=torch.float64, device=DEV)
    gains = torch.full((N, D), 3.0, device=DEV)
    stats = torch.tensor([-1.0, -7.5, -9.25, -11.0], dtype=torch.float64, device=DEV)
    before = Y.clone()
    with pytest.raises(ValueError, match="must not alias"):
        ops.tsne_step(Y, Y, *csr, update, gains, stats, ops.tsne_workspace(N, D), 0.5, 200.0, 0.01, True)
    torch.cuda.synchronize()
    assert same_bits(Y, before) and bool((update == 0.25).all()) and bool((gains == 3.0).all())      # nothing was launched
    assert stats.tolist() == [-1.0, -7.5, -9.25, -11.0]


@pytest.mark.parametrize("D", [1, 2, 3])
def test_three_step_ping_pong_chain(ops, oracle, D):
    """Three iterations with the buffers swapped as DeviceTSNE._gradient_descent swaps them.  The oracle evaluates its gradient at
    the positions the device holds (exact f32 data) and carries its own update and gains, so the error of the update accumulates
    as e_t = momentum e_(t-1) + lr (gain bound_t + u |gain g_t|).  A component stays in the comparison while it is decided at
    every step: |g_ref| > 4 bound, and the carried update either exactly 0 on both sides (the start) or |update_ref| > 4 e."""
    N, lr, momentum, min_gain = 1025, 200.0, 0.5, 0.01
    Y0 = with_coincident_neighbour(embedding("normal", N, D, seed=2))
    P = attraction(N, seed=2)
    csr = csr_dev(P)
    Ya, Yb = dev(Y0), torch.full((N, D), float("nan"), device=DEV)
    update = torch.zeros((N, D), dtype=torch.float64, device=DEV)
    gains = torch.ones((N, D), device=DEV)
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    ws = ops.tsne_workspace(N, D)
    u_ref, g_ref = np.zeros((N, D)), np.ones((N, D), np.float32)
    e = np.zeros((N, D))
    alive = np.ones((N, D), bool)
    for it in range(3):
        Yh = Ya.cpu().numpy()
        o = oracle.tsne_objective(Yh, *P, D)
        bound = grad_bound(o, N)
        alive &= (np.abs(o["grad"]) > 4 * bound) & ((e == 0) & (u_ref == 0) | (np.abs(u_ref) > 4 * e))
        assert alive.mean() >= 0.95, (it, alive.mean())     # too few decided components is a failure of the case, not of a bound
        note("chain: share dropped as undecided", 1.0 - alive.mean())
        Yr, u_ref, g_ref, gg = oracle.tsne_step(Yh, u_ref, g_ref, o["grad"], momentum, lr, min_gain)
        e = momentum * e + lr * (g_ref.astype(np.float64) * bound + U * np.abs(gg))
        ops.tsne_step(Ya, Yb, *csr, update, gains, stats, ws, momentum, lr, min_gain, it == 2)
        assert np.array_equal(Ya.cpu().numpy().view(np.int32), Yh.view(np.int32))
        Ya, Yb = Yb, Ya
        assert np.array_equal(gains.cpu().numpy()[alive], g_ref[alive])
        within(f"chain: update, step {it + 1}", np.abs(update.cpu().numpy() - u_ref)[alive], e[alive])
        y_ref = Yh.astype(np.float64) + u_ref
        within(f"chain: position, step {it + 1}", np.abs(Ya.cpu().numpy().astype(np.float64) - y_ref)[alive], (e + U * np.abs(y_ref))[alive])
    check_kl("chain: KL", oracle, Yh, P, o, float(stats[1]), float(stats[0]))


# ---------------------------------------------------------------------------------------------- the perplexity bisection
ROW_KINDS = 8


def perplexity_rows(N, k, rot, seed):
    """Row i is of kind (i + rot) % 8: random tie-free (sorted), unsorted, all zero, all equal, all 1e10, five zeros then 1e12,
    one 1e-30 then 3e38, exact ties."""
    rng = np.random.default_rng([seed, N, k])
    d = rng.gamma(3.0, 1.0, (N, k)) * 10.0 ** rng.uniform(-2.0, 2.0, (N, 1))
    kind = (np.arange(N) + rot) % ROW_KINDS
    d[kind == 0] = np.sort(d[kind == 0], 1)
    d[kind == 2] = 0.0
    d[kind == 3] = rng.uniform(0.5, 50.0, (int((kind == 3).sum()), 1))
    d[kind == 4] = 1e10
    five = np.full(k, 1e12)
    five[: min(5, max(k - 1, 1))] = 0.0
    d[kind == 5] = five
    far = np.full(k, 3e38)
    far[0] = 1e-30
    d[kind == 6] = far
    d[kind == 7] = np.round(2.0 * rng.uniform(0.0, 6.0, (int((kind == 7).sum()), k))) / 2.0
    return d.astype(np.float32)


# a pair with perplexity >= k is the regime that never converges: kept for the smallest two such perplexities of every k
PERPLEXITY_PAIRS = [(k, p) for k in (1, 2, 3, 16, 91, 151, 301) for p in (2.0, 5.0, 30.0, 50.0, 100.0)
                    if p < k or sum(q >= k for q in (2.0, 5.0, 30.0, 50.0, 100.0) if q < p) < 2]


@pytest.mark.parametrize("k,perplexity", PERPLEXITY_PAIRS)
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1000])
def test_perplexity_against_the_oracle(ops, oracle, N, k, perplexity):
    H = math.log(float(np.float32(perplexity)))
    for rot in (range(ROW_KINDS) if N < ROW_KINDS else (N % ROW_KINDS,)):
        sqd = perplexity_rows(N, k, rot, seed=3)
        P_ref, steps_ref, margin = oracle.tsne_binary_search_perplexity(sqd, perplexity)
        edge = margin < 1e-9
        assert edge.mean() <= 0.001, edge.mean()            # a condition on the case, from the oracle alone
        note("perplexity: edge share", edge.mean())
        d = dev(sqd)
        P, steps = ops.tsne_perplexity(d, perplexity)
        P2 = torch.full_like(P, float("nan"))
        raw_perplexity_without_steps(ops, d, P2, perplexity)
        assert same_bits(P, P2)                             # n_steps = NULL
        P, steps = P.cpu().numpy(), steps.cpu().numpy()
        assert P.shape == (N, k) and steps.shape == (N,) and np.all(np.isfinite(P))
        ok = ~edge
        assert np.array_equal(steps[ok], steps_ref[ok])
        err = np.abs(P - P_ref)[ok]
        tol = 1e-12 * np.abs(P_ref[ok]) + 1e-15 * P_ref[ok].max(1, keepdims=True)
        if err.size:
            note("perplexity: P error / tolerance", float(np.max(err / np.where(tol > 0, tol, 1.0), initial=0.0)))
        assert np.all(err <= tol)
        conv = ok & (steps > 0)
        assert np.all(np.abs(P[conv].sum(1) - 1.0) <= 1e-12)
        ent = -np.sum(P * np.log(np.where(P > 0, P, 1.0)), 1)
        assert np.all(np.abs(ent[conv] - H) <= TOL)


def test_perplexity_cases_hold_every_regime(oracle):
    assert any(p >= k for k, p in PERPLEXITY_PAIRS) and {k for k, _ in PERPLEXITY_PAIRS} == {1, 2, 3, 16, 91, 151, 301}
    assert {p for _, p in PERPLEXITY_PAIRS} == {2.0, 5.0, 30.0, 50.0, 100.0}
    sqd = perplexity_rows(1000, 91, 0, seed=3)
    _, steps, _ = oracle.tsne_binary_search_perplexity(sqd, 30.0)
    kind = np.arange(1000) % ROW_KINDS
    assert np.all(steps[kind <= 1] > 0) and np.all(steps[np.isin(kind, (2, 3, 4, 6))] == 0)        # converging and never-converging rows


# ---------------------------------------------------------------------------------------------- the symmetrisation
def neighbour_lists(N, k, seed):
    rng = np.random.default_rng([seed, N, k])
    idx = np.stack([np.sort(rng.choice(N - 1, k, replace=False)) for _ in range(N)])
    idx += idx >= np.arange(N)[:, None]                     # never the row itself
    return idx


SYM_CASES = {
    "mutual and one-sided": lambda: (neighbour_lists(300, 10, 4), "random", []),
    "rows of zeros": lambda: (neighbour_lists(300, 10, 5), "bisection", list(range(4, 300, 8))),
    "k = 1": lambda: (neighbour_lists(257, 1, 6), "random", [3, 200]),
    "N = 2": lambda: (np.asarray([[1], [0]]), "random", []),
    "N = 2, one-sided zero": lambda: (np.asarray([[1], [0]]), "random", [1]),
    "last index": lambda: (neighbour_lists(300, 3, 7), "random", [0]),
    "all zero": lambda: (neighbour_lists(40, 3, 8), "random", list(range(40))),
}


@pytest.mark.parametrize("case", sorted(SYM_CASES))
def test_symmetrize_against_the_oracle(ops, oracle, case):
    from velocyto_amd.tsne import _symmetrize
    idx, how, zero_rows = SYM_CASES[case]()
    if case == "last index":                                # every row but the last lists column N - 1 (rows are sorted: it comes last)
        idx[:-1, -1] = idx.shape[0] - 1
    N, k = idx.shape
    assert all(len(set(r)) == k and i not in r for i, r in enumerate(idx.tolist())) and idx.max() == N - 1
    rng = np.random.default_rng(9)
    if how == "bisection":                                  # rows of 1e10: the bisection's own exact zeros
        sqd = (rng.gamma(3.0, 1.0, (N, k)) * 3.0).astype(np.float32)
        sqd[zero_rows] = 1e10
        cond, _, _ = oracle.tsne_binary_search_perplexity(sqd, 3.0)
        assert not cond[zero_rows].any()
    else:
        cond = rng.uniform(0.01, 1.0, (N, k))
        cond /= cond.sum(1, keepdims=True)
        cond[zero_rows] = 0.0
    indptr_ref, indices_ref, val_ref = oracle.tsne_joint_p(idx, cond)
    indptr, indices, val = _symmetrize(dev(idx.astype(np.int64)), dev(cond))
    assert indptr.dtype == torch.int64 and indices.dtype == torch.int32 and val.dtype == torch.float64
    indptr, indices, val = indptr.cpu().numpy(), indices.cpu().numpy(), val.cpu().numpy()
    assert np.array_equal(indptr, indptr_ref) and np.array_equal(indices, indices_ref)
    if len(val_ref):
        # entry by entry the same addition, then one division on either side: up to the two normalisers every ratio is the same
        ratio = val / val_ref
        assert ratio.max() / ratio.min() - 1.0 <= 4 * 2.0 ** -53
        note("symmetrize: normaliser, device sum against fsum / 1e-15", abs(float(np.median(ratio)) - 1.0) / 1e-15)
    # the normaliser is a device tree sum of < 2^13 positive terms against the oracle's exact fsum: at most one rounding per
    # level (13 x 2^-53 = 1.4e-15 if all fell the same way, a few 1e-16 as they fall), inside the 1e-15 the values are held to
    np.testing.assert_allclose(val, val_ref, rtol=1e-15, atol=0)
    if len(val_ref):
        note("symmetrize: value error / 1e-15", float(np.max(np.abs(val - val_ref) / val_ref)) / 1e-15)
        assert abs(math.fsum(val) - 1.0) <= 1e-15 + 2.0 ** -52      # what the tolerance on the values leaves to their sum
        dense = np.zeros((N, N))
        dense[np.repeat(np.arange(N), np.diff(indptr)), indices] = val
        assert np.array_equal(dense, dense.T)
    if zero_rows and how == "bisection":
        assert len(val) < len(np.unique(np.concatenate([np.arange(N).repeat(k) * N + idx.ravel(), idx.ravel() * N + np.arange(N).repeat(k)])))
