"""The kNN search (csrc/knn.hip: k_knn_search in its three instances, ops.knn_search / ops.knn_query and the segment merge) at its
plan boundaries, its branches and the edges of its f32 candidate pass, against the plain f64 loop of knn_cases.knn_reference.

The contract is DESIGN section 13: (a) on an f32-decidable query the indices AND the distances are the reference's, bit for bit;
(b) on any query the list is sorted by (distance, index), free of repeats and of the excluded query, carries the exact f64 distances
of its indices, and holds no candidate beyond the f32 reach of the true top-ksel.  Which queries are decidable, and which branch a
constructed query takes, is established on the CPU by test_knn_oracle.py from the inputs alone; the cases here are the same objects."""
import numpy as np
import pytest

import knn_cases as kc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def _np(t):
    return t.cpu().numpy()


def _lib(ops):
    from velocyto_amd import _lib as L
    return L, L.lib()


def _feature_major(a32, ld, pad):
    """(P, ld) f32 device copy of a (n, P) f32 array, columns n.. filled with `pad`."""
    t = torch.full((a32.shape[1], ld), pad, dtype=torch.float32, device="cuda")
    t[:, :a32.shape[0]] = torch.from_numpy(np.ascontiguousarray(a32.T)).cuda()
    return t


def _abi_search(ops, x, k, include_self, q0, Q, ldx=None, pad=0.0, queries=None, ldq=None, qpad=0.0):
    """vcy_knn_search (queries None: rows q0.. of x) or vcy_knn_query (`queries`: ALL external query points, of which q0..q0+Q are
    searched) called directly, with the f32 copies of knn_cases.f32_copy.  Outputs are prefilled, so an untouched entry shows."""
    mod, L = _lib(ops)
    x = np.asarray(x, dtype=np.float64)
    C, P = x.shape
    x32, q32, _ = kc.f32_copy(x, queries)
    ldx = (C + 63) // 64 * 64 if ldx is None else ldx
    xt = _feature_major(x32, ldx, pad)
    x64 = torch.from_numpy(np.array(x)).cuda()
    idx = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((Q, k), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(int(L.vcy_knn_workspace_bytes(C, Q, k)), dtype=torch.uint8, device="cuda")
    if queries is None:
        rc = L.vcy_knn_search(xt.data_ptr(), x64.data_ptr(), idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), C, P, ldx, q0, Q, k,
                              int(include_self), ops._stream())
    else:
        nq = q32.shape[0]
        ldq = (nq + 63) // 64 * 64 if ldq is None else ldq
        qt = _feature_major(q32, ldq, qpad)
        q64 = torch.from_numpy(np.array(queries, dtype=np.float64)).cuda()
        rc = L.vcy_knn_query(xt.data_ptr(), x64.data_ptr(), qt.data_ptr(), q64.data_ptr(), ldq, idx.data_ptr(), dist.data_ptr(),
                             ws.data_ptr(), C, P, ldx, q0, Q, k, ops._stream())
    torch.cuda.synchronize()
    return rc, _np(idx), _np(dist)


def _hold(an, idx, dist, what, designated=()):
    wrong = kc.check_contract(an, _np(idx) if hasattr(idx, "cpu") else idx, _np(dist) if hasattr(dist, "cpu") else dist,
                              designated=designated, what=what)
    print(f"{what}: {int(an['decidable'].sum())} of {an['decidable'].size} queries decidable, {wrong} lists differ from the reference")
    return wrong


# ---------------------------------------------------------------- plan boundaries
def _plan_ws_bytes(k):
    pl = kc.plan(kc.PLAN_C, k)
    qpad = (kc.PLAN_Q + 7) // 8 * 8
    rows = (qpad // 8 if pl["row_free"] else qpad) * kc.PLAN_C * 4
    return rows + ((qpad // 8) * pl["nsort"] * 12 + 256 if pl["large"] else 0)


def test_plan_entry_points(ops):
    """nsort 128 -> 256 at k = 24/25 (no trace in the workspace), row-free -> rows at 120/121, threshold -> radix select at 504/505,
    the nsort cap at 1016/1017, LDS -> global sort at 4088/4089."""
    _, L = _lib(ops)
    plans = {k: kc.plan(kc.PLAN_C, k) for k in kc.PLAN_K}
    assert [plans[k]["nsort"] for k in kc.PLAN_K] == [128, 256, 512, 1024, 2048, 4096, 4096, 4096, 4096, 8192]
    assert [plans[k]["row_free"] for k in kc.PLAN_K] == [True, True, True] + [False] * 7
    assert [plans[k]["large"] for k in kc.PLAN_K] == [False] * 9 + [True]
    for k in kc.PLAN_K:
        assert L.vcy_knn_row_free(kc.PLAN_C, k) == int(plans[k]["row_free"]), k
        assert L.vcy_knn_workspace_bytes(kc.PLAN_C, kc.PLAN_Q, k) == _plan_ws_bytes(k), k
    ws = [L.vcy_knn_workspace_bytes(kc.PLAN_C, kc.PLAN_Q, k) for k in kc.PLAN_K]
    assert ws[0] == ws[1] == ws[2] and ws[3] == 8 * ws[2] and ws[3] == ws[4] == ws[5] == ws[6] == ws[7] == ws[8] and ws[9] > ws[8]


@pytest.mark.parametrize("include_self", [False, True])
@pytest.mark.parametrize("k", kc.PLAN_K)
def test_plan_boundaries(ops, k, include_self):
    """19 queries from row 1000 (a last workgroup of three) on either side of every boundary of the plan.  The two queries inside
    the block of 40 exact duplicates are undecidable by the count at k = 24 and 25 (39 candidates at distance 0 against ksel = 32
    and 33) and still exact: points with the same coordinates have the same f32 image, tie in f32 as they do in f64, and every
    select path takes tied candidates by index or all of them."""
    an = kc.analysed("plan", k, include_self)
    idx, dist = ops.knn_search(kc.plan_points(), k, include_self=include_self, q0=kc.PLAN_Q0, Q=kc.PLAN_Q)
    _hold(an, idx, dist, f"plan k={k} include_self={include_self}", designated=kc.PLAN_UNDECIDABLE.get(k, ()))
    assert np.array_equal(_np(idx), an["idx"]) and np.array_equal(_np(dist), an["dist"])
    assert list(_np(idx)[0, :3]) == [962, 963, 964] and (_np(dist)[0, :3] == 0).all()                # duplicates: by index


# ---------------------------------------------------------------- branches of the row-free kernel
@pytest.mark.parametrize("n", sorted(kc.OVER_CLASS))
def test_rowfree_overflow_count(ops, n):
    """n threads whose fourth tracked word is within the threshold: none, one, eight (the most the rescan takes) and nine (the row)."""
    x = kc.overflow_points(n)
    idx, dist = ops.knn_search(x, kc.OVER_K, q0=kc.BLOCK_Q0, Q=kc.BLOCK_Q)
    an = kc.analysed("overflow", n)
    assert an["decidable"][kc.OVER_Q - kc.BLOCK_Q0]
    assert _hold(an, idx, dist, f"overflow n={n}") == 0
    planted = {t + 256 * m for t in kc.OVER_TIDS[:n] for m in (0, 2, 4, 6, 8)}
    got = set(_np(idx)[kc.OVER_Q - kc.BLOCK_Q0].tolist())
    assert got <= planted if len(planted) > kc.OVER_K else planted <= got


def test_rowfree_too_many_within_threshold(ops):
    """No overflowing thread, but 300 tracked words within the threshold against a sort of 128: the row, and an exact result."""
    x = kc.count_points()
    idx, dist = ops.knn_search(x, kc.COUNT_K, q0=kc.BLOCK_Q0, Q=kc.BLOCK_Q)
    an = kc.analysed("count")
    assert an["decidable"][kc.COUNT_Q - kc.BLOCK_Q0]
    assert _hold(an, idx, dist, "count") == 0
    idx2, dist2 = ops.knn_search(x, kc.COUNT_K, include_self=True, q0=kc.COUNT_Q - 3, Q=5)
    an2 = kc.analyse(x, x[kc.COUNT_Q - 3:kc.COUNT_Q + 2], kc.COUNT_K)
    assert _hold(an2, idx2, dist2, "count include_self") == 0


@pytest.mark.parametrize("k", kc.CAP_K)
@pytest.mark.parametrize("C", [kc.CAP_C, kc.CAP_C + 1])
def test_slice_position_cap(ops, C, k):
    """The largest launch of the row-free kernel (ten position bits, positions up to 1019) and the smallest one that the position
    bits send to the rows kernel, straight at the ABI: the last 16 rows as queries, their neighbours in ONE thread's slice."""
    _, L = _lib(ops)
    assert L.vcy_knn_row_free(C, k) == int(C == kc.CAP_C) == int(kc.plan(C, k)["row_free"])
    x = kc.cap_points(kc.CAP_PLANT[k])[:C]
    rc, idx, dist = _abi_search(ops, x, k, False, kc.CAP_C - kc.CAP_Q, kc.CAP_Q)
    assert rc == 0
    an = kc.analysed("cap", C, k)
    assert an["decidable"].all() and (an["idx"] == 255).any()            # the candidate at slice position 1019 is in the lists
    assert _hold(an, idx, dist, f"cap C={C} k={k}") == 0


def test_segmentation_at_the_real_constant(ops):
    """ops.knn_search at KNN_SEGMENT points (one launch) and at KNN_SEGMENT + 1 (two segments, merged): the extra point is far from
    every query, so both give the same lists, and each gives the reference's."""
    S, Q, k = kc.SEGMENT, kc.SEGMENT_Q, kc.SEGMENT_K
    assert ops.KNN_SEGMENT == S and kc.plan(S, k)["row_free"]
    x = kc.segment_points()
    out = []
    for C in (S, S + 1):
        idx, dist = ops.knn_search(x[:C], k, q0=S - Q, Q=Q)
        assert _hold(kc.analysed("segment", C), idx, dist, f"segmentation C={C}") == 0
        out.append((_np(idx), _np(dist)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---------------------------------------------------------------- strides
@pytest.mark.parametrize("pad", [float("nan"), 1e30])
def test_strides_and_padding(ops, pad):
    """ldx > C and ldq > Q with the padding columns full of NaN / 1e30, external queries from q0 > 0: bit-equal to the tight, zero-padded
    call, and the reference's lists."""
    C, P, k = kc.STRIDE_C, kc.STRIDE_P, kc.STRIDE_K
    x, qs = kc.stride_points()
    rc, i0, d0 = _abi_search(ops, x, k, False, 690, 10)
    rc1, i1, d1 = _abi_search(ops, x, k, False, 690, 10, ldx=C + 37, pad=pad)
    assert rc == 0 and rc1 == 0 and np.array_equal(i0, i1) and np.array_equal(d0, d1)
    assert _hold(kc.analyse(x, x[690:700], k, kc.self_exclude(690, 10)), i1, d1, f"self search, padded with {pad}") == 0
    q0, Q = 13, 19
    rc, i0, d0 = _abi_search(ops, x, k, True, q0, Q, queries=qs)
    rc1, i1, d1 = _abi_search(ops, x, k, True, q0, Q, ldx=C + 37, pad=pad, queries=qs, ldq=40 + 5, qpad=pad)
    assert rc == 0 and rc1 == 0 and np.array_equal(i0, i1) and np.array_equal(d0, d1)
    assert _hold(kc.analyse(x, qs[q0:q0 + Q], k), i1, d1, f"external queries, padded with {pad}") == 0


# ---------------------------------------------------------------- feature counts
@pytest.mark.parametrize("P", kc.FEATURE_P)
def test_feature_counts(ops, P):
    x = kc.feature_points(P)
    idx, dist = ops.knn_search(x, kc.FEATURE_K)
    assert _hold(kc.analysed("feature", P), idx, dist, f"P={P}") == 0
    i2, d2 = ops.knn_query(x, x[5:50], kc.FEATURE_K)
    assert _hold(kc.analyse(x, x[5:50], kc.FEATURE_K), i2, d2, f"P={P} external") == 0


def test_feature_count_beyond_lds_raises(ops):
    """8 P floats of query coordinates next to the sort arrays: the first P that does not fit is refused before any launch."""
    mod, L = _lib(ops)
    pl = kc.plan(kc.FEATURE_C, kc.FEATURE_K, False)
    P = (150 * 1024 - pl["nsort"] * 12) // (8 * 4) + 1
    x = np.random.default_rng(91).normal(size=(kc.FEATURE_C, P))
    rc, idx, dist = _abi_search(ops, x, kc.FEATURE_K, False, 0, 16)
    assert rc != 0 and b"LDS" in L.vcy_last_error()
    assert (idx == -7).all() and (dist == -7.0).all()
    with pytest.raises(ValueError):
        ops.knn_search(x, kc.FEATURE_K)
    rc, idx, dist = _abi_search(ops, x[:, :P - 1], kc.FEATURE_K, False, 0, 16)
    assert rc == 0
    assert _hold(kc.analyse(x[:, :P - 1], x[:16, :P - 1], kc.FEATURE_K, kc.self_exclude(0, 16)), idx, dist, f"P={P - 1}, the largest") == 0


# ---------------------------------------------------------------- precision of the candidate pass
@pytest.mark.parametrize("name", list(kc.TRANSLATED) + list(kc.SCALED))
def test_precision_translated_and_scaled(ops, name):
    """Dyadic data far from the origin, and scaled far from 1: exact in f64, so the lists are those of the data at the origin."""
    an = kc.analysed("dyadic", name)
    assert an["decidable"].all()
    idx, dist = ops.knn_search(kc.dyadic_points(name), kc.PRECISION_K)
    assert _hold(an, idx, dist, name) == 0
    base = kc.analysed("dyadic", f"{name[:2]}_shift10")
    assert np.array_equal(_np(idx), base["idx"])


def test_precision_shell_within_the_margin(ops):
    (b,) = kc.SHELL_B["decidable"]
    an = kc.analysed("shell", b)
    assert an["decidable"].all() and an["count"][kc.SHELL_Q - kc.BLOCK_Q0] == an["ksel"]
    idx, dist = ops.knn_search(kc.shell_points(b), kc.SHELL_K, q0=kc.BLOCK_Q0, Q=kc.BLOCK_Q)
    assert _hold(an, idx, dist, f"shell b={b}") == 0


def test_precision_shell_strict_select(ops):
    """The same shell where the rows kernel selects exactly k + 8 candidates and the f32 pass ranks a member of the true list last
    of them: the margin of 8 is all used."""
    an = kc.analysed("strict")
    assert an["decidable"].all() and an["count"][kc.SHELL_Q - kc.BLOCK_Q0] == an["ksel"]
    idx, dist = ops.knn_search(kc.strict_shell_points(), kc.STRICT_K, q0=kc.BLOCK_Q0, Q=kc.BLOCK_Q)
    assert _hold(an, idx, dist, "strict shell") == 0


def test_precision_lattice_at_a_shell_end(ops):
    k = kc.LATTICE_K["decidable"]
    an = kc.analysed("lattice", k)
    assert an["decidable"].all()
    idx, dist = ops.knn_search(kc.lattice_points(), k, q0=0, Q=kc.LATTICE_INNER)
    assert _hold(an, idx, dist, f"lattice k={k}") == 0


def test_precision_queries_outside_the_point_set(ops):
    x, q = kc.outside_points()
    an = kc.analysed("outside")
    assert an["decidable"].all()
    idx, dist = ops.knn_query(x, q, kc.OUTSIDE_K)
    assert _hold(an, idx, dist, "queries outside") == 0


@pytest.mark.parametrize("b", kc.SHELL_B["undecidable"])
def test_undecidable_shell(ops, b):
    """More than 8 near-ties beyond rank k: property (b) only for that query, (a) for all the others."""
    an = kc.analysed("shell", b)
    assert not an["decidable"][kc.SHELL_Q - kc.BLOCK_Q0] and an["decidable"].sum() == kc.BLOCK_Q - 1
    idx, dist = ops.knn_search(kc.shell_points(b), kc.SHELL_K, q0=kc.BLOCK_Q0, Q=kc.BLOCK_Q)
    _hold(an, idx, dist, f"shell b={b}", designated=(kc.SHELL_Q - kc.BLOCK_Q0,))


@pytest.mark.parametrize("spread", kc.CLUSTER_SPREAD)
def test_undecidable_clusters(ops, spread):
    an = kc.analysed("cluster", spread)
    assert not an["decidable"].any()
    idx, dist = ops.knn_search(kc.cluster_points(spread), kc.CLUSTER_K)
    _hold(an, idx, dist, f"clusters spread={spread}", designated=range(kc.CLUSTER_C))


def test_undecidable_lattice_inside_a_shell(ops):
    k = kc.LATTICE_K["undecidable"]
    an = kc.analysed("lattice", k)
    assert not an["decidable"].any()
    idx, dist = ops.knn_search(kc.lattice_points(), k, q0=0, Q=kc.LATTICE_INNER)
    _hold(an, idx, dist, f"lattice k={k}", designated=range(kc.LATTICE_INNER))
