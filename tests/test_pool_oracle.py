"""The long-double reference of stage A (oracle.pool_reference) and its derived bound (oracle.pool_bound), checked on the CPU before
test_gpu_pool_kernels.py holds the HIP kernels to them:
  * the reference agrees with the f64 restatement (oracle.convolve_by_sparse_weights) and with the golden vectors of the reference
    implementation to f64 rounding - (2 n + 2) 2^-53 A for a multiply-add chain of n terms, A = sum |w s x|;
  * a plain numpy chain in the working type (oracle.pool_emulated) stays inside the bound on every case: a correct implementation
    can meet it;
  * the bound is small against a single term of the sum it bounds, so a dropped or doubled term cannot hide inside it: by a
    factor 1e6 in f64 on every case, by a factor 8 in f32 on every structural case (small counts, weights in [0.5, 1]).  The
    cases that f32 cannot resolve (counts of 1 next to 65535, factors 2^20 apart) are marked and must still meet the f64 condition."""
import numpy as np
import pytest
from scipy import sparse

import pool_cases as pc

U64 = 2.0 ** -53
f64 = lambda a: np.asarray(a, dtype=np.float64)


def _within(got, ref, bound, what):
    err = np.abs(np.asarray(got).astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(err <= bound), (what, float(np.max(err - bound)))
    assert np.all(f64(got)[f64(bound) == 0] == f64(ref)[f64(bound) == 0]), what
    with np.errstate(all="ignore"):
        return float(np.max(np.where(bound > 0, err / bound, 0.0))) if err.size else 0.0


def test_reference_against_f64_restatement_and_golden_neighbors(oracle, golden):
    g = golden("neighbors")
    C = g["space"].shape[0]
    indptr, indices, w = g["w_indptr"].astype(np.int64), g["w_indices"], g["w_data"]
    ref, A = oracle.pool_reference(indptr, indices, w, g["data"].T)
    n = np.diff(indptr)
    bound = (2.0 * n[:, None] + 2.0) * U64 * f64(A)
    wcsr = sparse.csr_matrix((w, indices, indptr), shape=(C, C))
    _within(oracle.convolve_by_sparse_weights(g["data"], wcsr).T, ref, bound, "convolve_by_sparse_weights")
    _within(g["convolved"].T, ref, bound, "golden convolved")
    mx, A2, own = oracle.pool_reference(indptr, indices, w, g["data"].T, maximum=True)
    assert np.array_equal(A2, A) and np.array_equal(f64(own), np.abs(g["data"].T))
    assert np.array_equal(mx, np.maximum(ref, g["data"].T.astype(np.longdouble)))


def test_reference_against_golden_pipeline(oracle, golden):
    """Sx, Ux (k = 12, diag 1) and max_Sx, max_Ux (diag 2, maximum) of the reference implementation from its own S_sz, U_sz and
    kNN graph; the weights are rebuilt here, so each may differ from the reference's by a rounding: (2 n + 6) 2^-53 A."""
    g = golden("pipeline")
    C = g["knn_indices"].shape[0]
    knn = sparse.csr_matrix((np.maximum(g["knn_dist"], 1e-300).ravel(), g["knn_indices"].ravel(), np.arange(0, C * 12 + 1, 12)), shape=(C, C))
    for diag, maximum, names in ((1.0, False, ("Sx", "Ux")), (2.0, True, ("max_Sx", "max_Ux"))):
        w = sparse.csr_matrix(oracle.connectivity_to_weights(knn, diag))
        w.sort_indices()
        indptr = w.indptr.astype(np.int64)
        for layer, name in zip(("S_sz", "U_sz"), names):
            res = oracle.pool_reference(indptr, w.indices, w.data, g[layer].T, maximum=maximum)
            bound = (2.0 * np.diff(indptr)[:, None] + 6.0) * U64 * f64(res[1])
            _within(g[name].T, res[0], bound, name)               # (np.maximum with the exact own row adds no error)


def test_reference_scale_cell0_and_empty_rows(oracle):
    """scale multiplies the SOURCE row, cell0 names the own row of `maximum`, an empty graph row pools to 0 (and to its own row with
    maximum); an array of own rows gives what the int gives."""
    cs = pc.count_case(17, "structural")
    blk = pc.block(cs["graph"], pc.BLOCK_CELL0, 9)
    out, A, own = oracle.pool_reference(blk[0], blk[1], blk[2], cs["S"], cs["sS"], maximum=True, cell0=pc.BLOCK_CELL0)
    plain, _ = oracle.pool_reference(blk[0], blk[1], blk[2], cs["S"] * cs["sS"][:, None])
    assert np.allclose(f64(out), np.maximum(f64(plain), (cs["S"] * cs["sS"][:, None])[pc.BLOCK_CELL0:pc.BLOCK_CELL0 + 9]), rtol=1e-15, atol=0)
    empty = np.flatnonzero(np.diff(blk[0]) == 0)
    assert empty.size and np.all(A[empty] == 0) and np.array_equal(out[empty], own[empty])
    again = oracle.pool_reference(blk[0], blk[1], blk[2], cs["S"], cs["sS"], maximum=True, cell0=pc.BLOCK_CELL0 + np.arange(9))
    assert all(np.array_equal(a, b) for a, b in zip(again, (out, A, own)))
    rows = pc.graph_rows(cs["graph"], [7, 2, 30])
    sub, subA = oracle.pool_reference(rows[0], rows[1], rows[2], cs["S"], cs["sS"])
    full, fullA = oracle.pool_reference(*cs["graph"][:3], cs["S"], cs["sS"])
    assert np.array_equal(sub, full[[7, 2, 30]]) and np.array_equal(subA, fullA[[7, 2, 30]])


def _all_cases():
    """(name, structural, counts, indptr, indices, w (f64), data, scale) of every fast case; w is rounded per working type by the caller."""
    for G in pc.FLOAT_G:
        for dt in pc.DTYPES:
            cs = pc.float_case(G, dt)
            g = cs["graph"]
            yield f"float G={G} {dt}", True, False, g[0], g[1], g[2], cs["data"], None, (dt,)
            yield f"float w2 G={G} {dt}", True, False, g[0], g[1], g[3], cs["data2"], None, (dt,)
    for G in pc.COUNT_G:
        for kind in ("structural", "range"):
            cs = pc.count_case(G, kind)
            g = cs["graph"]
            yield f"counts S {kind} G={G}", cs["structural"], True, g[0], g[1], g[2], cs["S"], cs["sS"], pc.DTYPES
            yield f"counts U {kind} G={G}", cs["structural"], True, g[0], g[1], g[2], cs["U"], cs["sU"], pc.DTYPES
    for G in pc.CSR_G:
        for wide in (False, True):
            cs = pc.csr_case(G, wide)
            g = cs["graph"]
            yield f"csr G={G} wide={wide}", cs["structural"], True, g[0], g[1], g[2], cs["dense"], cs["scale"], pc.DTYPES


@pytest.mark.parametrize("family", ["float", "counts", "csr"])
def test_emulated_chain_meets_the_bound_and_the_bound_resolves_a_term(oracle, family):
    worst = {dt: 0.0 for dt in pc.DTYPES}
    margin = {dt: np.inf for dt in pc.DTYPES}
    for name, structural, counts, indptr, indices, w, data, scale, dtypes in _all_cases():
        if not name.startswith(family):
            continue
        n = np.diff(indptr)
        for dt in dtypes:
            wd = pc.stored(w, dt)
            for maximum in (False, True):
                ref = oracle.pool_reference(indptr, indices, wd, data, scale, maximum=maximum)
                got = oracle.pool_emulated(indptr, indices, wd, data, scale, dt, maximum=maximum)
                # the emulation rounds product and sum separately in f64 (2 n roundings); in f32 its f64 intermediate adds nothing
                bound = oracle.pool_bound(ref[1], 2 * n if dt == "float64" else n, dt, counts, own=ref[2] if maximum else None)
                worst[dt] = max(worst[dt], _within(got, ref[0], bound, (name, dt, maximum)))
            bound = oracle.pool_bound(ref[1], n, dt, counts)              # (A does not depend on `maximum`)
            small = pc.smallest_term(indptr, indices, wd, data, scale)
            has = np.isfinite(small)
            assert np.array_equal(has, f64(ref[1]) > 0)
            if dt == "float64":
                assert np.all(small[has] >= 1e6 * bound[has]), (name, float((small[has] / bound[has]).min()))
            elif structural:
                assert np.all(small[has] >= 8.0 * bound[has]), (name, float((small[has] / bound[has]).min()))
            if has.any() and (dt == "float64" or structural):
                margin[dt] = min(margin[dt], float((small[has] / bound[has]).min()))
    print(f"pool {family}: emulated chain uses at most {worst['float32']:.3f} (f32) / {worst['float64']:.3f} (f64) of the bound; "
          f"smallest term / bound >= {margin['float32']:.1f} (f32, structural cases) / {margin['float64']:.3g} (f64)")


def test_marked_cases_are_the_ones_f32_cannot_resolve(oracle):
    """The cases excused from the f32 condition are excused for a reason: each holds an output whose smallest term is below 8 bounds."""
    for name, structural, counts, indptr, indices, w, data, scale, dtypes in _all_cases():
        if structural or name.startswith("counts S"):
            continue
        wd = pc.stored(w, "float32")
        _, A = oracle.pool_reference(indptr, indices, wd, data, scale)
        bound = oracle.pool_bound(A, np.diff(indptr), "float32", counts)
        small = pc.smallest_term(indptr, indices, wd, data, scale)
        has = np.isfinite(small)
        assert (small[has] < 8.0 * bound[has]).any(), name


def test_case_builders_hold_what_they_promise():
    g = pc.graph(pc.FLOAT_C)
    lens = set(np.diff(g[0]).tolist())
    assert set(range(10)) <= lens and {64, 65, 128, 129, 81} <= lens
    assert g[1][g[0][3]:g[0][4]].tolist() == [3] and g[1][g[0][2]] == g[1][g[0][2] + 1]
    assert g[2].min() >= 0.5 and g[2].max() <= 1.0
    w2 = pc.graph(pc.FLOAT_C, signed=True)[3]
    assert (w2 < 0).any() and (w2 > 0).any()
    for G in pc.COUNT_G:
        cs = pc.count_case(G, "range")
        assert cs["S"].max() <= 255 and max(np.diff(cs["graph"][0])) <= 9
        for s in (cs["sS"], cs["sU"]):
            assert np.all(s.astype(np.float32).astype(np.float64) != s) and s.min() < 2.0 ** -9 and s.max() >= 2.0 ** 9
    seen = set(np.unique(np.concatenate([pc.count_case(G, "range")["U"].ravel() for G in pc.COUNT_G])).tolist())
    assert set(pc.EDGE_COUNTS) <= seen
    for G in pc.CSR_G:
        for wide in (False, True):
            cs = pc.csr_case(G, wide)
            ptr, idx = cs["indptr"], cs["indices"]
            for r in range(cs["C"]):
                assert np.all(np.diff(idx[ptr[r]:ptr[r + 1]]) > 0)
            sp = pc.slab_ptr_reference(ptr, idx, G)
            seg = np.diff(sp, axis=1)
            assert set(pc.CSR_SEGMENTS) <= set(seg[:, 0].tolist()) or G < 300
            assert seg[1].sum() == 0 and seg[11].max() == min(G, pc.CSR_SLAB) and ptr[-1] - ptr[-2] == 1 and idx[-1] == G - 1
            assert {g for g in pc.CSR_PLANTED if g < G} | {G - 1} == set(idx[ptr[0]:ptr[1]].tolist())
            if wide:
                assert cs["dense"][11].min() > 255
