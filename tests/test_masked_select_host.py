"""CPU-side checks of the masked streamed select (vcy_gene_mselect_*): a numpy model of its protocol - digit histograms of the key
bits over the kept cells, the population and both ranks from the totals of the first histogram, numpy's lerp at the end - against
np.percentile(values[keep], q); the library's exports and argument validation; atlas.memory_plan's term for the extra state."""
import ctypes

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

SYMBOLS = ("vcy_gene_mselect_state_bytes", "vcy_gene_mselect_begin", "vcy_gene_mselect_count_block", "vcy_gene_mselect_advance",
           "vcy_gene_mselect_finish", "vcy_fit_weighted_moments_masked")
QS = [0, 1, 10, 50, 90, 99.9, 100]


def _keys(v: np.ndarray) -> np.ndarray:
    """Key<T>::enc: the value's bits, order-preserving as unsigned integers (negative: all bits flipped, else the sign bit set)."""
    u = v.view(np.uint32 if v.dtype == np.float32 else np.uint64)
    top = u.dtype.type(1) << u.dtype.type(8 * u.itemsize - 1)
    return np.where(u & top, ~u, u | top)


def _decode(k, dtype):
    u = np.array([k], dtype=np.uint32 if dtype == np.float32 else np.uint64)
    top = u.dtype.type(1) << u.dtype.type(8 * u.itemsize - 1)
    return np.where(u & top, u & ~top, ~u).view(dtype)[0]


def _lerp(a, b, t):
    """numpy's _lerp in float64; at t == 0 the upper value is not used."""
    a, b = np.float64(a), np.float64(b)
    d = b - a
    r = a + d * t
    if t >= 0.5:
        r = b - d * (1 - t)
    return a if t == 0 else r


def model_select(values: np.ndarray, keep: np.ndarray, qs, blocks):
    """The protocol on one gene: per pass, one 256-bin histogram per target summed over `blocks` (index arrays, any order) of the
    kept cells whose key matches the target's prefix; the first pass counts one histogram for all, and its total is the population."""
    keys = _keys(values)
    passes = values.dtype.itemsize
    nq = len(qs)
    prefix = np.zeros(2 * nq, dtype=np.uint64)
    rank = np.zeros(2 * nq, dtype=np.int64)
    frac = np.zeros(nq)
    n = None
    for p in range(passes):
        shift = 8 * (passes - 1 - p)
        hist = np.zeros((1 if p == 0 else 2 * nq, 256), dtype=np.uint32)
        for blk in blocks:
            k = keys[blk][keep[blk]].astype(np.uint64)
            d = ((k >> np.uint64(shift)) & np.uint64(0xff)).astype(np.int64)
            for t in range(hist.shape[0]):
                m = np.ones(k.shape, bool) if p == 0 else (k >> np.uint64(shift + 8)) == (prefix[t] >> np.uint64(shift + 8))
                hist[t] += np.bincount(d[m], minlength=256).astype(np.uint32)
        if p == 0:
            n = int(hist[0].sum())
            if n == 0:
                return np.full(nq, np.nan), 0
            for i, q in enumerate(qs):
                h = np.float64(n - 1) * (np.float64(q) / 100.0)
                lo = int(np.floor(h))
                rank[2 * i], rank[2 * i + 1], frac[i] = lo, min(lo + 1, n - 1), h - lo
        for t in range(2 * nq):
            c = np.cumsum(hist[0 if p == 0 else t].astype(np.int64))
            d = int(np.searchsorted(c, rank[t], side="right"))
            assert d < 256
            prefix[t] |= np.uint64(d) << np.uint64(shift)
            rank[t] -= c[d - 1] if d else 0
    out = [_lerp(_decode(prefix[2 * i], values.dtype), _decode(prefix[2 * i + 1], values.dtype), frac[i]) for i in range(nq)]
    return np.array(out), n


def _blockings(C, rng):
    whole = [np.arange(C)]
    ones = [np.array([c]) for c in range(C)][::-1]
    cut = sorted(set(rng.integers(0, C + 1, 3).tolist()) | {0, C})
    return [whole, ones, [np.arange(a, b) for a, b in zip(cut[:-1], cut[1:])]]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_keep", [0, 1, 2, 3, 101])
def test_model_equals_numpy_percentile(dtype, n_keep):
    rng = np.random.default_rng(100 + n_keep)
    C = n_keep + 37
    values = rng.gamma(0.7, 2.0, C).astype(dtype) * rng.choice([-1, 1], C).astype(dtype)
    values[rng.random(C) < 0.4] = 0
    keep = np.zeros(C, bool)
    keep[rng.permutation(C)[:n_keep]] = True
    for blocks in _blockings(C, rng):
        got, n = model_select(values, keep, QS, blocks)
        assert n == n_keep
        if n_keep == 0:
            assert np.isnan(got).all()
            continue
        want = np.percentile(values[keep].astype(np.float64), QS)
        assert np.array_equal(got, want), (n_keep, got, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_with_ties_and_signed_zeros(dtype):
    values = np.array([0.0, -0.0, 1.5, 1.5, 1.5, -2.0, 0.0, 1.5, -0.0, 3.0, 3.0] * 9 + [7.0, 7.0], dtype=dtype)
    keep = np.ones(values.size, bool)
    keep[::5] = False
    got, n = model_select(values, keep, QS, [np.arange(40), np.arange(40, values.size)])
    assert n == keep.sum()
    want = np.percentile(values[keep].astype(np.float64), QS)
    assert np.array_equal(got, want)
    # -0.0 sorts below +0.0: the minimum over {+0.0, -0.0} is the negative zero
    z, _ = model_select(np.array([0.0, -0.0, 0.0], dtype=dtype), np.ones(3, bool), [0, 100], [np.arange(3)])
    assert np.signbit(z[0]) and not np.signbit(z[1])


@settings(max_examples=60, deadline=None)
@given(st.lists(st.floats(min_value=-1e6, max_value=1e6, allow_nan=False, width=32), min_size=1, max_size=60),
       st.lists(st.booleans(), min_size=60, max_size=60), st.sampled_from(QS + [100.0 / 3, 12.5]))
def test_model_hypothesis(vals, keep, q):
    values = np.array(vals, dtype=np.float32)
    keep = np.array(keep[: values.size], bool)
    got, n = model_select(values, keep, [q], [np.arange(values.size)])
    assert n == keep.sum()
    if n == 0:
        assert np.isnan(got[0])
    else:
        assert got[0] == np.percentile(values[keep].astype(np.float64), q)


@pytest.fixture(scope="module")
def lib():
    import velocyto_amd
    velocyto_amd.build()
    from velocyto_amd import _lib
    return _lib


def test_library_exports_the_masked_entries(lib):
    L = lib.lib()
    for name in SYMBOLS:
        assert name in lib.SIGNATURES and hasattr(L, name), name
    # per gene: 2 nq x (prefix 8 + rank 4) + nq x 8 (fraction) + 8 (population)
    assert L.vcy_gene_mselect_state_bytes(30_000, 2) == 30_000 * (4 * 12 + 2 * 8 + 8)
    assert L.vcy_abi_version() == 4


def test_masked_entries_validate_before_they_touch_a_device(lib):
    L = lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    qs = (ctypes.c_double * 9)(50, 50, 50, 50, 50, 50, 50, 50, 50)
    rc = L.vcy_gene_mselect_begin(p, p, qs, 9, 1, 0, None)
    assert rc == -1 and b"nq outside" in L.vcy_last_error()
    rc = L.vcy_gene_mselect_begin(p, p, (ctypes.c_double * 1)(100.5), 1, 1, 0, None)
    assert rc == -1 and b"percentile outside" in L.vcy_last_error()
    rc = L.vcy_gene_mselect_begin(None, p, qs, 1, 1, 0, None)
    assert rc == -1 and b"null pointer" in L.vcy_last_error()
    rc = L.vcy_gene_mselect_count_block(p, None, None, 1, None, p, p, 0, 1, 4, 1, 1, 0, None)
    assert rc == -1 and b"bad mask arguments" in L.vcy_last_error()
    rc = L.vcy_gene_mselect_count_block(p, None, None, 3, None, p, p, 0, 1, 4, 1, 1, 0, None)
    assert rc == -1 and b"bad mask arguments" in L.vcy_last_error()
    rc = L.vcy_gene_mselect_count_block(p, None, None, 0, None, p, p, 4, 1, 4, 1, 1, 0, None)
    assert rc == -1 and b"pass outside" in L.vcy_last_error()
    rc = L.vcy_gene_mselect_count_block(p, None, None, 0, None, p, p, 0, 1, 4, 1, 1, 7, None)
    assert rc == -1 and b"bad dtype" in L.vcy_last_error()
    rc = L.vcy_gene_mselect_advance(p, p, 8, 1, 1, 1, None)
    assert rc == -1 and b"pass outside" in L.vcy_last_error()
    rc = L.vcy_gene_mselect_finish(p, 1, None, None, 1, 0, None)
    assert rc == -1 and b"null pointer" in L.vcy_last_error()
    rc = L.vcy_fit_weighted_moments_masked(p, p, 2, None, None, None, None, None, None, None, None, p, p, 4, 1, 1, 0, None)
    assert rc == -1 and b"null pointer" in L.vcy_last_error()


def test_memory_plan_counts_the_masked_selects():
    from velocyto_amd import atlas
    args = (1_000_000, 30_000, 2400, 8, 0)
    G = 30_000
    base = atlas.memory_plan(*args, fit="maxmin_diag")
    msel = lambda nq: G * (2 * nq * (256 * 4 + 8 + 4) + nq * 8 + 8) / 1e9
    assert atlas.memory_plan(*args, fit="maxmin_diag", fit_offset=True, fixperc_q=False, limit_gamma=False) == base
    assert atlas.memory_plan(*args, fit="maxmin_diag", fit_offset=False) == base
    assert atlas.memory_plan(*args, fit="maxmin_diag", fixperc_q=True) == base                       # ignored with fit_offset=True
    lim = atlas.memory_plan(*args, fit="maxmin_diag", limit_gamma=True)
    assert lim["fit_select_histograms_GB"] == pytest.approx(base["fit_select_histograms_GB"] + msel(2) + msel(1))
    fix = atlas.memory_plan(*args, fit="maxmin_diag", fit_offset=False, fixperc_q=True, limit_gamma=True)
    assert fix["fit_select_histograms_GB"] == pytest.approx(base["fit_select_histograms_GB"] + msel(1))
    assert atlas.memory_plan(*args, limit_gamma=True) == atlas.memory_plan(*args)                    # fit="slope" has no select
