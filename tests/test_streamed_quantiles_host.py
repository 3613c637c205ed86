"""CPU-side checks of the streamed per-gene select: the built library exports its entries and validates their arguments before
touching a device, the wrapper's target-rank rule is numpy.percentile's, and atlas.memory_plan accounts for the select's state."""
import ctypes

import numpy as np
import pytest

SYMBOLS = ("vcy_gene_select_digit_bits", "vcy_gene_select_passes", "vcy_gene_select_state_bytes", "vcy_gene_select_hist_bytes",
           "vcy_gene_select_begin", "vcy_gene_select_count_block", "vcy_gene_select_advance", "vcy_gene_select_finish")


@pytest.fixture(scope="module")
def lib():
    import velocyto_amd
    velocyto_amd.build()
    from velocyto_amd import _lib
    return _lib


def test_library_exports_the_select_entries(lib):
    L = lib.lib()
    for name in SYMBOLS:
        assert name in lib.SIGNATURES and hasattr(L, name), name
    assert L.vcy_gene_select_digit_bits() == 8
    assert L.vcy_gene_select_passes(0) == 4 and L.vcy_gene_select_passes(1) == 8 and L.vcy_gene_select_passes(2) == 0
    assert L.vcy_gene_select_hist_bytes(30_000, 4) == 4 * 30_000 * 256 * 4
    assert L.vcy_gene_select_state_bytes(30_000, 4) == 4 * 30_000 * 12


def test_select_entries_validate_before_they_touch_a_device(lib):
    L = lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ranks = (ctypes.c_int64 * 2)(0, 5)
    rc = L.vcy_gene_select_begin(p, p, ranks, 2, 2 ** 31, 1, 0, None)                 # counts are 32-bit: n_total <= 2^31 - 1
    assert rc == -1 and b"32-bit counts" in L.vcy_last_error()
    rc = L.vcy_gene_select_begin(p, p, ranks, 2, 5, 1, 0, None)
    assert rc == -1 and b"rank outside" in L.vcy_last_error()
    rc = L.vcy_gene_select_begin(p, p, ranks, 17, 10, 1, 0, None)
    assert rc == -1 and b"ntargets" in L.vcy_last_error()
    rc = L.vcy_gene_select_begin(None, p, ranks, 2, 10, 1, 0, None)
    assert rc == -1 and b"null pointer" in L.vcy_last_error()
    rc = L.vcy_gene_select_count_block(p, p, None, None, p, p, 0, 2, 4, 1, 1, 0, None)
    assert rc == -1 and b"go together" in L.vcy_last_error()
    rc = L.vcy_gene_select_count_block(p, None, None, None, p, p, 0, 2, 4, 1, 1, 7, None)
    assert rc == -1 and b"bad dtype" in L.vcy_last_error()
    rc = L.vcy_gene_select_advance(p, p, 8, 2, 1, 1, None)
    assert rc == -1 and b"pass outside" in L.vcy_last_error()
    lo, hi, t = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(2), (ctypes.c_double * 1)(0.5)
    rc = L.vcy_gene_select_finish(p, lo, hi, t, 1, 2, p, 1, 0, None)
    assert rc == -1 and b"out of range" in L.vcy_last_error()


def _numpy_lerp(a, b, t):
    """numpy's _lerp (function_base.py) in float64."""
    d = b - a
    r = a + d * t
    if t >= 0.5:
        r = b - d * (1 - t)
    return a if t == 0 else r


@pytest.mark.parametrize("n", [1, 2, 3, 1000, 1_000_000])
def test_target_ranks_follow_numpy_percentile(n):
    """On v = 0, 1, ..., n - 1 the order statistic of rank r is r itself, so numpy.percentile(v, q) must equal numpy's lerp between the
    wrapper's two ranks at the wrapper's fraction - for the percentiles the fit uses and for ones whose virtual index is an integer."""
    from velocyto_amd import ops
    v = np.arange(n, dtype=np.float64)
    qs = [0, 2, 50, 98, 99.9, 100, 25, 100.0 / 3, 12.5, 99.99999]
    ranks, lo_t, hi_t, ts = ops.percentile_targets(qs, n)
    assert ranks == sorted(set(ranks)) and 0 <= ranks[0] and ranks[-1] <= n - 1 and len(lo_t) == len(hi_t) == len(ts) == len(qs)
    want = np.percentile(v, qs)
    for q, il, ih, t, w in zip(qs, lo_t, hi_t, ts, want):
        lo, hi = ranks[il], ranks[ih]
        assert 0.0 <= t < 1.0 and lo == int(np.floor((n - 1) * (q / 100.0))) and (hi == min(lo + 1, n - 1) or (t == 0 and hi == lo))
        assert _numpy_lerp(float(lo), float(hi), t) == w, (n, q, lo, hi, t, w)
    # one percentile, the maximum: a single rank
    assert ops.percentile_targets([100], n)[0] == [n - 1]
    assert len(ops.percentile_targets([99.9, 100], n)[0]) <= 3 and len(ops.percentile_targets([2, 98], n)[0]) <= 4
    for bad in ([-1e-9], [100.0001], [float("nan")], []):
        with pytest.raises(ValueError):
            ops.percentile_targets(bad, n)
    with pytest.raises(ValueError):
        ops.percentile_targets([50], 0)


def test_memory_plan_reports_the_histogram_term():
    from velocyto_amd import atlas
    args = (1_000_000, 30_000, 2400, 8, 0)
    slope = atlas.memory_plan(*args)
    fit = atlas.memory_plan(*args, fit="maxmin_diag")
    assert slope["fit_select_histograms_GB"] == 0
    want = 2 * 3 * 30_000 * (256 * 4 + 8 + 4) / 1e9                # S and U x three ranks x (histogram + prefix + rank) per gene: 0.19 GB
    assert fit["fit_select_histograms_GB"] == pytest.approx(want) and 0.18 < want < 0.19
    assert fit["total_GB"] == pytest.approx(slope["total_GB"] + want)
    # O(genes): the term does not grow with the cell count or shrink with the ranks
    assert atlas.memory_plan(10_000, 30_000, 2400, 1, 0, fit="maxmin_diag")["fit_select_histograms_GB"] == pytest.approx(want)
