"""The streamed exact per-gene select (csrc/fit.hip k_select_*, vcy_gene_select_*, ops.StreamedGeneQuantiles) through `ops`.

Reference: ops.gene_quantiles on the concatenated matrix.  Both are exact selections followed by the same interpolation, so the
bar is bit-identical float64 output, no tolerance.  numpy.percentile on the stored values is compared under the tolerance of
test_gpu_ops.py::test_gene_quantiles (rtol 1e-14, atol 0), where numpy's own result is finite (its lerp turns inf - inf into
NaN; the kernels return the order statistic itself at t == 0); for Z = M/a + M2/b the bar is stated for the terms of the sum."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NP_T = {"float32": np.float32, "float64": np.float64}
N_PATTERNS = 12


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def _patterns(rng, C, G, np_t):
    """(C, G) of np_t; gene g holds pattern g % N_PATTERNS."""
    A = np.zeros((C, G), dtype=np_t)
    eps, tiny = np.finfo(np_t).eps, np.finfo(np_t).tiny
    for g in range(G):
        k = g % N_PATTERNS
        if k == 0:
            col = np.zeros(C)                                                      # all zeros
        elif k == 1:
            col = np.full(C, 3.5)                                                  # constant, non-zero
        elif k == 2:
            col = np.zeros(C); col[rng.integers(C)] = 7.25                         # a single non-zero among zeros
        elif k == 3:
            col = np.where(rng.random(C) < 0.99, 0.0, rng.gamma(1.0, 2.0, C))      # 99 % zeros: down = up = 0
        elif k == 4:
            col = rng.permutation(C) + 0.5                                         # all distinct
        elif k == 5:
            col = rng.integers(0, 3, C).astype(np.float64)                         # heavy ties at every selected rank
        elif k == 6:
            col = np.asarray(1.0 + rng.integers(0, 2, C) * eps, dtype=np_t)        # differ in the lowest mantissa bit only
        elif k == 7:
            col = rng.choice(np.array([-2.0, -0.0, 0.0, 1.0]), C)                  # negatives, -0.0 beside +0.0
        elif k == 8:
            col = np.asarray(rng.integers(0, 5, C) * (tiny / 4), dtype=np_t)       # denormals (and zeros)
        elif k == 9:
            col = rng.gamma(1.0, 2.0, C); col[rng.integers(C)] = np.inf            # one +inf
        elif k == 10:
            col = rng.gamma(1.0, 2.0, C) * (rng.random(C) < 0.5)                   # expression-like: ties at 0, then distinct
        else:
            col = rng.normal(size=C) * 1e3                                         # both signs, distinct
        A[:, g] = np.asarray(col, dtype=np_t)
    return A


def _splits(C):
    """Block boundaries: a single block; equal sizes; unequal sizes including a block of one cell."""
    out = [[0, C]]
    if C >= 2:
        n = min(4, C)
        out.append(sorted(set(int(round(i * C / n)) for i in range(n + 1))))
    if C >= 3:
        out.append(sorted({0, 1, 1 + (C - 1) // 3, C}))
    return out


def _qsets(C):
    sets = [[0], [100], [2, 98], [99.9, 100], [50]]
    sets.append([100.0 * (C // 2) / (C - 1)] if C > 1 else [25])                   # h = (C - 1) q / 100 is an integer (up to rounding of q)
    sets.append([0, 25, 50, 75, 100] if (C - 1) % 4 == 0 else [0, 100])            # ... exactly an integer at C = 1, 257, 1025
    sets.append([100.0 * (C - 1.5) / (C - 1)] if C > 2 else [60])                  # lo + 1 = n - 1
    return sets


def _bits(t):
    return t.contiguous().view(torch.int64)


def _streamed(ops, M, qs, bounds, M2=None, sa=None, sb=None, order=None):
    sel = ops.StreamedGeneQuantiles(M.G, qs, M.C, M.dtype, two=M2 is not None)
    blocks = list(zip(bounds[:-1], bounds[1:]))
    if order is not None:
        blocks = [blocks[i] for i in order]
    n = 0
    while not sel.done:
        for (a, b) in blocks:
            sel.add_block(M.rows(a, b), None if M2 is None else M2.rows(a, b), sa, sb)
        sel.advance()
        n += 1
    assert n == sel.passes == (4 if M.dtype == torch.float32 else 8)
    return sel.result()


@pytest.mark.parametrize("C", [1, 2, 3, 255, 256, 257, 1025])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 257, 700])
def test_streamed_quantiles_equal_gene_quantiles_bit_for_bit(ops, G, C):
    rng = np.random.default_rng(1000 * G + C)
    for dtype in ("float32", "float64"):
        np_t = NP_T[dtype]
        A = _patterns(rng, C, G, np_t)
        B = np.asarray(rng.gamma(1.0, 1.0, (C, G)) * (rng.random((C, G)) < 0.7), dtype=np_t)
        sa, sb = rng.random(G) + 0.5, rng.random(G) + 0.5
        M, M2 = ops.CellMatrix.from_cells_major(A, dtype), ops.CellMatrix.from_cells_major(B, dtype)
        assert M.ld % 64 == 0 and (M.ld > G or G % 64 == 0)                        # ld padded wherever G is no multiple of 64
        assert np.array_equal(M.to_cells_major(np_t).view(np.uint8), A.view(np.uint8))     # the device holds the patterns' bits
        tsa, tsb = torch.from_numpy(sa).cuda(), torch.from_numpy(sb).cuda()
        with np.errstate(invalid="ignore", over="ignore"):
            Za, Zb = A / sa.astype(np_t)[None, :], B / sb.astype(np_t)[None, :]
            Z = Za + Zb
            scale = np.max(np.where(np.isfinite(Za), np.abs(Za), 0).astype(np.float64) + np.abs(Zb).astype(np.float64), axis=0)
        splits = _splits(C)
        for iq, qs in enumerate(_qsets(C)):
            for two in (False, True):
                kw = dict(M2=M2, scale_a=tsa, scale_b=tsb) if two else {}
                ref = ops.gene_quantiles(M, qs, **kw)
                for bounds in (splits if iq < 5 else splits[-1:]):
                    got = _streamed(ops, M, qs, bounds, *((M2, tsa, tsb) if two else ()))
                    assert got.shape == (len(qs), G) and got.dtype == torch.float64
                    bad = (_bits(got) != _bits(ref)).nonzero()
                    assert bad.numel() == 0, (dtype, qs, two, bounds, bad[:5].tolist(), got[tuple(bad[0])].item(), ref[tuple(bad[0])].item())
                with np.errstate(invalid="ignore"):
                    want = np.percentile((Z if two else A).astype(np.float64), qs, axis=0)
                ok = np.isfinite(want)
                # Z = M/a + M2/b: each quotient is good to the last bit of ITSELF, so where the two cancel (negative M) the sum carries
                # an absolute error of that size; 1e-14 of the largest term of the gene is the same bar stated for the operands
                atol = np.broadcast_to(1e-14 * scale[None, :] if two else 0.0, want.shape)
                err = np.abs(ref.cpu().numpy() - want)
                assert np.all(err[ok] <= 1e-14 * np.abs(want[ok]) + atol[ok]), (dtype, qs, two, float(np.nanmax(np.where(ok, err, 0))))


def test_thresholds_of_a_mostly_zero_gene_are_zero(ops):
    """99 % zeros: percentiles 2 and 98 are both exactly 0, whatever the blocking."""
    rng = np.random.default_rng(5)
    C, G = 1025, 65
    A = np.where(rng.random((C, G)) < 0.99, 0.0, rng.gamma(1.0, 2.0, (C, G))).astype(np.float32)
    M = ops.CellMatrix.from_cells_major(A, "float32")
    got = _streamed(ops, M, [2, 98], [0, 1, 300, C])
    assert bool((got == 0).all()) and not bool(torch.signbit(got).any())


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_result_does_not_depend_on_blocking_order_or_run(ops, dtype):
    rng = np.random.default_rng(17)
    C, G = 1025, 257
    M = ops.CellMatrix.from_cells_major(_patterns(rng, C, G, NP_T[dtype]), dtype)
    M2 = ops.CellMatrix.from_cells_major(np.asarray(rng.gamma(1.0, 1.0, (C, G)), dtype=NP_T[dtype]), dtype)
    sa, sb = (torch.from_numpy(rng.random(G) + 0.5).cuda() for _ in range(2))
    seven = sorted(set(int(round(i * C / 7)) for i in range(8)))
    for qs, two in (([2, 98], True), ([99.9, 100], False), ([50], False)):
        extra = (M2, sa, sb) if two else ()
        base = _bits(_streamed(ops, M, qs, [0, C], *extra))
        for bounds, order in (([0, C], None), ([0, 500, C], None), (seven, None), (seven, [3, 0, 6, 1, 5, 2, 4]), ([0, 500, C], [1, 0])):
            assert torch.equal(_bits(_streamed(ops, M, qs, bounds, *extra, order=order)), base), (qs, bounds, order)
        assert torch.equal(base, _bits(ops.gene_quantiles(M, qs, **(dict(M2=M2, scale_a=sa, scale_b=sb) if two else {}))))


def test_bad_arguments_are_refused_by_name(ops):
    G, C = 65, 40
    M = ops.CellMatrix.from_cells_major(np.random.default_rng(0).random((C, G)), "float32")
    for q in (-0.5, 100.5, float("nan")):
        with pytest.raises(ValueError, match=r"outside \[0, 100\]"):
            ops.StreamedGeneQuantiles(G, [50, q], C, "float32")
    sel = ops.StreamedGeneQuantiles(G, [2, 98], C, "float32")
    with pytest.raises(RuntimeError, match="no block was added"):
        sel.advance()
    sel.add_block(M.rows(0, 10))
    with pytest.raises(ValueError, match="genes"):
        sel.add_block(ops.CellMatrix.from_cells_major(np.zeros((5, G + 1)), "float32"))
    with pytest.raises(ValueError, match="dtype"):
        sel.add_block(ops.CellMatrix.from_cells_major(np.zeros((5, G)), "float64"))
    with pytest.raises(ValueError, match="two=True"):
        sel.add_block(M.rows(10, 20), M2=M.rows(10, 20))
    with pytest.raises(ValueError, match="n_total"):             # a pass that saw too few cells is not advanced into garbage
        sel.advance()
    with pytest.raises(ValueError, match="more than n_total"):
        sel.add_block(M)
    with pytest.raises(RuntimeError, match="passes done"):
        sel.result()
    # the state is intact: finishing the pass properly still gives the right answer
    sel.add_block(M.rows(10, C))
    sel.advance()
    while not sel.done:
        sel.add_block(M)
        sel.advance()
    assert torch.equal(_bits(sel.result()), _bits(ops.gene_quantiles(M, [2, 98])))
    with pytest.raises(RuntimeError, match="every pass is done"):
        sel.add_block(M)
    # the C entry refuses what the wrapper never sends
    from velocyto_amd import _lib
    L = _lib.lib()
    rc = L.vcy_gene_select_count_block(M.t.data_ptr(), None, None, None, sel.state.data_ptr(), sel.hist.data_ptr(), 4, sel.nt, C, G, M.ld, 0, None)
    assert rc == -1 and b"pass outside" in L.vcy_last_error()
    rc = L.vcy_gene_select_count_block(M.t.data_ptr(), None, None, None, sel.state.data_ptr(), sel.hist.data_ptr(), 0, sel.nt, C, G, G - 1, 0, None)
    assert rc == -1 and b"bad shape" in L.vcy_last_error()
    torch.cuda.synchronize()
