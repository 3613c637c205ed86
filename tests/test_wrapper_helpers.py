"""CPU checks of the Python layer between the callers and the C ABI: the launch helper of the partial stage-D entry points (with a
stand-in for the library call), the argument helper of the pooling entry points, and the argument resolution / sampling plan that
VelocytoLoom.estimate_transition_prob and ShardedLoom.estimate_transition_prob share.  No GPU, no library call."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd  # noqa: F401
    from velocyto_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def analysis():
    import velocyto_amd  # noqa: F401
    from velocyto_amd import analysis as _analysis
    return _analysis


C_OUT, CELL0, N_ROWS = 5, 3, 40
ORDERS = {"none": None, "perm": [4, 0, 3, 1, 2], "subset": [3, 1], "empty": []}


def _lists(nr, is_sorted):
    ixs = np.random.default_rng(nr).integers(0, N_ROWS, (C_OUT, nr))       # 257 and 700 draws out of 40 rows: duplicates in every row
    return np.sort(ixs, axis=1) if is_sorted else ixs


@pytest.mark.parametrize("n_out", [1, 2])
@pytest.mark.parametrize("order_name", list(ORDERS))
@pytest.mark.parametrize("nr,is_sorted,presorted", [(nr, s, p) for nr, s, p in itertools.product((1, 256, 257, 700), (False, True), (None, True, False))
                                                    if s or p is not True])
def test_partial_launch_with_a_stand_in_launch(ops, nr, is_sorted, presorted, order_name, n_out):
    """ops._partial_launch around a launch that writes out[c, n] = 1000 (cell0 + c) + ix[c, n] (and minus that into the second output)
    for the scheduled rows only: whatever the width, the sortedness, `presorted` and the schedule, the caller finds every scheduled
    value in ITS column order and every other row untouched."""
    ixs = _lists(nr, is_sorted)
    order = None if ORDERS[order_name] is None else torch.tensor(ORDERS[order_name], dtype=torch.int64)
    rows = list(range(C_OUT)) if order is None else ORDERS[order_name]
    seen = []

    def launch(ix, outs, order_dev, n_sched):
        seen.append(ix.clone())
        assert ix.dtype == torch.int32 and ix.is_contiguous() and ix.shape == (C_OUT, nr) and len(outs) == n_out
        assert (order_dev is None) == (order is None) and n_sched == len(rows)
        if order_dev is not None:
            assert order_dev.dtype == torch.int32 and order_dev.tolist() == rows
        for c in rows:
            v = 1000.0 * (CELL0 + c) + ix[c].double()
            outs[0][c] = v
            if n_out == 2:
                outs[1][c] = -v
        return 0

    e = SimpleNamespace(t=torch.zeros(1, dtype=torch.float64), C=N_ROWS, dtype=torch.float64)
    given = (torch.full((C_OUT, nr), 5.0, dtype=torch.float64), torch.full((C_OUT, nr), 9.0, dtype=torch.float64))[:n_out]
    got = ops._partial_launch("stand-in", launch, e, 8, 2, ixs, ops.LINEAR, CELL0, order, given, True, presorted)
    assert len(got) == n_out and all(g is o for g, o in zip(got, given))
    want = 1000.0 * (CELL0 + np.arange(C_OUT))[:, None] + ixs
    for o, sign, sentinel in zip(given, (1.0, -1.0), (5.0, 9.0)):
        o = o.numpy()
        named = np.zeros(C_OUT, bool)
        named[rows] = True
        assert np.array_equal(o[named], sign * want[named])
        assert np.array_equal(o[~named].view(np.int64), np.full((int((~named).sum()), nr), sentinel).view(np.int64))
    if not rows:
        assert not seen                                  # an empty schedule launches nothing
        return
    assert len(seen) == 1
    # lists wider than a tile reach the launch sorted by index (as they came, if they were); narrow ones as they are
    assert np.array_equal(seen[0].numpy(), np.sort(ixs, axis=1) if nr > ops.TILE_COLS else ixs)


def test_partial_launch_allocates_and_validates(ops):
    e = SimpleNamespace(t=torch.zeros(1, dtype=torch.float32), C=N_ROWS, dtype=torch.float32)
    calls = []
    launch = lambda ix, outs, order, n_sched: calls.append(n_sched) or 0
    a, b = ops._partial_launch("stand-in", launch, e, 8, 2, _lists(7, False), ops.LINEAR, CELL0, None, (None, None), True, None)
    assert a.shape == b.shape == (C_OUT, 7) and a.dtype == b.dtype == torch.float32 and a is not b and calls == [C_OUT]
    for bad in (-1, N_ROWS):
        ixs = _lists(7, False)
        ixs[2, 3] = bad
        with pytest.raises(ValueError, match="neighbour index out of range"):
            ops._partial_launch("stand-in", launch, e, 8, 2, ixs, ops.LINEAR, CELL0, None, (None,), True, None)
        ops._partial_launch("stand-in", launch, e, 8, 2, ixs, ops.LINEAR, CELL0, None, (None,), False, None)
    with pytest.raises(AssertionError):                  # cell0 + C_out beyond the rows of d
        ops._partial_launch("stand-in", launch, e, 4, 2, _lists(7, False), ops.LINEAR, CELL0, None, (None,), True, None)
    with pytest.raises(AssertionError):                  # a schedule longer than the block
        ops._partial_launch("stand-in", launch, e, 8, 2, _lists(7, False), ops.LINEAR, CELL0, torch.arange(C_OUT + 1), (None,), True, None)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_pool_args(ops, as_tensor):
    """ops._pool_args: numpy arrays or tensors of any integer / float type in, contiguous (int64, int32, working dtype, int32) out."""
    cpu, n_rows, C_out = torch.device("cpu"), 9, 3
    indptr, indices = np.array([0, 2, 2, 5], dtype=np.int32), np.array([8, 0, 3, 3, 1], dtype=np.int64)
    w, w2 = np.linspace(0.0, 1.0, 10)[::2], np.arange(5, dtype=np.float32)              # (a strided view: not contiguous)
    order = torch.tensor([2, 0, 1], dtype=torch.int64)
    conv = (lambda a: torch.from_numpy(np.ascontiguousarray(a))) if as_tensor else (lambda a: a)
    for dt in (torch.float32, torch.float64):
        ip, ix, ws, od = ops._pool_args(cpu, dt, n_rows, C_out, conv(indptr), conv(indices), (conv(w), conv(w2)), order, True)
        assert ip.dtype == torch.int64 and ix.dtype == torch.int32 and od.dtype == torch.int32 and [x.dtype for x in ws] == [dt, dt]
        assert all(t.is_contiguous() for t in (ip, ix, od, *ws))
        assert ip.tolist() == indptr.tolist() and ix.tolist() == indices.tolist() and od.tolist() == [2, 0, 1]
        assert np.array_equal(ws[0].numpy(), w.astype(ws[0].numpy().dtype)) and np.array_equal(ws[1].numpy(), w2.astype(ws[1].numpy().dtype))
    assert ops._pool_args(cpu, torch.float32, n_rows, C_out, conv(indptr), conv(indices), (conv(w),), None, True)[3] is None
    with pytest.raises(AssertionError):                  # indptr of the wrong length
        ops._pool_args(cpu, torch.float32, n_rows, C_out, conv(indptr[:-1]), conv(indices), (conv(w),), None, True)
    with pytest.raises(AssertionError):                  # a weight vector of another length than the indices
        ops._pool_args(cpu, torch.float32, n_rows, C_out, conv(indptr), conv(indices), (conv(w), conv(w2[:-1])), None, True)
    with pytest.raises(AssertionError):                  # order of the wrong length
        ops._pool_args(cpu, torch.float32, n_rows, C_out, conv(indptr), conv(indices), (conv(w),), order[:2], True)
    for bad in (-1, n_rows):
        ixb = indices.copy()
        ixb[1] = bad
        with pytest.raises(ValueError, match="neighbour index out of range"):
            ops._pool_args(cpu, torch.float32, n_rows, C_out, conv(indptr), conv(ixb), (conv(w),), None, True)
        assert ops._pool_args(cpu, torch.float32, n_rows, C_out, conv(indptr), conv(ixb), (conv(w),), None, False)[1].tolist() == ixb.tolist()
    # indptr: starts at 0, never decreases, ends at len(indices) - a row outside that reads (and, in the CSR kernel, writes) out of bounds
    for bad in ([1, 2, 2, 5], [0, 3, 2, 5], [0, 2, 2, 4], [0, 2, 2, 6], [0, 6, 6, 5]):
        with pytest.raises(ValueError, match="indptr must start at 0"):
            ops._pool_args(cpu, torch.float32, n_rows, C_out, conv(np.array(bad, dtype=np.int64)), conv(indices), (conv(w),), None, True)
        assert ops._pool_args(cpu, torch.float32, n_rows, C_out, conv(np.array(bad, dtype=np.int64)), conv(indices), (conv(w),), None, False)[0].tolist() == bad
    # order: a permutation of range(C_out) - a repeated cell leaves another unwritten, a cell out of range is written out of bounds
    for bad in ([0, 1, 1], [0, 1, 3], [-1, 0, 1], [2, 2, 2]):
        ob = torch.tensor(bad, dtype=torch.int64)
        with pytest.raises(ValueError, match="order must be a permutation"):
            ops._pool_args(cpu, torch.float32, n_rows, C_out, conv(indptr), conv(indices), (conv(w),), ob, True)
        assert ops._pool_args(cpu, torch.float32, n_rows, C_out, conv(indptr), conv(indices), (conv(w),), ob, False)[3].tolist() == bad
    assert ops._pool_args(cpu, torch.float32, n_rows, C_out, conv(indptr), conv(indices), (conv(w),), np.array([1, 2, 0]), True)[3].tolist() == [1, 2, 0]
    empty = ops._pool_args(cpu, torch.float32, n_rows, 2, conv(np.zeros(3, dtype=np.int64)), conv(indices[:0]), (conv(w[:0]),), None, True)
    assert empty[0].tolist() == [0, 0, 0] and empty[1].numel() == 0


def test_check_pool_out(ops):
    """ops._check_pool_out, what knn_pool / knn_pool2 / knn_pool_counts ask of an `out=` buffer BEFORE they launch: rows for every
    output cell, the gene count and dtype of the result and - for the kernels that take one leading dimension for input and
    output - that leading dimension.  (A stand-in with the four attributes: CellMatrix itself only holds device tensors.)"""
    from types import SimpleNamespace as NS
    ok = NS(C=5, G=70, dtype=torch.float32, ld=128)
    ops._check_pool_out(ok, 5, 70, torch.float32, 128)
    ops._check_pool_out(ok, 3, 70, torch.float32)                       # more rows than C_out are fine, ld unconstrained
    for args in ((6, 70, torch.float32, 128), (5, 71, torch.float32, 128), (5, 70, torch.float64, 128), (5, 70, torch.float32, 64)):
        with pytest.raises(AssertionError, match="out= buffer"):
            ops._check_pool_out(ok, *args)


def test_scale_vec(ops):
    cpu = torch.device("cpu")
    assert ops._scale_vec(None, 4, cpu).tolist() == [1.0] * 4 and ops._scale_vec(None, 4, cpu).dtype == torch.float64
    for v in ([1, 2, 3], np.array([1, 2, 3], dtype=np.float32), torch.tensor([1, 2, 3], dtype=torch.int32)):
        t = ops._scale_vec(v, 3, cpu)
        assert t.dtype == torch.float64 and t.is_contiguous() and t.tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(AssertionError):
        ops._scale_vec([1.0, 2.0], 3, cpu)


# (C, transform, hidim, ndims, n_sight, n_neighbors, psc) -> (n_neighbors, psc, delta_transform mode, kernel transform name), written
# out by hand from the reference's estimate_transition_prob (analysis.py:1511-1526); modes and transforms: ops.delta_transform's table
STAGE_D_CALLS = [
    ((1003, "sqrt", "Sx_sz", None, None, None, None), (200, 1e-10, 1, "SQRT")),           # int(1003 / 5)
    ((4, "linear", "Sx_sz", None, None, None, None), (0, 0, 0, "LINEAR")),
    ((500, "log", "Sx_sz", None, 30, None, None), (30, 1.0, 2, "LOG10")),                 # n_sight alone
    ((500, "logratio", "Sx", None, None, 40, None), (40, 1.0, 3, "LINEAR")),              # n_neighbors alone
    ((500, "sqrt", "Sx_sz", None, 25, 25, 0.5), (25, 0.5, 1, "SQRT")),                    # both, equal; psc given
    ((500, "linear", "Sx_sz", None, None, 7, 0.0), (7, 0.0, 0, "LINEAR")),
]
STAGE_D_REFUSALS = [
    ((500, "sqrt", "Sx_sz", None, 25, 26, None), ValueError, "different names for the same parameter"),
    ((500, "cube", "Sx_sz", None, None, None, None), NotImplementedError, "transform=cube is not a valid parameter"),
    ((500, "sqrt", "pcs", None, None, None, None), NotImplementedError, "hidim='pcs'"),
    ((500, "sqrt", "Sx_sz", 3, None, None, None), ValueError, "ndims was set to 3 but hidim != 'pcs'"),
    # several things wrong: the first in the facade's order wins (n_sight / n_neighbors, transform, hidim, ndims)
    ((500, "cube", "pcs", 3, 25, 26, None), ValueError, "different names for the same parameter"),
    ((500, "cube", "pcs", 3, None, None, None), NotImplementedError, "transform=cube"),
    ((500, "sqrt", "pcs", 3, None, None, None), NotImplementedError, "hidim='pcs'"),
]


@pytest.mark.parametrize("args,want", STAGE_D_CALLS)
def test_stage_d_args(ops, analysis, args, want):
    n_neighbors, psc, mode, kern = analysis.stage_d_args(*args)
    assert (n_neighbors, psc, mode, kern) == (want[0], want[1], want[2], getattr(ops, want[3]))
    assert type(n_neighbors) is int


@pytest.mark.parametrize("args,exc,text", STAGE_D_REFUSALS)
def test_stage_d_args_refusals(analysis, args, exc, text):
    with pytest.raises(exc, match=text):
        analysis.stage_d_args(*args)


def test_sampling_plan(analysis):
    p, size = analysis.sampling_plan((0.5, 0.1), 11, 0.3, 10)
    ref = np.linspace(0.5, 0.1, 11)
    assert np.array_equal(p, ref / ref.sum()) and size == 3 and type(size) is int
    assert analysis.sampling_plan((0.5, 0.1), 201, 0.3, 200)[1] == 60                     # int(0.3 * 201) = int(60.3)
