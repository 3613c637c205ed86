"""Stage A, kNN pooling (csrc/pool.hip: vcy_knn_pool, _pool2, _pool_w2, _pool_counts; csrc/poolcsr.hip: vcy_csr_slab_ptr,
vcy_knn_pool_csr) against the long-double oracle.pool_reference, at the shapes where the kernels change path (pool_cases.py
restates the thresholds).  Every output buffer is pre-filled with NaN, holds rows the kernel must not touch and zeroed padding.

Two kinds of assertion, nothing measured in either:
  * |device - reference| <= oracle.pool_bound element by element - (n + 2) u A for float matrices, (n + 4) u A from counts,
    max(that, 2 u own) with `maximum` - exactly 0 where A == 0, and no NaN anywhere (test_pool_oracle.py shows on the CPU that
    a plain chain meets the bound and that the bound resolves a single term);
  * bit equality wherever two launches run the same fma chain per output: every slab_genes, every order, a cell block against
    the rows of the full run, uint8 against uint16 storage, knn_pool2 / knn_pool_w2 against two poolings, CSR against dense.
The worst error / bound per kernel and working type is printed (DESIGN.md quotes it); it is information, not a tolerance."""
import numpy as np
import pytest

import pool_cases as pc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TD = {"float32": torch.float32, "float64": torch.float64}
LDBL = np.longdouble


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from velocyto_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def oracle():
    import oracle as _oracle
    return _oracle


# ---------------------------------------------------------------- buffers
def cell_matrix(ops, a, pad=0.0):
    """(C, G) numpy array of the working type -> CellMatrix whose padding [G, ld) holds `pad`."""
    C, G = a.shape
    t = torch.full((C, ops.padded_ld(G)), pad, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    t[:, :G] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return ops.CellMatrix(t, G)


def count_matrix(ops, a, wide, pad=0):
    """(C, G) integer counts -> CountMatrix held as uint16 bits (wide) or uint8, padding [G, ld) filled with the byte `pad`."""
    C, G = a.shape
    if wide:
        t = torch.full((C, ops.padded_ld(G)), -1 if pad else 0, dtype=torch.int16, device="cuda")
        t[:, :G] = torch.from_numpy(a.astype(np.uint16).view(np.int16)).cuda()
    else:
        assert a.max(initial=0) <= 255
        t = torch.full((C, ops.padded_ld(G)), pad, dtype=torch.uint8, device="cuda")
        t[:, :G] = torch.from_numpy(a.astype(np.uint8)).cuda()
    return ops.CountMatrix(t, G)


def out_buffer(ops, C_out, G, dtype, extra=2):
    """NaN everywhere a result may go, `extra` rows the kernel must leave alone, padding zeroed as CellMatrix.empty leaves it."""
    t = torch.full((C_out + extra, ops.padded_ld(G)), float("nan"), dtype=TD[dtype], device="cuda")
    t[:, G:] = 0.0
    return ops.CellMatrix(t, G)


def written(out, C_out):
    """The (C_out, G) result; rows past C_out still NaN, padding still +0 in every row."""
    h = out.t.cpu().numpy()
    assert np.isnan(h[C_out:, :out.G]).all(), "rows past C_out were written"
    assert not h[:, out.G:].view(np.int32 if h.dtype == np.float32 else np.int64).any(), "padding is no longer zero"
    return np.ascontiguousarray(h[:C_out, :out.G])


def same_bits(a, b):
    v = np.int32 if a.dtype == np.float32 else np.int64
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(v), np.ascontiguousarray(b).view(v))


WORST = {}


def held(kernel, dtype, got, ref, bound, what):
    """No NaN, every element within its bound, exact where the bound is 0; records the worst error / bound."""
    assert not np.isnan(got).any(), (what, "NaN in the result")
    err = np.abs(got.astype(LDBL) - ref).astype(np.float64)
    assert np.all(err <= bound), (what, float(np.max(err / np.where(bound > 0, bound, 1.0))), int((err > bound).sum()))
    zero = bound == 0
    assert np.all(got[zero] == 0) and not np.signbit(got[zero]).any(), what
    r = float(np.max(err[~zero] / bound[~zero])) if (~zero).any() else 0.0
    WORST[(kernel, dtype)] = max(WORST.get((kernel, dtype), 0.0), r)
    return r


def report(*kernels):
    print("; ".join(f"{k} {dt}: worst error / bound {WORST[(k, dt)]:.3f}" for k in kernels for dt in pc.DTYPES if (k, dt) in WORST))


def reference(oracle, g, data, scale, dtype, counts, maximum, cell0=0):
    """(reference, bound) of one pooling: oracle.pool_reference and oracle.pool_bound with n = the row's entry count."""
    res = oracle.pool_reference(g[0], g[1], g[2], data, scale, maximum=maximum, cell0=cell0)
    return res[0], oracle.pool_bound(res[1], np.diff(g[0]), dtype, counts, own=res[2] if maximum else None)


# ---------------------------------------------------------------- float matrices
def run_pool(ops, data, g, dtype, C_out, **kw):
    out = out_buffer(ops, C_out, data.G, dtype)
    assert ops.knn_pool(data, g[0], g[1], g[2], C_out=C_out, out=out, **kw) is out
    return written(out, C_out)


@pytest.mark.parametrize("G", pc.FLOAT_G)
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_knn_pool(ops, oracle, dtype, G):
    """vcy_knn_pool on pool_cases.float_case: graph rows of 0 .. 9, 64, 65, 81, 128, 129 entries (the 4-unrolled gather loop and its
    remainder), repeated neighbours, a row naming only itself, an all-zero gene (exactly 0).
    WORKGROUP SIZE and VECTOR PATH / SCALAR GENE TAIL: every slab_genes of FLOAT_SLABS - 64 / 128 / 256 threads, slabs rounded up
    to N and clipped to G, and at G = 257, 515, 1029 a last slab that holds nothing but the G % N tail genes - must give the bits of
    the default slab (128 threads in f32), as must every `order`, a NaN-filled input padding, and a cell block of 1, 7, 8 or 9
    rows from cell 0 or BLOCK_CELL0 against the rows of the full run."""
    cs = pc.float_case(G, dtype)
    g, C = cs["graph"], cs["C"]
    data = cell_matrix(ops, cs["data"])
    for maximum in (False, True):
        full = run_pool(ops, data, g, dtype, C, maximum=maximum)
        ref, bound = reference(oracle, g, cs["data"], None, dtype, False, maximum)
        held("knn_pool", dtype, full, ref, bound, (G, maximum))
        for slab in pc.FLOAT_SLABS[1:]:
            assert same_bits(run_pool(ops, data, g, dtype, C, maximum=maximum, slab_genes=slab), full), (G, maximum, slab)
        order = torch.from_numpy(pc.order_for(C, G)).cuda()
        assert same_bits(run_pool(ops, data, g, dtype, C, maximum=maximum, order=order, slab_genes=6), full), (G, maximum, "order")
        assert same_bits(run_pool(ops, cell_matrix(ops, cs["data"], pad=float("nan")), g, dtype, C, maximum=maximum), full), (G, maximum, "padding")
        for i, C_out in enumerate(pc.BLOCK_COUT):
            for cell0 in (0, pc.BLOCK_CELL0):
                for order in (None, torch.from_numpy(pc.order_for(C_out, cell0)).cuda()):
                    got = run_pool(ops, data, pc.block(g, cell0, C_out), dtype, C_out, maximum=maximum, cell0=cell0, order=order,
                                   slab_genes=pc.FLOAT_SLABS[(i + cell0) % len(pc.FLOAT_SLABS)])
                    assert same_bits(got, full[cell0:cell0 + C_out]), (G, maximum, C_out, cell0, order is not None)
    report("knn_pool")


@pytest.mark.parametrize("G", pc.FLOAT_G)
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_knn_pool2_and_w2(ops, oracle, dtype, G):
    """ops.knn_pool2 (no other test calls it): two matrices over one graph, the second with negative entries, equal bit for bit to
    two knn_pool calls with and without `maximum`, through `out=` / `out2=` buffers and without them, for a cell block too.
    ops.knn_pool_w2: one matrix, two weight sets (the second signed), equal to two poolings; both held to the reference."""
    cs = pc.float_case(G, dtype)
    g, C = cs["graph"], cs["C"]
    g2 = (g[0], g[1], g[3], None)
    d1, d2 = cell_matrix(ops, cs["data"]), cell_matrix(ops, cs["data2"])
    for maximum in (False, True):
        one, two = run_pool(ops, d1, g, dtype, C, maximum=maximum), run_pool(ops, d2, g, dtype, C, maximum=maximum)
        ref, bound = reference(oracle, g, cs["data2"], None, dtype, False, maximum)
        held("knn_pool2", dtype, two, ref, bound, (G, maximum))
        for slab in (0, 6, 1024):
            o1, o2 = out_buffer(ops, C, G, dtype), out_buffer(ops, C, G, dtype)
            r1, r2 = ops.knn_pool2(d1, d2, g[0], g[1], g[2], maximum=maximum, slab_genes=slab, out=o1, out2=o2)
            assert r1 is o1 and r2 is o2 and same_bits(written(o1, C), one) and same_bits(written(o2, C), two), (G, maximum, slab)
        r1, r2 = ops.knn_pool2(d1, d2, g[0], g[1], g[2], maximum=maximum)
        assert (r1.C, r1.ld, r2.C, r2.ld) == (C, d1.ld, C, d1.ld) and same_bits(r1.t.cpu().numpy()[:, :G], one) and same_bits(r2.t.cpu().numpy()[:, :G], two)
        assert not r1.t[:, G:].any() and not r2.t[:, G:].any()
        blk, c0, m = pc.block(g, pc.BLOCK_CELL0, 9), pc.BLOCK_CELL0, 9
        o1, o2 = out_buffer(ops, m, G, dtype), out_buffer(ops, m, G, dtype)
        ops.knn_pool2(d1, d2, blk[0], blk[1], blk[2], maximum=maximum, cell0=c0, C_out=m, out=o1, out2=o2, order=torch.from_numpy(pc.order_for(m)).cuda())
        assert same_bits(written(o1, m), one[c0:c0 + m]) and same_bits(written(o2, m), two[c0:c0 + m]), (G, maximum, "block")
    one, two = run_pool(ops, d1, g, dtype, C), run_pool(ops, d1, g2, dtype, C)
    ref, bound = reference(oracle, g2, cs["data"], None, dtype, False, False)
    held("knn_pool_w2", dtype, two, ref, bound, (G, "w2"))
    for slab in pc.FLOAT_SLABS:
        a, b = ops.knn_pool_w2(d1, g[0], g[1], g[2], g[3], slab_genes=slab)
        assert same_bits(a.t.cpu().numpy()[:, :G], one) and same_bits(b.t.cpu().numpy()[:, :G], two), (G, slab)
        assert not a.t[:, G:].any() and not b.t[:, G:].any()
    blk = pc.block(g, pc.BLOCK_CELL0, 8)
    a, b = ops.knn_pool_w2(d1, blk[0], blk[1], blk[2], blk[3], cell0=pc.BLOCK_CELL0, C_out=8, order=torch.from_numpy(pc.order_for(8)).cuda())
    assert same_bits(a.t.cpu().numpy()[:, :G], one[pc.BLOCK_CELL0:pc.BLOCK_CELL0 + 8]) and same_bits(b.t.cpu().numpy()[:, :G], two[pc.BLOCK_CELL0:pc.BLOCK_CELL0 + 8])
    report("knn_pool2", "knn_pool_w2")


# ---------------------------------------------------------------- dense count layers
def run_counts(ops, cS, cU, sS, sU, g, dtype, C_out, **kw):
    o1 = out_buffer(ops, C_out, cS.G, dtype)
    o2 = None if cU is None else out_buffer(ops, C_out, cS.G, dtype)
    res = ops.knn_pool_counts(cS, cU, sS, sU, g[0], g[1], g[2], dtype=TD[dtype], C_out=C_out, out=o1, out2=o2, **kw)
    assert (res is o1) if cU is None else (res[0] is o1 and res[1] is o2)
    return written(o1, C_out), None if cU is None else written(o2, C_out)


@pytest.mark.parametrize("kind", ["structural", "range"])
@pytest.mark.parametrize("G", pc.COUNT_G)
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_knn_pool_counts(ops, oracle, dtype, G, kind):
    """vcy_knn_pool_counts on pool_cases.count_case: G around the 8- and 16-gene gathers (the vector that straddles G is masked and
    stored whole), counts 0, 1, 255, 256, 32767, 32768, 65535 with factors over 2^-10 .. 2^10 that no f32 holds ("range"), graph rows
    of up to 129 entries ("structural").  Both layers at once, S only, and mixed storage widths (the wrapper widens S).
    WORKGROUP SIZE: every slab_genes of COUNT_SLABS - 64 threads at the default slab for uint8, 128 for uint16, 256 from 4096 / 2048,
    slabs rounded up to 16 / 8 genes and clipped to G - gives the bits of the default.  UINT8 AGAINST UINT16 storage of the same
    counts, every `order`, 0xFF bytes in the input padding and cell blocks give the same bits as well."""
    cs = pc.count_case(G, kind)
    g, C = pc.case_graph(cs, dtype), cs["C"]
    S8, S16, U16 = count_matrix(ops, cs["S"], False), count_matrix(ops, cs["S"], True), count_matrix(ops, cs["U"], True)
    sS, sU = cs["sS"], cs["sU"]
    for maximum in (False, True):
        fS, fU = run_counts(ops, S16, U16, sS, sU, g, dtype, C, maximum=maximum)
        for layer, got, scale in (("S", fS, sS), ("U", fU, sU)):
            ref, bound = reference(oracle, g, cs[layer], scale, dtype, True, maximum)
            held("knn_pool_counts", dtype, got, ref, bound, (G, kind, layer, maximum))
        for slab in pc.COUNT_SLABS:
            assert same_bits(run_counts(ops, S8, None, sS, None, g, dtype, C, maximum=maximum, slab_genes=slab)[0], fS), (G, kind, maximum, slab, "uint8")
            assert same_bits(run_counts(ops, U16, None, sU, None, g, dtype, C, maximum=maximum, slab_genes=slab)[0], fU), (G, kind, maximum, slab, "uint16")
        mS, mU = run_counts(ops, S8, U16, sS, sU, g, dtype, C, maximum=maximum, slab_genes=24)
        assert same_bits(mS, fS) and same_bits(mU, fU), (G, kind, maximum, "mixed widths")
        order = torch.from_numpy(pc.order_for(C, G)).cuda()
        oS, oU = run_counts(ops, S16, U16, sS, sU, g, dtype, C, maximum=maximum, order=order, slab_genes=8)
        assert same_bits(oS, fS) and same_bits(oU, fU), (G, kind, maximum, "order")
        for wide in (False, True):
            dirty = count_matrix(ops, cs["S"], wide, pad=255)
            assert same_bits(run_counts(ops, dirty, None, sS, None, g, dtype, C, maximum=maximum)[0], fS), (G, kind, maximum, wide, "padding")
        for i, C_out in enumerate(pc.BLOCK_COUT):
            for cell0 in (0, pc.BLOCK_CELL0):
                order = None if (i + cell0) % 2 else torch.from_numpy(pc.order_for(C_out, cell0)).cuda()
                bS, bU = run_counts(ops, S8 if i % 2 else S16, U16, sS, sU, pc.block(g, cell0, C_out), dtype, C_out, maximum=maximum, cell0=cell0,
                                    order=order, slab_genes=pc.COUNT_SLABS[(i + cell0) % len(pc.COUNT_SLABS)])
                assert same_bits(bS, fS[cell0:cell0 + C_out]) and same_bits(bU, fU[cell0:cell0 + C_out]), (G, kind, maximum, C_out, cell0)
    report("knn_pool_counts")


# ---------------------------------------------------------------- CSR layers
def csr_counts(ops, cs):
    data = cs["data"].astype(np.uint16).view(np.int16) if cs["wide"] else cs["data"].astype(np.uint8)
    return ops.CsrCounts(torch.from_numpy(cs["indptr"]).cuda(), torch.from_numpy(cs["indices"]).cuda(), torch.from_numpy(data).cuda(), cs["G"])


def run_csr(ops, counts, scale, g, dtype, C_out, **kw):
    out = out_buffer(ops, C_out, counts.G, dtype)
    assert ops.knn_pool_csr(counts, scale, g[0], g[1], g[2], dtype=TD[dtype], C_out=C_out, out=out, **kw) is out
    return written(out, C_out)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("G", pc.CSR_G)
def test_csr_slab_ptr(ops, lib, G, wide):
    """vcy_csr_slab_ptr at the ABI against np.searchsorted for every row of every CSR case (an empty row, a full row, non-zeros
    at genes 2047 / 2048 / 4095 / 4096 / G - 1), into a buffer with a sentinel behind the table."""
    cs = pc.csr_case(G, wide)
    L = lib.lib()
    assert int(L.vcy_csr_slab_genes()) == pc.CSR_SLAB
    want = pc.slab_ptr_reference(cs["indptr"], cs["indices"], G)
    buf = torch.full((want.size + 64,), -7, dtype=torch.int32, device="cuda")
    ip, ix = torch.from_numpy(cs["indptr"]).cuda(), torch.from_numpy(cs["indices"]).cuda()
    lib.check(L.vcy_csr_slab_ptr(ip.data_ptr(), ix.data_ptr(), buf.data_ptr(), cs["C"], G, ops._stream()), "csr_slab_ptr")
    h = buf.cpu().numpy()
    assert np.array_equal(h[:want.size].reshape(want.shape), want) and np.all(h[want.size:] == -7)
    assert np.array_equal(csr_counts(ops, cs).slabptr.cpu().numpy(), want)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("G", pc.CSR_G)
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_knn_pool_csr(ops, oracle, dtype, G, wide):
    """vcy_knn_pool_csr on pool_cases.csr_case, held to the reference and bit-equal to vcy_knn_pool_counts on the densified layer.
    A SLAB SEGMENT OF MORE THAN 256 NON-ZEROS: rows with 257 and 300 non-zeros in one slab and a full row (2048 per slab) enter the
    element-wise loop behind the 64 quads; segments of 1 .. 5, 255, 256 end inside, or exactly on, a quad or the pass.
    GRAPH ROWS OF EXACTLY 64, 65, 128, 129 ENTRIES (and 81): the batch boundaries `last = pb + 64 >= p1` and the reload of the
    partial sums from `out`, with and without `maximum` (applied after the last batch only).
    UINT16 EXTRACTION (`wide`): rows in which every count exceeds 255, the full row among them - whole quads of two-byte counts.
    Also: an empty row, a one-element row at the very end of the arrays (its quad is pulled back inside them), non-zeros at genes
    0, 2047, 2048, 4095, 4096, G - 1; every `order` and cell blocks (several waves per slab range: C_out = 1 .. 9 splits every slab)."""
    cs = pc.csr_case(G, wide)
    g, C, scale = pc.case_graph(cs, dtype), cs["C"], cs["scale"]
    counts, dense = csr_counts(ops, cs), count_matrix(ops, cs["dense"], wide)
    assert np.array_equal(counts.to_dense().t.cpu().numpy(), dense.t.cpu().numpy())
    for maximum in (False, True):
        full = run_csr(ops, counts, scale, g, dtype, C, maximum=maximum)
        ref, bound = reference(oracle, g, cs["dense"], scale, dtype, True, maximum)
        held("knn_pool_csr", dtype, full, ref, bound, (G, wide, maximum))
        assert same_bits(full, run_counts(ops, dense, None, scale, None, g, dtype, C, maximum=maximum)[0]), (G, wide, maximum, "dense")
        order = torch.from_numpy(pc.order_for(C, G)).cuda()
        assert same_bits(run_csr(ops, counts, scale, g, dtype, C, maximum=maximum, order=order), full), (G, wide, maximum, "order")
        for i, C_out in enumerate(pc.BLOCK_COUT):
            for cell0 in (0, pc.BLOCK_CELL0):
                order = None if (i + cell0) % 2 else torch.from_numpy(pc.order_for(C_out, cell0)).cuda()
                got = run_csr(ops, counts, scale, pc.block(g, cell0, C_out), dtype, C_out, maximum=maximum, cell0=cell0, order=order)
                assert same_bits(got, full[cell0:cell0 + C_out]), (G, wide, maximum, C_out, cell0)
    report("knn_pool_csr")


@pytest.mark.parametrize("shape", pc.MULTI_SHAPES, ids=lambda s: f"C_out{s[0]}")
def test_knn_pool_csr_several_slabs_per_wave(ops, lib, oracle, shape):
    """A WAVE WALKING MORE THAN ONE GENE SLAB - the hand-over `lo_l = hi_l; hi_l = sp_l[s + 2]` that the production shape uses
    (one wave, 15 slabs) and that no other fast test reaches (C_out <= 20480 / nslab splits every slab off).  G = 4097 is three
    slabs; C_out = 10241 gives two waves per cell with the ranges [0, 2) and [2, 3) (a short last range), C_out = 20480 one wave
    with all three (f32 only).  vcy_knn_pool_csr_splits says so, or the test is not on the path it means to be on.  Graph rows
    of 64, 65 and 129 entries walk the slabs once per batch.  The whole output must equal the dense kernel's bit for bit (compared
    on the device); a sample of rows is held to the long-double reference."""
    C_out, splits, dtypes = shape
    cs = pc.multi_case()
    L = lib.lib()
    nslab = (cs["G"] + int(L.vcy_csr_slab_genes()) - 1) // int(L.vcy_csr_slab_genes())
    assert nslab == 3 and L.vcy_knn_pool_csr_splits(C_out, cs["G"]) == splits < nslab
    assert L.vcy_knn_pool_csr_splits(10239, cs["G"]) == nslab               # (just below: every slab has a wave of its own)
    dense = ops.CountMatrix(torch.zeros((cs["C"], ops.padded_ld(cs["G"])), dtype=torch.uint8, device="cuda"), cs["G"])
    dense.t[:, :cs["G"]] = torch.from_numpy(cs["dense"]).cuda()
    counts = ops.CsrCounts.from_dense(dense)
    assert counts.nnz == int(np.count_nonzero(cs["dense"]))
    g = pc.block(cs["graph"], 0, C_out)
    sample = cs["sample"][cs["sample"] < C_out]
    ip, ix = torch.from_numpy(g[0]).cuda(), torch.from_numpy(g[1]).cuda()
    for dtype in dtypes:
        w = torch.from_numpy(pc.stored(g[2], dtype)).cuda()
        bits = torch.int32 if dtype == "float32" else torch.int64
        for maximum in (False, True):
            a, b = out_buffer(ops, C_out, cs["G"], dtype, extra=1), out_buffer(ops, C_out, cs["G"], dtype, extra=1)
            ops.knn_pool_csr(counts, cs["scale"], ip, ix, w, dtype=TD[dtype], maximum=maximum, C_out=C_out, out=a, validate=False)
            ops.knn_pool_counts(dense, None, cs["scale"], None, ip, ix, w, dtype=TD[dtype], maximum=maximum, C_out=C_out, out=b, validate=False)
            assert torch.equal(a.t.view(bits), b.t.view(bits)), (C_out, dtype, maximum)
            assert bool(torch.isnan(a.t[C_out:, :cs["G"]]).all()) and not bool(torch.isnan(a.t[:C_out]).any()) and not bool(a.t[:, cs["G"]:].any())
            sub = pc.graph_rows((g[0], g[1], pc.stored(g[2], dtype), None), sample)
            res = oracle.pool_reference(sub[0], sub[1], sub[2], cs["dense"], cs["scale"], maximum=maximum, cell0=sample)
            bound = oracle.pool_bound(res[1], np.diff(sub[0]), dtype, True, own=res[2] if maximum else None)
            held("knn_pool_csr", dtype, a.t[torch.from_numpy(sample).cuda()][:, :cs["G"]].cpu().numpy(), res[0], bound, (C_out, dtype, maximum))
    report("knn_pool_csr")


# ---------------------------------------------------------------- the wrappers refuse before they launch
def test_wrappers_refuse_bad_buffers_and_graphs_before_any_launch(ops):
    """THE WRAPPERS.  knn_pool / knn_pool2 / knn_pool_counts / knn_pool_csr with an `out=` / `out2=` buffer of too few rows, another
    gene count, another dtype or - for the float kernels, which take ONE ld for data and output - another leading dimension raise
    AssertionError; a graph whose indptr does not start at 0, decreases or does not end at len(indices), an index out of range or an
    `order` that is no permutation raise ValueError.  Nothing is launched: the NaN-filled buffers are untouched afterwards."""
    dtype, G = "float32", 66
    cs = pc.float_case(G, dtype)
    g, C = cs["graph"], cs["C"]
    d1, d2 = cell_matrix(ops, cs["data"]), cell_matrix(ops, cs["data2"])
    cc = pc.count_case(65, "structural")
    gc = pc.case_graph(cc, dtype)
    S8, U16 = count_matrix(ops, cc["S"], False), count_matrix(ops, cc["U"], True)
    kc = pc.csr_case(700, False)
    counts = csr_counts(ops, kc)
    nan = lambda rows, cols, dt=torch.float32: torch.full((rows, cols), float("nan"), dtype=dt, device="cuda")
    good = ops.CellMatrix(nan(C, d1.ld), G)
    bad = [ops.CellMatrix(nan(C - 1, d1.ld), G), ops.CellMatrix(nan(C, d1.ld), G - 1), ops.CellMatrix(nan(C, d1.ld, torch.float64), G),
           ops.CellMatrix(nan(C, d1.ld + 64), G)]
    for b in bad:
        with pytest.raises(AssertionError, match="out= buffer"):
            ops.knn_pool(d1, g[0], g[1], g[2], out=b)
        with pytest.raises(AssertionError, match="out= buffer"):
            ops.knn_pool2(d1, d2, g[0], g[1], g[2], out=b, out2=good)
        with pytest.raises(AssertionError, match="out= buffer"):
            ops.knn_pool2(d1, d2, g[0], g[1], g[2], out=good, out2=b)
    cgood = ops.CellMatrix(nan(cc["C"], ops.padded_ld(65)), 65)
    cbad = [ops.CellMatrix(nan(cc["C"] - 1, 128), 65), ops.CellMatrix(nan(cc["C"], 128), 64), ops.CellMatrix(nan(cc["C"], 128, torch.float64), 65)]
    for b in cbad:
        with pytest.raises(AssertionError, match="out= buffer"):
            ops.knn_pool_counts(S8, None, cc["sS"], None, gc[0], gc[1], gc[2], dtype=torch.float32, out=b)
        with pytest.raises(AssertionError, match="out= buffer"):
            ops.knn_pool_counts(S8, U16, cc["sS"], cc["sU"], gc[0], gc[1], gc[2], dtype=torch.float32, out=cgood, out2=b)
    wide = ops.CellMatrix(nan(cc["C"], 192), 65)                       # the two outputs of one count launch share ld_out
    with pytest.raises(AssertionError, match="out= buffer"):
        ops.knn_pool_counts(S8, U16, cc["sS"], cc["sU"], gc[0], gc[1], gc[2], dtype=torch.float32, out=cgood, out2=wide)
    # graphs
    ptr_bad = [g[0] + 1, np.concatenate([g[0][:3], g[0][3:4] - 70, g[0][4:]]), np.concatenate([g[0][:-1], g[0][-1:] + 1]), np.concatenate([g[0][:-1], g[0][-1:] - 1])]
    ix_bad = g[1].copy()
    ix_bad[5] = C
    order_bad = torch.arange(C, dtype=torch.int32)
    order_bad[3] = 2
    gk = pc.case_graph(kc, dtype)
    kgood = ops.CellMatrix(nan(kc["C"], ops.padded_ld(700)), 700)
    for ptr, ix, order, msg in [(p, g[1], None, "indptr must start at 0") for p in ptr_bad] + [(g[0], ix_bad, None, "neighbour index out of range"),
                                                                                                 (g[0], g[1], order_bad, "order must be a permutation")]:
        with pytest.raises(ValueError, match=msg):
            ops.knn_pool(d1, ptr, ix, g[2], out=good, order=order)
        with pytest.raises(ValueError, match=msg):
            ops.knn_pool2(d1, d2, ptr, ix, g[2], out=good, out2=good, order=order)
        with pytest.raises(ValueError, match=msg):
            ops.knn_pool_w2(d1, ptr, ix, g[2], g[3], order=order)
    assert np.array_equal(gc[0], g[0]) and np.array_equal(gk[0][:10], g[0][:10])        # (one graph builder: the same row lengths)
    for ptr in ptr_bad:
        with pytest.raises(ValueError, match="indptr must start at 0"):
            ops.knn_pool_counts(S8, U16, cc["sS"], cc["sU"], ptr, gc[1], gc[2], dtype=torch.float32, out=cgood, out2=cgood)
    kptr = gk[0].copy()
    kptr[4] = kptr[3] - 1
    with pytest.raises(ValueError, match="indptr must start at 0"):
        ops.knn_pool_csr(counts, kc["scale"], kptr, gk[1], gk[2], dtype=torch.float32, out=kgood)
    torch.cuda.synchronize()
    for b in bad + cbad + [good, cgood, wide, kgood]:
        assert bool(torch.isnan(b.t).all())
