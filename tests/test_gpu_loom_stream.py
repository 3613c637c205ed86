"""The streamed .loom ingest on the device: the vcy_loom_tile_* kernels at the C ABI against numpy (np.nonzero of the transposed
tile, sum, max) - bit for bit, at the edges of their launch plan - and the routes built on them, read_layer_csr(engine="stream")
and VelocytoLoom(path, ingest="stream"), against the default routes on the same files.  Exact comparison throughout."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DTYPES = ("uint8", "uint16", "uint32", "int32", "int64", "float32", "float64")
CELLS = (1, 63, 64, 65, 129)
INT16_FILL, INT32_FILL = 0x5A5A, -7


@pytest.fixture(scope="module")
def env():
    import torch
    import velocyto_amd
    velocyto_amd.build()
    from velocyto_amd import _lib, loom_io, ops
    dev = ops.require_gpu()

    class E:
        pass
    e = E()
    e.torch, e.vcy, e.L, e.check, e.ops, e.loom_io, e.dev = torch, velocyto_amd, _lib.lib(), _lib.check, ops, loom_io, dev
    e.slab = int(e.L.vcy_loom_tile_slab_genes())
    # 64: the compaction's sub-tile, 128: the dense kernel's, slab: genes per workgroup - one value just past each
    e.genes = (1, 15, 16, 17, 64, 65, 129, e.slab + 1)
    return e


def _tile(rng, G, B, dtype, density=0.3):
    hi = 256 if dtype == "uint8" else 65536
    a = (rng.random((G, B)) < density) * rng.integers(1, hi, (G, B))
    if G * B > 8 and dtype != "uint8":
        a.flat[rng.integers(0, G * B, 3)] = (255, 256, 65535)
    return a.astype(dtype)


def _upload(env, tile, ldt):
    """the tile in a (G, ldt) device buffer whose padding columns hold a non-zero the kernels must never read"""
    G, B = tile.shape
    host = np.full((G, ldt), 77, dtype=tile.dtype)
    host[:, :B] = tile
    return env.torch.from_numpy(host).to(env.dev)


def _expect(tile):
    """(indptr, indices, data as uint16, sums, result block) of a VALID tile, by numpy"""
    T = np.ascontiguousarray(tile.T)
    rows, cols = np.nonzero(T)
    indptr = np.concatenate([[0], np.cumsum(np.count_nonzero(T, axis=1))]).astype(np.int64)
    data = T[rows, cols].astype(np.uint16)
    sums = T.astype(np.int64).sum(1)
    mx = int(T.max()) if T.size else 0
    return indptr, cols.astype(np.int32), data, sums, np.array([0, 0, 0, max(mx, 0)], dtype=np.int64)


def _count(env, d_tile, G, B, ldt, dtype):
    t = env.torch
    ws = env.ops.loom_tile_workspace(G, B, env.dev)
    nnz, sums = t.full((B,), -1, dtype=t.int64, device=env.dev), t.full((B,), -1, dtype=t.int64, device=env.dev)
    res = t.full((4,), -1, dtype=t.int64, device=env.dev)
    env.check(env.L.vcy_loom_tile_count(d_tile.data_ptr(), nnz.data_ptr(), sums.data_ptr(), res.data_ptr(), ws.data_ptr(), G, B, ldt,
                                        env.ops.LOOM_ELEM[np.dtype(dtype)], env.ops._stream()), "loom_tile_count")
    return nnz.cpu().numpy(), sums.cpu().numpy(), res.cpu().numpy(), ws


def _fill(env, d_tile, ws, nnz, G, B, ldt, dtype, front, back):
    """the block placed `front` elements into arrays that go on for `back` more; everything outside must keep its sentinel"""
    t = env.torch
    total = int(nnz.sum())
    row_start = t.from_numpy((front + np.concatenate([[0], np.cumsum(nnz)])).astype(np.int64)).to(env.dev)
    n = front + total + back
    idx = t.full((n,), INT32_FILL, dtype=t.int32, device=env.dev)
    dat = t.full((n,), INT16_FILL, dtype=t.int16, device=env.dev)
    env.check(env.L.vcy_loom_tile_fill(d_tile.data_ptr(), ws.data_ptr(), row_start.data_ptr(), idx.data_ptr(), dat.data_ptr(), n, G, B, ldt,
                                       env.ops.LOOM_ELEM[np.dtype(dtype)], env.ops._stream()), "loom_tile_fill")
    idx, dat = idx.cpu().numpy(), dat.cpu().numpy().view(np.uint16)
    assert np.all(idx[:front] == INT32_FILL) and np.all(idx[front + total:] == INT32_FILL)
    assert np.all(dat[:front] == INT16_FILL) and np.all(dat[front + total:] == INT16_FILL)
    return idx[front:front + total], dat[front:front + total]


def _dense(env, d_tile, G, B, ldt, dtype, s, C):
    t = env.torch
    ld = env.ops.padded_ld(G)
    ws = env.ops.loom_tile_workspace(ld, B, env.dev)
    out = t.full((C, ld), INT16_FILL, dtype=t.int16, device=env.dev)
    sums, res = t.full((B,), -1, dtype=t.int64, device=env.dev), t.full((4,), -1, dtype=t.int64, device=env.dev)
    env.check(env.L.vcy_loom_tile_dense(d_tile.data_ptr(), out.data_ptr(), sums.data_ptr(), res.data_ptr(), ws.data_ptr(), G, B, ldt,
                                        env.ops.LOOM_ELEM[np.dtype(dtype)], s, C, ld, env.ops._stream()), "loom_tile_dense")
    return out.cpu().numpy().view(np.uint16), sums.cpu().numpy(), res.cpu().numpy()


def _check_tile(env, tile, ldt, front=0, back=0, s=0, extra_rows=0):
    G, B = tile.shape
    dtype = tile.dtype.name
    indptr, indices, data, sums, result = _expect(tile)
    d_tile = _upload(env, tile, ldt)
    nnz, got_sums, got_res, ws = _count(env, d_tile, G, B, ldt, dtype)
    tag = (dtype, G, B, ldt)
    assert np.array_equal(nnz, np.diff(indptr)), tag
    assert np.array_equal(got_sums, sums) and np.array_equal(got_res, result), tag
    got_idx, got_dat = _fill(env, d_tile, ws, nnz, G, B, ldt, dtype, front, back)
    assert np.array_equal(got_idx, indices) and np.array_equal(got_dat, data), tag
    C = s + B + extra_rows
    out, d_sums, d_res = _dense(env, d_tile, G, B, ldt, dtype, s, C)
    assert np.array_equal(out[s:s + B, :G], tile.T.astype(np.uint16)) and not out[s:s + B, G:].any(), tag
    assert np.all(out[:s] == INT16_FILL) and np.all(out[s + B:] == INT16_FILL), tag
    assert np.array_equal(d_sums, sums) and np.array_equal(d_res, result), tag


@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_kernels_every_shape(env, dtype):
    rng = np.random.default_rng(DTYPES.index(dtype))
    for G in env.genes:
        for B in CELLS:
            tile = _tile(rng, G, B, dtype)
            _check_tile(env, tile, B)
            _check_tile(env, tile, B + 5, front=11, back=9, s=3, extra_rows=2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_kernels_degenerate_tiles(env, dtype):
    rng = np.random.default_rng(40 + DTYPES.index(dtype))
    for G, B in ((65, 65), (env.slab + 1, 129)):
        _check_tile(env, np.zeros((G, B), dtype=dtype), B + 5, front=4, back=4, s=1, extra_rows=1)           # all zero
        full = rng.integers(1, 256, (G, B)).astype(dtype)                                                      # no zero
        _check_tile(env, full, B, front=4, back=4)
        last = np.zeros((G, B), dtype=dtype)                                                                   # only the last element
        last[-1, -1] = 255
        _check_tile(env, last, B + 5, front=2, back=2, s=2, extra_rows=3)


def _flags(env, tile):
    G, B = tile.shape
    d_tile = _upload(env, tile, B + 5)
    nnz, _, res, _ = _count(env, d_tile, G, B, B + 5, tile.dtype.name)
    _, _, d_res = _dense(env, d_tile, G, B, B + 5, tile.dtype.name, 0, B)
    assert np.array_equal(res, d_res)
    assert np.array_equal(nnz, np.count_nonzero(tile.T, axis=1))           # the structure never depends on validity (NaN != 0)
    return res.tolist()


def test_result_block_flags(env):
    """255 / 256 / 65535 are counts; 65536, -1, 1.5, NaN, +inf and 2^40 each set exactly their flag; -0.0 is a zero"""
    rng = np.random.default_rng(7)
    for G, B, at in ((17, 65, (16, 64)), (env.slab + 1, 129, (env.slab, 3))):
        for dtype in DTYPES:
            base = _tile(rng, G, B, dtype, 0.1)
            base[base > 200] = 3                                            # a background of small counts
            cases = [(255, [0, 0, 0, 255])]
            if dtype != "uint8":
                cases += [(256, [0, 0, 0, 256]), (65535, [0, 0, 0, 65535])]
            if dtype not in ("uint8", "uint16"):
                cases += [(65536, [0, 0, 1, 65536])]
            if dtype in ("int32", "int64", "float32", "float64"):
                cases += [(-1, [0, 1, 0, 200])]
            if dtype == "int64":
                cases += [(2 ** 40, [0, 0, 1, 2 ** 40])]
            if dtype in ("float32", "float64"):
                cases += [(1.5, [1, 0, 0, 200]), (float("nan"), [1, 0, 0, 200]), (float("inf"), [1, 0, 0, 200])]
            for value, want in cases:
                tile = base.copy()
                tile[0, 0] = 200                                            # the maximum when the special value does not count
                tile[at] = value
                assert _flags(env, tile) == want, (dtype, G, B, value)
    for dtype in ("float32", "float64"):
        tile = np.zeros((17, 65), dtype=dtype)
        tile[3, 5], tile[16, 64], tile[4, 4] = -0.0, -0.0, 9.0
        _check_tile(env, tile, 70)                                          # np.nonzero skips -0.0 as well
        assert _flags(env, tile) == [0, 0, 0, 9]


# ------------------------------------------------------------------------------------------------------------------ routes
@pytest.fixture(scope="module")
def files(env, tmp_path_factory):
    d = tmp_path_factory.mktemp("loom_stream")
    rng = np.random.default_rng(11)
    G, C = 900, 700
    S = (rng.random((G, C)) < 0.08) * rng.integers(1, 200, (G, C))
    S[450, 350] = 3000                                                      # one count that needs uint16
    U = (rng.random((G, C)) < 0.05) * rng.integers(1, 256, (G, C))          # fits uint8
    A = (rng.random((G, C)) < 0.02) * rng.integers(1, 9, (G, C))
    out = {}
    out["counts"] = str(d / "counts.loom")
    env.loom_io.write_loom(out["counts"], {"spliced": S.astype(np.uint16), "unspliced": U.astype(np.uint16), "ambiguous": A.astype(np.uint16)},
                           chunks=(64, 64), compression=2)
    frac = S.astype(np.float32)
    frac[10, 20] = 1.5
    big = U.astype(np.int32)
    big[5, 6] = 70000
    neg = A.astype(np.int64)
    neg[7, 8] = -1
    out["bad"] = str(d / "bad.loom")
    env.loom_io.write_loom(out["bad"], {"spliced": frac, "unspliced": big, "ambiguous": neg}, chunks=(64, 64), compression=2)
    # float layers holding integers, an int64 layer, a float non-count ambiguous layer: the facade's other branches
    out["mixed"] = str(d / "mixed.loom")
    env.loom_io.write_loom(out["mixed"], {"spliced": S.astype(np.float64), "unspliced": U.astype(np.int64), "ambiguous": frac},
                           {"CellID": np.array([f"c{i}" for i in range(C)]), "Clusters": rng.integers(0, 4, C)},
                           {"Gene": np.array([f"g{i}" for i in range(G)])}, chunks=(64, 64), compression=2, shuffle=True)
    out["v2"], out["v3"] = os.path.join(GOLDEN, "loompy_v2.loom"), os.path.join(GOLDEN, "loompy_v3.loom")
    return out


def _same_csr(env, a, b):
    t = env.torch
    return (a.G == b.G and a.data.dtype == b.data.dtype and t.equal(a.indptr, b.indptr) and t.equal(a.indices, b.indices)
            and t.equal(a.data, b.data))


@pytest.fixture(scope="module")
def hyperslab(env, files):
    """engine="hyperslab" once per (file, layer, cell range): the reference of every stream run below"""
    out = {}
    for f in ("counts", "v2", "v3"):
        for layer in ("spliced", "unspliced"):
            for rng_ in ((0, None), (123, 577)) if f == "counts" else ((0, None), (3, 11)):
                out[f, layer, rng_] = env.loom_io.read_layer_csr(files[f], layer, c0=rng_[0], c1=rng_[1])
    return out


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("cell_block", [64, 100, 256, 8192])
def test_read_layer_csr_stream_equals_hyperslab(env, files, hyperslab, cell_block, threads):
    for (f, layer, (c0, c1)), ref in hyperslab.items():
        cb = cell_block if f == "counts" else max(1, cell_block // 32)      # the 17-cell fixtures: blocks of 2, 3, 8 and all cells
        got = env.loom_io.read_layer_csr(files[f], layer, cell_block=cb, c0=c0, c1=c1, engine="stream", threads=threads)
        assert _same_csr(env, got, ref), (f, layer, c0, c1, cb, threads)
    assert hyperslab["counts", "spliced", (0, None)].data.dtype == env.torch.int16
    assert hyperslab["counts", "unspliced", (0, None)].data.dtype == env.torch.uint8


def test_read_layer_csr_stream_raises_what_hyperslab_raises(env, files):
    for layer, text in (("spliced", "holds non-integer values: not a count layer"), ("unspliced", "counts outside 0..65535 cannot be held as uint16"),
                        ("ambiguous", "counts outside 0..65535 cannot be held as uint16")):
        msgs = []
        for engine in ("hyperslab", "stream"):
            with pytest.raises(ValueError) as exc:
                env.loom_io.read_layer_csr(files["bad"], layer, cell_block=256, engine=engine)
            msgs.append(str(exc.value))
        assert msgs[0] == msgs[1] and text in msgs[0] and f"layer {layer}" in msgs[0]
    with pytest.raises(ValueError, match="engine"):
        env.loom_io.read_layer_csr(files["counts"], "spliced", engine="other")


@pytest.mark.parametrize("which", ["counts", "mixed", "bad", "v2", "v3"])
def test_velocytoloom_stream_equals_whole(env, files, which, caplog):
    import logging
    t = env.torch
    VL = env.vcy.analysis.VelocytoLoom
    whole = VL(files[which])
    with caplog.at_level(logging.INFO):
        stream = VL(files[which], ingest="stream")
    if which in ("mixed", "bad"):                                           # a layer that is no count layer is read whole, and says so
        assert any("read whole" in r.getMessage() for r in caplog.records)
    for name in ("S", "U", "A"):
        assert (name in whole._dev) == (name in stream._dev)
        if name not in whole._dev:
            continue
        a, b = getattr(whole, name), getattr(stream, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
        assert whole.dev(name).t.dtype == stream.dev(name).t.dtype and t.equal(whole.dev(name).t, stream.dev(name).t), name
    cw, cs = whole.__dict__.get("_counts", {}), stream.__dict__.get("_counts", {})
    assert set(cw) == set(cs)
    for k in cw:
        assert cw[k].G == cs[k].G and cw[k].t.dtype == cs[k].t.dtype and t.equal(cw[k].t, cs[k].t), k
    if which == "counts":
        assert cw["S"].t.dtype == t.int16 and cw["U"].t.dtype == t.uint8
    for a, b in ((whole.ca, stream.ca), (whole.ra, stream.ra)):
        assert list(a) == list(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    for name in ("initial_cell_size", "initial_Ucell_size"):
        a, b = getattr(whole, name), getattr(stream, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    with pytest.raises(ValueError, match="ingest"):
        VL(files[which], ingest="other")
