"""Host side of the streamed .loom ingest (loom_io.LayerBlockReader, vcy_loom_block_host): every tile must hold the bytes
read_layer_block returns for the same cells - dtype included - whatever the chunking, the filters, the block size and the
number of threads, and storage the reader does not take directly must come out the same through its fallback.  CPU-only."""
import ctypes
import os
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DTYPES = ("uint8", "uint16", "uint32", "int32", "int64", "float32", "float64")


@pytest.fixture(scope="module")
def loom_io():
    import velocyto_amd
    velocyto_amd.build()
    from velocyto_amd import loom_io as m
    m._lib()
    return m


def _layer(rng, G, C, dtype):
    a = rng.poisson(0.4, (G, C)) * rng.integers(1, 200, (G, C))
    return a.astype(dtype)


def _check(loom_io, path, layer, direct, cell_blocks=(1, 50, 64, 8192), ranges=((0, None),), threads=(1, 4)):
    for th in threads:
        for cb in cell_blocks:
            for c0, c1 in ranges:
                with loom_io.LayerBlockReader(path, layer, cb, c0, c1, th) as r:
                    assert r.direct == direct, r.why_not
                    stop = r.C if c1 is None else c1
                    want = list(range(c0, stop, cb))
                    got = []
                    for s, e, tile in r:
                        ref = loom_io.read_layer_block(path, layer, s, e)
                        assert tile.dtype == ref.dtype and tile.shape == ref.shape and tile.flags.c_contiguous
                        assert tile.tobytes() == ref.tobytes(), (path, layer, th, cb, s, e)
                        got.append(s)
                        assert e == min(stop, s + cb)
                    assert got == want


@pytest.mark.parametrize("name", ["loompy_v2.loom", "loompy_v3.loom"])
def test_committed_fixtures(loom_io, name):
    """23 x 17 inside one partial (64, 64) chunk, uint16 and uint32, written by the HDF5 C library as loompy lays files out"""
    path = os.path.join(GOLDEN, name)
    for layer in ("spliced", "unspliced"):
        _check(loom_io, path, layer, True, cell_blocks=(1, 5, 17, 64), ranges=((0, None), (3, 11)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunked_gzip_every_shape(loom_io, tmp_path, dtype):
    rng = np.random.default_rng(len(dtype) + ord(dtype[0]))
    for G in (1, 63, 64, 65, 130):
        for C in (1, 63, 64, 65, 200):
            path = str(tmp_path / f"g{G}_c{C}.loom")
            a = _layer(rng, G, C, dtype)
            loom_io.write_loom(path, {"spliced": a, "unspliced": a[::-1].copy()}, chunks=(64, 64), compression=2)
            assert np.array_equal(loom_io.read_layer_block(path, "spliced", 0, C), a)
            _check(loom_io, path, "spliced", True)
            if C == 200:                                          # blocks that start and end inside chunks
                _check(loom_io, path, "unspliced", True, ranges=((37, 101),))


def test_shuffle_unfiltered_rectangular_and_contiguous(loom_io, tmp_path):
    rng = np.random.default_rng(5)
    for dtype in ("uint16", "int64", "float32"):
        a = _layer(rng, 130, 200, dtype)
        for tag, kw, direct in (("shuffle", dict(chunks=(64, 64), compression=2, shuffle=True), True),
                                ("plain", dict(chunks=(64, 64)), True),
                                ("rect", dict(chunks=(32, 128), compression=2), True),
                                ("contiguous", {}, False)):
            path = str(tmp_path / f"{tag}_{dtype}.loom")
            loom_io.write_loom(path, {"spliced": a, "unspliced": a}, **kw)
            _check(loom_io, path, "spliced", direct, cell_blocks=(50, 8192), ranges=((0, None), (37, 101)))
    with loom_io.LayerBlockReader(str(tmp_path / "contiguous_uint16.loom"), "spliced") as r:
        assert r.why_not == "layout is not chunked"


def test_threads_default_and_cap(loom_io):
    path = os.path.join(GOLDEN, "loompy_v2.loom")
    for given, used in ((None, 8), (1, 1), (16, 16), (64, 16), (0, 1)):
        with loom_io.LayerBlockReader(path, "spliced", threads=given) as r:
            assert r.threads == used
    with pytest.raises(IndexError):
        loom_io.LayerBlockReader(path, "spliced", c0=3, c1=18)
    with loom_io.LayerBlockReader(path, "spliced", c0=5, c1=5) as r:
        assert list(r) == []


def _create_chunked(loom_io, path, G, C, dtype, chunk, deflate):
    """/layers/spliced created empty through the module's own bound calls -> (file id, dataset id)"""
    L = loom_io._lib()
    hs = loom_io.hsize_t
    f = L.H5Fcreate(path.encode(), loom_io.H5F_ACC_TRUNC, 0, 0)
    g = L.H5Gcreate2(f, b"layers", 0, 0, 0)
    sp = L.H5Screate_simple(2, (hs * 2)(G, C), None)
    dcpl = L.H5Pcreate(loom_io.hid_t.in_dll(L, "H5P_CLS_DATASET_CREATE_ID_g").value)
    assert L.H5Pset_chunk(dcpl, 2, (hs * 2)(*chunk)) >= 0
    if deflate:
        assert L.H5Pset_deflate(dcpl, 2) >= 0
    d = L.H5Dcreate2(g, b"spliced", L._native[loom_io._NP2H5[np.dtype(dtype)]], sp, 0, dcpl, 0)
    assert d >= 0
    L.H5Pclose(dcpl)
    L.H5Sclose(sp)
    L.H5Gclose(g)
    return f, d


def test_unwritten_chunks_read_as_zeros(loom_io, tmp_path):
    """Only one corner of the dataset was ever written (a hyperslab H5Dwrite): the other chunks do not exist in the file."""
    L = loom_io._lib()
    hs = loom_io.hsize_t
    path = str(tmp_path / "corner.loom")
    G, C = 150, 210
    f, d = _create_chunked(loom_io, path, G, C, "uint16", (64, 64), True)
    corner = np.arange(1, 40 * 70 + 1, dtype=np.uint16).reshape(40, 70)
    fsp = L.H5Dget_space(d)
    assert L.H5Sselect_hyperslab(fsp, loom_io.H5S_SELECT_SET, (hs * 2)(100, 130), None, (hs * 2)(40, 70), None) >= 0
    msp = L.H5Screate_simple(2, (hs * 2)(40, 70), None)
    assert L.H5Dwrite(d, L._native["UINT16"], msp, fsp, 0, corner.ctypes.data) >= 0
    for h in (msp, fsp):
        L.H5Sclose(h)
    L.H5Dclose(d)
    L.H5Fclose(f)
    full = loom_io.read_layer_block(path, "spliced", 0, C)
    assert np.array_equal(full[100:140, 130:200], corner) and full.sum() == corner.sum(dtype=np.int64)
    _check(loom_io, path, "spliced", True, cell_blocks=(50, 64, 8192), ranges=((0, None), (37, 201)))
    # the staging buffers are reused: a block of zeros must overwrite what the block before left there
    with loom_io.LayerBlockReader(path, "spliced", 64, 64, None, 2) as r:
        tiles = [(s, t.copy()) for s, _, t in r]
    assert [s for s, _ in tiles] == [64, 128, 192] and not tiles[0][1].any() and tiles[1][1].any()


def test_truncated_deflate_stream_raises(loom_io, tmp_path):
    """One chunk holds the first half of its deflate stream (written raw with H5Dwrite_chunk): IOError naming the chunk."""
    L = loom_io._lib()
    hs = loom_io.hsize_t
    L.H5Dwrite_chunk.restype = ctypes.c_int
    L.H5Dwrite_chunk.argtypes = [loom_io.hid_t, loom_io.hid_t, ctypes.c_uint32, ctypes.POINTER(hs), ctypes.c_size_t, ctypes.c_void_p]
    path = str(tmp_path / "cut.loom")
    rng = np.random.default_rng(3)
    f, d = _create_chunked(loom_io, path, 128, 128, "uint16", (64, 64), True)
    chunks = {}
    for at in ((0, 0), (0, 64), (64, 0), (64, 64)):
        chunks[at] = rng.poisson(2.0, (64, 64)).astype(np.uint16)
        z = zlib.compress(chunks[at].tobytes(), 2)
        if at == (64, 0):
            z = z[: len(z) // 2]
        assert L.H5Dwrite_chunk(d, 0, 0, (hs * 2)(*at), len(z), z) >= 0
    L.H5Dclose(d)
    L.H5Fclose(f)
    for th in (1, 4):
        with loom_io.LayerBlockReader(path, "spliced", 64, 64, 128, th) as r:            # the cells of the good chunks only
            (s, e, tile), = list(r)
            assert np.array_equal(tile, np.vstack([chunks[(0, 64)], chunks[(64, 64)]]))
        with loom_io.LayerBlockReader(path, "spliced", 64, threads=th) as r:
            with pytest.raises(IOError, match=r"gene 64, cell 0"):
                list(r)


def _write_loom_before(loom_io, path, layers, col_attrs=None, row_attrs=None, matrix=None):
    """write_loom as it was before it learnt chunks / compression / shuffle, kept here to pin the default's bytes"""
    L = loom_io._lib()
    hsize_t, _check, _NP2H5 = loom_io.hsize_t, loom_io._check, loom_io._NP2H5
    f = _check(L.H5Fcreate(path.encode(), loom_io.H5F_ACC_TRUNC, 0, 0), f"create {path}")

    def put(parent, name, arr):
        arr = np.asarray(arr)
        if arr.dtype.kind in ("U", "O"):
            arr = np.char.encode(arr.astype(str), "utf-8")
        arr = np.ascontiguousarray(arr)
        dims = (hsize_t * arr.ndim)(*arr.shape)
        sp = L.H5Screate_simple(arr.ndim, dims, None)
        if arr.dtype.kind == "S":
            tp = L.H5Tcopy(L._c_s1)
            L.H5Tset_size(tp, max(arr.dtype.itemsize, 1))
        else:
            tp = L._native[_NP2H5[arr.dtype]]
        d = _check(L.H5Dcreate2(parent, name.encode(), tp, sp, 0, 0, 0), f"create {name}")
        _check(L.H5Dwrite(d, tp, 0, 0, 0, arr.ctypes.data), f"write {name}")
        L.H5Dclose(d)
        L.H5Sclose(sp)
        if arr.dtype.kind == "S":
            L.H5Tclose(tp)

    try:
        first = next(iter(layers.values()))
        put(f, "matrix", np.asarray(matrix if matrix is not None else sum(np.asarray(v, dtype=np.float32) for v in layers.values()), dtype=np.float32))
        for grp, items in (("layers", layers), ("col_attrs", col_attrs or {"CellID": np.arange(first.shape[1])}),
                           ("row_attrs", row_attrs or {"Gene": np.arange(first.shape[0])})):
            g = _check(L.H5Gcreate2(f, grp.encode(), 0, 0, 0), f"create group {grp}")
            for k, v in items.items():
                put(g, k, v)
            L.H5Gclose(g)
    finally:
        L.H5Fclose(f)


def test_write_loom_defaults_write_the_same_bytes(loom_io, tmp_path):
    rng = np.random.default_rng(9)
    layers = {"spliced": rng.poisson(3, (37, 53)).astype(np.uint16), "unspliced": rng.poisson(1, (37, 53)).astype(np.uint32),
              "ambiguous": rng.random((37, 53))}
    ca = {"CellID": np.array([f"c{i}" for i in range(53)]), "x": rng.normal(size=53)}
    ra = {"Gene": np.array([f"g{i}" for i in range(37)])}
    for i, (c, r) in enumerate(((ca, ra), (None, None))):
        new, old = str(tmp_path / f"new{i}.loom"), str(tmp_path / f"old{i}.loom")
        loom_io.write_loom(new, layers, c, r)
        _write_loom_before(loom_io, old, layers, c, r)
        assert open(new, "rb").read() == open(old, "rb").read()
    with pytest.raises(ValueError):
        loom_io.write_loom(str(tmp_path / "x.loom"), layers, compression=2)
    chunked = str(tmp_path / "chunked.loom")
    loom_io.write_loom(chunked, layers, ca, ra, chunks=(64, 64), compression=2, shuffle=True)
    got, ca2, ra2 = loom_io.read_loom(chunked)
    assert all(got[k].dtype == layers[k].dtype and np.array_equal(got[k], layers[k]) for k in layers)
    assert list(ca2["CellID"]) == list(ca["CellID"]) and list(ra2["Gene"]) == list(ra["Gene"])
    names, ca3, ra3 = loom_io.read_loom_attrs(chunked)
    assert set(names) == set(layers) and set(ca3) == set(ca2) and np.array_equal(ca3["x"], ca2["x"])
    assert np.array_equal(loom_io.read_layer(chunked, "ambiguous"), layers["ambiguous"])
