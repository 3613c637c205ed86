""".loom ingest / export without loompy or h5py (analysis.py:56-64 reads the layers
``spliced`` / ``unspliced`` / ``ambiguous`` plus row/col attributes; the writer side is
commands/_run.py:283-297).

A .loom file is plain HDF5: ``/matrix`` (genes x cells), ``/layers/<name>`` (same shape),
``/row_attrs/<name>`` (length genes), ``/col_attrs/<name>`` (length cells).  The image ships the HDF5
C library (libhdf5 1.10, /opt/conda/lib) but no Python binding, so this module binds the dozen C
calls it needs with ctypes.  If h5py is importable it is preferred.

Only what the analysis path needs is implemented: contiguous/chunked/compressed numeric datasets of
rank 1-2 and fixed- or variable-length string attributes.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional, Tuple

import numpy as np

_HDF5_CANDIDATES = ("libhdf5.so", "/opt/conda/lib/libhdf5.so", "/usr/lib/x86_64-linux-gnu/libhdf5_serial.so",
                    "/usr/lib/x86_64-linux-gnu/libhdf5.so")
_H5 = None

hid_t = ctypes.c_int64
hsize_t = ctypes.c_uint64
H5F_ACC_RDONLY, H5F_ACC_TRUNC = 0, 2
H5P_DEFAULT, H5S_ALL = 0, 0
H5T_INTEGER, H5T_FLOAT, H5T_STRING, H5T_ENUM = 0, 1, 3, 8
H5S_SELECT_SET = 0
H5_INDEX_NAME, H5_ITER_INC = 0, 0
H5T_VARIABLE = ctypes.c_size_t(-1).value


def _lib():
    global _H5
    if _H5 is None:
        last = None
        for cand in _HDF5_CANDIDATES:
            try:
                L = ctypes.CDLL(cand)
                break
            except OSError as e:
                last = e
        else:
            raise ImportError(f"no HDF5 library found (tried {_HDF5_CANDIDATES}): {last}")
        L.H5open()
        for name, res, args in (
                ("H5Fopen", hid_t, [ctypes.c_char_p, ctypes.c_uint, hid_t]), ("H5Fcreate", hid_t, [ctypes.c_char_p, ctypes.c_uint, hid_t, hid_t]),
                ("H5Fclose", ctypes.c_int, [hid_t]), ("H5Gopen2", hid_t, [hid_t, ctypes.c_char_p, hid_t]),
                ("H5Gcreate2", hid_t, [hid_t, ctypes.c_char_p, hid_t, hid_t, hid_t]), ("H5Gclose", ctypes.c_int, [hid_t]),
                ("H5Dopen2", hid_t, [hid_t, ctypes.c_char_p, hid_t]), ("H5Dclose", ctypes.c_int, [hid_t]),
                ("H5Dget_space", hid_t, [hid_t]), ("H5Dget_type", hid_t, [hid_t]),
                ("H5Dread", ctypes.c_int, [hid_t, hid_t, hid_t, hid_t, hid_t, ctypes.c_void_p]),
                ("H5Dwrite", ctypes.c_int, [hid_t, hid_t, hid_t, hid_t, hid_t, ctypes.c_void_p]),
                ("H5Dcreate2", hid_t, [hid_t, ctypes.c_char_p, hid_t, hid_t, hid_t, hid_t, hid_t]),
                ("H5Sget_simple_extent_ndims", ctypes.c_int, [hid_t]),
                ("H5Sget_simple_extent_dims", ctypes.c_int, [hid_t, ctypes.POINTER(hsize_t), ctypes.POINTER(hsize_t)]),
                ("H5Screate_simple", hid_t, [ctypes.c_int, ctypes.POINTER(hsize_t), ctypes.POINTER(hsize_t)]),
                ("H5Sclose", ctypes.c_int, [hid_t]), ("H5Tget_class", ctypes.c_int, [hid_t]), ("H5Tget_size", ctypes.c_size_t, [hid_t]),
                ("H5Tget_sign", ctypes.c_int, [hid_t]), ("H5Tis_variable_str", ctypes.c_int, [hid_t]), ("H5Tclose", ctypes.c_int, [hid_t]),
                ("H5Tcopy", hid_t, [hid_t]), ("H5Tset_size", ctypes.c_int, [hid_t, ctypes.c_size_t]),
                ("H5Lexists", ctypes.c_int, [hid_t, ctypes.c_char_p, hid_t]),
                ("H5Gget_num_objs", ctypes.c_int, [hid_t, ctypes.POINTER(hsize_t)]),
                ("H5Lget_name_by_idx", ctypes.c_ssize_t, [hid_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, hsize_t, ctypes.c_char_p, ctypes.c_size_t, hid_t]),
                ("H5Dvlen_reclaim", ctypes.c_int, [hid_t, hid_t, hid_t, ctypes.c_void_p]),
                ("H5Pcreate", hid_t, [hid_t]), ("H5Pset_chunk", ctypes.c_int, [hid_t, ctypes.c_int, ctypes.POINTER(hsize_t)]),
                ("H5Pset_deflate", ctypes.c_int, [hid_t, ctypes.c_uint]), ("H5Pclose", ctypes.c_int, [hid_t]),
                ("H5Sselect_hyperslab", ctypes.c_int, [hid_t, ctypes.c_int, ctypes.POINTER(hsize_t), ctypes.POINTER(hsize_t), ctypes.POINTER(hsize_t), ctypes.POINTER(hsize_t)]),
                ("H5Tenum_create", hid_t, [hid_t]), ("H5Tenum_insert", ctypes.c_int, [hid_t, ctypes.c_char_p, ctypes.c_void_p]),
                ("H5Tget_nmembers", ctypes.c_int, [hid_t]),
                ("H5Aget_num_attrs", ctypes.c_int, [hid_t]),
                ("H5Aopen_by_idx", hid_t, [hid_t, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, hsize_t, hid_t, hid_t]),
                ("H5Aget_name", ctypes.c_ssize_t, [hid_t, ctypes.c_size_t, ctypes.c_char_p]), ("H5Aget_type", hid_t, [hid_t]),
                ("H5Aget_space", hid_t, [hid_t]), ("H5Aread", ctypes.c_int, [hid_t, hid_t, ctypes.c_void_p]), ("H5Aclose", ctypes.c_int, [hid_t]),
                # what LayerBlockReader asks about a layer's storage
                ("H5Dget_create_plist", hid_t, [hid_t]),
                ("H5Pget_layout", ctypes.c_int, [hid_t]), ("H5Pget_chunk", ctypes.c_int, [hid_t, ctypes.c_int, ctypes.POINTER(hsize_t)]),
                ("H5Pget_nfilters", ctypes.c_int, [hid_t]),
                ("H5Pget_filter2", ctypes.c_int, [hid_t, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_size_t),
                                                  ctypes.POINTER(ctypes.c_uint), ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint)]),
                ("H5Pfill_value_defined", ctypes.c_int, [hid_t, ctypes.POINTER(ctypes.c_int)]),
                ("H5Pget_fill_value", ctypes.c_int, [hid_t, hid_t, ctypes.c_void_p]),
                ("H5Tget_order", ctypes.c_int, [hid_t]),
                ("H5Pset_shuffle", ctypes.c_int, [hid_t]), ("H5is_library_threadsafe", ctypes.c_int, [ctypes.POINTER(ctypes.c_bool)]),
                ("H5Dget_chunk_storage_size", ctypes.c_int, [hid_t, ctypes.POINTER(hsize_t), ctypes.POINTER(hsize_t)]),
                ("H5Dread_chunk", ctypes.c_int, [hid_t, hid_t, ctypes.POINTER(hsize_t), ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        L._native = {k: hid_t.in_dll(L, f"H5T_NATIVE_{k}_g").value for k in
                     ("FLOAT", "DOUBLE", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64")}
        L._c_s1 = hid_t.in_dll(L, "H5T_C_S1_g").value
        _H5 = L
    return _H5


_NP2H5 = {np.dtype(k): v for k, v in (("float32", "FLOAT"), ("float64", "DOUBLE"), ("int8", "INT8"), ("uint8", "UINT8"), ("int16", "INT16"),
                                      ("uint16", "UINT16"), ("int32", "INT32"), ("uint32", "UINT32"), ("int64", "INT64"), ("uint64", "UINT64"))}


def _check(v, what):
    if v < 0:
        raise IOError(f"HDF5 call failed: {what}")
    return v


def _read_dataset(L, parent: int, name: str) -> np.ndarray:
    d = _check(L.H5Dopen2(parent, name.encode(), H5P_DEFAULT), f"open dataset {name}")
    try:
        sp, tp = L.H5Dget_space(d), L.H5Dget_type(d)
        nd = L.H5Sget_simple_extent_ndims(sp)
        dims = (hsize_t * max(nd, 1))()
        if nd > 0:
            L.H5Sget_simple_extent_dims(sp, dims, None)
        shape = tuple(int(dims[i]) for i in range(nd))
        cls, size = L.H5Tget_class(tp), L.H5Tget_size(tp)
        if cls == H5T_FLOAT:
            dt = np.dtype(np.float32 if size == 4 else np.float64)
        elif cls == H5T_INTEGER:
            dt = np.dtype(("u" if L.H5Tget_sign(tp) == 0 else "i") + str(size))
        elif cls == H5T_STRING:
            n = int(np.prod(shape)) if shape else 1
            if L.H5Tis_variable_str(tp) > 0:
                buf = (ctypes.c_char_p * n)()
                _check(L.H5Dread(d, tp, H5S_ALL, H5S_ALL, H5P_DEFAULT, buf), f"read {name}")
                out = np.array([(b or b"").decode("utf-8", "replace") for b in buf], dtype=object).reshape(shape)
                L.H5Dvlen_reclaim(tp, sp, H5P_DEFAULT, buf)
            else:
                raw = np.empty(n, dtype=f"S{size}")
                _check(L.H5Dread(d, tp, H5S_ALL, H5S_ALL, H5P_DEFAULT, raw.ctypes.data), f"read {name}")
                out = np.char.decode(raw, "utf-8").reshape(shape)
            L.H5Tclose(tp)
            L.H5Sclose(sp)
            return out
        elif cls == H5T_ENUM and size == 1:
            # h5py stores numpy bool arrays as an 8-bit enum {FALSE = 0, TRUE = 1} (what the reference's dump_hdf5 writes for
            # boolean attributes such as cv_mean_selected; serialization.py:44-92): read the bytes through the file's own type
            raw = np.empty(shape, dtype=np.int8)
            _check(L.H5Dread(d, tp, H5S_ALL, H5S_ALL, H5P_DEFAULT, raw.ctypes.data), f"read {name}")
            L.H5Tclose(tp)
            L.H5Sclose(sp)
            return raw.astype(np.bool_)
        else:
            raise IOError(f"dataset {name}: unsupported HDF5 type class {cls}")
        out = np.empty(shape, dtype=dt)
        _check(L.H5Dread(d, L._native[_NP2H5[dt]], H5S_ALL, H5S_ALL, H5P_DEFAULT, out.ctypes.data), f"read {name}")
        L.H5Tclose(tp)
        L.H5Sclose(sp)
        return out
    finally:
        L.H5Dclose(d)


def _group_members(L, parent: int, name: str):
    if L.H5Lexists(parent, name.encode(), H5P_DEFAULT) <= 0:
        return None, []
    g = _check(L.H5Gopen2(parent, name.encode(), H5P_DEFAULT), f"open group {name}")
    n = hsize_t()
    L.H5Gget_num_objs(g, ctypes.byref(n))
    names = []
    for i in range(n.value):
        ln = L.H5Lget_name_by_idx(g, b".", H5_INDEX_NAME, H5_ITER_INC, i, None, 0, H5P_DEFAULT)
        buf = ctypes.create_string_buffer(ln + 1)
        L.H5Lget_name_by_idx(g, b".", H5_INDEX_NAME, H5_ITER_INC, i, buf, ln + 1, H5P_DEFAULT)
        names.append(buf.value.decode())
    return g, names


def read_loom(path: str) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """-> (layers {spliced, unspliced, ambiguous?}, col_attrs, row_attrs), arrays as stored (genes x cells)."""
    try:
        import h5py
        with h5py.File(path, "r") as f:
            layers = {k: f["layers"][k][:, :] for k in ("spliced", "unspliced", "ambiguous") if k in f["layers"]}
            return layers, {k: f["col_attrs"][k][...] for k in f["col_attrs"]}, {k: f["row_attrs"][k][...] for k in f["row_attrs"]}
    except ImportError:
        pass
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    L = _lib()
    f = _check(L.H5Fopen(path.encode(), H5F_ACC_RDONLY, H5P_DEFAULT), f"open {path}")
    try:
        g, names = _group_members(L, f, "layers")
        if g is None or "spliced" not in names or "unspliced" not in names:
            raise IOError(f"{path}: not a velocyto loom file (needs /layers/spliced and /layers/unspliced)")
        layers = {k: _read_dataset(L, g, k) for k in ("spliced", "unspliced", "ambiguous") if k in names}
        L.H5Gclose(g)
        attrs = []
        for grp in ("col_attrs", "row_attrs"):
            g, names = _group_members(L, f, grp)
            attrs.append({k: _read_dataset(L, g, k) for k in names} if g is not None else {})
            if g is not None:
                L.H5Gclose(g)
        return layers, attrs[0], attrs[1]
    finally:
        L.H5Fclose(f)


def read_file_attrs(path: str) -> Dict[str, object]:
    """File-level attributes of a .loom file: the datasets under /attrs (LOOM_SPEC_VERSION >= 3.0.0) and the HDF5 attributes
    of the root group (loompy 2 wrote LOOM_SPEC_VERSION, CreationDate, ... there).  Values as str / numpy scalars or arrays."""
    L = _lib()
    f = _check(L.H5Fopen(path.encode(), H5F_ACC_RDONLY, H5P_DEFAULT), f"open {path}")
    out: Dict[str, object] = {}
    try:
        root = _check(L.H5Gopen2(f, b"/", H5P_DEFAULT), "open root group")
        n = L.H5Aget_num_attrs(root)
        for i in range(max(n, 0)):
            a = _check(L.H5Aopen_by_idx(root, b".", H5_INDEX_NAME, H5_ITER_INC, i, H5P_DEFAULT, H5P_DEFAULT), "open attribute")
            ln = L.H5Aget_name(a, 0, None)
            nb = ctypes.create_string_buffer(ln + 1)
            L.H5Aget_name(a, ln + 1, nb)
            tp = L.H5Aget_type(a)
            cls, size = L.H5Tget_class(tp), L.H5Tget_size(tp)
            # the attribute's dataspace decides the buffer: loompy 2 allows array-valued global attributes, and H5Aread writes
            # npoints * size bytes whatever the caller allocated
            sp = L.H5Aget_space(a)
            nd = L.H5Sget_simple_extent_ndims(sp)
            dims = (hsize_t * max(nd, 1))()
            if nd > 0:
                L.H5Sget_simple_extent_dims(sp, dims, None)
            shape = tuple(int(dims[j]) for j in range(max(nd, 0)))
            npts = int(np.prod(shape)) if shape else 1
            key = nb.value.decode()
            if cls == H5T_STRING and npts > 0:
                if L.H5Tis_variable_str(tp) > 0:
                    buf = (ctypes.c_char_p * npts)()
                    L.H5Aread(a, tp, buf)
                    vals = [(buf[j] or b"").decode("utf-8", "replace") for j in range(npts)]
                    L.H5Dvlen_reclaim(tp, sp, H5P_DEFAULT, buf)          # the library allocated the strings: hand them back
                else:
                    raw = ctypes.create_string_buffer(size * npts + 1)
                    L.H5Aread(a, tp, raw)
                    vals = [raw.raw[j * size:(j + 1) * size].split(b"\0", 1)[0].decode("utf-8", "replace") for j in range(npts)]
                out[key] = vals[0] if not shape else np.array(vals, dtype=object).reshape(shape)
            elif cls in (H5T_INTEGER, H5T_FLOAT) and npts > 0:
                dt = np.dtype(np.float32 if size == 4 else np.float64) if cls == H5T_FLOAT else np.dtype(("u" if L.H5Tget_sign(tp) == 0 else "i") + str(size))
                v = np.empty(shape, dtype=dt)
                L.H5Aread(a, L._native[_NP2H5[dt]], v.ctypes.data)
                out[key] = v[()] if not shape else v
            L.H5Sclose(sp)
            L.H5Tclose(tp)
            L.H5Aclose(a)
        L.H5Gclose(root)
        g, names = _group_members(L, f, "attrs")
        if g is not None:
            for k in names:
                v = _read_dataset(L, g, k)
                out[k] = v[()] if getattr(v, "shape", None) == () else v
            L.H5Gclose(g)
        return out
    finally:
        L.H5Fclose(f)


def layer_shape(path: str, layer: str = "spliced") -> Tuple[int, int]:
    """(genes, cells) of /layers/<layer> without reading it."""
    L = _lib()
    f = _check(L.H5Fopen(path.encode(), H5F_ACC_RDONLY, H5P_DEFAULT), f"open {path}")
    try:
        d = _check(L.H5Dopen2(f, f"layers/{layer}".encode(), H5P_DEFAULT), f"open layer {layer}")
        sp = L.H5Dget_space(d)
        dims = (hsize_t * 2)()
        L.H5Sget_simple_extent_dims(sp, dims, None)
        L.H5Sclose(sp)
        L.H5Dclose(d)
        return int(dims[0]), int(dims[1])
    finally:
        L.H5Fclose(f)


def read_layer_block(path: str, layer: str, c0: int, c1: int) -> np.ndarray:
    """The columns (cells) c0..c1-1 of /layers/<layer>, all genes, as stored: one hyperslab read (chunked / gzip-compressed
    layers are decoded by the HDF5 library)."""
    L = _lib()
    f = _check(L.H5Fopen(path.encode(), H5F_ACC_RDONLY, H5P_DEFAULT), f"open {path}")
    try:
        d = _check(L.H5Dopen2(f, f"layers/{layer}".encode(), H5P_DEFAULT), f"open layer {layer}")
        sp, tp = L.H5Dget_space(d), L.H5Dget_type(d)
        dims = (hsize_t * 2)()
        L.H5Sget_simple_extent_dims(sp, dims, None)
        G, C = int(dims[0]), int(dims[1])
        if not (0 <= c0 < c1 <= C):
            raise IndexError(f"cells {c0}:{c1} outside 0:{C}")
        cls, size = L.H5Tget_class(tp), L.H5Tget_size(tp)
        dt = (np.dtype(np.float32 if size == 4 else np.float64) if cls == H5T_FLOAT else np.dtype(("u" if L.H5Tget_sign(tp) == 0 else "i") + str(size)))
        start, count = (hsize_t * 2)(0, c0), (hsize_t * 2)(G, c1 - c0)
        _check(L.H5Sselect_hyperslab(sp, H5S_SELECT_SET, start, None, count, None), "select hyperslab")
        msp = L.H5Screate_simple(2, count, None)
        out = np.empty((G, c1 - c0), dtype=dt)
        _check(L.H5Dread(d, L._native[_NP2H5[dt]], msp, sp, H5P_DEFAULT, out.ctypes.data), f"read layer {layer}")
        L.H5Sclose(msp); L.H5Sclose(sp); L.H5Tclose(tp); L.H5Dclose(d)
        return out
    finally:
        L.H5Fclose(f)


def read_loom_attrs(path: str) -> Tuple[Tuple[str, ...], Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """-> (names under /layers, col_attrs, row_attrs): what read_loom returns beside the layers, without reading a layer."""
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    L = _lib()
    f = _check(L.H5Fopen(path.encode(), H5F_ACC_RDONLY, H5P_DEFAULT), f"open {path}")
    try:
        g, names = _group_members(L, f, "layers")
        if g is None or "spliced" not in names or "unspliced" not in names:
            raise IOError(f"{path}: not a velocyto loom file (needs /layers/spliced and /layers/unspliced)")
        L.H5Gclose(g)
        attrs = []
        for grp in ("col_attrs", "row_attrs"):
            g, members = _group_members(L, f, grp)
            attrs.append({k: _read_dataset(L, g, k) for k in members} if g is not None else {})
            if g is not None:
                L.H5Gclose(g)
        return tuple(names), attrs[0], attrs[1]
    finally:
        L.H5Fclose(f)


def read_layer(path: str, layer: str) -> np.ndarray:
    """/layers/<layer> whole, as stored (genes x cells): one H5Dread, what read_loom does per layer."""
    L = _lib()
    f = _check(L.H5Fopen(path.encode(), H5F_ACC_RDONLY, H5P_DEFAULT), f"open {path}")
    try:
        g = _check(L.H5Gopen2(f, b"layers", H5P_DEFAULT), "open group layers")
        try:
            return _read_dataset(L, g, layer)
        finally:
            L.H5Gclose(g)
    finally:
        L.H5Fclose(f)


H5D_CHUNKED, H5Z_FILTER_DEFLATE, H5Z_FILTER_SHUFFLE = 2, 1, 2
READER_THREADS, READER_MAX_THREADS = 8, 16        # never os.cpu_count(): a job is given a few CPUs of a much larger machine


class LayerBlockReader:
    """Iterator over ``(s, e, tile)``: the cells s..e-1 of /layers/<layer>, all genes, as a C-contiguous ``(G, e - s)`` array in
    the FILE's element type - the bytes read_layer_block(path, layer, s, e) returns - for s = c0, c0 + cell_block, ... < c1.

    The block's chunks are found (dataset creation plist: H5Pget_chunk), their stored bytes fetched (H5Dread_chunk), inflated and
    placed on `threads` host threads (vcy_loom_block_host: C++ threads, because a Python loop over 16 KB chunks is
    bound by the interpreter lock, not by zlib), while the caller works on the block before: a background thread keeps one
    block ahead.  threads=None means 8; at most 16 are used.

    Storage taken directly: chunked layout, rank 2, little-endian integer or IEEE float elements of 1, 2, 4 or 8 bytes, filter
    pipeline empty, deflate or shuffle + deflate (the per-chunk filter mask honoured), fill value zero (a chunk
    that was never written reads as zeros).  Anything else - contiguous layout, other filters, big-endian, a non-zero fill value -
    is read block by block with read_layer_block into the same buffers: never an error (`direct` says which).  A chunk that does
    not inflate to the chunk size raises IOError naming the chunk.

    Buffers.  Tiles live in two staging buffers, allocated once (page-locked when a GPU is present, so the upload can be
    asynchronous) and used alternately.  A tile is valid until the caller asks for the next block: at that point its buffer is
    handed back, and the reader fills it with the block after the next one.  A caller that copies a tile asynchronously records
    an event behind the copy and passes it to ``copied(event)`` before it asks for the next block: the reader then waits for
    that event (``event.synchronize()``) before it writes into the buffer again - a buffer is overwritten after the consumer's
    copy event, never before."""

    def __init__(self, path: str, layer: str, cell_block: int = 8192, c0: int = 0, c1: Optional[int] = None, threads: Optional[int] = None):
        import threading
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.path, self.layer = path, layer
        self.cell_block = int(cell_block)
        if self.cell_block < 1:
            raise ValueError("cell_block must be positive")
        self.threads = max(1, min(READER_MAX_THREADS, READER_THREADS if threads is None else int(threads)))
        L = self._L = _lib()
        self._f = self._d = None
        self._thread = None
        self._f = _check(L.H5Fopen(path.encode(), H5F_ACC_RDONLY, H5P_DEFAULT), f"open {path}")
        try:
            self._d = _check(L.H5Dopen2(self._f, f"layers/{layer}".encode(), H5P_DEFAULT), f"open layer {layer}")
            sp, tp = L.H5Dget_space(self._d), L.H5Dget_type(self._d)
            nd = L.H5Sget_simple_extent_ndims(sp)
            dims = (hsize_t * max(nd, 2))()
            L.H5Sget_simple_extent_dims(sp, dims, None)
            L.H5Sclose(sp)
            try:
                if nd != 2:
                    raise IOError(f"layer {layer}: rank {nd}, expected (genes, cells)")
                self.G, self.C = int(dims[0]), int(dims[1])
                cls, size = L.H5Tget_class(tp), int(L.H5Tget_size(tp))
                self.dtype = (np.dtype(np.float32 if size == 4 else np.float64) if cls == H5T_FLOAT
                              else np.dtype(("u" if L.H5Tget_sign(tp) == 0 else "i") + str(size)))        # as read_layer_block
                self.c0, self.c1 = int(c0), self.C if c1 is None else int(c1)
                if not (0 <= self.c0 <= self.c1 <= self.C):
                    raise IndexError(f"cells {self.c0}:{self.c1} outside 0:{self.C}")
                self._plan(tp, cls, size)
            finally:
                L.H5Tclose(tp)
        except BaseException:
            self.close()
            raise
        self.width = max(1, min(self.cell_block, self.c1 - self.c0))
        self._owners = []                                  # the page-locked tensors behind the buffers
        self._buffers = [self._staging(self.G * self.width * self.dtype.itemsize) for _ in range(2)]
        self._events = [None, None]
        self._free = [threading.Semaphore(1), threading.Semaphore(1)]
        self._held = None                                  # buffer of the tile handed out last
        self._queue = None
        self._stop = False

    # ---- what the dataset's storage allows
    def _plan(self, tp, cls, size) -> None:
        L = self._L
        self.direct, self.why_not = False, None
        self.chunk, self.filters = None, 0

        def no(why):
            self.why_not = why

        if cls not in (H5T_INTEGER, H5T_FLOAT) or size not in (1, 2, 4, 8) or (cls == H5T_FLOAT and size not in (4, 8)):
            return no("element type")
        if size > 1 and L.H5Tget_order(tp) != 0:
            return no("big-endian")
        if self.G == 0 or self.C == 0:
            return no("empty dataset")
        dcpl = L.H5Dget_create_plist(self._d)
        try:
            if L.H5Pget_layout(dcpl) != H5D_CHUNKED:
                return no("layout is not chunked")
            ch = (hsize_t * 2)()
            if L.H5Pget_chunk(dcpl, 2, ch) != 2:
                return no("chunk rank")
            ids = []
            for i in range(max(L.H5Pget_nfilters(dcpl), 0)):
                flags, n, cfg = ctypes.c_uint(), ctypes.c_size_t(0), ctypes.c_uint()
                ids.append(L.H5Pget_filter2(dcpl, i, ctypes.byref(flags), ctypes.byref(n), None, 0, None, ctypes.byref(cfg)))
            if ids not in ([], [H5Z_FILTER_DEFLATE], [H5Z_FILTER_SHUFFLE, H5Z_FILTER_DEFLATE]):
                return no(f"filter pipeline {ids}")
            status = ctypes.c_int(-1)
            if L.H5Pfill_value_defined(dcpl, ctypes.byref(status)) < 0 or status.value not in (1, 2):
                return no("fill value undefined")
            if status.value == 2:                          # set by the writer: only zero lets an unwritten chunk be skipped
                fv = np.ones(1, dtype=self.dtype)
                if L.H5Pget_fill_value(dcpl, L._native[_NP2H5[self.dtype]], fv.ctypes.data) < 0 or fv[0] != 0:
                    return no("non-zero fill value")
        finally:
            L.H5Pclose(dcpl)
        safe = ctypes.c_bool(False)
        if self.threads > 1 and (L.H5is_library_threadsafe(ctypes.byref(safe)) < 0 or not safe.value):
            return no("HDF5 library is not a thread-safe build")
        from . import _lib as hip
        self._hip = hip.lib()
        # the stored bytes come through the library (H5Dread_chunk), so a user block needs no care; H5Dget_chunk_info_by_coord + pread
        # is not used: that call of 1.10 walks the chunk index from its start (milliseconds per chunk in an atlas file)
        self._calls = (ctypes.c_void_p * 4)(*(ctypes.cast(getattr(L, n), ctypes.c_void_p) for n in
                                              ("H5Dget_chunk_storage_size", "H5Dread_chunk", "H5Eset_auto2", "H5Eclear2")))
        self.chunk, self.filters, self.direct = (int(ch[0]), int(ch[1])), len(ids), True

    def _staging(self, nbytes: int) -> np.ndarray:
        try:
            import torch
            if torch.cuda.is_available():
                t = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True)
                self._owners.append(t)
                return t.numpy()
        except ImportError:
            pass
        return np.empty(max(nbytes, 1), dtype=np.uint8)

    def blocks(self):
        return [(s, min(self.c1, s + self.cell_block)) for s in range(self.c0, self.c1, self.cell_block)]

    def _fill(self, buf: np.ndarray, s: int, e: int) -> np.ndarray:
        tile = buf[: self.G * (e - s) * self.dtype.itemsize].view(self.dtype).reshape(self.G, e - s)
        if not self.direct:
            tile[...] = read_layer_block(self.path, self.layer, s, e)
            return tile
        bad = ctypes.c_int64(-1)
        rc = self._hip.vcy_loom_block_host(self._calls, self._d, self.G, self.C, self.chunk[0], self.chunk[1], self.dtype.itemsize,
                                           self.filters, s, e, tile.ctypes.data, e - s, self.threads, ctypes.byref(bad))
        if rc != 0:
            ncc = (e - 1) // self.chunk[1] - s // self.chunk[1] + 1
            at = (bad.value // ncc * self.chunk[0], (s // self.chunk[1] + bad.value % ncc) * self.chunk[1])
            what = {-4: "does not inflate to the chunk size", -5: "could not be read"}.get(rc, f"failed ({rc})")
            raise IOError(f"{self.path}: layer {self.layer}: the chunk at (gene {at[0]}, cell {at[1]}) {what}")
        return tile

    def _work(self) -> None:
        try:
            for i, (s, e) in enumerate(self.blocks()):
                k = i & 1
                self._free[k].acquire()
                if self._stop:
                    return
                if self._events[k] is not None:            # the caller's copy out of this buffer
                    self._events[k].synchronize()
                    self._events[k] = None
                self._queue.put((k, s, e, self._fill(self._buffers[k], s, e)))
            self._queue.put(None)
        except BaseException as exc:                       # handed to the caller, raised from __next__
            self._queue.put(exc)

    def __iter__(self):
        import queue
        import threading
        if self._thread is not None:
            raise RuntimeError("a LayerBlockReader is iterated once")
        self._queue = queue.Queue()
        self._thread = threading.Thread(target=self._work, name="loom-block-reader", daemon=True)
        self._thread.start()
        return self

    def pinned_tile(self):
        """The tile handed out last as a flat page-locked torch.uint8 tensor (None when the buffers are plain host memory)."""
        if self._held is None or not self._owners:
            return None
        return self._owners[self._held]

    def copied(self, event) -> None:
        """`event` (anything with synchronize()) is reached when the caller's copy of the tile handed out last is done."""
        if self._held is not None:
            self._events[self._held] = event

    def __next__(self):
        if self._queue is None:
            iter(self)
        if self._held is not None:                         # asking for block i + 1 hands the buffer of block i back: block i + 2 goes there,
            self._free[self._held].release()               # after the event given to copied(), while block i + 1 (filled already) is worked on
            self._held = None
        item = self._queue.get()
        if item is None:
            self._queue.put(None)
            raise StopIteration
        if isinstance(item, BaseException):
            self._queue.put(None)
            raise item
        self._held, s, e, tile = item
        return s, e, tile

    def close(self) -> None:
        self._stop = True
        if self._thread is not None:
            for sem in self._free:
                sem.release()
            self._thread.join()
            self._thread = None
        self._buffers, self._owners = [], []
        if self._d is not None:
            self._L.H5Dclose(self._d)
            self._d = None
        if self._f is not None:
            self._L.H5Fclose(self._f)
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_layer_csr(path: str, layer: str, cell_block: int = 8192, c0: int = 0, c1: Optional[int] = None, engine: str = "hyperslab",
                   threads: Optional[int] = None):
    """A count layer of a .loom file straight into the device CSR form of the atlas path (ops.CsrCounts, cells-major): the
    file is read in blocks of `cell_block` cells (hyperslabs of the genes x cells dataset), each block is transposed and
    compacted on the device, so neither the host nor the device ever holds the dense layer (analysis.py:59-61 loads it
    whole as float64).  c0:c1 restricts to a range of cells (a rank's shard).

    engine="stream" (opt-in) returns the same CsrCounts, bit for bit, by another route: a LayerBlockReader inflates the
    block's chunks on `threads` host threads while the block before it is on the device, and the block goes up in the file's
    element type to be validated, transposed and compacted by the vcy_loom_tile_* kernels (ops.csr_from_tiles)."""
    import torch
    from . import ops
    if engine not in ("hyperslab", "stream"):
        raise ValueError(f"engine must be 'hyperslab' or 'stream', got {engine!r}")
    dev = ops.require_gpu()
    if engine == "stream":
        with LayerBlockReader(path, layer, cell_block, c0, c1, threads) as reader:
            if reader.dtype in ops.LOOM_ELEM and reader.G > 0:        # int8 / int16 / uint64 layers: the kernels do not take them
                return ops.csr_from_tiles(reader)
    G, C = layer_shape(path, layer)
    c1 = C if c1 is None else c1
    ptr, idx, dat = [torch.zeros(1, dtype=torch.int64, device=dev)], [], []
    base, wide = 0, False
    for s in range(c0, c1, cell_block):
        e = min(c1, s + cell_block)
        blk = read_layer_block(path, layer, s, e)
        if blk.dtype.kind == "f":
            if not np.array_equal(blk, np.rint(blk)):
                raise ValueError(f"layer {layer} holds non-integer values: not a count layer")
        if blk.size and (blk.min() < 0 or blk.max() > 65535):
            raise ValueError(f"layer {layer}: counts outside 0..65535 cannot be held as uint16")
        t = torch.from_numpy(np.ascontiguousarray(blk.astype(np.int32))).to(dev).t().contiguous()          # (cells, genes)
        nz = t != 0
        cnt = nz.sum(1)
        ptr.append(base + torch.cumsum(cnt, 0))
        base += int(cnt.sum())
        idx.append(torch.nonzero(nz, as_tuple=False)[:, 1].to(torch.int32))
        vals = t[nz]
        wide = wide or bool(vals.numel() and int(vals.max()) > 255)
        dat.append(vals)
    cat = lambda xs, dt: torch.cat(xs) if xs else torch.empty(0, dtype=dt, device=dev)
    vals = cat(dat, torch.int32)
    data = vals.to(torch.int16) if wide else vals.to(torch.uint8)                                     # int16 holds the uint16 bit pattern
    return ops.CsrCounts(torch.cat(ptr), cat(idx, torch.int32), data, G)


def write_loom(path: str, layers: Dict[str, np.ndarray], col_attrs: Optional[Dict[str, np.ndarray]] = None,
               row_attrs: Optional[Dict[str, np.ndarray]] = None, matrix: Optional[np.ndarray] = None,
               chunks: Optional[Tuple[int, int]] = None, compression: Optional[int] = None, shuffle: bool = False) -> None:
    """Write the layout velocyto's counting pipeline produces (commands/_run.py:283-297): /matrix float32,
    /layers/<name>, /row_attrs/<name>, /col_attrs/<name> (numeric or fixed-length string arrays).
    chunks=(genes, cells): /matrix and the layers are written chunked (the shape clipped to the dataset's), with gzip at level
    `compression` if given and the byte shuffle in front of it if `shuffle` - what loompy writes ((64, 64), gzip 2).  The
    defaults write contiguous datasets, as before."""
    L = _lib()
    if chunks is None and (compression or shuffle):
        raise ValueError("compression and shuffle need chunks=(genes, cells)")
    f = _check(L.H5Fcreate(path.encode(), H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT), f"create {path}")

    def put(parent, name, arr, chunked=False):
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
        dcpl = H5P_DEFAULT
        if chunked and chunks is not None and arr.ndim == 2 and arr.size:
            dcpl = _check(L.H5Pcreate(hid_t.in_dll(L, "H5P_CLS_DATASET_CREATE_ID_g").value), "H5Pcreate")
            ch = (hsize_t * 2)(max(1, min(int(chunks[0]), arr.shape[0])), max(1, min(int(chunks[1]), arr.shape[1])))
            _check(L.H5Pset_chunk(dcpl, 2, ch), "H5Pset_chunk")
            if shuffle:
                _check(L.H5Pset_shuffle(dcpl), "H5Pset_shuffle")
            if compression:
                _check(L.H5Pset_deflate(dcpl, min(int(compression), 9)), "H5Pset_deflate")
        d = _check(L.H5Dcreate2(parent, name.encode(), tp, sp, H5P_DEFAULT, dcpl, H5P_DEFAULT), f"create {name}")
        if dcpl != H5P_DEFAULT:
            L.H5Pclose(dcpl)
        _check(L.H5Dwrite(d, tp, H5S_ALL, H5S_ALL, H5P_DEFAULT, arr.ctypes.data), f"write {name}")
        L.H5Dclose(d)
        L.H5Sclose(sp)
        if arr.dtype.kind == "S":
            L.H5Tclose(tp)

    try:
        first = next(iter(layers.values()))
        put(f, "matrix", np.asarray(matrix if matrix is not None else sum(np.asarray(v, dtype=np.float32) for v in layers.values()), dtype=np.float32), True)
        for grp, items in (("layers", layers), ("col_attrs", col_attrs or {"CellID": np.arange(first.shape[1])}),
                           ("row_attrs", row_attrs or {"Gene": np.arange(first.shape[0])})):
            g = _check(L.H5Gcreate2(f, grp.encode(), H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), f"create group {grp}")
            for k, v in items.items():
                put(g, k, v, grp == "layers")
            L.H5Gclose(g)
    finally:
        L.H5Fclose(f)


# ----------------------------------------------------------------------------------------------------------
# Flat HDF5 dump / load of a dict of arrays: the container format of velocyto/serialization.py:44-115
# (every ndarray attribute -> a dataset under its name; anything else -> pickle + zlib -> uint8 dataset "&name").
def hdf5_dump(path: str, arrays: Dict[str, np.ndarray], compression: int = 0, chunks: Tuple[int, int] = (2048, 2048)) -> None:
    """compression > 0: 2-d numeric datasets are written chunked (`chunks`, clipped to the shape) with gzip at that level,
    like serialization.dump_hdf5's data_compression / chunks (serialization.py:44-92)."""
    L = _lib()
    f = _check(L.H5Fcreate(path.encode(), H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT), f"create {path}")
    try:
        for name, arr in arrays.items():
            arr = np.asarray(arr)
            if arr.dtype.kind in ("U", "O"):
                arr = np.char.encode(arr.astype(str), "utf-8")
            is_bool = arr.dtype == np.bool_
            if is_bool:
                arr = arr.astype(np.int8)
            arr = np.ascontiguousarray(arr)
            nd = max(arr.ndim, 1)
            shape = arr.shape if arr.ndim else (1,)
            dims = (hsize_t * nd)(*shape)
            sp = L.H5Screate_simple(nd, dims, None)
            if is_bool:
                # the 8-bit enum h5py uses for numpy bools, so that masks come back as bool arrays (and checkpoints stay
                # interchangeable with files written through h5py by the reference)
                tp = _check(L.H5Tenum_create(L._native["INT8"]), "H5Tenum_create")
                for label, val in ((b"FALSE", 0), (b"TRUE", 1)):
                    v = ctypes.c_int8(val)
                    _check(L.H5Tenum_insert(tp, label, ctypes.byref(v)), "H5Tenum_insert")
            elif arr.dtype.kind == "S":
                tp = L.H5Tcopy(L._c_s1)
                L.H5Tset_size(tp, max(arr.dtype.itemsize, 1))
            elif arr.dtype in _NP2H5:
                tp = L._native[_NP2H5[arr.dtype]]
            else:
                raise TypeError(f"{name}: dtype {arr.dtype} cannot be stored")
            dcpl = H5P_DEFAULT
            if compression > 0 and arr.ndim == 2 and arr.size and arr.dtype.kind != "S":
                dcpl = _check(L.H5Pcreate(hid_t.in_dll(L, "H5P_CLS_DATASET_CREATE_ID_g").value), "H5Pcreate")
                ch = (hsize_t * 2)(min(int(chunks[0]), arr.shape[0]), min(int(chunks[1]), arr.shape[1]))
                _check(L.H5Pset_chunk(dcpl, 2, ch), "H5Pset_chunk")
                _check(L.H5Pset_deflate(dcpl, min(int(compression), 9)), "H5Pset_deflate")
            d = _check(L.H5Dcreate2(f, name.encode(), tp, sp, H5P_DEFAULT, dcpl, H5P_DEFAULT), f"create {name}")
            if dcpl != H5P_DEFAULT:
                L.H5Pclose(dcpl)
            if arr.size:
                _check(L.H5Dwrite(d, tp, H5S_ALL, H5S_ALL, H5P_DEFAULT, arr.ctypes.data), f"write {name}")
            L.H5Dclose(d)
            L.H5Sclose(sp)
            if arr.dtype.kind == "S" or is_bool:
                L.H5Tclose(tp)
    finally:
        L.H5Fclose(f)


def hdf5_load(path: str) -> Dict[str, np.ndarray]:
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    L = _lib()
    f = _check(L.H5Fopen(path.encode(), H5F_ACC_RDONLY, H5P_DEFAULT), f"open {path}")
    try:
        g, names = _group_members(L, f, "/")
        out = {k: _read_dataset(L, f, k) for k in names}
        if g is not None:
            L.H5Gclose(g)
        return out
    finally:
        L.H5Fclose(f)
