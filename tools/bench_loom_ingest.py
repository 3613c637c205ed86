"""What reading a .loom count layer costs, the streamed ingest beside the route it is an alternative to, measured in one process.
Writes profiles/loom_ingest.txt (or OUT=...).
usage: python tools/bench_loom_ingest.py write        # the synthetic files, once, under the system temp directory (or DIR=...)
       python tools/bench_loom_ingest.py              # the measurement (needs the files and a GPU)
       [G=30000] [CELLS=65536] [FACADE_CELLS=16384] [BLOCK=8192] [REPS=5] [ONLY=engines,parts,facade]

files:   layer.loom   /layers/spliced, G x CELLS uint16, chunks (64, 64), gzip 2, gamma-Poisson counts at about 8 % density
         facade.loom  /layers/spliced + unspliced, G x FACADE_CELLS, the same storage, plus the two attribute groups
engines: loom_io.read_layer_csr(engine="hyperslab") - the code as it was, the baseline - and engine="stream", alternating, two runs each,
         the file in the page cache for both (it is read once before the first timed run).  Wall seconds around the call, which ends
         in a device synchronise; inflated GB/s = G x CELLS x 2 bytes over that.  The two results are compared (torch.equal).
parts:   on the first block of BLOCK cells, each on its own -
           lookup + read: H5Dget_chunk_storage_size and H5Dread_chunk per chunk from Python, one thread (the ctypes overhead is in it);
           block fill: vcy_loom_block_host (lookup, read, inflate, place) at 1 / 4 / 8 / 16 threads, wall seconds, inflated GB/s;
           the same block filled by a Python loop (zlib.decompress + a numpy placement per chunk, the stored bytes fetched beforehand) on
           a thread pool of 1 / 4 / 8 threads - the form vcy_loom_block_host replaced;
           upload: the page-locked tile to the device, device events;
           kernels: vcy_loom_tile_count, _fill, _dense, device events, median of REPS after a warm-up, with the bytes each must move
           (count: the tile; fill: the tile + 6 B per non-zero; dense: the tile + the uint16 rows) over the time, beside the 6.29 TB/s
           a float4 copy reaches on this part (8 TB/s peak).
facade:  VelocytoLoom(path) with ingest="whole" and ingest="stream" on facade.loom, alternating, two runs each, wall seconds.
The 1M-cell figure at the end is an extrapolation (time per cell x 1e6), not a measurement."""
import ctypes
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from velocyto_amd import loom_io

G = int(os.environ.get("G", 30000))
CELLS = int(os.environ.get("CELLS", 65536))
FACADE_CELLS = int(os.environ.get("FACADE_CELLS", 16384))
BLOCK = int(os.environ.get("BLOCK", 8192))
REPS = int(os.environ.get("REPS", 5))
ONLY = [w for w in os.environ.get("ONLY", "engines,parts,facade").split(",") if w]       # sections to run
DIR = os.environ.get("DIR", os.path.join(tempfile.gettempdir(), "velocyto_amd_loom_ingest"))
LAYER, FACADE = os.path.join(DIR, "layer.loom"), os.path.join(DIR, "facade.loom")
HBM_COPY = 6.29e12


def synth(rng, genes, cells, mean):
    """gamma-Poisson counts: a gene's rate is gamma distributed, a cell's depth log-normal; about 8 % of the entries are non-zero at mean 0.1"""
    rate = rng.gamma(0.3, mean / 0.3, genes)[:, None] * rng.lognormal(0.0, 0.4, cells)[None, :]
    return np.minimum(rng.poisson(rate), 65535).astype(np.uint16)


def write_layers(path, layers, cells, attrs):
    """the layers written in blocks of 4096 cells (hyperslabs), so the host never holds a whole layer"""
    L, hs = loom_io._lib(), loom_io.hsize_t
    f = loom_io._check(L.H5Fcreate(path.encode(), loom_io.H5F_ACC_TRUNC, 0, 0), "create")
    g = L.H5Gcreate2(f, b"layers", 0, 0, 0)
    rng = np.random.default_rng(2024)
    nnz = 0
    for name, mean in layers:
        sp = L.H5Screate_simple(2, (hs * 2)(G, cells), None)
        dcpl = L.H5Pcreate(loom_io.hid_t.in_dll(L, "H5P_CLS_DATASET_CREATE_ID_g").value)
        L.H5Pset_chunk(dcpl, 2, (hs * 2)(64, 64))
        L.H5Pset_deflate(dcpl, 2)
        d = loom_io._check(L.H5Dcreate2(g, name.encode(), L._native["UINT16"], sp, 0, dcpl, 0), "create layer")
        for s in range(0, cells, 4096):
            e = min(cells, s + 4096)
            blk = synth(rng, G, e - s, mean)
            nnz += int(np.count_nonzero(blk))
            fsp = L.H5Dget_space(d)
            L.H5Sselect_hyperslab(fsp, loom_io.H5S_SELECT_SET, (hs * 2)(0, s), None, (hs * 2)(G, e - s), None)
            msp = L.H5Screate_simple(2, (hs * 2)(G, e - s), None)
            loom_io._check(L.H5Dwrite(d, L._native["UINT16"], msp, fsp, 0, blk.ctypes.data), "write block")
            L.H5Sclose(msp); L.H5Sclose(fsp)
        L.H5Dclose(d); L.H5Pclose(dcpl); L.H5Sclose(sp)
    L.H5Gclose(g)
    L.H5Fclose(f)
    if attrs:
        f = L.H5Fopen(path.encode(), 1, 0)                                       # H5F_ACC_RDWR
        for grp, name, n in (("col_attrs", "CellID", cells), ("row_attrs", "Gene", G)):
            gg = L.H5Gcreate2(f, grp.encode(), 0, 0, 0)
            arr = np.arange(n, dtype=np.int64)
            sp = L.H5Screate_simple(1, (hs * 1)(n), None)
            d = L.H5Dcreate2(gg, name.encode(), L._native["INT64"], sp, 0, 0, 0)
            L.H5Dwrite(d, L._native["INT64"], 0, 0, 0, arr.ctypes.data)
            L.H5Dclose(d); L.H5Sclose(sp); L.H5Gclose(gg)
        L.H5Fclose(f)
    return nnz


def write_files():
    os.makedirs(DIR, exist_ok=True)
    for path, layers, cells, attrs in ((LAYER, (("spliced", 0.1),), CELLS, False), (FACADE, (("spliced", 0.1), ("unspliced", 0.04)), FACADE_CELLS, True)):
        if os.path.exists(path) and loom_io.layer_shape(path, "spliced") == (G, cells):
            print(f"{path}: already there", flush=True)
            continue
        t0 = time.perf_counter()
        nnz = write_layers(path, layers, cells, attrs)
        print(f"{path}: {G} x {cells}, {len(layers)} layer(s), density {nnz / (G * cells * len(layers)):.3f}, {os.path.getsize(path) / 1e9:.2f} GB on disk, "
              f"written in {time.perf_counter() - t0:.0f} s", flush=True)


def measure():
    import torch
    from velocyto_amd import _lib, analysis, ops
    dev = ops.require_gpu()
    L = _lib.lib()
    OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "loom_ingest.txt"))
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    fh = open(OUT, "w")

    def say(s=""):
        print(s, flush=True)
        fh.write(s + "\n")
        fh.flush()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def dev_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), min(ts), max(ts)

    shape = loom_io.layer_shape(LAYER, "spliced")
    assert shape == (G, CELLS), f"{LAYER} holds {shape}: run `write` with the same G / CELLS"
    raw = G * CELLS * 2
    say(f"# loom ingest: {G} genes x {CELLS} cells uint16, chunks (64, 64), gzip 2; {os.path.getsize(LAYER) / 1e9:.2f} GB stored, {raw / 1e9:.2f} GB inflated; "
        f"{torch.cuda.get_device_name(0)}; host threads available to this process: {len(os.sched_getaffinity(0))}")
    with open(LAYER, "rb") as f:                                              # page cache for both engines
        while f.read(1 << 26):
            pass
    # ---- engines
    say("\n## read_layer_csr, whole layer, alternating (wall seconds; inflated GB/s)")
    res = {}
    for run in range(2 if "engines" in ONLY else 0):
        for engine, kw in (("hyperslab", {}), ("stream", {"threads": 8})):
            t, r = wall(lambda: loom_io.read_layer_csr(LAYER, "spliced", cell_block=BLOCK, engine=engine, **kw))
            res.setdefault(engine, []).append(t)
            say(f"run {run}  engine={engine:9s} {'threads=8' if kw else '         '}  {t:8.2f} s  {raw / 1e9 / t:6.2f} GB/s   nnz {r.nnz}  data {r.data.dtype}")
            if engine == "hyperslab":
                ref = r
            else:
                same = torch.equal(ref.indptr, r.indptr) and torch.equal(ref.indices, r.indices) and torch.equal(ref.data, r.data) and ref.data.dtype == r.data.dtype
                say(f"       stream == hyperslab: {same}")
                assert same
            del r
    torch.cuda.empty_cache()
    for th in (1, 4, 16) if "engines" in ONLY else ():
        t, r = wall(lambda: loom_io.read_layer_csr(LAYER, "spliced", cell_block=BLOCK, engine="stream", threads=th))
        say(f"       engine=stream    threads={th:<2d} {t:8.2f} s  {raw / 1e9 / t:6.2f} GB/s")
        del r
    best = {k: min(v) for k, v in res.items()}
    if best:
        say(f"best of two: hyperslab {best['hyperslab']:.2f} s, stream (8 threads) {best['stream']:.2f} s: x{best['hyperslab'] / best['stream']:.2f}")
    if "parts" in ONLY:
        parts(say, dev_ms, torch, dev, L, _lib, ops)
    # ---- facade
    fshape = loom_io.layer_shape(FACADE, "spliced") if "facade" in ONLY else None
    if fshape:
        facade(say, wall, torch, analysis, fshape)
    if best:
        say(f"\n## extrapolation, not a measurement: a 1M-cell layer of {G} genes at the rates above - hyperslab {best['hyperslab'] / CELLS * 1e6:.0f} s, "
            f"stream (8 threads) {best['stream'] / CELLS * 1e6:.0f} s ({raw / CELLS * 1e6 / 1e9:.0f} GB inflated)")
    fh.close()


def py_fill(tile, chunks, B, threads):
    """the block filled chunk by chunk from Python: what a thread pool gets out of zlib.decompress (which releases the interpreter lock)
    and a numpy placement (which does not) per 8 KB chunk"""
    import zlib
    from concurrent.futures import ThreadPoolExecutor

    def one(c):
        g0, x0, z = c
        a = np.frombuffer(zlib.decompress(z), dtype=np.uint16).reshape(64, 64)
        g1, x1 = min(G, g0 + 64), min(B, x0 + 64)
        tile[g0:g1, x0:x1] = a[: g1 - g0, : x1 - x0]

    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(one, chunks, chunksize=64))


def parts(say, dev_ms, torch, dev, L, _lib, ops):
    B = min(BLOCK, CELLS)
    blk_raw = G * B * 2
    say(f"\n## parts, first block of {B} cells ({blk_raw / 1e6:.0f} MB inflated, {((G + 63) // 64) * ((B + 63) // 64)} chunks)")
    H = loom_io._lib()
    with loom_io.LayerBlockReader(LAYER, "spliced", B, 0, B, 1) as r:
        assert r.direct, r.why_not
        t0 = time.perf_counter()
        at, mask, size = (loom_io.hsize_t * 2)(), ctypes.c_uint32(), loom_io.hsize_t()
        buf = ctypes.create_string_buffer(2 * 64 * 64 * 2 + 4096)
        stored, table = 0, []
        for g0 in range(0, G, 64):
            for x0 in range(0, B, 64):
                at[0], at[1] = g0, x0
                H.H5Dget_chunk_storage_size(r._d, at, ctypes.byref(size))
                H.H5Dread_chunk(r._d, 0, at, ctypes.byref(mask), buf)
                stored += size.value
                table.append((g0, x0, buf.raw[: size.value]))
        t = time.perf_counter() - t0
        say(f"stored bytes of every chunk from Python (H5Dget_chunk_storage_size + H5Dread_chunk), 1 thread: {t:.3f} s for {stored / 1e6:.1f} MB stored")
        for th in (1, 4, 8, 16):
            r.threads = th
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                tile = r._fill(r._buffers[0], 0, B)
                ts.append(time.perf_counter() - t0)
            say(f"block fill (lookup, read, inflate, place), {th:2d} threads: {min(ts):.3f} s  {blk_raw / 1e9 / min(ts):6.2f} GB/s inflated (best of 3)")
        check = tile.copy()
        for th in (1, 4, 8):
            tile[...] = 0
            t0 = time.perf_counter()
            py_fill(tile, table, B, th)
            t = time.perf_counter() - t0
            assert np.array_equal(tile, check)
            say(f"the same block from a Python loop over the chunk table,  {th:2d} threads: {t:.3f} s  {blk_raw / 1e9 / t:6.2f} GB/s inflated")
        del check
        pinned = r._owners[0][:blk_raw] if r._owners else torch.from_numpy(tile.reshape(-1).view(np.uint8))
        d_tile = torch.empty(blk_raw, dtype=torch.uint8, device=dev)
        ms = dev_ms(lambda: d_tile.copy_(pinned, non_blocking=True))
        say(f"upload of the tile: {ms[0]:.2f} ms ({ms[1]:.2f} .. {ms[2]:.2f})  {blk_raw / 1e9 / (ms[0] / 1e3):.1f} GB/s")
    st = ops._stream()
    ws = ops.loom_tile_workspace(ops.padded_ld(G), B, dev)
    nnz, sums = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    result = torch.empty(4, dtype=torch.int64, device=dev)
    count = lambda: _lib.check(L.vcy_loom_tile_count(d_tile.data_ptr(), nnz.data_ptr(), sums.data_ptr(), result.data_ptr(), ws.data_ptr(), G, B, B, 1, st))
    ms = dev_ms(count)
    say(f"vcy_loom_tile_count (3 launches): {ms[0]:.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {blk_raw / 1e9 / (ms[0] / 1e3):7.0f} GB/s of {blk_raw / 1e6:.0f} MB "
        f"= {100 * blk_raw / (ms[0] / 1e3) / HBM_COPY:.0f} % of the copy rate")
    row_start = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    torch.cumsum(nnz, 0, out=row_start[1:])
    total = int(row_start[-1])
    ii, dd = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int16, device=dev)
    ms = dev_ms(lambda: _lib.check(L.vcy_loom_tile_fill(d_tile.data_ptr(), ws.data_ptr(), row_start.data_ptr(), ii.data_ptr(), dd.data_ptr(), total, G, B, B, 1, st)))
    moved = blk_raw + 6 * total
    say(f"vcy_loom_tile_fill ({total} non-zeros): {ms[0]:.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {moved / 1e9 / (ms[0] / 1e3):7.0f} GB/s of {moved / 1e6:.0f} MB "
        f"= {100 * moved / (ms[0] / 1e3) / HBM_COPY:.0f} % of the copy rate")
    ld = ops.padded_ld(G)
    dense = torch.empty((B, ld), dtype=torch.int16, device=dev)
    ms = dev_ms(lambda: _lib.check(L.vcy_loom_tile_dense(d_tile.data_ptr(), dense.data_ptr(), sums.data_ptr(), result.data_ptr(), ws.data_ptr(), G, B, B, 1, 0, B, ld, st)))
    moved = blk_raw + B * ld * 2
    say(f"vcy_loom_tile_dense (3 launches): {ms[0]:.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})  {moved / 1e9 / (ms[0] / 1e3):7.0f} GB/s of {moved / 1e6:.0f} MB "
        f"= {100 * moved / (ms[0] / 1e3) / HBM_COPY:.0f} % of the copy rate")
    del dense, ii, dd, d_tile
    torch.cuda.empty_cache()


def facade(say, wall, torch, analysis, fshape):
    say(f"\n## VelocytoLoom(path), {fshape[0]} x {fshape[1]}, spliced + unspliced, alternating (wall seconds)")
    with open(FACADE, "rb") as f:
        while f.read(1 << 26):
            pass
    fres = {}
    for run in range(2):
        for ingest in ("whole", "stream"):
            t, v = wall(lambda: analysis.VelocytoLoom(FACADE, ingest=ingest))
            fres.setdefault(ingest, []).append(t)
            say(f"run {run}  ingest={ingest:6s} {t:8.2f} s   molecules {int(v.initial_cell_size.sum())}")
            del v
            torch.cuda.empty_cache()
    say(f"best of two: whole {min(fres['whole']):.2f} s, stream {min(fres['stream']):.2f} s: x{min(fres['whole']) / min(fres['stream']):.2f}")


if __name__ == "__main__":
    if "write" in sys.argv[1:]:
        write_files()
    else:
        measure()
