"""The f64 matrix-core kernels of perform_PCA (csrc/gram.hip: vcy_col_means, vcy_gram, vcy_gram_tn, vcy_gemm_nt) at their tile, slab and
split edges, against the extended-precision oracle of tests/pca_cases.py.

Bars.  Integer cases: bit for bit the int64 result, in both storage types and every kernel form.  Real-valued cases (the recipe of
test_gpu_preprocess.py, and an ill-conditioned set with mean 1e6 and spread 1): |got - reference| <= the bound derived in pca_cases's
docstring, entry by entry; the worst error / bound is printed per kernel.  Symmetric bits of the Gram matrix, run-to-run identity, free
output and operand pitches at the C ABI with sentinels beside what is written, the documented rejections, the cell split actually taken,
NaN / inf locality, and the kernel forms behind VCY_GRAM_DMA=0 and VCY_GEMM_NT_SHAPE=1, 2, 3 (one child process each)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pca_cases as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["float64", "float32"]
WORST = {}                                                            # kernel / form -> worst error / bound seen in this run


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd  # noqa: F401
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def _dev(ops, a):
    return None if a is None else torch.as_tensor(np.array(a), device=ops.require_gpu())


def _gram_checks(ops, C, G, L, dtype, kinds, form="dma"):
    """gram and gram_tn of one case in the given kinds, centred and (integer cases, and the recipe below the split) uncentred; returns
    the worst ratios."""
    worst = {"gram": 0.0, "gram_tn": 0.0}
    for kind in kinds:
        for centred in ((True, False) if kind == "exact" or (kind == "recipe" and C < 2048) else (True,)):
            got = pc.run_gram_case(ops, torch, C, G, L, kind, dtype, centred)
            exp = pc.gram_expect(C, G, L, kind, dtype, centred)
            what = f"C={C} G={G} L={L} {kind} {dtype} centred={centred}"
            worst["gram"] = max(worst["gram"], pc.check(got["gram"], exp["gram"], "gram " + what))
            worst["gram_tn"] = max(worst["gram_tn"], pc.check(got["tn"], exp["tn"], "gram_tn " + what))
            assert pc.same_bits(got["gram"], got["gram"].T), f"gram {what}: the two triangles differ in their bits"
            if kind == "recipe" and centred:
                again = pc.run_gram_case(ops, torch, C, G, L, kind, dtype, centred)
                assert pc.same_bits(again["gram"], got["gram"]) and pc.same_bits(again["tn"], got["tn"]), f"{what}: not run-to-run identical"
    for k, v in worst.items():
        _note(f"{k} ({form})", v)
    return worst


# ------------------------------------------------------------------------------------------------------------------------ col_means
@pytest.mark.parametrize("dtype", DTYPES)
def test_col_means(ops, dtype):
    """C around the 64 partial blocks, G around the 256-gene workgroup; the row padding is NaN (never read).  Integer columns: the sum is
    exact and the division the only rounding, so the mean is numpy's sum / C bit for bit."""
    worst = 0.0
    for C, G in pc.MEANS:
        for kind in pc.KINDS:
            X = pc.means_inputs(C, G, kind, dtype)
            M = pc.cell_matrix(ops, torch, X, dtype)
            assert M.ld > G and bool(torch.isnan(M.t[:, G:]).all())
            got = ops.col_means(M).cpu().numpy()
            assert pc.same_bits(ops.col_means(M).cpu().numpy(), got)
            if kind == "exact":
                assert pc.same_bits(got, X.astype(np.int64).sum(0).astype(np.float64) / C), (C, G)
            else:
                ref, S = pc.col_means_reference(X)
                worst = max(worst, pc.check(got, (ref, pc.col_means_bound(S, C)), f"col_means C={C} G={G} {kind} {dtype}"))
    _note("col_means", worst)
    print(f"col_means {dtype}: worst error / bound {worst:.3g}")
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------------- gram and gram_tn
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", pc.SMALL_C)
def test_gram_small_cell_counts(ops, dtype, C):
    """Every exit of the double-buffer loop (C modulo 32) at G = 1, 2, 127, 128, 129, 257 (and 513 with C = 33: 15 triangular tiles),
    the thin block at L around the 64- / 128-column tile switch.  NaN in the row padding of X."""
    cases = [c for c in pc.GRAM_SMALL if c[0] == C]
    assert len(cases) == len(pc.SMALL_G) + (C == 33)
    worst = {"gram": 0.0, "gram_tn": 0.0}
    for _, G, L in cases:
        w = _gram_checks(ops, C, G, L, dtype, pc.KINDS)
        worst = {k: max(worst[k], w[k]) for k in worst}
    print(f"gram C={C} {dtype}: worst error / bound {worst['gram']:.3g} (gram), {worst['gram_tn']:.3g} (gram_tn) over {len(cases)} shapes")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,G,Ls", pc.GRAM_SPLIT)
def test_gram_cell_split(ops, dtype, C, G, Ls):
    """The cells split over two or three workgroups per tile, partials folded by k_gram_reduce: the first cell count that splits, splits
    that end on a slab and one cell past it, two -> three splits."""
    lib = ops._lib.lib()
    assert int(lib.vcy_gram_workspace_bytes(C, G, G, 1)) == (3 if C >= 3072 else 2) * G * G * 8, "the Gram product of this case must take the split"
    worst = {"gram": 0.0, "gram_tn": 0.0}
    for L in Ls:
        w = _gram_checks(ops, C, G, L, dtype, ("exact", "recipe") + (("ill",) if C in (2049, 3073) else ()))
        worst = {k: max(worst[k], w[k]) for k in worst}
    print(f"split C={C} {dtype}: worst error / bound {worst['gram']:.3g} (gram), {worst['gram_tn']:.3g} (gram_tn), L = {Ls}")


def test_split_actually_taken(ops):
    """The split count read back from vcy_gram_workspace_bytes (ks G L 8 bytes of partials wherever that exceeds the 64 G 8 bytes of the
    column-mean partials): G = 130 splits in two from 2048 cells on and in three at 3072.  For thin blocks whose partials are smaller
    than the means buffer (130 x 1: 3 x 1040 bytes) the count cannot be read back; those cases are held by their results alone."""
    lib = ops._lib.lib()
    G = 130
    means = 64 * G * 8

    def splits(C, L, sym):
        b = int(lib.vcy_gram_workspace_bytes(C, G, L, int(sym)))
        assert b >= means
        if b == means:
            return None
        assert b % (G * L * 8) == 0
        return b // (G * L * 8)

    for C in (1, 1024, 2047):
        assert splits(C, G, True) is None and splits(C, 129, False) is None
    for C in (2048, 2049, 2081, 3000, 3071):
        assert splits(C, G, True) == 2 and splits(C, 129, False) == 2 and splits(C, 128, False) == 2 and splits(C, 65, False) == 2, C
        assert splits(C, 1, False) is None
    for C in (3072, 3073):
        assert splits(C, G, True) == 3 and splits(C, 129, False) == 3 and splits(C, 64, False) == 3, C


# ---------------------------------------------------------------------------------------------------------------------------- gemm_nt
@pytest.mark.parametrize("ta,tb", pc.TYPE_PAIRS)
def test_gemm_nt(ops, ta, tb):
    """M around the 64- / 128-row tiles, N around the shape pick and the columns of tiles, K = 1 .. 11 slabs of 16 (f64 A) or 32 (f32 A)
    genes against the two or three slab buffers; with the three corrections and without; into a column block of a wider buffer."""
    worst = 0.0
    for M, N, K in pc.GEMM_NT:
        for kind in pc.KINDS:
            for corrected in ((True, False) if kind == "exact" else (True,)):
                what = f"gemm_nt M={M} N={N} K={K} {kind} {ta} x {tb} corrected={corrected}"
                got = pc.run_gemm_case(ops, torch, M, N, K, kind, ta, tb, corrected)
                worst = max(worst, pc.check(got, pc.gemm_expect(M, N, K, kind, ta, tb, corrected), what))
                if kind == "recipe":
                    wide = torch.full((M, N + 3), 7.0, dtype=torch.float64, device=ops.require_gpu())
                    pc.run_gemm_case(ops, torch, M, N, K, kind, ta, tb, corrected, out=wide[:, :N])
                    w = wide.cpu().numpy()
                    assert pc.same_bits(w[:, :N], got) and (w[:, N:] == 7.0).all(), what + ": strided output / not run-to-run identical"
    _note("gemm_nt (default shapes)", worst)
    print(f"gemm_nt {ta} x {tb}: worst error / bound {worst:.3g} over {len(pc.GEMM_NT)} shapes")


# -------------------------------------------------------------------------------------------------------------------- at the C ABI
def _guarded_workspace(ops, nbytes, guard=8192):
    """A workspace of exactly nbytes inside a larger allocation, all of it NaN (0xff bytes): returns (pointer tensor, check())."""
    buf = torch.full((nbytes + guard,), 0xFF, dtype=torch.uint8, device=ops.require_gpu())

    def untouched():
        return bool((buf[nbytes:] == 0xFF).all())
    return buf, untouched


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [49, 2065])
def test_free_pitches_at_the_abi(ops, dtype, C):
    """vcy_gram with ldg > G, vcy_gram_tn with Y a column block of a wider buffer (NaN beside it) and ldo > L, without (C = 49) and with
    (C = 2065) the cell split - the partials are compact, the output is not.  The integer case bit for bit, the recipe case bit for bit
    what the wrapper returns; sentinels beside the written columns and behind the workspace survive; the workspace starts as NaN."""
    lib = ops._lib.lib()
    G = 130
    dev = ops.require_gpu()
    for L in (65, 128, 1):
        for kind in ("exact", "recipe"):
            X, mean, Y = pc.gram_inputs(C, G, L, kind, dtype)
            exp = pc.gram_expect(C, G, L, kind, dtype)
            M = pc.cell_matrix(ops, torch, X, dtype, extra=4)
            m = _dev(ops, mean)
            # gram
            ldg = G + 3
            out = torch.full((G, ldg), 7.0, dtype=torch.float64, device=dev)
            nb = int(lib.vcy_gram_workspace_bytes(C, G, G, 1))
            assert (nb > 64 * G * 8) == (C >= 2048)
            ws, untouched = _guarded_workspace(ops, nb)
            rc = lib.vcy_gram(M.t.data_ptr(), m.data_ptr(), out.data_ptr(), ws.data_ptr(), C, G, M.ld, ldg, M.code, ops._stream())
            assert rc == 0, lib.vcy_last_error()
            o = out.cpu().numpy()
            assert (o[:, G:] == 7.0).all() and untouched(), "gram wrote beside its columns or behind its workspace"
            pc.check(o[:, :G].copy(), exp["gram"], f"vcy_gram ldg={ldg} C={C} {kind} {dtype}")
            assert pc.same_bits(o[:, :G], ops.gram(pc.cell_matrix(ops, torch, X, dtype), m).cpu().numpy())
            # gram_tn: Y at columns 2 .. 2 + L of a buffer of an even pitch, NaN around it
            ldy = L + 4 + (L % 2)
            Yb = torch.full((C + 1, ldy), float("nan"), dtype=torch.float64, device=dev)    # (C rows of pitch ldy from column 2 on end inside row C)
            Yb[:C, 2:2 + L] = _dev(ops, Y)
            ldo = L + 3
            out = torch.full((G, ldo), 7.0, dtype=torch.float64, device=dev)
            nb = int(lib.vcy_gram_workspace_bytes(C, G, L, 0))
            ws, untouched = _guarded_workspace(ops, nb)
            rc = lib.vcy_gram_tn(M.t.data_ptr(), m.data_ptr(), Yb.data_ptr() + 16, out.data_ptr(), ws.data_ptr(), C, G, L, M.ld, ldy, ldo, M.code,
                                 ops._stream())
            assert rc == 0, lib.vcy_last_error()
            o = out.cpu().numpy()
            assert (o[:, L:] == 7.0).all() and untouched(), "gram_tn wrote beside its columns or behind its workspace"
            pc.check(o[:, :L].copy(), exp["tn"], f"vcy_gram_tn ldy={ldy} ldo={ldo} C={C} L={L} {kind} {dtype}")
            assert pc.same_bits(o[:, :L], ops.gram_tn(pc.cell_matrix(ops, torch, X, dtype), m, _dev(ops, Y)).cpu().numpy())


@pytest.mark.parametrize("ta,tb", pc.TYPE_PAIRS)
def test_gemm_nt_free_output_pitch(ops, ta, tb):
    lib = ops._lib.lib()
    dev = ops.require_gpu()
    code = {"float64": ops.F64, "float32": ops.F32}
    for M, N, K in ((65, 129, 33), (129, 64, 81), (257, 1, 17)):
        for kind in ("exact", "recipe"):
            A, B, rc_, cc, c0 = pc.gemm_inputs(M, N, K, kind, ta, tb)
            Am, Bm = pc.cell_matrix(ops, torch, A, ta, pad_nan=False), pc.cell_matrix(ops, torch, B, tb, pad_nan=False, extra=64)
            ldo = N + 5
            out = torch.full((M, ldo), 7.0, dtype=torch.float64, device=dev)
            rd, cd = _dev(ops, rc_), _dev(ops, cc)
            rc = lib.vcy_gemm_nt(Am.t.data_ptr(), Bm.t.data_ptr(), rd.data_ptr(), cd.data_ptr(), c0, out.data_ptr(), M, N, K,
                                 Am.ld, Bm.ld, ldo, code[ta], code[tb], ops._stream())
            assert rc == 0, lib.vcy_last_error()
            o = out.cpu().numpy()
            assert (o[:, N:] == 7.0).all()
            pc.check(o[:, :N].copy(), pc.gemm_expect(M, N, K, kind, ta, tb), f"vcy_gemm_nt ldo={ldo} ldb={Bm.ld} {M}x{N}x{K} {kind} {ta} x {tb}")
            assert pc.same_bits(o[:, :N], pc.run_gemm_case(ops, torch, M, N, K, kind, ta, tb))


def test_documented_rejections(ops):
    """Odd pitches, misaligned pointers, a pitch shorter than whole slabs, f64 A beside f32 B, a missing workspace when a split is taken:
    the error code, the message, and no launch (the output keeps its sentinel)."""
    lib = ops._lib.lib()
    dev = ops.require_gpu()
    st = ops._stream()
    C, G, L = 2048, 130, 66
    X64 = torch.ones((C + 1, 200), dtype=torch.float64, device=dev)
    X32 = torch.ones((C + 1, 200), dtype=torch.float32, device=dev)
    Y = torch.ones((C + 1, 200), dtype=torch.float64, device=dev)      # (every buffer holds whatever pitch a call below states)
    out = torch.full((300, 300), 7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.vcy_gram_workspace_bytes(C, G, G, 1)), dtype=torch.uint8, device=dev)
    assert ws.numel() == 2 * G * G * 8
    p64, p32, py, po, pw = X64.data_ptr(), X32.data_ptr(), Y.data_ptr(), out.data_ptr(), ws.data_ptr()

    def refused(rc, text):
        msg = lib.vcy_last_error()
        assert rc == -1 and text in msg, (rc, msg)

    refused(lib.vcy_gram(p64, None, po, pw, C, G, 199, 300, ops.F64, st), b"gram: rows of X must be 16-byte aligned")
    refused(lib.vcy_gram(p32, None, po, pw, C, G, 198, 300, ops.F32, st), b"gram: rows of X must be 16-byte aligned")
    refused(lib.vcy_gram(p64 + 8, None, po, pw, C, G, 200, 300, ops.F64, st), b"gram: rows of X must be 16-byte aligned")
    refused(lib.vcy_gram(p64, None, po, pw, C, G, 200, G - 1, ops.F64, st), b"gram: bad shape")
    refused(lib.vcy_gram(p64, None, po, None, C, G, 200, 300, ops.F64, st), b"gram: workspace missing")
    refused(lib.vcy_gram_tn(p64, None, py, po, None, C, G, 129, 200, 130, 300, ops.F64, st), b"gram: workspace missing")
    refused(lib.vcy_gram_tn(p64, None, py, po, pw, C, G, L, 199, 70, 300, ops.F64, st), b"gram_tn: rows of X must be 16-byte aligned")
    refused(lib.vcy_gram_tn(p64, None, py, po, pw, C, G, L, 200, 67, 300, ops.F64, st), b"gram_tn: Y must be")
    refused(lib.vcy_gram_tn(p64, None, py + 8, po, pw, C, G, L, 200, 70, 300, ops.F64, st), b"gram_tn: Y must be")
    refused(lib.vcy_gram_tn(p64, None, py, po, pw, C, G, L, 200, 64, 300, ops.F64, st), b"gram_tn: Y must be")
    refused(lib.vcy_gram_tn(p64, None, None, po, pw, C, G, L, 200, 70, 300, ops.F64, st), b"gram_tn: Y must be")
    gn = lambda a, b, K, lda, ldb, ca, cb, ldo=300: lib.vcy_gemm_nt(a, b, None, None, 0.0, po, 100, 100, K, lda, ldb, ldo, ca, cb, st)
    refused(gn(p64, p64, 17, 30, 200, ops.F64, ops.F64), b"gemm_nt: both row pitches must hold whole slabs")
    refused(gn(p64, p64, 17, 200, 16, ops.F64, ops.F64), b"gemm_nt: both row pitches must hold whole slabs")
    refused(gn(p32, p32, 33, 48, 200, ops.F32, ops.F32), b"gemm_nt: both row pitches must hold whole slabs")
    refused(gn(p64, p32, 17, 200, 200, ops.F64, ops.F32), b"gemm_nt: A is f32 or f64, B of A's type or f64")
    refused(gn(p64, p64, 17, 199, 200, ops.F64, ops.F64), b"gemm_nt: rows must be 16-byte aligned")
    refused(gn(p32, p64, 17, 198, 200, ops.F32, ops.F64), b"gemm_nt: rows must be 16-byte aligned")
    refused(gn(p64 + 8, p64, 17, 200, 200, ops.F64, ops.F64), b"gemm_nt: rows must be 16-byte aligned")
    refused(gn(p32, p32 + 8, 17, 200, 200, ops.F32, ops.F32), b"gemm_nt: rows must be 16-byte aligned")
    refused(gn(p64, p64, 17, 200, 200, ops.F64, ops.F64, ldo=99), b"gemm_nt: bad shape")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote to its output"


# ------------------------------------------------------------------------------------------------------------------ NaN and inf
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,cells", [(49, (5, 48)), (2065, (5, 2064))])
def test_nan_locality(ops, dtype, C, cells):
    """One NaN at an interior (c, i) - in the first slab of the first split, then in the tail slab of the last (one valid cell) - turns
    exactly row i and column i of the Gram matrix, row i of the thin product and row i of gemm_nt into NaN; every other entry keeps the
    bits of the clean run: a column of the operands only reaches its own row / column."""
    G, L, i = 130, 65, 77
    X, mean, Y = pc.gram_inputs(C, G, L, "recipe", dtype)
    m, Yd = _dev(ops, mean), _dev(ops, Y)
    clean = pc.cell_matrix(ops, torch, X, dtype)
    g0, t0 = ops.gram(clean, m).cpu().numpy(), ops.gram_tn(clean, m, Yd).cpu().numpy()
    assert np.isfinite(g0).all() and np.isfinite(t0).all()
    for c in cells:
        M = pc.cell_matrix(ops, torch, X, dtype)
        M.t[c, i] = float("nan")
        g, t = ops.gram(M, m).cpu().numpy(), ops.gram_tn(M, m, Yd).cpu().numpy()
        want = np.zeros((G, G), bool)
        want[i, :] = want[:, i] = True
        assert np.array_equal(np.isnan(g), want), (c, np.argwhere(np.isnan(g) != want)[:5])
        assert pc.same_bits(np.where(want, 0.0, g), np.where(want, 0.0, g0)), f"NaN at cell {c} changed entries outside row / column {i}"
        assert np.array_equal(np.isnan(t), np.broadcast_to((np.arange(G) == i)[:, None], t.shape))
        assert pc.same_bits(np.delete(t, i, 0), np.delete(t0, i, 0))
    # gemm_nt: A (C2, K) with one NaN at (i, g): row i
    ta = dtype
    for (Mr, N, K), (i2, g) in (((129, 65, 81), (70, 80)), ((257, 129, 33), (256, 0))):
        A, B, rc, cc, c0 = pc.gemm_inputs(Mr, N, K, "recipe", ta, "float64")
        Am = pc.cell_matrix(ops, torch, A, ta, pad_nan=False)
        Bd = _dev(ops, B)
        o0 = ops.gemm_nt(Am, Bd, row_corr=_dev(ops, rc), col_corr=_dev(ops, cc), c0=c0).cpu().numpy()
        Am.t[i2, g] = float("nan")
        o = ops.gemm_nt(Am, Bd, row_corr=_dev(ops, rc), col_corr=_dev(ops, cc), c0=c0).cpu().numpy()
        assert np.isfinite(o0).all() and np.array_equal(np.isnan(o), np.broadcast_to((np.arange(Mr) == i2)[:, None], o.shape))
        assert pc.same_bits(np.delete(o, i2, 0), np.delete(o0, i2, 0))


def test_infinities_follow_ieee(ops):
    """+inf at two cells of one column, one of them the only valid cell of the tail slab (whose clamped copies are zeroed, not
    multiplied): an entry whose two infinite terms agree in sign is that infinity, one whose terms disagree is NaN - as numpy's fp64
    sum of the same terms says; every other entry keeps its bits."""
    C, G, L, i = 49, 130, 65, 77
    X, mean, Y = pc.gram_inputs(C, G, L, "recipe", "float64")
    m, Yd = _dev(ops, mean), _dev(ops, Y)
    clean = pc.cell_matrix(ops, torch, X, "float64")
    g0, t0 = ops.gram(clean, m).cpu().numpy(), ops.gram_tn(clean, m, Yd).cpu().numpy()
    Xi = X.copy()
    Xi[[7, 48], i] = np.inf
    M = pc.cell_matrix(ops, torch, Xi, "float64")
    g, t = ops.gram(M, m).cpu().numpy(), ops.gram_tn(M, m, Yd).cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        A = Xi - mean[None, :]
        row_g = (A[:, i:i + 1] * A).sum(0)
        row_t = (A[:, i:i + 1] * Y).sum(0)
    assert np.isnan(row_g).any() and np.isposinf(row_g).any() and np.isneginf(row_g).any() and np.isposinf(row_g[i])
    cls = lambda v: np.where(np.isnan(v), 2, np.where(np.isposinf(v), 1, np.where(np.isneginf(v), -1, 0)))
    assert np.array_equal(cls(g[i]), cls(row_g)) and np.array_equal(cls(g[:, i]), cls(row_g)) and np.array_equal(cls(t[i]), cls(row_t))
    keep = np.ones((G, G), bool)
    keep[i, :] = keep[:, i] = False
    assert pc.same_bits(np.where(keep, g, 0.0), np.where(keep, g0, 0.0)) and pc.same_bits(np.delete(t, i, 0), np.delete(t0, i, 0))


# ------------------------------------------------------------------------------------------------------------ the other kernel forms
def _child(tmp_path, env, what):
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pca_products_worker.py"), out, what], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


def test_register_staged_gram(ops, tmp_path):
    """VCY_GRAM_DMA=0: k_gram, the slabs staged through registers and centred on the way into LDS - every integer case bit for bit, the
    thinned real-valued list within the bounds."""
    got = _child(tmp_path, {"VCY_GRAM_DMA": "0"}, "gram")
    worst = {"gram": 0.0, "tn": 0.0}
    n = 0
    for C, G, L, kind, dtype in pc.worker_gram_jobs():
        for centred in ((True, False) if kind == "exact" else (True,)):
            exp = pc.gram_expect(C, G, L, kind, dtype, centred)
            for name in ("gram", "tn"):
                what = f"register-staged {name} C={C} G={G} L={L} {kind} {dtype} centred={centred}"
                worst[name] = max(worst[name], pc.check(got[pc.key(name, C, G, L, kind, dtype, int(centred))], exp[name], what))
                n += 1
            g = got[pc.key("gram", C, G, L, kind, dtype, int(centred))]
            assert pc.same_bits(g, g.T)
    _note("gram (register-staged)", worst["gram"])
    _note("gram_tn (register-staged)", worst["tn"])
    print(f"VCY_GRAM_DMA=0: {n} results; worst error / bound {worst['gram']:.3g} (gram), {worst['tn']:.3g} (gram_tn)")


@pytest.mark.parametrize("shape", [1, 2, 3])
def test_gemm_nt_tile_shapes(ops, tmp_path, shape):
    """VCY_GEMM_NT_SHAPE = 1 (64 rows x 128-byte slab rows x 3 buffers, for every N), 2 and 3 (256-byte slab rows, 2 / 3 buffers: the
    64-element row padding of CellMatrix always holds them; pitches of exactly one 128-byte slab are refused, with the message and no
    launch)."""
    got = _child(tmp_path, {"VCY_GEMM_NT_SHAPE": str(shape)}, "gemm_nt")
    worst, n = 0.0, 0
    for M, N, K, kind, ta, tb in pc.worker_gemm_jobs():
        for corrected in ((True, False) if kind == "exact" else (True,)):
            what = f"shape {shape} gemm_nt M={M} N={N} K={K} {kind} {ta} x {tb} corrected={corrected}"
            worst = max(worst, pc.check(got[pc.key("gemm_nt", M, N, K, kind, ta, tb, int(corrected))], pc.gemm_expect(M, N, K, kind, ta, tb, corrected), what))
            n += 1
    for dtype, K in (("float64", 16), ("float32", 32)):
        rc, msg, out = int(got[pc.key("narrow", dtype, "rc")]), bytes(got[pc.key("narrow", dtype, "msg")]), got[pc.key("narrow", dtype, "out")]
        if shape == 1:
            assert rc == 0 and (out == float(K)).all()
        else:
            assert rc == -1 and b"gemm_nt: VCY_GEMM_NT_SHAPE asks for 256-byte slab rows the pitches do not hold" in msg and (out == 7.0).all()
    _note(f"gemm_nt (shape {shape})", worst)
    print(f"VCY_GEMM_NT_SHAPE={shape}: {n} results; worst error / bound {worst:.3g}")


def test_worst_ratios(ops):
    """The worst error / bound of every kernel and form this run met (the tests above fail on any entry above 1)."""
    for name in sorted(WORST):
        print(f"worst error / bound, {name}: {WORST[name]:.3g}")
    assert all(v <= 1.0 for v in WORST.values())
