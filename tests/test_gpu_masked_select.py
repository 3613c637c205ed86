"""The masked streamed select (csrc/fit.hip k_select_count<.., MK>, vcy_gene_mselect_*, ops.StreamedMaskedGeneQuantiles) and the
cell-masked weighted moments (vcy_fit_weighted_moments_masked) through `ops`.

Reference: ops.gene_quantiles(M, qs, mask_src=, mask_thr=, mask_mode=) on the whole matrix - for a cell mask, on the gathered rows.
Both are exact selections over the same kept values followed by the same interpolation, so the bar is bit-identical float64 output
with NaN in the same places, no tolerance; the populations are compared with a numpy count.  The data is finite (a kept +inf is the
one place where the whole-matrix form, which stores masked-out entries as +inf, and the streamed form, which skips them, may part).
The masked moments: an all-ones mask gives the unmasked bits; a random mask is within 2 n 2^-53 relative of the moments of the
gathered rows (non-negative terms in two summation orders; n = the kept cells), Sw - a count - exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_T = {"float32": np.float32, "float64": np.float64}
QSETS = ([10], [50], [0, 100], [1, 50, 99.9])
N_PATTERNS = 8


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(got, ref, what):
    bad = (_bits(got) != _bits(ref)).nonzero()
    assert bad.numel() == 0, (what, bad[:5].tolist(), got[tuple(bad[0])].item(), ref[tuple(bad[0])].item())


def constructed(rng, C, G, np_t, first=0):
    """(src, thr): the mask's source (C, G) of np_t and its thresholds (G); gene g holds pattern (g + first) % N_PATTERNS."""
    S = np.zeros((C, G), dtype=np_t)
    thr = np.zeros(G)
    for g in range(G):
        k = (g + first) % N_PATTERNS
        if k == 0:                                                   # threshold above every value: mode 1 keeps no cell, mode 2 all
            col = rng.gamma(1.0, 2.0, C); t = 1e30
        elif k == 1:                                                 # threshold = the maximum: equal values stay out of mode 1, in mode 2
            col = rng.integers(0, 4, C).astype(np.float64); t = float(np.asarray(col, np_t).max())
        elif k == 2:                                                 # all distinct, exactly one cell above the threshold
            col = rng.permutation(C) + 0.5; t = C - 1.0
        elif k == 3:                                                 # a NaN threshold keeps nothing in either mode
            col = rng.gamma(1.0, 2.0, C); t = float("nan")
        elif k == 4:                                                 # -0.0 beside +0.0 at a threshold of +0.0
            col = rng.choice(np.array([-2.0, -0.0, 0.0, 1.0]), C); t = 0.0
        elif k == 5:                                                 # threshold below every value: mode 1 keeps all, mode 2 none
            col = rng.gamma(1.0, 2.0, C); t = -1.0
        elif k == 6:                                                 # expression-like, the threshold is one of the values (ties at it)
            col = np.round(rng.gamma(1.0, 2.0, C) * (rng.random(C) < 0.5), 1); t = float(np.asarray(col, np_t)[rng.integers(C)])
        else:                                                        # both signs, exactly one cell at or below the threshold
            col = rng.permutation(C) - C / 2.0; t = float(col.min())
        S[:, g] = np.asarray(col, dtype=np_t)
        thr[g] = t
    return S, thr


def _blockings(C):
    out = [("whole", [(0, C)])]
    if 1 < C <= 63:
        out.append(("one cell per block", [(c, c + 1) for c in range(C)]))
    if C > 71:
        uneven = [(0, 7), (7, 71), (71, C)]
    elif C > 7:
        uneven = [(0, 7), (7, C)]
    else:
        uneven = [(0, 1), (1, C)] if C > 1 else None
    if uneven:
        out += [("uneven", uneven), ("uneven, reversed", uneven[::-1])]
    return out


def _streamed(ops, M, qs, blocks, src=None, thr=None, mode=0, cells=None):
    sel = ops.StreamedMaskedGeneQuantiles(M.G, qs, M.dtype)
    n = 0
    while not sel.done:
        for (a, b) in blocks:
            sel.add_block(M.rows(a, b), None if src is None else (M.rows(a, b) if src is M else src.rows(a, b)), thr, mode,
                          None if cells is None else cells[a:b])
        sel.advance()
        n += 1
    assert n == sel.passes == (4 if M.dtype == torch.float32 else 8)
    return sel.result(), sel.counts()


def _kept(S, thr, mode, cells=None):
    with np.errstate(invalid="ignore"):
        k = np.ones(S.shape, bool) if mode == 0 else (S.astype(np.float64) > thr[None, :] if mode == 1 else S.astype(np.float64) <= thr[None, :])
    return k if cells is None else k & cells[:, None]


@pytest.mark.parametrize("C", [1, 2, 63, 257, 1000])
@pytest.mark.parametrize("G", [1, 64, 65, 130])
def test_masked_select_equals_gene_quantiles_bit_for_bit(ops, G, C):
    rng = np.random.default_rng(7000 * G + C)
    n_blockings = 0
    for dtype in ("float32", "float64"):
        np_t = NP_T[dtype]
        S_np, thr_np = constructed(rng, C, G, np_t, first=C)
        B_np = np.asarray(rng.gamma(1.0, 1.0, (C, G)) * (rng.random((C, G)) < 0.7) * rng.choice([1.0, 1.0, -1.0], (C, G)), dtype=np_t)
        S, B = ops.CellMatrix.from_cells_major(S_np, dtype), ops.CellMatrix.from_cells_major(B_np, dtype)
        thr = torch.from_numpy(thr_np).cuda()
        for mode in (0, 1, 2):
            for own in ((False,) if mode == 0 else (False, True)):           # own: the mask's source is M itself (read once)
                M, M_np = (S, S_np) if own else (B, B_np)
                kw = dict(mask_src=S, mask_thr=thr, mask_mode=mode) if mode else {}
                n_ref = torch.from_numpy(_kept(S_np, thr_np, mode).sum(0)).cuda()
                for qs in QSETS:
                    ref = ops.gene_quantiles(M, qs, **kw)
                    assert bool((torch.isnan(ref) == (n_ref == 0)[None, :]).all())
                    if mode == 0:
                        plain = ops.StreamedGeneQuantiles(G, qs, C, dtype)
                        while not plain.done:
                            plain.add_block(M)
                            plain.advance()
                        _same(plain.result(), ref, "StreamedGeneQuantiles")
                    for name, blocks in _blockings(C):
                        got, n = _streamed(ops, M, qs, blocks, S if mode and not own else (M if mode else None), thr if mode else None, mode)
                        assert got.shape == (len(qs), G) and got.dtype == torch.float64 and n.dtype == torch.int64
                        assert torch.equal(n, n_ref), (dtype, mode, own, qs, name)
                        _same(got, ref, (dtype, mode, own, qs, name))
                        n_blockings += 1
                # numpy on the kept values, where it is defined: the reference itself is what np.percentile gives
                keep = _kept(S_np, thr_np, mode)
                g = int(np.argmax(keep.sum(0)))
                if keep[:, g].any():
                    want = np.percentile(M_np[keep[:, g], g].astype(np.float64), QSETS[-1])
                    np.testing.assert_allclose(ops.gene_quantiles(M, QSETS[-1], **kw)[:, g].cpu().numpy(), want, rtol=1e-14, atol=0)
    assert n_blockings >= 2 * 5 * len(QSETS)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("C,G", [(257, 65), (1000, 130)])
def test_cell_mask_equals_the_gathered_rows(ops, dtype, C, G):
    """A cell mask alone and together with a value mask, one block removed whole: the reference is the same call on the gathered rows."""
    rng = np.random.default_rng(C + G)
    np_t = NP_T[dtype]
    S_np, thr_np = constructed(rng, C, G, np_t)
    B_np = np.asarray(rng.gamma(1.0, 1.0, (C, G)) * (rng.random((C, G)) < 0.7), dtype=np_t)
    S, B = ops.CellMatrix.from_cells_major(S_np, dtype), ops.CellMatrix.from_cells_major(B_np, dtype)
    thr = torch.from_numpy(thr_np).cuda()
    cells_np = rng.random(C) < 0.5
    cells_np[7:71] = False                                            # the block (7, 71) of the uneven blocking has no cell left
    cells = torch.from_numpy(cells_np).cuda()
    Sg, Bg = ops.select_cells(S, cells), ops.select_cells(B, cells)
    for mode in (0, 1, 2):
        for own in ((False,) if mode == 0 else (False, True)):
            M, Mg = (S, Sg) if own else (B, Bg)
            kw = dict(mask_src=Sg, mask_thr=thr, mask_mode=mode) if mode else {}
            n_ref = torch.from_numpy(_kept(S_np, thr_np, mode, cells_np).sum(0)).cuda()
            for qs in QSETS:
                ref = ops.gene_quantiles(Mg, qs, **kw)
                for name, blocks in _blockings(C):
                    for cm in (cells, cells.to(torch.uint8), cells_np):                       # bool, uint8 and host masks are one mask
                        got, n = _streamed(ops, M, qs, blocks, S if mode and not own else (M if mode else None), thr if mode else None, mode, cm)
                        assert torch.equal(n, n_ref), (mode, own, qs, name)
                        _same(got, ref, (mode, own, qs, name))
                        if name != "whole" or qs != QSETS[0]:
                            break
    # every cell masked out: all populations 0, all results NaN
    got, n = _streamed(ops, B, [50], [(0, C)], cells=torch.zeros(C, dtype=torch.bool))
    assert bool(torch.isnan(got).all()) and int(n.abs().sum()) == 0
    # rows the cell mask removes are not read: garbage (NaN, inf) in them changes nothing
    Bx = B_np.copy()
    Bx[~cells_np] = np.nan
    Bx[7:40] = np.inf
    got, n = _streamed(ops, ops.CellMatrix.from_cells_major(Bx, dtype), [1, 50, 99.9], [(0, 7), (7, 71), (71, C)], cells=cells)
    _same(got, ops.gene_quantiles(Bg, [1, 50, 99.9]), "masked-out rows hold NaN / inf")


@pytest.mark.parametrize("C", [32768, 32769])
def test_constant_column_at_the_counter_and_range_edges(ops, C):
    """G = 64, every cell of a gene in ONE bin of every digit: the count a 16-bit LDS counter and a range of SEL_MAXCELLS cells can see
    at most (the launcher cuts a block into ranges of at most 32 768 cells, fewer wherever the grid would not fill the device)."""
    G = 64
    A = np.full((C, G), 3.5, dtype=np.float32)
    A[:, 1] = -0.0
    M = ops.CellMatrix.from_cells_major(A, "float32")
    thr = torch.full((G,), 3.5, dtype=torch.float64).cuda()
    thr[2] = 3.0
    for mode, src in ((0, None), (2, M), (1, M)):
        got, n = _streamed(ops, M, [0, 50, 100], [(0, C)], src, thr if mode else None, mode)
        keep = np.ones(G, bool) if mode == 0 else ((A[0].astype(np.float64) <= thr.cpu().numpy()) if mode == 2 else (A[0].astype(np.float64) > thr.cpu().numpy()))
        assert torch.equal(n.cpu(), torch.from_numpy(np.where(keep, C, 0).astype(np.int64)))
        want = np.where(keep[None, :], A[:1].astype(np.float64).repeat(3, 0), np.nan)
        assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64)), mode


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_two_selects_fed_halves_with_their_histograms_added(ops, dtype):
    """What a cell-sharded run does: each rank counts its own cells, the integer histograms are added before advance, and every rank
    derives the same populations, ranks and fractions."""
    rng = np.random.default_rng(3)
    C, G = 513, 130
    S_np, thr_np = constructed(rng, C, G, NP_T[dtype])
    S = ops.CellMatrix.from_cells_major(S_np, dtype)
    B = ops.CellMatrix.from_cells_major(np.asarray(rng.gamma(1.0, 1.0, (C, G)), dtype=NP_T[dtype]), dtype)
    thr = torch.from_numpy(thr_np).cuda()
    cells = torch.from_numpy(rng.random(C) < 0.7).cuda()
    qs = [1, 50, 99.9]
    half = 200
    sels = [ops.StreamedMaskedGeneQuantiles(G, qs, dtype) for _ in range(2)]
    while not sels[0].done:
        for sel, (a, b) in zip(sels, ((0, half), (half, C))):
            sel.add_block(B.rows(a, b), S.rows(a, b), thr, 1, cells[a:b])
        total = sels[0].hist + sels[1].hist
        for sel in sels:
            sel.hist.copy_(total)
            sel.advance()
    ref = ops.gene_quantiles(ops.select_cells(B, cells), qs, mask_src=ops.select_cells(S, cells), mask_thr=thr, mask_mode=1)
    n_ref = torch.from_numpy(_kept(S_np, thr_np, 1, cells.cpu().numpy()).sum(0)).cuda()
    for sel in sels:
        _same(sel.result(), ref, "half")
        assert torch.equal(sel.counts(), n_ref)


def test_two_ranks_equal_one(ops, tmp_path):
    out = str(tmp_path / "msel.npz")
    cfg = dict(C=700, G=130, qs=[1, 50, 99.9], mode=1, seed=11)
    env = dict(os.environ, VCY_SINGLE_DEVICE="1", VCY_DIST_BACKEND="gloo", MASTER_PORT="29631", MASTER_ADDR="127.0.0.1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29631", os.path.join(ROOT, "tests", "masked_select_worker.py"), out, json.dumps(cfg)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = dict(np.load(out))
    import masked_select_worker as w
    B_np, S_np, thr_np, cells_np = w.make_data(cfg)
    B, S = ops.CellMatrix.from_cells_major(B_np, "float32"), ops.CellMatrix.from_cells_major(S_np, "float32")
    cells = torch.from_numpy(cells_np).cuda()
    ref = ops.gene_quantiles(ops.select_cells(B, cells), cfg["qs"], mask_src=ops.select_cells(S, cells), mask_thr=torch.from_numpy(thr_np).cuda(),
                             mask_mode=cfg["mode"]).cpu().numpy()
    n_ref = _kept(S_np, thr_np, cfg["mode"], cells_np).sum(0)
    assert z["result"].shape == (2, len(cfg["qs"]), cfg["G"])
    for r_ in range(2):
        assert np.array_equal(z["result"][r_].view(np.int64), ref.view(np.int64)), r_
        assert np.array_equal(z["counts"][r_], n_ref), r_


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_masked_moments(ops, dtype):
    rng = np.random.default_rng(23)
    C, G = 1000, 130
    np_t = NP_T[dtype]
    X = ops.CellMatrix.from_cells_major(np.asarray(rng.gamma(1.0, 2.0, (C, G)) * (rng.random((C, G)) < 0.6), dtype=np_t), dtype)
    Y = ops.CellMatrix.from_cells_major(np.asarray(rng.gamma(1.0, 1.0, (C, G)) * (rng.random((C, G)) < 0.6), dtype=np_t), dtype)
    W = ops.CellMatrix.from_cells_major(np.asarray(rng.random((C, G)), dtype=np_t), dtype)
    dS, dU = ops.gene_quantiles(X, [99.9])[0], ops.gene_quantiles(Y, [99.9])[0]
    th = ops.gene_quantiles(X, [2, 98], M2=Y, scale_a=dS, scale_b=dU)
    modes = ((0, dict(W=W)), (1, dict(M=X, M2=Y, scale_a=dS, scale_b=dU, down=th[0], up=th[1])), (1, dict(M=X, down=th[0], up=th[1])), (2, {}))
    cells = torch.from_numpy(rng.random(C) < 0.5).cuda()
    cells[32:96] = False                                               # two of the kernel's 32 fixed cell blocks (32 cells each) left empty
    n = int(cells.sum())
    take = lambda m: ops.select_cells(m, cells)
    for wmode, kw in modes:
        plain = ops.fit_weighted_moments(Y, X, wmode, **kw)
        ones = ops.fit_weighted_moments(Y, X, wmode, cell_mask=torch.ones(C, dtype=torch.bool), **kw)
        assert torch.equal(_bits(ones), _bits(plain)), wmode
        got = ops.fit_weighted_moments(Y, X, wmode, cell_mask=cells, **kw).cpu().numpy()
        kwg = {k: (take(v) if isinstance(v, ops.CellMatrix) else v) for k, v in kw.items()}
        ref = ops.fit_weighted_moments(take(Y), take(X), wmode, **kwg).cpu().numpy()
        assert (ref >= 0).all() and (got >= 0).all()
        rel = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
        print(f"{dtype}, weight mode {wmode}: largest relative difference of a moment {rel.max():.3g} (bar {2 * n * 2.0 ** -53:.3g})")
        assert rel.max() <= 2 * n * 2.0 ** -53
        if wmode != 0:
            assert np.array_equal(got[5], ref[5]), "Sw is a count"
    with pytest.raises(ValueError, match="one value per cell"):
        ops.fit_weighted_moments(Y, X, 2, cell_mask=torch.ones(C - 1, dtype=torch.bool))


def test_misuse_is_refused_by_name(ops):
    G, C = 65, 40
    M = ops.CellMatrix.from_cells_major(np.random.default_rng(0).random((C, G)), "float32")
    thr = torch.zeros(G, dtype=torch.float64).cuda()
    for q in (-0.5, 100.5, float("nan")):
        with pytest.raises(ValueError, match=r"outside \[0, 100\]"):
            ops.StreamedMaskedGeneQuantiles(G, [50, q], "float32")
    with pytest.raises(ValueError, match="between 1 and 8"):
        ops.StreamedMaskedGeneQuantiles(G, list(range(9)), "float32")
    with pytest.raises(ValueError, match="between 1 and 8"):
        ops.StreamedMaskedGeneQuantiles(G, [], "float32")
    sel = ops.StreamedMaskedGeneQuantiles(G, [10, 50], "float32")
    assert sel.state_bytes == G * (4 * (256 * 4 + 12) + 2 * 8 + 8)
    with pytest.raises(RuntimeError, match="no block was added"):
        sel.advance()
    with pytest.raises(RuntimeError, match="first pass"):
        sel.counts()
    sel.add_block(M.rows(0, 10), M.rows(0, 10), thr, 1)
    with pytest.raises(ValueError, match="genes"):
        sel.add_block(ops.CellMatrix.from_cells_major(np.zeros((5, G + 1)), "float32"))
    with pytest.raises(ValueError, match="dtype"):
        sel.add_block(ops.CellMatrix.from_cells_major(np.zeros((5, G)), "float64"))
    with pytest.raises(ValueError, match="mask_mode"):
        sel.add_block(M.rows(10, 20), M.rows(10, 20), thr, 3)
    with pytest.raises(ValueError, match="go with mask_mode"):
        sel.add_block(M.rows(10, 20), None, thr, 1)
    with pytest.raises(ValueError, match="go with mask_mode"):
        sel.add_block(M.rows(10, 20), M.rows(10, 20), thr, 0)
    with pytest.raises(ValueError, match="one value per gene"):
        sel.add_block(M.rows(10, 20), M.rows(10, 20), thr[:-1], 1)
    with pytest.raises(ValueError, match="one value per cell"):
        sel.add_block(M.rows(10, 20), M.rows(10, 20), thr, 1, cell_mask=torch.ones(9, dtype=torch.bool))
    sel.add_block(M.rows(10, C), M.rows(10, C), thr, 1)
    sel.advance()
    with pytest.raises(RuntimeError, match="passes done"):
        sel.result()
    sel.add_block(M.rows(0, 10), M.rows(0, 10), thr, 1)
    with pytest.raises(ValueError, match="the first pass saw"):          # a pass that saw too few cells is not advanced into garbage
        sel.advance()
    sel.add_block(M.rows(10, C), M.rows(10, C), thr, 1)                  # the state is intact: finishing the pass properly still works
    sel.advance()
    while not sel.done:
        sel.add_block(M, M, thr, 1)
        sel.advance()
    _same(sel.result(), ops.gene_quantiles(M, [10, 50], mask_src=M, mask_thr=thr, mask_mode=1), "after the refusals")
    with pytest.raises(RuntimeError, match="every pass is done"):
        sel.add_block(M)
    with pytest.raises(RuntimeError, match="every pass is done"):
        sel.advance()
    from velocyto_amd import _lib
    L = _lib.lib()
    rc = L.vcy_gene_mselect_count_block(M.t.data_ptr(), None, None, 0, None, sel.state.data_ptr(), sel.hist.data_ptr(), 0, sel.nq, C, G, G - 1, 0, None)
    assert rc == -1 and b"bad shape" in L.vcy_last_error()
    torch.cuda.synchronize()
