"""vcy_fit_weighted_moments_fused at the C ABI: the (10, G) moments with the weight of vcy_gamma_weights formed inside the fold.

Bars.  Against the two-step route on the same device matrices - vcy_gamma_weights into a dense W, then
vcy_fit_weighted_moments[_masked](weight_mode 0) - BIT-IDENTICAL, NaN payloads aside, in f32 and f64, modes 0-3, with and without a
cell mask, at every shape where the kernel's cell blocking (FIT_CB = 32 partials) or its gene tiling (256 lanes) takes another
path, with row padding (ld > G) whose contents must not matter.  In f64 also against numpy's restatement of analysis.py:1182-1219
with the same thresholds: the weights of modes 0, 1, 3 are IEEE divisions, comparisons and one product, so W is numpy's bit for
bit and the moments are two summation orders of the same non-negative terms, within 2 C 2^-53 relative; mode 2 goes through the
device's pow, whose distance from numpy's on these inputs is measured here (fit_weight_cases.POW_W_ULPS, in ulps of W) and added."""
import numpy as np
import pytest

import fit_weight_cases as wc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DTYPES = ["float64", "float32"]
MODES = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def _cm(ops, a, dtype, pad):
    """Cells-major (C, G) array -> device matrix of `dtype` whose padding columns hold `pad`."""
    m = ops.CellMatrix.from_cells_major(np.ascontiguousarray(a), dtype)
    if m.ld > m.G:
        m.t[:, m.G:] = pad
    return m


def _vec(v):
    return None if v is None else torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).cuda().contiguous()


def _p(t):
    return None if t is None else (t.data_ptr() if isinstance(t, torch.Tensor) else t.t.data_ptr())


def _mask(m):
    return None if m is None else torch.as_tensor(np.asarray(m, dtype=np.uint8)).cuda().contiguous()


def _fused(ops, d, mode, args, power=15.0, mask=None):
    """vcy_fit_weighted_moments_fused, the output and the workspace pre-filled with NaN: -> (10, G) numpy."""
    Y, X, S, U = d["Y"], d["X"], d["S"], d["U"]
    mom = torch.full((10, Y.G), float("nan"), dtype=torch.float64, device="cuda")
    ws = ops._fit_workspace(Y.G, Y.t.device)
    ws.fill_(255)
    keep = [_vec(v) for v in args]
    cm = _mask(mask)
    L = ops._lib
    L.check(L.lib().vcy_fit_weighted_moments_fused(_p(Y), _p(X), int(mode), _p(S), None if mode == 2 else _p(U), *[_p(k) for k in keep], float(power),
                                                   _p(cm), mom.data_ptr(), ws.data_ptr(), Y.C, Y.G, Y.ld, Y.code, ops._stream()), "fused")
    return mom.cpu().numpy()


def _two_step(ops, d, mode, args, power=15.0, mask=None):
    """vcy_gamma_weights -> vcy_fit_weighted_moments[_masked](weight_mode 0): -> ((10, G) numpy, W as a (C, G) f64 numpy array)."""
    Y, X, S, U = d["Y"], d["X"], d["S"], d["U"]
    L = ops._lib
    W = ops.CellMatrix(torch.full_like(S.t, float("nan")), S.G)
    keep = [_vec(v) for v in args]
    L.check(L.lib().vcy_gamma_weights(_p(S), None if mode == 2 else _p(U), _p(W), *[_p(k) for k in keep], S.C, S.G, S.ld, int(mode), float(power),
                                      S.code, ops._stream()), "gamma_weights")
    mom = torch.full((10, Y.G), float("nan"), dtype=torch.float64, device="cuda")
    ws = ops._fit_workspace(Y.G, Y.t.device)
    ws.fill_(255)
    cm = _mask(mask)
    if cm is None:
        L.check(L.lib().vcy_fit_weighted_moments(_p(Y), _p(X), 0, _p(W), None, None, None, None, None, None, mom.data_ptr(), ws.data_ptr(), Y.C, Y.G,
                                                 Y.ld, Y.code, ops._stream()), "moments")
    else:
        L.check(L.lib().vcy_fit_weighted_moments_masked(_p(Y), _p(X), 0, _p(W), None, None, None, None, None, None, _p(cm), mom.data_ptr(),
                                                        ws.data_ptr(), Y.C, Y.G, Y.ld, Y.code, ops._stream()), "moments_masked")
    return mom.cpu().numpy(), W.t[:, :W.G].double().cpu().numpy()


def _bits_equal(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    nan = np.isnan(got) & np.isnan(ref)
    return bool(np.all((got.view(np.uint64) == ref.view(np.uint64)) | nan))


def _device(ops, c, dtype, pad):
    return {n: _cm(ops, c[n], dtype, pad) for n in ("S", "U", "X", "Y")}


def _masks(C):
    rng = np.random.default_rng(C)
    single = np.zeros(C, dtype=np.uint8)
    single[C // 2] = 1
    return {"none": None, "ones": np.ones(C, dtype=np.uint8), "single": single, "random": (rng.random(C) < 0.5).astype(np.uint8),
            "zeros": np.zeros(C, dtype=np.uint8)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G", wc.GENES)
def test_fused_moments_are_the_two_step_moments_bit_for_bit(ops, G, dtype):
    """Every C of fit_weight_cases.CELLS, modes 0-3, no mask / all ones / one kept cell / a random half / all zero; the row padding
    filled with a sentinel, then with NaN: neither route's output depends on it."""
    for C in wc.CELLS:
        c = wc.case(C, G, dtype)
        d, d_nan = _device(ops, c, dtype, 7777.0), _device(ops, c, dtype, float("nan"))
        for mode in MODES:
            args = wc.mode_args(c, mode)
            plain = None
            for name, m in _masks(C).items():
                got = _fused(ops, d, mode, args, mask=m)
                ref, _ = _two_step(ops, d, mode, args, mask=m)
                assert not np.isnan(got[:5]).any()                 # the unweighted moments of finite data: every output was written
                assert _bits_equal(got, ref), (C, G, mode, name)
                assert _bits_equal(_fused(ops, d_nan, mode, args, mask=m), got), (C, G, mode, name, "padding")
                if name == "none":
                    plain = got
                elif name == "ones":
                    assert _bits_equal(got, plain), (C, G, mode, "an all-ones mask is no mask")
                elif name == "zeros":
                    assert np.array_equal(got, np.zeros_like(got)), (C, G, mode, "a block without a kept cell adds zeros")
                elif name == "single":
                    k = C // 2
                    x, y = c["X"][k], c["Y"][k]
                    assert np.array_equal(got[:5], np.stack([x, y, x * x, x * y, y * y])), (C, G, mode, "one kept cell")


@pytest.mark.parametrize("dtype", DTYPES)
def test_degenerate_genes_bit_for_bit(ops, dtype):
    """p99 = 0 (x / 0 and 0 / 0 in "sum" / "prod"), down == up (0 / 0 in "maxmin_weighted"), a constant gene, an all-zero gene, huge
    and tiny values; power 1, 15 and 2.5: the fused moments are the two-step moments bit for bit, non-finite ones included."""
    c = wc.degenerate(dtype)
    C = c["S"].shape[0]
    d = _device(ops, c, dtype, 7777.0)
    half = (np.arange(C) % 2 == 0).astype(np.uint8)
    seen_nonfinite = 0
    for mode in MODES:
        args = wc.mode_args(c, mode)
        for power in (wc.POWERS if mode == 2 else (15.0,)):
            for m in (None, half):
                got = _fused(ops, d, mode, args, power=power, mask=m)
                ref, W = _two_step(ops, d, mode, args, power=power, mask=m)
                assert _bits_equal(got, ref), (mode, power, m is not None)
                assert np.array_equal(np.isfinite(got), np.isfinite(ref))
                seen_nonfinite += int((~np.isfinite(got)).sum())
                if mode in (0, 1):
                    assert not np.isfinite(W[:, 3]).all() and np.isnan(W[:, 1]).all()        # x / 0 and 0 / 0 really happened
                if mode == 2:
                    assert np.isnan(W[:, 4]).all() and np.isnan(W[:, 2]).all()               # 0 / 0: down == up
    assert seen_nonfinite > 0


def _rel(got, ref):
    """Largest relative difference over the finite entries; non-finite entries must sit in the same places, zeros be zeros."""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert (ref[fin] >= 0).all() and (got[fin] >= 0).all()
    zero = fin & (ref == 0)
    assert np.array_equal(got[zero], ref[zero])
    pos = fin & (ref > 0)
    return float((np.abs(got[pos] - ref[pos]) / ref[pos]).max()) if pos.any() else 0.0


@pytest.mark.parametrize("G", wc.GENES)
def test_f64_against_numpy_with_the_same_thresholds(ops, G):
    """analysis.py:1182-1219 restated in numpy on the stored values, the thresholds np.percentile's.  Modes 0, 1, 3: the device's W is
    numpy's bit for bit and every moment within 2 C 2^-53 relative.  Mode 2, powers 1, 15 and 2.5: the device's W within
    POW_W_ULPS ulps of numpy's (the measured error of the device's pow on these inputs), every moment within
    2 C 2^-53 + POW_W_ULPS 2^-52 relative (non-negative terms, each off by at most that)."""
    dtype = "float64"
    worst_w = worst_bin = worst_pow = 0.0
    for C in wc.CELLS:
        c = wc.case(C, G, dtype)
        d = _device(ops, c, dtype, 7777.0)
        keep = np.arange(C) % 3 != 1
        for mode in MODES:
            args = wc.mode_args(c, mode)
            for power in (wc.POWERS if mode == 2 else (15.0,)):
                Wn = wc.numpy_weights(c, mode, power)
                _, Wd = _two_step(ops, d, mode, args, power=power)
                assert np.array_equal(np.isnan(Wd), np.isnan(Wn)) and np.array_equal(np.isinf(Wd), np.isinf(Wn))
                fin = np.isfinite(Wn)
                if mode == 2:
                    ulps = np.abs(Wd[fin] - Wn[fin]) / np.spacing(np.abs(Wn[fin]))
                    worst_w = max(worst_w, float(ulps.max()) if ulps.size else 0.0)
                else:
                    assert np.array_equal(Wd[fin], Wn[fin]), (C, G, mode)
                for m in (None, keep):
                    if m is not None and not m.any():
                        continue
                    got = _fused(ops, d, mode, args, power=power, mask=m)
                    rel = _rel(got, wc.numpy_moments(c, Wn, None if m is None else m))
                    n = C if m is None else int(m.sum())
                    if mode == 2:
                        worst_pow = max(worst_pow, rel)
                        assert rel <= 2 * n * 2.0 ** -53 + wc.POW_W_ULPS * 2.0 ** -52, (C, G, mode, power, rel)
                    else:
                        worst_bin = max(worst_bin, rel / (2 * n * 2.0 ** -53))
                        assert rel <= 2 * n * 2.0 ** -53, (C, G, mode, rel)
    print(f"G {G}: W of maxmin_weighted at most {worst_w:.3g} ulps from numpy's (recorded {wc.POW_W_ULPS}); largest relative difference of a "
          f"moment: {worst_pow:.3g} with pow, {worst_bin:.3g} of the bar 2 C 2^-53 without")
    assert worst_w <= wc.POW_W_ULPS


def test_bad_arguments_are_refused(ops):
    c = wc.case(33, 1, "float64")
    d = _device(ops, c, "float64", 0.0)
    L = ops._lib.lib()
    v = _vec(np.ones(1))
    mom = torch.zeros((10, 1), dtype=torch.float64, device="cuda")
    ws = ops._fit_workspace(1, mom.device)
    call = lambda mode, U, pc: L.vcy_fit_weighted_moments_fused(_p(d["Y"]), _p(d["X"]), mode, _p(d["S"]), U, _p(v), _p(v), pc, pc, pc, pc, 15.0, None,
                                                                mom.data_ptr(), ws.data_ptr(), 33, 1, d["Y"].ld, d["Y"].code, None)
    assert call(4, _p(d["U"]), _p(v)) != 0 and call(-1, _p(d["U"]), _p(v)) != 0
    assert call(0, None, None) != 0                       # "sum" reads U
    assert call(3, _p(d["U"]), None) != 0                 # "maxmin_double" needs pc, pd, sa, sb
    assert call(2, None, None) == 0                       # "maxmin_weighted" reads neither
    with pytest.raises(ValueError, match="fused_mode"):
        ops.fit_weighted_moments_fused(d["Y"], d["X"], 4, d["S"], d["U"], v, v)
    with pytest.raises(ValueError, match="one value per gene"):
        ops.fit_weighted_moments_fused(d["Y"], d["X"], 0, d["S"], d["U"], _vec(np.ones(2)), v)
    got = ops.fit_weighted_moments_fused(d["Y"], d["X"], 0, d["S"], d["U"], c["p99_S"], c["p99_U"]).cpu().numpy()
    assert _bits_equal(got, _fused(ops, d, 0, wc.mode_args(c, 0)))
