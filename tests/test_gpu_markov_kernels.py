"""Stage E/F and the Markov chain (csrc/misc.hip from k_corr_fixup down, csrc/markov.hip) against the long-double references of oracle.py, at the
ops wrapper or the C ABI, at the shapes where the kernels change path.  Every output is pre-filled with NaN or a sentinel.

Tolerances - each is one of three things:
  * an ulp count of single roundings (tp: 4 ulps of the storage type; dense() in f32: 2 f32 ulps + the renormalisation);
  * a bound the reference computes, times a constant measured on the CPU and recorded in markov_cases.py:
      one factored step   |y - ref| <= 4 K u S_j + 2^-cut n max|u|          (MARKOV_K, pinned by test_markov_oracle.py; the sparse
                          half, f64 in every compute type, adds its textbook (terms / 64 + 10) 2^-52 sum |v s|)
      delta_embedding     |de - ref| <= 2 c n 2^-53 sum_n |p - 1/n|         (TP_C)
      sums of products    (terms + 2) eps sum |a b|                          (the textbook bound of a recursive sum);
  * bit-equality (corr_fixup, wdiff in f64, target-range steps, accumulators)."""
import functools

import numpy as np
import pytest

import markov_cases as mc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LD = np.longdouble
EPS = 2.0 ** -53
f64 = lambda a: np.asarray(a, dtype=np.float64)
TD = {"float32": torch.float32, "float64": torch.float64}


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


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(TD[dtype] if isinstance(dtype, str) else dtype)


def nans(shape, dtype=torch.float64):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=dtype, device="cuda")


def nan_bytes(nbytes):
    return torch.full((int(nbytes),), 255, dtype=torch.uint8, device="cuda")          # every f32 / f64 read out of it is a NaN


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------- corr_fixup
@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (8200, 257)])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_corr_fixup(ops, dtype, shape):
    """Self pairs, NaNs and both in one slot; the last shape has more than 8192 x 256 elements (the grid-stride loop runs)."""
    C_out, n = shape
    rng = np.random.default_rng(C_out + n)
    for cell0 in (0, 37):
        vals = mc.stored(rng.uniform(-1, 1, shape), dtype)
        ixs = rng.integers(0, cell0 + C_out + 3, shape).astype(np.int32)
        rows = cell0 + np.arange(C_out)
        ixs[::2, 0] = rows[::2]                                        # self pairs
        vals[rng.random(shape) < 0.1] = np.nan
        vals[::4, 0] = np.nan                                          # a NaN in a self slot
        if C_out > 1:
            vals[1, n - 1] = np.nan
        self_ = ixs == rows[:, None]
        for zero_self in (True, False):
            for fix_nan in (True, False):
                for nan_to in (1.0, -2.5):
                    want = vals.copy()
                    if zero_self:
                        want[self_] = 0.0
                    isn = np.isnan(want)
                    if fix_nan:
                        want[isn] = nan_to
                    t = dev(vals, dtype)
                    cnt = ops.corr_fixup(t, dev(ixs), cell0, zero_self, fix_nan, nan_to)
                    assert cnt == int(isn.sum())
                    assert np.array_equal(host(t).astype(np.float64), want, equal_nan=True)


# ---------------------------------------------------------------- transition_prob
def _transition_prob(ops, lib, cs, dtype, sigma, want_tp=True, want_wdiff=True):
    """At the ABI: tp and wdiff are the two halves of one sentinel-filled buffer, so a half that is not asked for can be watched."""
    C_out, n = cs["corr"].shape
    buf = torch.full((2, C_out, n), -7.0, dtype=TD[dtype], device="cuda")
    de = nans((C_out, cs["edim"]))
    corr, ixs, emb = dev(cs["corr"], dtype), dev(cs["ixs"]), dev(cs["emb"])
    lib.check(lib.lib().vcy_transition_prob(corr.data_ptr(), ixs.data_ptr(), emb.data_ptr(), cs["edim"], buf[0].data_ptr() if want_tp else None,
                                            buf[1].data_ptr() if want_wdiff else None, de.data_ptr(), cs["cell0"], C_out, n, float(sigma),
                                            ops._DT[TD[dtype]], ops._stream()), "transition_prob")
    return host(buf[0]).astype(np.float64), host(buf[1]).astype(np.float64), host(de)


@pytest.mark.parametrize("sigma", [0.05, 0.005])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_transition_prob(ops, lib, dtype, sigma):
    """Every (n, C_out) of markov_cases.tp_cases: corr up to +-1 (exp(200) at sigma 0.005), global ixs / emb with cell0 0 and 41,
    lists that name their own cell, a twin of cell0 (NaN unit vector), edim 1 .. 4."""
    worst = dict(tp=0.0, de=0.0)
    for cs in mc.tp_cases(dtype, sigma):
        n = cs["n"]
        tp, wd, de = _transition_prob(ops, lib, cs, dtype, sigma)
        ulps = np.abs(tp - cs["tp"]).astype(np.float64) / mc.ulp(cs["tp"], dtype)
        worst["tp"] = max(worst["tp"], float(ulps.max()))
        assert ulps.max() <= 4.0, (n, cs["C_out"], float(ulps.max()))
        if dtype == "float64":
            assert np.array_equal(wd, tp - 1.0 / n)                     # the f64 p the kernel stored, minus 1/n in f64
        else:                                                           # p - 1/n in f64 (p within 4 f64 ulps), rounded once to f32
            slack = 0.5 * np.maximum(mc.ulp(cs["wd"], dtype), mc.ulp(wd, dtype)) + 4.0 * mc.ulp(cs["tp"], "float64")
            assert np.all(np.abs(wd - cs["wd"]).astype(np.float64) <= slack)
        ref = f64(cs["de"])
        assert np.array_equal(np.isnan(de), np.isnan(ref)), (n, cs["C_out"])
        bound = 2.0 * mc.TP_C * n * EPS * f64(cs["cond"])[:, None]
        err = np.abs(de - cs["de"]).astype(np.float64)
        ok = ~np.isnan(ref)
        assert np.all(err[ok] <= np.broadcast_to(bound, err.shape)[ok]), (n, cs["C_out"], float(np.nanmax(err / bound)))
        with np.errstate(all="ignore"):
            worst["de"] = max(worst["de"], float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        # a buffer that is not asked for stays as it was, and what is asked for does not change
        tp2, wd2, de2 = _transition_prob(ops, lib, cs, dtype, sigma, want_wdiff=False)
        assert np.all(wd2 == -7.0) and np.array_equal(tp2, tp) and np.array_equal(de2, de, equal_nan=True)
        tp3, wd3, de3 = _transition_prob(ops, lib, cs, dtype, sigma, want_tp=False)
        assert np.all(tp3 == -7.0) and np.array_equal(wd3, wd) and np.array_equal(de3, de, equal_nan=True)
    print(f"transition_prob {dtype} sigma {sigma}: worst tp {worst['tp']:.2f} ulps, delta_embedding uses {worst['de']:.2f} of its bound")


def test_transition_prob_wrapper_and_refusals(ops, lib):
    cs = next(c for c in mc.tp_cases("float64", 0.05) if c["n"] == 65 and c["C_out"] == 130)
    tp, wd, de = ops.transition_prob(dev(cs["corr"]), cs["ixs"], cs["emb"], 0.05, cell0=cs["cell0"])
    t0, w0, d0 = _transition_prob(ops, lib, cs, "float64", 0.05)
    assert np.array_equal(host(tp), t0) and np.array_equal(host(wd), w0) and np.array_equal(host(de), d0, equal_nan=True)
    t1, w1, _ = ops.transition_prob(dev(cs["corr"]), cs["ixs"], cs["emb"], 0.05, cell0=cs["cell0"], want_tp=False, want_wdiff=False)
    assert t1 is None and w1 is None
    with pytest.raises(ValueError):                                     # edim 5: refused before any launch
        ops.transition_prob(dev(cs["corr"]), cs["ixs"], np.zeros((cs["emb"].shape[0], 5)), 0.05)


# ---------------------------------------------------------------- row_cosproj
@pytest.mark.parametrize("G", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_row_cosproj(ops, dtype, C, G):
    rng = np.random.default_rng(G + C)
    A = mc.stored(rng.normal(size=(C, G)) * 1e6, dtype)
    B = mc.stored(rng.normal(size=(C, G)), dtype)
    if C > 1:
        B[2] = 0.0                                                      # 0 / sqrt(0)
    ld = ops.padded_ld(G)
    mats = []
    for M in (A, B):
        t = nans((C, ld), TD[dtype])                                    # NaN padding: a read past G would show
        t[:, :G] = dev(M, dtype)
        mats.append(ops.CellMatrix(t, G))
    got = host(ops.row_cosproj(*mats))
    a, b = A.astype(LD), B.astype(LD)
    with np.errstate(all="ignore"):
        den = np.sqrt((b * b).sum(1))
        ref = (a * b).sum(1) / den
        bound = f64(G * np.finfo(np.float64).eps * np.abs(a * b).sum(1) / den)
    assert np.array_equal(np.isnan(got), np.isnan(f64(ref))) and (C == 1 or np.isnan(got[2]))
    ok = ~np.isnan(got)
    assert np.all(np.abs(got - ref).astype(np.float64)[ok] <= bound[ok])


# ---------------------------------------------------------------- dense and CSC steps
def _dense_parts(n):
    return 64 if n >= 4096 else (16 if n >= 512 else 1)


@pytest.mark.parametrize("n", [1, 2, 511, 512, 513, 1023, 1024, 4095, 4096])
@pytest.mark.parametrize("tdtype", ["float32", "float64"])
def test_dense_step(ops, lib, n, tdtype):
    """Around the nparts thresholds (512, 4096) and the 16-byte-load threshold (1024): one step at the ABI, five through
    ops.diffuse, with and without the accumulator.  Each column is a sum of n products split into nparts runs: the textbook
    bound is (n / nparts + nparts + 2) eps sum |x T| per step."""
    rng = np.random.default_rng(n)
    tr = rng.random((n, n)) ** 8 + 1e-9
    tr = mc.stored(tr / tr.sum(1, keepdims=True), tdtype)
    x0 = rng.random(n) + 1e-3
    x0 /= x0.sum()
    T = dev(tr, tdtype)
    Tl = tr.astype(LD)
    iters = [x0.astype(LD)]
    for _ in range(5):
        iters.append(iters[-1] @ Tl)
    g = (-(-n // _dense_parts(n)) + _dense_parts(n) + 2) * 2 * EPS
    # one step at the ABI
    x, y, acc = dev(x0), nans(n), dev(np.arange(n, dtype=np.float64))
    ws = nan_bytes(lib.lib().vcy_diffuse_workspace_bytes(n))
    lib.check(lib.lib().vcy_diffuse_step_dense(T.data_ptr(), x.data_ptr(), y.data_ptr(), acc.data_ptr(), ws.data_ptr(), n, ops._DT[T.dtype], ops._stream()), "dense")
    assert np.all(np.abs(host(y) - iters[1]).astype(np.float64) <= g * f64(iters[1]))
    assert np.array_equal(host(acc), np.arange(n, dtype=np.float64) + host(y))
    assert lib.lib().vcy_diffuse_step_dense(T.data_ptr(), x.data_ptr(), x.data_ptr(), None, ws.data_ptr(), n, ops._DT[T.dtype], ops._stream()) != 0   # x == y
    for accumulate in (False, True):
        xf, xa = ops.diffuse(x0, T, 5, accumulate=accumulate)
        assert np.all(np.abs(host(xf) - iters[5]).astype(np.float64) <= 5 * g * f64(iters[5]))
        if accumulate:
            want = sum(iters[1:])
            assert np.all(np.abs(host(xa) - want).astype(np.float64) <= 5 * g * f64(want))
        else:
            assert xa is None


@pytest.mark.parametrize("vdtype", ["float32", "float64"])
def test_csc_step_at_the_abi(ops, lib, vdtype):
    """vcy_diffuse_step_csc with f32 and f64 values: an empty column, columns of exactly 64, 65 and 200 entries (one, two and
    four rounds of the wave), the accumulator set."""
    n = 300
    rng = np.random.default_rng(64)
    lens = rng.integers(1, 12, n)
    lens[[0, 5, 6, 299]] = 0, 64, 65, 200
    lens[17] = 0
    colptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rowidx = np.concatenate([np.sort(rng.choice(n, l, replace=False)) for l in lens]).astype(np.int32)
    val = mc.stored(rng.normal(size=rowidx.size), vdtype)
    x0 = rng.normal(size=n)
    col = np.repeat(np.arange(n), lens)
    ref, mag = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    np.add.at(ref, col, val.astype(LD) * x0[rowidx])
    np.add.at(mag, col, np.abs(val.astype(LD) * x0[rowidx]))
    y, acc0 = nans(n), rng.normal(size=n)
    acc = dev(acc0)
    cp, ri, v, x = dev(colptr), dev(rowidx), dev(val, vdtype), dev(x0)
    L = lib.lib()
    lib.check(L.vcy_diffuse_step_csc(cp.data_ptr(), ri.data_ptr(), v.data_ptr(), x.data_ptr(), y.data_ptr(), acc.data_ptr(), n, ops._DT[v.dtype], ops._stream()), "csc")
    got = host(y)
    assert got[0] == 0.0 and got[17] == 0.0
    assert np.all(np.abs(got - ref).astype(np.float64) <= (lens / 64 + 9) * 2 * EPS * f64(mag))
    assert np.array_equal(host(acc), acc0 + got)
    assert L.vcy_diffuse_step_csc(cp.data_ptr(), ri.data_ptr(), v.data_ptr(), x.data_ptr(), x.data_ptr(), None, n, ops._DT[v.dtype], ops._stream()) != 0


# ---------------------------------------------------------------- prepare_markov, prepare_markov_factored
def _centred(emb):
    return emb - 0.5 * (emb.min(0) + emb.max(0))


def _check_factors(oracle, fac, Pd, emb, sD, sW, compute):
    colptr, rowidx, scsc, tot, kw = oracle.markov_factors_reference(Pd.indptr, Pd.indices, Pd.data, emb, sD, sW)
    assert np.array_equal(host(fac.colptr), colptr) and np.array_equal(host(fac.rowidx), rowidx)
    for got, ref in ((fac.scsc, scsc), (fac.tot, tot), (fac.kw, kw)):
        got, ref = host(got), f64(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        ok = ~np.isnan(ref)
        np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-12, atol=0)
    es = oracle.markov_scaled_coords(_centred(emb), sW)
    # es = (compute type)(centred * sqrt(log2 e / (2 sigma^2))): the constant, the quotient, the root and the product round once each
    # in f64 (1.5 ulps where an ulp is smallest against the value, so up to 3 of the value's own), then once to the compute type
    assert np.all(np.abs(host(fac.es) - es).astype(np.float64) <= (3.0 if compute == "float64" else 0.5 + 2.0 ** -20) * mc.ulp(es, compute))
    assert np.array_equal(host(fac.embedding), emb)                                          # the caller's own coordinates


@pytest.mark.parametrize("n", mc.PREP_N)
def test_prepare_markov_and_its_factors(ops, oracle, n):
    """Rows of 300 entries, of a diagonal only, with a diagonal that is / is not the maximum, twins - both directions, edim 1 .. 4:
    dense() in f64 at rtol 1e-12, in f32 storage at 2 f32 ulps plus the renormalisation (the stored row sums to 1 within
    2^-23), the factors against markov_factors_reference."""
    for edim in (1, 2, 3, 4):
        P, emb = mc.prepare_problem(n, edim)
        for direction in ("forward", "backwards"):
            Pd = mc.directed(P, direction)
            ref = oracle.markov_reference(Pd.indptr, Pd.indices, Pd.data, emb, 0.9, 1.6)
            assert not np.isnan(f64(ref)).any()
            tr = host(ops.prepare_markov(Pd.indptr, Pd.indices, Pd.data, emb, 0.9, 1.6))
            np.testing.assert_allclose(tr, f64(ref), rtol=1e-12, atol=0)
            tr32 = host(ops.prepare_markov(Pd.indptr, Pd.indices, Pd.data, emb, 0.9, 1.6, dtype=torch.float32)).astype(np.float64)
            assert np.all(np.abs(tr32 - ref).astype(np.float64) <= 2 * mc.ulp(ref, "float32") + 2.0 ** -23 * f64(ref))
            for compute in ("float32", "float64"):
                fac = ops.prepare_markov_factored(Pd.indptr, Pd.indices, Pd.data, emb, 0.9, 1.6, compute_dtype=TD[compute], cull=False)
                _check_factors(oracle, fac, Pd, emb, 0.9, 1.6, compute)
            assert torch.equal(fac.dense(), ops.prepare_markov(Pd.indptr, Pd.indices, Pd.data, emb, 0.9, 1.6))


def test_prepare_markov_row_without_entries(ops, oracle):
    """A row of P that stores nothing is a NaN row of the chain, as in the reference; no other row is touched."""
    P, emb = mc.prepare_problem(257, 2, empty_row=True)
    ref = oracle.markov_reference(P.indptr, P.indices, P.data, emb, 0.9, 1.6)
    nan_rows = np.isnan(f64(ref)).all(1)
    assert nan_rows.sum() == 1 and nan_rows[2] and np.isnan(f64(ref)).sum() == 257
    for dtype in (torch.float64, torch.float32):
        tr = host(ops.prepare_markov(P.indptr, P.indices, P.data, emb, 0.9, 1.6, dtype=dtype)).astype(np.float64)
        assert np.array_equal(np.isnan(tr), np.isnan(f64(ref)))
        if dtype == torch.float64:
            np.testing.assert_allclose(tr[~nan_rows], f64(ref)[~nan_rows], rtol=1e-12, atol=0)
    fac = ops.prepare_markov_factored(P.indptr, P.indices, P.data, emb, 0.9, 1.6, compute_dtype=torch.float64, cull=False)
    _check_factors(oracle, fac, P, emb, 0.9, 1.6, "float64")
    assert np.isnan(host(fac.tot)[2]) and np.isnan(host(fac.tot)).sum() == 1


# ---------------------------------------------------------------- one factored step at the ABI
def _factors(ops, p, compute, culled, cut=None):
    fac = ops.prepare_markov_factored(p["indptr"], p["indices"], p["pval"], p["emb"], mc.SIGMA_D, mc.SIGMA_W, compute_dtype=TD[compute], cull=False)
    return fac.enable_culling(cut) if culled else fac


def _step(ops, lib, fac, x, y, accum=None, prepared=0, ws=None):
    L = lib.lib()
    n = fac.n
    ws = nan_bytes(L.vcy_markov_factored_workspace_bytes(n)) if ws is None else ws
    code = ops._DT[fac.compute_dtype]
    if fac.cull is not None:
        es_sorted, rank, boxes, cut, order = fac.cull
        rc = L.vcy_diffuse_step_factored_culled(x.data_ptr(), y.data_ptr(), ops._p(accum), fac.colptr.data_ptr(), fac.rowidx.data_ptr(), fac.scsc.data_ptr(),
                                                fac.tot.data_ptr(), fac.kw.data_ptr(), es_sorted.data_ptr(), rank.data_ptr(), order.data_ptr(), boxes.data_ptr(),
                                                fac.edim, fac.sigma_W, cut, ws.data_ptr(), n, prepared, code, ops._stream())
    else:
        rc = L.vcy_diffuse_step_factored(x.data_ptr(), y.data_ptr(), ops._p(accum), fac.colptr.data_ptr(), fac.rowidx.data_ptr(), fac.scsc.data_ptr(),
                                         fac.tot.data_ptr(), fac.kw.data_ptr(), fac.es.data_ptr(), fac.edim, fac.sigma_W, ws.data_ptr(), n, prepared, code,
                                         ops._stream())
    lib.check(rc, "diffuse_step_factored")
    return ws


_REF = {}


def _step_reference(ops, oracle, n, edim, M, shift=0.0):
    """(y, (S, T, terms), max |u|, M of the centred coordinates) of one step from x = p["x"], from the device's own f64 factors and the centred
    coordinates in long double - computed once per problem and shared by every variant of the step."""
    key = (n, edim, M, shift)
    if key not in _REF:
        p = mc.chain_problem(n, edim, M, shift=shift)
        fac = _factors(ops, p, "float64", False)
        es = oracle.markov_scaled_coords(_centred(p["emb"]), mc.SIGMA_W)
        tot, kw = host(fac.tot), host(fac.kw)
        y, S = oracle.gauss_step_reference(p["x"], tot, kw, host(fac.colptr), host(fac.rowidx), host(fac.scsc), es, mc.SIGMA_W)
        umax = float(np.abs(0.2 / np.sqrt(2 * np.pi * mc.SIGMA_W ** 2) * p["x"] / (tot * kw)).max())
        _, T, terms = oracle.sparse_half_reference(p["x"], tot, host(fac.colptr), host(fac.rowidx), host(fac.scsc))
        _REF[key] = (y, (S, T, terms), umax, float(np.abs(es).max()))
    return _REF[key]


def _share(got, y, bound):
    err = np.abs(got - y).astype(np.float64)
    assert not np.isnan(got).any()
    return float((err / bound).max())


@pytest.mark.parametrize("n", mc.STEP_N)
def test_one_factored_step(ops, lib, oracle, n):
    """vcy_diffuse_step_factored[_culled] with prepared = 0 against gauss_step_reference: f32 and f64, edim 1 .. 4 (edim 4 is the
    default: branch of every switch), plain and culled, around the 256 / 512 target blocks, the chunks of 32 and the folds of 8."""
    worst = 0.0
    for edim in ((2, 3) if n == 1025 else (1, 2, 3, 4)):                               # (n = 1025 runs every edim in the sweep below)
        p = mc.chain_problem(n, edim, 100.0)
        y, S, umax, _ = _step_reference(ops, oracle, n, edim, 100.0)
        x = dev(p["x"])
        for compute in ("float32", "float64"):
            for culled in (False, True):
                fac = _factors(ops, p, compute, culled)
                out, acc = nans(n), dev(np.ones(n))
                _step(ops, lib, fac, x, out, accum=acc)
                got = host(out)
                bound = mc.step_bound(S[0], compute, n, umax, fac.cull[3] if culled else None, S[1], S[2])
                share = _share(got, y, bound)
                assert share <= 1.0, (edim, compute, culled, share)
                assert np.array_equal(host(acc), 1.0 + got)
                worst = max(worst, share)
                if culled and n >= 1025:                                # some chunks are skipped and some are not
                    skipped, kept = mc.culled_box_census(host(fac.cull[0]), fac.cull[3])
                    assert skipped > 0 and kept > 0, (skipped, kept)
    print(f"one factored step, n = {n}: the kernels use at most {worst:.3f} of 4 K u S")


@pytest.mark.parametrize("M", mc.SWEEP_M)
def test_factored_step_conditioning_sweep(ops, lib, oracle, M):
    """The same bound as the embedding grows against the kernel: M = max |es| from 6 to 1e4 at n = 1025."""
    n = 1025
    for edim in (1, 2, 3, 4):
        p = mc.chain_problem(n, edim, M)
        y, S, umax, Mc = _step_reference(ops, oracle, n, edim, M)
        for compute in ("float32", "float64"):
            for culled in (False, True):
                fac = _factors(ops, p, compute, culled)
                out = nans(n)
                _step(ops, lib, fac, dev(p["x"]), out)
                got = host(out)
                share = _share(got, y, mc.step_bound(S[0], compute, n, umax, fac.cull[3] if culled else None, S[1], S[2]))
                rel = float((np.abs(got - y) / y).max())
                print(f"sweep M = {M:g} (centred {Mc:.0f}) edim {edim} {compute} {'culled' if culled else 'plain'}: share {share:.3f}, worst relative error {rel:.2e},"
                      f" worst relative bound {float((mc.step_bound(S[0], compute, n, umax, None, S[1], S[2]) / f64(y)).max()):.2e}")
                assert share <= 1.0, (edim, compute, culled, share)


def test_culled_transform_keeps_a_chunk_at_exactly_the_cut(ops, lib):
    """A chunk is skipped when its box is FARTHER than sqrt(cut) from the targets' box.  Integer coordinates in f64, cut = 4:
    256 cells on {0, 1} (one block of targets, eight chunks), 32 cells on 3 (a chunk at distance exactly 2 from that block) and
    32 on 100.  The reference sums exactly the chunks the rule keeps; what the far chunk would add is below 2^-9000."""
    n, cut = 320, 4.0
    rng = np.random.default_rng(4)
    es = np.concatenate([rng.integers(0, 2, 256), np.full(32, 3), np.full(32, 100)]).astype(np.float64)[:, None]
    es[0], es[255] = 0.0, 1.0
    x0 = rng.random(n) + 0.1
    tot, kw = rng.random(n) + 0.5, rng.random(n) + 0.5
    L = lib.lib()
    es_d, ident = dev(es), dev(np.arange(n, dtype=np.int32))
    boxes = nan_bytes(L.vcy_markov_cull_boxes_bytes(n, 1, ops.F64))
    lib.check(L.vcy_markov_cull_boxes(es_d.data_ptr(), boxes.data_ptr(), n, 1, ops.F64, ops._stream()), "boxes")
    colptr, rowidx, scsc = dev(np.zeros(n + 1, dtype=np.int64)), dev(np.zeros(1, dtype=np.int32)), dev(np.zeros(1))
    ws, y = nan_bytes(L.vcy_markov_factored_workspace_bytes(n)), nans(n)
    x_d, tot_d, kw_d = dev(x0), dev(tot), dev(kw)
    lib.check(L.vcy_diffuse_step_factored_culled(x_d.data_ptr(), y.data_ptr(), None, colptr.data_ptr(), rowidx.data_ptr(), scsc.data_ptr(),
                                                 tot_d.data_ptr(), kw_d.data_ptr(), es_d.data_ptr(), ident.data_ptr(), ident.data_ptr(), boxes.data_ptr(),
                                                 1, 1.0, cut, ws.data_ptr(), n, 0, ops.F64, ops._stream()), "culled")
    u = 0.2 / np.sqrt(2 * LD(np.pi)) * x0.astype(LD) / (tot.astype(LD) * kw)
    g = np.exp2(-(es.astype(LD) - es.astype(LD).T) ** 2)               # [c, j]
    keep = np.ones((n, n), dtype=bool)
    keep[288:, :256] = False                                           # block 0 never sees the chunk on 100 (gap 99); every other gap is <= 2
    ref = (u[:, None] * g * keep).sum(0)
    S = (np.abs(u)[:, None] * g * keep * (1 + 100.0 * np.abs(es - es.T))).sum(0)
    assert mc.culled_box_census(es, cut) == (1, 19)
    assert _share(host(y), ref, mc.step_bound(S, "float64", n, 0.0)) <= 1.0


BIG_N = 64 * 64 * 32 + 300            # more than 64 chunks per part of the culled transform: a second round of box tests


def test_culled_step_with_a_second_ballot_round(ops, lib, oracle):
    """n = 131 372: 4106 chunks over 64 parts, 65 per part - the 65th is tested in a second round.  The reference is taken at 48
    targets (the first and last cells of the sorted order and cells in between) from all sources; f32 and f64."""
    n, edim = BIG_N, 2
    rng = np.random.default_rng(9)
    scale = float(np.sqrt(np.log2(np.e) / 2.0))
    lab = np.sort(rng.integers(0, 9, n))
    emb = (rng.uniform(-60, 60, (9, edim))[lab] + rng.normal(size=(n, edim)) * 1.5) / scale
    first, count = np.searchsorted(lab, lab), np.bincount(lab)[lab]
    ix = first[:, None] + (np.arange(n)[:, None] - first[:, None] + np.arange(1, 4)[None, :] * 7) % count[:, None]   # three distinct cells of the cluster
    ix = np.sort(np.concatenate([np.arange(n)[:, None], ix], 1), 1).astype(np.int32)
    indptr = np.arange(0, 4 * n + 1, 4)
    pval = rng.random(4 * n) + 0.01
    x0 = rng.random(n) + 1e-3
    x0 /= x0.sum()
    ref = None
    for compute in ("float64", "float32"):
        fac = ops.prepare_markov_factored(indptr, ix.ravel(), pval, emb, mc.SIGMA_D, mc.SIGMA_W, compute_dtype=TD[compute], cull=True)
        order = host(fac.cull[4])
        assert -(-((n + 31) // 32) // 64) == 65
        if ref is None:
            targets = np.unique(np.concatenate([order[:16], order[-16:], order[np.linspace(0, n - 1, 16).astype(int)]]))
            es = oracle.markov_scaled_coords(_centred(emb), mc.SIGMA_W)
            tot, kw = host(fac.tot), host(fac.kw)
            ref = oracle.gauss_step_reference(x0, tot, kw, host(fac.colptr), host(fac.rowidx), host(fac.scsc), es, mc.SIGMA_W, targets=targets)
            umax = float(np.abs(0.2 / np.sqrt(2 * np.pi) * x0 / (tot * kw)).max())
            _, T, terms = oracle.sparse_half_reference(x0, tot, host(fac.colptr), host(fac.rowidx), host(fac.scsc))
        out = nans(n)
        _step(ops, lib, fac, dev(x0), out)
        got = host(out)
        assert not np.isnan(got).any()
        share = _share(got[targets], ref[0], mc.step_bound(ref[1], compute, n, umax, fac.cull[3], T[targets], terms[targets]))
        print(f"second ballot round, {compute}: share {share:.3f}")
        assert share <= 1.0


# ---------------------------------------------------------------- chains
@functools.lru_cache(maxsize=None)
def _chain_reference(n, edim, M, steps):
    """Iterates x_1 .. x_steps of the dense long-double chain and the one-step L1 bounds' ingredients sum_j S_j(x_t)."""
    import oracle
    p = mc.chain_problem(n, edim, M)
    args = (p["indptr"], p["indices"], p["pval"], p["emb"], mc.SIGMA_D, mc.SIGMA_W)
    tr = oracle.markov_reference(*args)
    _, _, _, tot, kw = oracle.markov_factors_reference(*args)
    A, W = oracle.gauss_step_matrices(tot, kw, oracle.markov_scaled_coords(_centred(p["emb"]), mc.SIGMA_W), mc.SIGMA_W)
    umat = float(np.abs(A).max())                                       # max |u| <= max x max |A|: x <= 1
    xs, S1 = [p["x"].astype(LD)], []
    for _ in range(steps):
        S1.append(float((xs[-1] @ W).sum()))
        xs.append(xs[-1] @ tr)
    return xs, S1, umat


def _chain_l1_bounds(S1, compute, n, umat, cut):
    """L1 error bound of the iterate after t steps: the sum of the one-step L1 bounds so far (the chain is stochastic: an error
    made at one step does not grow in L1 at the next)."""
    sparse = (264 / 64.0 + 10.0) * 2.0 ** -52          # sum_j T_j <= 0.8 sum x = 0.8 < 1, no column of these problems is longer than 264
    one = [4.0 * mc.MARKOV_K[compute] * mc.U[compute] * s + sparse + (0.0 if cut is None else 2.0 ** -cut * n * n * umat) for s in S1]
    return np.cumsum(one)


@pytest.mark.parametrize("n", [33, 513])
@pytest.mark.parametrize("compute", ["float32", "float64"])
def test_factored_chain(ops, oracle, compute, n):
    """3 steps (one launch each) and 41 (the graph-replayed loop; `prepared` is 1 from the second step on), time evolution and
    path integral, plain and culled."""
    edim, M = 2, 100.0
    p = mc.chain_problem(n, edim, M)
    xs, S1, umat = _chain_reference(n, edim, M, 41)
    for culled in (False, True):
        fac = _factors(ops, p, compute, culled)
        b = _chain_l1_bounds(S1, compute, n, umat, fac.cull[3] if culled else None)
        for steps in (3, 41):
            for accumulate in (False, True):
                xf, xa = ops.diffuse(p["x"], fac, steps, accumulate=accumulate)
                e1 = float(np.abs(host(xf) - xs[steps]).sum())
                assert e1 <= b[steps - 1], (culled, steps, e1, b[steps - 1])
                if accumulate:
                    ea = float(np.abs(host(xa) - sum(xs[1:steps + 1])).sum())
                    assert ea <= b[:steps].sum(), (culled, steps, ea)
                else:
                    assert xa is None
                print(f"chain n = {n} {compute} {'culled' if culled else 'plain'} {steps} steps: L1 error {e1:.2e} of {b[steps - 1]:.2e}")


@pytest.mark.parametrize("shift", [0.0, 1e2, 1e5])
def test_f32_chain_does_not_depend_on_the_origin(ops, oracle, shift):
    """The chain is a function of coordinate differences; the f32 transform's error is a function of max |es|.  A chain on
    emb + t must stay within the bound evaluated with M of the CENTRED coordinates, wherever the origin is: t = 1e5 sigma_W puts
    es near 8.5e4, where two cells a kernel width apart differ in the last three bits of an f32."""
    n, edim, M = 513, 2, 100.0
    p = mc.chain_problem(n, edim, M)
    xs, S1, umat = _chain_reference(n, edim, M, 41)
    emb = p["emb"] + shift * mc.SIGMA_W
    for culled in (False, True):
        fac = ops.prepare_markov_factored(p["indptr"], p["indices"], p["pval"], emb, mc.SIGMA_D, mc.SIGMA_W, compute_dtype=torch.float32, cull=culled)
        assert np.array_equal(host(fac.embedding), emb)
        b = _chain_l1_bounds(S1, "float32", n, umat, fac.cull[3] if culled else None)
        for steps in (3, 41):
            xf, _ = ops.diffuse(p["x"], fac, steps, accumulate=False)
            e1 = float(np.abs(host(xf) - xs[steps]).sum())
            print(f"origin at {shift:g} sigma_W, {'culled' if culled else 'plain'}, {steps} steps: L1 error {e1:.2e} of {b[steps - 1]:.2e}")
            assert e1 <= b[steps - 1], (shift, culled, steps, e1, b[steps - 1])


# ---------------------------------------------------------------- target ranges
@pytest.mark.parametrize("n", [300, 1100])
@pytest.mark.parametrize("compute", ["float32", "float64"])
def test_target_range_steps(ops, lib, compute, n):
    """diffuse_step_rows over (0, 1), (1, 255), (255, 257), (257, n) and an empty range: bit-equal to the full step inside the
    range, y and the accumulator untouched outside it; and the refusals of the ABI."""
    p = mc.chain_problem(n, 2, 100.0)
    x = dev(p["x"])
    for culled in (False, True):
        fac = _factors(ops, p, compute, culled)
        full, facc = nans(n), dev(np.ones(n))
        _step(ops, lib, fac, x, full, accum=facc)
        pos = fac.target_order()
        y, acc = torch.full((n,), -3.0, dtype=torch.float64, device="cuda"), dev(np.ones(n))
        done = torch.zeros(n, dtype=torch.bool, device="cuda")
        # (n = 1100: (257, n) is also cut at 600, so that the plain launch, 512 targets a block, starts at a block other than the first)
        for t0, t1 in ((255, 257), (0, 1)) + (((257, 600), (600, n)) if n > 600 else ((257, n),)) + ((100, 100), (1, 255)):
            ops.diffuse_step_rows(fac, x, y, t0, t1, accum=acc, workspace=nan_bytes(lib.lib().vcy_markov_factored_workspace_bytes(n)))
            done[pos[t0:t1]] = True
            assert torch.equal(y[done], full[done]) and torch.equal(acc[done], facc[done]), (culled, t0, t1)
            assert bool((y[~done] == -3.0).all()) and bool((acc[~done] == 1.0).all()), (culled, t0, t1)
        assert bool(done.all())
        with pytest.raises(ValueError):
            ops.diffuse_step_rows(fac, x, y, 0, n + 1)                  # t1 > n
        with pytest.raises(ValueError):
            ops.diffuse_step_rows(fac, x, x, 0, 1)                      # x == y
