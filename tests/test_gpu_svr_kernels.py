"""The SVR kernels (csrc/svr.hip) against references that share none of their state: every fit held to the long-double optimality
certificate of svr_cases.py (residuals recomputed from coef alone - a carried residual that drifted, missed its lazy update or was
handed over wrongly from registers cannot pass), every instantiation k_svr_smo<1|2|4|8|0> on one and on many workgroups held to
the SAME trajectory on data with exact ties, k_svr_finish's midpoint branch with support vectors present, k_svr_predict against a
plain long-double sum within a derived bound, the workspace size and the argument checks at the ABI.  test_svr_oracle.py shows on
the CPU that the certificate passes the reference solutions and rejects wrong ones."""
import numpy as np
import pytest

import svr_cases as sv

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_ORACLE_FITS = {}


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def _oracle_fit(oracle, name):
    """The oracle's solution of a case, fitted once and never modified."""
    if name not in _ORACLE_FITS:
        x, t, kw = sv.case(name)
        coef, b, it = oracle.svr_rbf_fit(x, t, **kw)
        coef.setflags(write=False)
        _ORACLE_FITS[name] = (coef, float(b), int(it))
    return _ORACLE_FITS[name]


def _fit(ops, x, t, **kw):
    coef, b, info = ops.svr_fit(x, t, **kw)
    return coef.cpu().numpy(), float(b), info.cpu().numpy()


def _env(monkeypatch, wg, glob):
    for name, v in (("VCY_SVR_WG", wg), ("VCY_SVR_GLOBAL", glob)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


# ------------------------------------------------------------------------------------------------------------------ the certificate
@pytest.mark.parametrize("name", list(sv.CASES))
def test_every_case_passes_the_certificate(ops, oracle, monkeypatch, name):
    _env(monkeypatch, None, None)
    x, t, kw = sv.case(name)
    C, gamma, tol = kw["C"], kw["gamma"], kw["tol"]
    coef, b, info = _fit(ops, x, t, **kw)
    assert info[1] == 1 and info[2] == 0
    it = int(info[0])
    cert = sv.certificate(x, t, coef, b, C, kw["epsilon"], gamma)
    ocoef, ob, oit = _oracle_fit(oracle, name)
    print(f"{name}: steps {it} (oracle {oit}) workgroups {int(info[3])} violation {float(cert.violation):.6e} "
          f"(violation - tol) / slack {sv.violation_ratio(cert, C, tol, it, t, coef):.4g} gap {float(cert.gap):.3e}")
    bad = sv.accept(cert, b, C, tol, it, len(x), t, coef)
    assert not bad, bad
    a = np.abs(coef)
    if name in sv.NONE_FREE:                             # k_svr_finish takes the midpoint branch, and with support vectors present
        assert not ((a > 0) & (a < C)).any() and np.count_nonzero(coef) > 0
    if name == "eps0":
        assert np.count_nonzero(coef) == len(x)
    xq = np.linspace(x.min(), x.max(), 101)
    got = ops.svr_predict(x, coef, b, xq, gamma).cpu().numpy()
    want = oracle.svr_rbf_predict(x, ocoef, ob, xq, gamma)
    bar = 1e-7 * max(1.0, np.abs(t).max()) if it == oit else 8e-3 * max(1.0, C / 20)            # else: two stopped solvers
    print(f"{name}: prediction against the oracle's {float(np.abs(got - want).max()):.3e} (bar {bar:.1e})")
    np.testing.assert_allclose(got, want, rtol=0, atol=bar)


# ------------------------------------------------------------------------------------------------------------------ launch shapes
# n = 1300, kernel_for: per = ceil(n / (workgroups * 256)) points per thread -> <1>, <2>, <4>, <8> for per <= 1, 2, 4, 8, else <0>;
# VCY_SVR_GLOBAL set: <0> whatever the shape.  (VCY_SVR_WG, VCY_SVR_GLOBAL, workgroups)
SHAPES = [(None, None, 3),      # default ceil(1300 / 512) = 3 workgroups, per = 2: <2>
          (1, None, 1),         # per = 6: <8>, __syncthreads only
          (2, None, 2),         # per = 3: <4>
          (6, None, 6),         # per = 1: <1>, 236 idle threads in the last workgroup
          (64, None, 64),       # per = 1: <1>, 58 workgroups without a point
          (1, 1, 1),            # <0>
          (3, 1, 3),            # <0>
          (64, 1, 64)]          # <0>


@pytest.mark.parametrize("name", ["cv1300", "tied1300"])
def test_every_instantiation_takes_the_same_path(ops, monkeypatch, name):
    """Bit-identical coef, intercept and step count on every launch shape and from registers or global memory.  On tied1300 most
    selections are between exactly equal candidates, so this holds only if every reduction level prefers the lowest index."""
    x, t, kw = sv.case(name)
    assert len(x) == 1300
    if name == "tied1300":
        assert len(np.unique(np.stack([x, t]), axis=1).T) < 400
    res = []
    for wg, glob, _ in SHAPES:
        _env(monkeypatch, wg, glob)
        res.append(_fit(ops, x, t, **kw))
    assert [int(r[2][3]) for r in res] == [s[2] for s in SHAPES]
    assert all(r[2][1] == 1 and r[2][2] == 0 for r in res)
    for r, s in zip(res[1:], SHAPES[1:]):
        assert r[2][0] == res[0][2][0], s
        np.testing.assert_array_equal(r[0], res[0][0], err_msg=str(s))
        assert r[1] == res[0][1], s


def test_the_global_memory_solver_is_reached_by_size(ops, monkeypatch):
    """cv2100 on one workgroup: per = 9 > 8, k_svr_smo<0> without the switch; on 5 workgroups per = 2, <2>."""
    x, t, kw = sv.case("cv2100")
    res = []
    for wg in (1, 5):
        _env(monkeypatch, wg, None)
        res.append(_fit(ops, x, t, **kw))
    assert [int(r[2][3]) for r in res] == [1, 5] and all(r[2][1] == 1 and r[2][2] == 0 for r in res)
    assert res[0][2][0] == res[1][2][0] and res[0][1] == res[1][1]
    np.testing.assert_array_equal(res[0][0], res[1][0])


def test_max_iter_stops_an_unconverged_solve(ops, monkeypatch):
    x, t, kw = sv.case("C100")
    res = []
    for wg in (1, 2):
        _env(monkeypatch, wg, None)
        res.append(_fit(ops, x, t, max_iter=100, **kw))
    for coef, b, info in res:
        assert info[0] == 100 and info[1] == 0 and info[2] == 0
    assert [int(r[2][3]) for r in res] == [1, 2]
    coef, b, _ = res[0]
    cert = sv.certificate(x, t, coef, b, kw["C"], kw["epsilon"], kw["gamma"])
    print(f"C100 capped at 100 steps: violation {float(cert.violation):.3e}")
    assert float(cert.violation) >= kw["tol"]
    assert float(cert.max_abs_coef) <= kw["C"] and abs(float(cert.sum_coef)) <= 4 * sv.U53 * (100 + len(x)) * kw["C"]
    np.testing.assert_array_equal(res[1][0], coef)
    assert res[1][1] == b


# ------------------------------------------------------------------------------------------------------------------ predict
def _queries(x, m, gamma, rng):
    """One query exactly on a data point (the one of index 1: its coefficient is not zero), then queries a kernel width from data
    points, inside the data and outside it."""
    lo, hi = float(x.min()), float(x.max())
    near = x[rng.integers(0, len(x), m)] + rng.normal(size=m) / np.sqrt(max(gamma, 1.0))
    xq = np.where(np.arange(m) % 3 == 0, near, np.where(np.arange(m) % 3 == 1, rng.uniform(lo, hi, m), np.where(rng.random(m) < 0.5, lo - rng.random(m) * 3, hi + rng.random(m) * 3)))
    xq[0] = x[min(1, len(x) - 1)]
    return xq


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2049])
def test_predict_against_the_long_double_sum(ops, n):
    """The LDS tiling of k_svr_predict: less than a tile, exactly one, one entry more (odd tail of one), two tiles and one; query
    blocks of 1, 255, 256 and 257."""
    rng = np.random.default_rng(n)
    x, coef, b = rng.normal(size=n), rng.normal(size=n), 0.37
    coef[::3] = 0.0
    worst, where = 0.0, None
    for gamma in (0.0, 0.7, 1e6):
        for m in (1, 255, 256, 257):
            xq = _queries(x, m, gamma, rng)
            got = ops.svr_predict(x, coef, np.array([b]), xq, gamma).cpu().numpy()
            assert got.shape == (m,)
            ref = sv.predict_reference(x, coef, b, xq, gamma)
            bound = sv.predict_bound(x, coef, b, xq, gamma)
            err = np.abs(got - ref).astype(np.float64)
            if float((err / bound).max()) > worst:
                worst, where = float((err / bound).max()), (gamma, m)
            assert np.all(err <= bound), (gamma, m, float((err / bound).max()), int(np.argmax(err / bound)))
            if gamma == 0.0:
                flat = np.sum(coef.astype(np.longdouble)) + np.longdouble(b)
                assert np.all(np.abs(got - flat).astype(np.float64) <= bound)
                assert np.all(got == got[0])
            if n == 1:
                assert np.all(got == b)                                    # its only coefficient is one of the zeros
    print(f"k_svr_predict n={n}: worst error / bound {worst:.3g} at (gamma, m) = {where}")


def test_predict_with_every_coefficient_zero(ops):
    rng = np.random.default_rng(7)
    x = rng.normal(size=1025)
    for gamma in (0.0, 0.7, 1e6):
        got = ops.svr_predict(x, np.zeros(1025), np.array([-2.625]), _queries(x, 257, gamma, rng), gamma).cpu().numpy()
        assert np.all(got == -2.625)


# ------------------------------------------------------------------------------------------------------------------ the ABI
def _abi_fit(ops, x, t, ws, n=None, x_null=False, ws_null=False, C=1.0, eps=0.1, gamma=0.5, tol=1e-3, out=None):
    dev = ops.require_gpu()
    L = ops._lib.lib()
    xd, td = (torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev) for a in (x, t))
    if out is None:
        out = (torch.empty(len(x), dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev),
               torch.empty(4, dtype=torch.int32, device=dev))
    coef, b, info = out
    rc = L.vcy_svr_rbf_fit(None if x_null else xd.data_ptr(), td.data_ptr(), coef.data_ptr(), b.data_ptr(), info.data_ptr(),
                           None if ws_null else ws.data_ptr(), len(x) if n is None else n, C, eps, gamma, tol, -1, ops._stream())
    torch.cuda.synchronize()
    return rc, coef, b, info


@pytest.mark.parametrize("n,glob", [(1, None), (255, None), (257, None), (1300, None), (1300, 1)])
def test_a_fit_stays_inside_its_workspace(ops, monkeypatch, n, glob):
    _env(monkeypatch, None, glob)
    L = ops._lib.lib()
    x, t = sv._cv_like(n, np.random.default_rng(n))
    nbytes = int(L.vcy_svr_workspace_bytes(n))
    assert nbytes >= 25 * n
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=ops.require_gpu())
    rc, coef, b, info = _abi_fit(ops, x, t, ws)
    assert rc == 0, L.vcy_last_error()
    info = info.cpu().numpy()
    assert info[1] == 1 and info[2] == 0 and info[3] == (n + 511) // 512
    assert bool((ws[nbytes:] == 0xA5).all()), "the fit wrote past vcy_svr_workspace_bytes(n)"
    assert not bool((ws[:nbytes] == 0xA5).all())
    _env(monkeypatch, None, None)
    want = _fit(ops, x, t, C=1.0, epsilon=0.1, gamma=0.5, tol=1e-3)               # the wrapper's own workspace: the same fit
    np.testing.assert_array_equal(coef.cpu().numpy(), want[0])
    assert float(b) == want[1] and info[0] == want[2][0]


def test_workspace_bytes_of_a_negative_size(ops):
    assert ops._lib.lib().vcy_svr_workspace_bytes(-1) == 0


def test_bad_arguments_are_refused_before_any_launch(ops):
    L = ops._lib.lib()
    dev = ops.require_gpu()
    n = 40
    x, t = sv._cv_like(n, np.random.default_rng(n))
    ws = torch.full((int(L.vcy_svr_workspace_bytes(n)),), 0xA5, dtype=torch.uint8, device=dev)
    out = (torch.full((n,), -7.5, dtype=torch.float64, device=dev), torch.full((1,), -7.5, dtype=torch.float64, device=dev),
           torch.full((4,), -77, dtype=torch.int32, device=dev))
    for bad in (dict(x_null=True), dict(ws_null=True), dict(n=0), dict(C=0.0), dict(tol=0.0), dict(gamma=-1e-300), dict(eps=-1e-300)):
        rc, coef, b, info = _abi_fit(ops, x, t, ws, out=out, **bad)
        assert rc == -1 and b"svr_rbf_fit" in L.vcy_last_error(), bad                        # VCY_ERR_INVALID
        assert bool((coef == -7.5).all()) and bool((b == -7.5).all()) and bool((info == -77).all()), bad
        assert bool((ws == 0xA5).all()), bad
    rc, coef, b, info = _abi_fit(ops, x, t, ws, out=out)                                     # and the same buffers are fine otherwise
    assert rc == 0 and int(info[1]) == 1 and not bool((coef == -7.5).any())
