"""The two edges of a grouped stage-D launch (csrc/coldeltacor.hip, k_cdc_partial_grouped / launch_grouped):

  * the short last gene chunk, of which only the lane-vectors that hold data are evaluated (rounded up to two), and
  * the groups beyond the last full round of the device, which run as narrower column tiles.

Everything goes through the C ABI on cuda:0 and is compared with the CPU oracle (oracle.coldeltacor_partial_compact) at the project's
bars - 1e-10 absolute in f64, 5e-5 in f32, the same NaN pattern - and, for the tail, bit for bit with a launch that has no tail.
The chunk and vector lengths come from the constants of the source, not from numbers repeated here."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSC = 1e-10
BAR = {"float64": 1e-10, "float32": 5e-5}
C_EDGE, NR_EDGE = 48, 16                          # the grouped path needs C >= 4 GC (GC <= 8) and nrndm >= 8


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def _constants():
    text = open(os.path.join(ROOT, "velocyto.py_amd", "csrc", "coldeltacor.hip")).read()
    return dict((k, int(v)) for k, v in re.findall(r"\b(GRP_[A-Z0-9_]+) = (\d+)", text))


def _shape(dtype):
    """(V, K, GC): genes per lane-vector (64 lanes x 16 bytes), genes per chunk of the single-control instance, cells per group."""
    c = _constants()
    V = 64 * (16 // (8 if dtype == "float64" else 4))
    if dtype == "float64":
        assert c["GRP_NV_F64"] * V == 1024                       # the dual f64 instance runs at the same chunk length (GRP_NV_F64)
        return V, c["GRP_NV_F64"] * V, c["GRP_GC_F64"]
    assert c["GRP_NV"] * V == 1536 and c["GRP_NV_DUAL"] == c["GRP_NV"]
    return V, c["GRP_NV"] * V, c["GRP_GC"]


def _edge_G(dtype):
    V, K, _ = _shape(dtype)
    return [1, V - 1, V, V + 1, 2 * V + 1, K - 1, K, K + 1, K + V, K + V + 1, K + 2 * V - 1, 2 * K - 1, 2 * K + 1]


EDGE_CASES = [(dt, i) for dt in ("float64", "float32") for i in range(13)]
_cache = {}


def _problem(ops, oracle, dtype, G, last_only):
    """Made once per (dtype, G, last_only) and never written: count-like pooled rows (exact zeros, so t = 0 in many genes), a d for the
    plain entries, a control d2, and Ux / gamma / q for the fused entry.  last_only: d, d2 and Ux are zero outside the last lane-vector
    that holds data (gamma and q zero: the fused d is f(Ux)) - a vector dropped by mistake then takes sum A b with it in every pair.
    The matrices are rounded to the storage type first, so that the oracle sees what the kernels see."""
    key = (dtype, G, last_only)
    if key in _cache:
        return _cache[key]
    V, K, _ = _shape(dtype)
    rng = np.random.default_rng(7 * G + (dtype == "float32") + 2 * last_only)
    C, nr = C_EDGE, NR_EDGE
    npdt = np.dtype(dtype)
    f = rng.gamma(8.0, 0.125, 3 * C)

    def pool(lam):
        counts = rng.poisson(lam, (3 * C, G)) * f[:, None]
        return np.stack([counts[rng.choice(3 * C, 4, replace=False)].mean(0) for _ in range(C)])

    s, u = pool(0.6).astype(npdt).astype(np.float64), pool(0.3).astype(npdt).astype(np.float64)          # cells-major (C, G)
    d = rng.normal(size=(C, G)).astype(npdt).astype(np.float64)
    d2 = rng.normal(size=(C, G)).astype(npdt).astype(np.float64)
    gam = rng.gamma(2.0, 0.3, G).astype(np.float32)
    q = rng.gamma(1.0, 0.05, G).astype(np.float32)
    if last_only:
        first = (G - 1) // V * V                                 # first gene of the last lane-vector that holds data
        assert first > 0 and (G - 1) % K >= V                   # ... and it is not the first vector of its chunk
        for a in (d, d2, u):
            a[:, :first] = 0.0
        u[:, first:] += 0.25                                     # no zero-variance d in the fused entry
        gam[:], q[:] = 0.0, 0.0
    ixs = np.stack([rng.choice(C, nr, replace=False) for _ in range(C)])
    ixs[0, 0] = 0                                                # a cell that lists itself: zero variance in A, NaN
    Sx, Ux, D, D2 = (ops.CellMatrix.from_cells_major(a, dtype) for a in (s, u, d, d2))
    tg, tq = torch.as_tensor(gam), torch.as_tensor(q)
    p = dict(Sx=Sx, Ux=Ux, D=D, D2=D2, gam=tg, q=tq, ixs=ixs, s=s, d=d, d2=d2, want={}, dmat={})
    for name, tr in (("sqrt", ops.SQRT), ("log10", ops.LOG10)):
        dm = ops.velocity_chain(Sx, Ux, tg, tq, want=("dmat",), transform=tr, psc=PSC)["dmat"]
        dmat = dm.t[:, :G].double().cpu().numpy()                # the d the fused launch builds while staging, as stored
        p["want"][name] = tuple(oracle.coldeltacor_partial_compact(np.ascontiguousarray(s.T), np.ascontiguousarray(x.T), ixs, name, PSC)
                                for x in (d, d2, dmat))
    _cache[key] = p
    return p


def _check(got, want, dtype, what):
    got = got.double().cpu().numpy()
    ok = ~np.isnan(want)
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    print(f"{what}: max |r - oracle| {err:.3g} over {int(ok.sum())} pairs, NaN in the oracle {int((~ok).sum())}, NaN here {int(np.isnan(got).sum())}")
    assert np.array_equal(np.isnan(got), ~ok), what
    assert err <= BAR[dtype], (what, err)


def _run_entries(ops, p, dtype, transform, what):
    tr = ops.TRANSFORMS[transform]
    w, w2, wf = p["want"][transform]
    ixs = p["ixs"]
    assert np.isnan(w[0, 0])
    _check(ops.coldeltacor_partial(p["Sx"], p["D"], ixs, tr, ops.RULES_PARTIAL, PSC), w, dtype, f"{what} single")
    _check(ops.coldeltacor_partial_fused(p["Sx"], p["Ux"], p["gam"], p["q"], ixs, tr, ops.RULES_PARTIAL, PSC), wf, dtype, f"{what} fused")
    a, a2 = ops.coldeltacor_partial_dual(p["Sx"], p["D"], p["D2"], ixs, tr, ops.RULES_PARTIAL, PSC)
    _check(a, w, dtype, f"{what} dual")
    _check(a2, w2, dtype, f"{what} dual control")


@pytest.mark.gpu
@pytest.mark.parametrize("transform", ["sqrt", "log10"])
@pytest.mark.parametrize("dtype,gi", EDGE_CASES)
def test_short_last_chunk(ops, oracle, dtype, gi, transform):
    """48 cells x 16 neighbours on the grouped kernels; G = 1, V-1, V, V+1, 2V+1, K-1, K, K+1, K+V, K+V+1, K+2V-1, 2K-1, 2K+1 (V: genes of
    a lane-vector, K: of a chunk): a short chunk of one to NV lane-vectors, odd and even, alone or after full ones, and a full last chunk."""
    G = _edge_G(dtype)[gi]
    p = _problem(ops, oracle, dtype, G, False)
    _run_entries(ops, p, dtype, transform, f"{dtype} {transform} G {G}")


@pytest.mark.gpu
@pytest.mark.parametrize("transform", ["sqrt", "log10"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("where", ["2V+1", "K+V+1", "K+2V+1"])
def test_d_only_in_the_last_vector(ops, oracle, dtype, where, transform):
    """d (and the control, and the Ux the fused d is made of) is zero outside the last lane-vector that holds data - the third of an only
    chunk, the second and the third of a short chunk after a full one: without that vector every sum A b is zero and every correlation
    is another one."""
    V, K, _ = _shape(dtype)
    G = {"2V+1": 2 * V + 1, "K+V+1": K + V + 1, "K+2V+1": K + 2 * V + 1}[where]
    p = _problem(ops, oracle, dtype, G, True)
    w = p["want"][transform][0]
    assert np.nanmin(np.abs(w)) > 0                              # (so a lost vector cannot pass for the value)
    _run_entries(ops, p, dtype, transform, f"{dtype} {transform} G {G}, d in the last vector only")


# --------------------------------------------------------------------------- the tail of the launch
_tail = {}


def _tail_problem(ops, oracle, dtype):
    """2 GC W cells (W: the device's CUs) x 32 neighbours x 64 genes: launched whole it is two full rounds and has no tail."""
    if dtype in _tail:
        return _tail[dtype]
    _, _, GC = _shape(dtype)
    W = torch.cuda.get_device_properties(0).multi_processor_count
    C, G, nr = 2 * GC * W, 64, 32
    rng = np.random.default_rng(5 + GC)
    npdt = np.dtype(dtype)
    e = (rng.gamma(2.0, 1.0, (C, G)) * (rng.random((C, G)) < 0.6)).astype(npdt).astype(np.float64)
    d = rng.normal(size=(C, G)).astype(npdt).astype(np.float64)
    ixs = rng.integers(0, C, (C, nr))
    ixs[0, 0] = 0
    E, D = ops.CellMatrix.from_cells_major(e, dtype), ops.CellMatrix.from_cells_major(d, dtype)
    want = oracle.coldeltacor_partial_compact(np.ascontiguousarray(e.T), np.ascontiguousarray(d.T), ixs, "sqrt", PSC)
    whole = ops.coldeltacor_partial(E, D, ixs, ops.SQRT, ops.RULES_PARTIAL, PSC)
    _check(whole, want, dtype, f"{dtype} two full rounds")
    _tail[dtype] = dict(E=E, D=D, ixs=ixs, want=want, whole=whole, GC=GC, W=W)
    return _tail[dtype]


@pytest.mark.gpu
@pytest.mark.parametrize("left", ["1", "W/2", "W/2+1", "W-1"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_groups_beyond_the_last_full_round(ops, oracle, dtype, left):
    """One full round and `left` groups more: every cell against the oracle, and bit for bit what the two-round launch of the same
    cells (no tail) returns for them - tiles only regroup pairs, a pair's sums keep their lanes and their order."""
    p = _tail_problem(ops, oracle, dtype)
    W, GC = p["W"], p["GC"]
    n = GC * (W + {"1": 1, "W/2": W // 2, "W/2+1": W // 2 + 1, "W-1": W - 1}[left])
    got = ops.coldeltacor_partial(p["E"], p["D"], p["ixs"][:n], ops.SQRT, ops.RULES_PARTIAL, PSC)
    assert got.shape == (n, 32)
    _check(got, p["want"][:n], dtype, f"{dtype} left {left} ({n} cells)")
    it = torch.int64 if dtype == "float64" else torch.int32
    assert torch.equal(got.view(it), p["whole"][:n].view(it))
