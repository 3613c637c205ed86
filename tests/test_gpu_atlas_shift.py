"""AtlasPath(shift=True): calculate_embedding_shift (stage E) per streamed block, delta_S never formed.

Bars.  The kernel (vcy_embedding_scaling_fused): BIT-IDENTICAL to vcy_velocity_chain's delta_S + vcy_embedding_scaling (the same operations
in the same order), and within the derived bound of atlas_shift_cases.cos_reference (numpy fp64 on the stored values; the bound is
stated there: recursive sum of the estimate, rounding of the on-the-fly delta_S, fp64 fold).  The path in one block: corr and gamma
untouched by shift=True, tp / delta_embedding / scaling bit-identical to the resident recipe (dense pooling, velocity_chain,
analysis.embedding_shift).  In blocks and over ranks, against the expectation built from the run's own stored outputs: tp and the
unscaled shift bit-identical to one transition_prob call over all cells, scaling within the bound, delta_embedding the exact product."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import atlas_shift_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, G, P, K, NN = 1500, 2100, 10, 10, 80
BLOCK = 397                                                  # four blocks, not a multiple of 8, the last one of 309 cells
OUT = ("corr", "neigh", "tp", "delta_embedding", "delta_embedding_unscaled", "scaling")


@pytest.fixture(scope="module")
def ops():
    import velocyto_amd
    from velocyto_amd import ops as _ops
    _ops.require_gpu()
    return _ops


def _data(ops, c, g):
    from velocyto_amd import atlas
    cS, cU, totS, totU, pcs, emb = atlas.synth_atlas(c, g, P, ops.require_gpu(), density=0.08)
    fS, fU = atlas.size_factors(totS, totU, c)
    return cS, cU, fS, fU, pcs, emb


@pytest.fixture(scope="module")
def data(ops):
    return _data(ops, C, G)


@pytest.fixture(scope="module")
def pooled(ops, data):
    """Sx, Ux of all cells by the dense pooling, per dtype: computed once, never modified."""
    return {dt: sc.dense_pool(ops, data, K, dt) for dt in (torch.float32, torch.float64)}


def _path(data, n_neighbors=NN, **kw):
    from velocyto_amd import atlas
    return atlas.AtlasPath(*data, k=K, n_neighbors=n_neighbors, sampled_fraction=0.5, sigma_corr=sc.SIGMA, **kw)


def _got(p):
    got = {n: (None if getattr(p, n) is None else getattr(p, n).clone()) for n in OUT}
    return dict(got, gamma=p.gamma.clone(), q=None if p.q is None else p.q.clone())


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("C_,G_,n", [(9, 70, 3), (100, 1003, 17), (333, 4100, 64), (70, 515, 256)])
def test_fused_kernel_at_the_abi(ops, dtype, C_, G_, n):
    """Ragged last group, G no multiple of the vector width, more than one sweep of the eight waves; q given and NULL, dt_shift 1 and
    0.37, Ux with exactly C_out < C rows, natural and permuted order, a repeated neighbour and a cell that lists itself, an all-zero
    weight row (NaN), gamma entries that are 0 and a gene where Ux == gamma Sx + q exactly (delta_S = 0)."""
    rng = np.random.default_rng(C_ + n)
    tdt = getattr(torch, dtype)
    S_np, U_np = rng.gamma(1.0, 2.0, (C_, G_)), rng.gamma(1.0, 1.0, (C_, G_))
    gamma = rng.gamma(2.0, 0.3, G_).astype(np.float32)
    gamma[::5] = 0.0
    q_np = (rng.normal(size=G_) * 0.1).astype(np.float32)
    j0 = G_ // 2
    gamma[j0], q_np[j0] = 0.5, 0.25
    S_np[:, j0] = rng.integers(0, 8, C_)
    ixs = np.stack([rng.choice(C_, n, replace=n > C_) for _ in range(C_)]).astype(np.int32)
    ixs[0, :min(n, 2)] = 0
    w = rng.normal(size=(C_, n)) * 0.1
    w[1] = 0.0
    hi = ops.CellMatrix.from_cells_major(S_np, tdt)
    dev = hi.t.device
    W = torch.as_tensor(w, device=dev).to(tdt)
    g_t = torch.as_tensor(gamma, device=dev)
    worst = 0.0
    for with_q, dt, C_out, permuted in ((True, 1.0, C_, False), (False, 0.37, C_ - 3, True), (True, 0.37, C_ - 3, False), (False, 1.0, C_, True)):
        q_t = torch.as_tensor(q_np, device=dev) if with_q else None
        Uc = U_np[:C_out].copy()
        Uc[:, j0] = 0.5 * S_np[:C_out, j0] + (0.25 if with_q else 0.0)
        Ux = ops.CellMatrix.from_cells_major(Uc, tdt)
        assert Ux.C == C_out
        order = torch.as_tensor(rng.permutation(C_out).astype(np.int32), device=dev) if permuted else None
        dS = ops.velocity_chain(hi.rows(0, C_out), Ux, g_t, q_t, want=("delta_S",), dt_shift=dt)["delta_S"]
        assert bool((dS.t[:, j0] == 0).all()) and bool((dS.t[:, :G_] != 0).any())
        dSm = ops.CellMatrix(torch.zeros_like(hi.t), G_)
        dSm.t[:C_out] = dS.t
        (ref,) = ops.embedding_scaling(hi, dSm, ixs[:C_out], W[:C_out], order=order)
        (got,) = ops.embedding_scaling_fused(hi, Ux, g_t, q_t, ixs[:C_out], W[:C_out], dt_shift=dt, order=order)
        assert got.dtype == torch.float64 and got.shape == (C_out,)
        assert sc.same(got, ref), "the fused fold differs from the kernel on the materialised delta_S"
        (again,) = ops.embedding_scaling_fused(hi, Ux, g_t, q_t, ixs[:C_out], W[:C_out], dt_shift=dt, order=order)
        assert sc.same(again, got)
        cos, N, D, bound = sc.cos_reference(hi.t[:, :G_].cpu().numpy(), Ux.t[:, :G_].cpu().numpy(), gamma, q_np if with_q else None,
                                            ixs[:C_out], W[:C_out].cpu().numpy(), dt)
        g = got.cpu().numpy()
        assert D[1] == 0 and np.isnan(g[1]) and np.array_equal(np.isnan(g), D == 0)
        ok = D > 0
        ratio = np.abs(g - cos)[ok] / bound[ok]
        worst = max(worst, float(ratio.max()))
        assert np.all(np.abs(g - cos)[ok] <= bound[ok]), (float(ratio.max()), int(np.argmax(ratio)))
    print(f"fused scaling {dtype} C={C_} G={G_} n={n}: worst error / bound {worst:.3g}")
    if n == 256:
        wide = np.concatenate([ixs, ixs[:, :1]], 1)
        assert ops.embedding_scaling_fused(hi, Ux, g_t, None, wide[:C_out], torch.zeros((C_out, n + 1), dtype=tdt, device=dev)) is None
        L = ops._lib.lib()
        cosbuf = torch.empty(C_out, dtype=torch.float64, device=dev)
        wz = torch.zeros((C_out, n + 1), dtype=tdt, device=dev)
        wi = torch.as_tensor(wide[:C_out].copy(), device=dev)
        rc = L.vcy_embedding_scaling_fused(hi.t.data_ptr(), Ux.t.data_ptr(), g_t.data_ptr(), None, wi.data_ptr(), wz.data_ptr(), None, cosbuf.data_ptr(),
                                           hi.C, hi.G, hi.ld, C_out, n + 1, 1.0, hi.code, ops._stream())
        assert rc == -3 and b"wider" in L.vcy_last_error()
        rc = L.vcy_embedding_scaling_fused(hi.t.data_ptr(), Ux.t.data_ptr(), None, None, wi.data_ptr(), wz.data_ptr(), None, cosbuf.data_ptr(),
                                           hi.C, hi.G, hi.ld, C_out, n, 1.0, hi.code, ops._stream())
        assert rc == -1 and b"null pointer" in L.vcy_last_error()


# ------------------------------------------------------------------------------------------------------------------ the path
@pytest.mark.parametrize("fit", ["slope", "maxmin_diag"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_one_block_equals_the_resident_recipe(ops, data, pooled, dt, fit):
    from velocyto_amd import analysis
    a = _path(data, block_cells=0, dtype=dt, fit=fit)
    ca, ga, qa = a.run().clone(), a.gamma.clone(), a.q
    assert a.tp is None and a.delta_embedding is None and a._emb_full is None and len(a.stage_ms) == 4 and a.stage_e_ms == 0.0
    b = _path(data, block_cells=0, dtype=dt, fit=fit, shift=True)
    cb = b.run()
    assert sc.same(cb, ca) and torch.equal(b.gamma, ga), "shift=True changed corr or gamma"
    assert (qa is None) == (fit == "slope") and (qa is None or torch.equal(b.q, qa))
    Sx, Ux = pooled[dt]
    assert torch.equal(b._resident[0].t[:C], Sx.t) and torch.equal(b._resident[1].t, Ux.t)
    dS = ops.velocity_chain(Sx, Ux, b.gamma, b.q, want=("delta_S",))["delta_S"]
    fixed = sc.fixed_corr(ops, cb, b.neigh)
    ((tp, de, scl),) = analysis.embedding_shift(Sx, dS, None, b.neigh, b.neigh, fixed, None, data[5], sc.SIGMA, True, 1.0)
    assert b.tp.dtype == dt and b.tp.shape == (C, 40) and b.delta_embedding.shape == (C, 2) and b.scaling.shape == (C,)
    assert sc.same(b.tp, tp) and sc.same(b.delta_embedding, de) and sc.same(b.scaling, scl)
    assert float(torch.isfinite(b.scaling).float().mean()) > 0.99 and float((b.scaling > 0).float().mean()) > 0.5
    assert sc.same(b.delta_embedding, b.delta_embedding_unscaled * b.scaling[:, None])


@pytest.mark.parametrize("fit", ["slope", "maxmin_diag"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_blocks(ops, data, pooled, dt, fit):
    p = _path(data, block_cells=BLOCK, dtype=dt, fit=fit, shift=True)
    assert [b1 - b0 for b0, b1 in p.blocks()] == [397, 397, 397, 309]
    p.run(timed=True)
    assert len(p.stage_ms) == 4 and p.stage_e_ms > 0
    sc.check_shift(ops, *pooled[dt], data[5], _got(p), what=f"four blocks, {dt}, fit={fit}")


def test_options(ops, data, pooled):
    dt = torch.float32
    p = _path(data, block_cells=BLOCK, dtype=dt, shift=True, expression_scaling=False)
    p.run()
    assert p.scaling is None and sc.same(p.delta_embedding, p.delta_embedding_unscaled)
    sc.check_shift(ops, *pooled[dt], data[5], _got(p), what="expression_scaling=False")
    assert p.gathered_shift()[1] is None
    h = _path(data, block_cells=BLOCK, dtype=dt, shift=True, scaling_penalty=2.0)
    h.run()
    sc.check_shift(ops, *pooled[dt], data[5], _got(h), penalty=2.0, what="scaling_penalty=2")
    with pytest.raises(AssertionError):
        _path(data, block_cells=BLOCK, dtype=dt).gathered_shift()


def test_wide_lists_take_the_two_step_route(ops):
    """Lists of 260 > vcy_embedding_scaling_max_neighbors(): the block's delta_S is materialised and pooled (knn_pool + row_cosproj)."""
    c, g = 900, 700
    data = _data(ops, c, g)
    dt = torch.float32
    p = _path(data, n_neighbors=520, block_cells=BLOCK, dtype=dt, fit="maxmin_diag", shift=True)
    assert p.nrndm == 260 > int(ops._lib.lib().vcy_embedding_scaling_max_neighbors()) and len(p.blocks()) == 3
    p.run()
    sc.check_shift(ops, *sc.dense_pool(ops, data, K, dt), data[5], _got(p), what="lists of 260")


def test_garbage_in_the_staging_buffers(ops, data):
    """The staging buffers holding what a caching allocator may hand out before the first block is pooled: stage E reads no row that
    its block has not written."""
    kw = dict(block_cells=BLOCK, dtype=torch.float64, fit="maxmin_diag", shift=True)
    ref = _path(data, **kw)
    ref.run()
    g = _path(data, **kw)
    g._plan_blocks()
    g._ebuf.t[:, :G] = 1e308
    g._ebuf.t[::7, :G] = float("nan")
    g._ubuf.t[:, :G] = float("inf")
    g.run()
    for n in OUT:
        assert sc.same(getattr(g, n), getattr(ref, n)), n


def _run_worker(world, out, cfg, port):
    env = dict(os.environ, VCY_SINGLE_DEVICE="1", VCY_DIST_BACKEND="gloo", MASTER_PORT=str(port), MASTER_ADDR="127.0.0.1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "atlas_shift_worker.py"), out, json.dumps(cfg)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


@pytest.mark.parametrize("world,block_cells,dtype,fit", [(2, 0, "float32", "slope"), (3, 0, "float64", "maxmin_diag"), (2, 300, "float32", "maxmin_diag")])
def test_sharded_ranks(ops, data, pooled, tmp_path, world, block_cells, dtype, fit):
    """2 and 3 ranks on one GPU (gloo transport), once with several blocks per rank: the gathered results meet the checks of the blocks."""
    cfg = dict(C=C, G=G, P=P, k=K, n_neighbors=NN, block_cells=block_cells, dtype=dtype, fit=fit, sigma_corr=sc.SIGMA)
    many = _run_worker(world, str(tmp_path / "many.npz"), cfg, port=29931 + 2 * world + (block_cells > 0))
    assert int(many["world"]) == world and (int(many["blocks"]) == 3 if block_cells else int(many["blocks"]) == 1)
    dev = data[5].device
    got = {n: torch.as_tensor(many[n], device=dev) for n in OUT + ("gamma",)}
    got["q"] = torch.as_tensor(many["q"], device=dev) if many["q"].size else None
    assert (got["q"] is None) == (fit == "slope") and got["tp"].dtype == getattr(torch, dtype)
    sc.check_shift(ops, *pooled[getattr(torch, dtype)], data[5], got, what=f"{world} ranks, block_cells={block_cells}, {dtype}, fit={fit}")


def test_grid_arrows_of_the_atlas_result(ops, oracle, data):
    """atlas.grid_arrows (= analysis.grid_arrows, the body of VelocytoLoom.calculate_grid_arrows) on the gathered one-block result against
    the oracle, at the tolerance of the facade's test on tests/golden/next.npz.  (A cell without an estimate has a NaN arrow, which
    np.percentile would spread over the whole grid in both: such cells count as no shift here.)"""
    from velocyto_amd import atlas
    p = _path(data, block_cells=0, dtype=torch.float32, shift=True)
    p.run()
    de, scl = p.gathered_shift()
    assert de.shape == (C, 2) and scl.shape == (C,) and int(torch.isnan(de).any(1).sum()) <= C // 100
    de = torch.nan_to_num(de, nan=0.0)
    got = atlas.grid_arrows(data[5], de, smooth=0.5, steps=(12, 9), n_neighbors=30)
    ref = oracle.calculate_grid_arrows(data[5].cpu().numpy(), de.cpu().numpy(), smooth=0.5, steps=(12, 9), n_neighbors=30)
    assert got[0].shape == (108, 2) and np.isfinite(ref[1]).all() and float(np.abs(ref[1]).max()) > 0
    for a, b in zip(got, ref):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-14)
