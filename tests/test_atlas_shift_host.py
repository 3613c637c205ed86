"""The reference the GPU tests of the atlas path's stage E lean on, checked where no GPU is needed: atlas_shift_cases.cos_reference
(numpy fp64 in neighbour-list form, with the derived bound) pinned on the dense oracle - oracle.velocity_chain for delta_S, then
oracle.calculate_embedding_shift - and the new public surface (ABI table, ops wrapper, AtlasPath arguments, analysis.grid_arrows)."""
import inspect

import numpy as np
import pytest

import atlas_shift_cases as sc


def _case(rng, C=60, G=45, n=12, with_q=True):
    Sx = rng.gamma(1.0, 2.0, (G, C))
    Ux = rng.gamma(1.0, 1.0, (G, C))
    gamma = rng.gamma(2.0, 0.3, G).astype(np.float32)
    gamma[::7] = 0.0
    q = (rng.normal(size=G) * 0.1).astype(np.float32) if with_q else None
    emb = rng.normal(size=(C, 2))
    ixs = np.stack([rng.choice(np.delete(np.arange(C), c), n, replace=False) for c in range(C)])
    corr = rng.uniform(-0.3, 0.3, (C, C))
    return Sx, Ux, gamma, q, emb, ixs, corr


@pytest.mark.parametrize("with_q,dt_shift,penalty", [(True, 1.0, 1.0), (False, 0.37, 1.0), (True, 0.37, 2.0)])
def test_cos_reference_is_the_dense_oracle(oracle, with_q, dt_shift, penalty):
    rng = np.random.default_rng(11 + with_q)
    Sx, Ux, gamma, q, emb, ixs, corr = _case(rng, with_q=with_q)
    C, n = ixs.shape
    _, _, dS, _ = oracle.velocity_chain(Sx, Ux, gamma, q, delta_t_shift=dt_shift)
    tp, de, scaling = oracle.calculate_embedding_shift(corr, ixs, emb, hi_dim=Sx, delta_S=dS, sigma_corr=sc.SIGMA, scaling_penalty=penalty)
    wdiff = tp[np.arange(C)[:, None], ixs] - 1.0 / n
    cos, N, D, bound = sc.cos_reference(np.ascontiguousarray(Sx.T), np.ascontiguousarray(Ux.T), gamma, q, ixs, wdiff, dt_shift)
    assert np.isfinite(cos).all() and (D > 0).all()
    np.testing.assert_allclose(np.clip(cos / penalty, 0, 1), scaling, rtol=0, atol=1e-12)
    assert 0 < int((scaling > 0).sum()) and int((scaling < 1).sum()) > C // 2          # not clipped away
    np.testing.assert_allclose(cos, N / np.sqrt(D), rtol=0, atol=0)
    # the bound: finite, positive, a few thousand roundoffs of fp64 at this size - and 2^29 times that when the stored values are f32
    assert np.isfinite(bound).all() and (bound > 0).all() and bound.max() < 1e-10
    b32 = sc.cos_reference(np.ascontiguousarray(Sx.T).astype(np.float32), np.ascontiguousarray(Ux.T).astype(np.float32), gamma, q, ixs, wdiff, dt_shift)[3]
    assert 1e-8 < b32.max() < 1e-3


def test_float32_arithmetic_in_the_kernels_order_meets_the_bound():
    """A numpy float32 restatement of what the kernel does to one cell - neighbours added one after the other in float32, delta_S formed in
    float32, the fold in fp64 - stays inside the bound cos_reference derives, with room: the bound is a bound on that arithmetic."""
    rng = np.random.default_rng(5)
    C, G, n = 40, 300, 17
    H = rng.gamma(1.0, 2.0, (C, G)).astype(np.float32)
    U = rng.gamma(1.0, 1.0, (C, G)).astype(np.float32)
    gamma, q = rng.gamma(2.0, 0.3, G).astype(np.float32), (rng.normal(size=G) * 0.1).astype(np.float32)
    ixs = np.stack([rng.choice(C, n, replace=False) for _ in range(C)])
    w = (rng.normal(size=(C, n)) * 0.1).astype(np.float32)
    w[3] = 0.0
    dt = np.float32(0.37)
    est = np.zeros((C, G), dtype=np.float32)
    for k in range(n):
        est = (w[:, k, None].astype(np.float64) * H[ixs[:, k]].astype(np.float64) + est.astype(np.float64)).astype(np.float32)      # one fma
    dS = dt * (U - ((gamma[None, :].astype(np.float64) * H.astype(np.float64) + q[None, :].astype(np.float64)).astype(np.float32)))
    assert dS.dtype == np.float32
    with np.errstate(invalid="ignore"):
        got = (dS.astype(np.float64) * est.astype(np.float64)).sum(1) / np.sqrt((est.astype(np.float64) ** 2).sum(1))
    cos, N, D, bound = sc.cos_reference(H, U, gamma, q, ixs, w, float(dt))
    assert D[3] == 0 and np.isnan(cos[3]) and np.isnan(got[3]) and np.isinf(bound[3])
    ok = D > 0
    ratio = np.abs(got - cos)[ok] / bound[ok]
    assert ratio.max() <= 1.0 and ratio.max() > 1e-4, ratio.max()


def test_the_public_surface_is_there():
    import velocyto_amd
    from velocyto_amd import _lib, analysis, atlas, ops
    res, args = _lib.SIGNATURES["vcy_embedding_scaling_fused"]
    assert len(args) == 16 and _lib.EXPECTED_ABI == 4
    p = inspect.signature(ops.embedding_scaling_fused).parameters
    assert list(p)[:6] == ["hi", "Ux", "gamma", "q", "ixs", "wdiff"] and p["dt_shift"].default == 1.0 and p["order"].default is None
    p = inspect.signature(atlas.AtlasPath.__init__).parameters
    assert (p["shift"].default, p["sigma_corr"].default, p["expression_scaling"].default, p["scaling_penalty"].default) == (False, 0.05, True, 1.0)
    assert list(inspect.signature(analysis.grid_arrows).parameters) == ["embedding", "delta_embedding", "smooth", "steps", "n_neighbors"]
    assert callable(atlas.grid_arrows) and callable(atlas.AtlasPath.gathered_shift)
