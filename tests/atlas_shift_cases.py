"""Shared by tests/test_atlas_shift_host.py and tests/test_gpu_atlas_shift.py: the fp64 reference of the fused expression scaling
(vcy_embedding_scaling_fused) with its derived error bound, the dense pooling the atlas path's blocks are compared with, and the checks
every blocked / sharded run of AtlasPath(shift=True) has to meet.

The bound.  u = unit roundoff of the storage type (2^-24 / 2^-53).  For one cell with weights w_k, neighbour rows x_k, own rows S, U:
    est_g = sum_k w_k x_kg        A_g = sum_k |w_k x_kg|        dS_g = dt (U_g - (gamma_g S_g + q_g))
    N = sum_g dS_g est_g          D = sum_g est_g^2             cos = N / sqrt(D)
The kernel sums est_g recursively in the storage type (n fused multiply-adds: |d est_g| <= n u A_g), forms dS_g with three roundings of
the storage type (|d dS_g| <= 3 u (|U_g| + |gamma_g S_g| + |q_g|), first order) and folds N and D in fp64 over G terms and a tree of
partial sums ((G + 2) 2^-53 relative to the sum of the absolute terms).  First-order propagation through N / sqrt(D):
    bound = n u [ sum_g |dS_g| A_g / sqrt(D) + |N| sum_g |est_g| A_g / D^1.5 ]
          + 3 u sum_g (|U_g| + |gamma_g S_g| + |q_g|) |est_g| / sqrt(D)
          + (G + 2) 2^-53 sum_g |dS_g est_g| / sqrt(D)
Nothing in it is fitted to what the kernel returns."""
import numpy as np

SIGMA = 0.05


def cos_reference(hi, Ux, gamma, q, ixs, wdiff, dt_shift=1.0, chunk=64):
    """numpy fp64 on the STORED values.  hi: (C, G) array of the storage type (its dtype sets u), the cells themselves its first rows;
    Ux: (>= C_out, G); gamma, q: (G) (q may be None); ixs, wdiff: (C_out, n).  Returns (cos, N, D, bound), each (C_out) fp64; a cell
    whose D is 0 has cos = NaN (0 / 0, as the reference's division) and bound = inf."""
    hi = np.asarray(hi)
    u = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}[hi.dtype]
    H = hi.astype(np.float64)
    ixs = np.asarray(ixs).astype(np.int64)
    W = np.asarray(wdiff).astype(np.float64)
    C_out, n = ixs.shape
    G = H.shape[1]
    g = np.asarray(gamma).astype(np.float64)
    qq = np.zeros(G) if q is None else np.asarray(q).astype(np.float64)
    S, U = H[:C_out], np.asarray(Ux)[:C_out].astype(np.float64)
    dS = dt_shift * (U - (g[None, :] * S + qq[None, :]))
    mag = np.abs(U) + np.abs(g[None, :] * S) + np.abs(qq)[None, :]
    Ha = np.abs(H)
    N, D, t1, t2, t3, t4 = (np.zeros(C_out) for _ in range(6))
    for a in range(0, C_out, chunk):
        sl = slice(a, min(C_out, a + chunk))
        est = np.matmul(W[sl, None, :], H[ixs[sl]])[:, 0, :]
        A = np.matmul(np.abs(W[sl, None, :]), Ha[ixs[sl]])[:, 0, :]
        N[sl], D[sl] = (dS[sl] * est).sum(1), (est ** 2).sum(1)
        t1[sl], t2[sl] = (np.abs(dS[sl]) * A).sum(1), (np.abs(est) * A).sum(1)
        t3[sl], t4[sl] = (mag[sl] * np.abs(est)).sum(1), np.abs(dS[sl] * est).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rD = np.sqrt(D)
        cos = N / rD
        bound = n * u * (t1 / rD + np.abs(N) * t2 / D ** 1.5) + 3 * u * t3 / rD + (G + 2) * 2.0 ** -53 * t4 / rD
    bound[D == 0] = np.inf
    return cos, N, D, bound


def dense_pool(ops, data, k, dtype):
    """Sx, Ux of ALL cells by the dense pooling kernel on the densified layers, with the graph AtlasPath builds (the first half of
    test_gpu_atlas.py's _dense_reference, in `dtype`): bit-identical to the path's CSR pooling (test_gpu_atlas.py holds that)."""
    import torch
    cS, cU, fS, fU, pcs, emb = data
    C = cS.C
    idx, dist = ops.knn_search(pcs, k, include_self=False)
    conn = (dist > 0).to(dtype)
    w = torch.cat([torch.ones((C, 1), device=idx.device, dtype=dtype), conn], 1)
    w = w / w.sum(1, keepdim=True)
    ind = torch.cat([torch.arange(C, device=idx.device, dtype=torch.int32)[:, None], idx], 1)
    ind, w = ops.canonical_graph_rows(ind, w)
    ptr = torch.arange(0, (C + 1) * (k + 1), k + 1, device=idx.device, dtype=torch.int64)
    return ops.knn_pool_counts(cS.to_dense(), cU.to_dense(), fS, fU, ptr, ind, w, dtype=dtype, validate=False)


def same(a, b):
    """Bit-for-bit with NaNs matched (two tensors of one dtype)."""
    import torch
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


def fixed_corr(ops, corr, neigh, cell0=0):
    """The NaN -> 1 copy stage E works on (analysis.py:1604-1607)."""
    fixed = corr.clone()
    ops.corr_fixup(fixed, neigh, cell0=cell0, zero_self=True, fix_nan=True, nan_to=1.0)
    return fixed


def check_shift(ops, Sx, Ux, emb, got, penalty=1.0, what=""):
    """The three checks of a blocked or sharded run against the expectation built from its OWN stored outputs.  got: corr, gamma, q
    (or None), neigh, tp, delta_embedding, delta_embedding_unscaled, scaling (or None) of ALL cells as device tensors; Sx, Ux: the
    densely pooled matrices of all cells in the run's dtype.
      1. tp and delta_embedding_unscaled bit-identical to ONE ops.transition_prob call over all cells with global numbers;
      2. scaling within cos_reference's bound of clip(cos_reference / penalty, 0, 1) (clipping is 1-Lipschitz); cells whose bound is
         >= 1e-3 or whose reference D is exactly 0 are left out of the value check - at most 1 % of the cells, asserted - and the
         D == 0 cells must be NaN on the device;
      3. delta_embedding == delta_embedding_unscaled * scaling[:, None] exactly.
    Returns the worst observed error / bound."""
    G = Sx.G
    fixed = fixed_corr(ops, got["corr"], got["neigh"])
    tp, wd, de = ops.transition_prob(fixed, got["neigh"], emb, SIGMA, cell0=0)
    assert same(got["tp"], tp), f"{what}: tp differs from one transition_prob call over all cells"
    assert same(got["delta_embedding_unscaled"], de), f"{what}: the unscaled shift differs from one transition_prob call over all cells"
    if got["scaling"] is None:
        assert same(got["delta_embedding"], de)
        return 0.0
    q = None if got["q"] is None else got["q"].cpu().numpy()
    cos, N, D, bound = cos_reference(Sx.t[:, :G].cpu().numpy(), Ux.t[:, :G].cpu().numpy(), got["gamma"].cpu().numpy(), q,
                                     got["neigh"].cpu().numpy(), wd.cpu().numpy(), 1.0)
    sc = got["scaling"].cpu().numpy()
    zero = D == 0
    left = zero | ~(bound < 1e-3)
    assert np.isnan(sc[zero]).all(), f"{what}: a cell with a zero estimate must be NaN"
    share = float(left.mean())
    ref = np.clip(cos / penalty, 0, 1)
    err = np.abs(sc - ref)[~left]
    ratio = err / bound[~left]
    print(f"{what}: scaling in [{np.nanmin(sc):.3g}, {np.nanmax(sc):.3g}], {100 * float((sc > 0).mean()):.0f} % positive; left out {int(left.sum())} "
          f"of {left.size} cells; largest bound {bound[~left].max():.3g}, largest error {err.max():.3g}, worst error / bound {ratio.max():.3g}")
    assert share <= 0.01, f"{what}: {share:.3%} of the cells are left out of the value check"
    assert np.all(err <= bound[~left]), (what, int(np.nanargmax(ratio)), float(np.nanmax(ratio)), int(np.isnan(err).sum()))
    assert same(got["delta_embedding"], got["delta_embedding_unscaled"] * got["scaling"][:, None]), f"{what}: delta_embedding is not unscaled * scaling"
    return float(ratio.max())
