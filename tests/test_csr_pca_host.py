"""CPU-side checks of the PCA-from-CSR layer: the two C-ABI entries refuse bad arguments before they touch a device, the host
queries answer, and the index plumbing of CsrCounts.transposed (ops.transpose_csr works on host tensors too) gives scipy's
transpose for any block size."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def L():
    import velocyto_amd
    velocyto_amd.build()
    from velocyto_amd import _lib
    return _lib.lib()


# any non-null value: validation must fail before a pointer is followed
P = 0x1000


def _spmm(lib, **kw):
    a = dict(indptr=P, indices=P, data=P, scale=P, B=P, out=P, ws=P, R=4, N=5, nnz=3, max_row=0, L=2, ldb=2, ldo=2, pcount=1.0, scale_on=0, code=3)
    a.update(kw)
    return lib.vcy_csr_lognorm_spmm(a["indptr"], a["indices"], a["data"], a["scale"], a["B"], a["out"], a["ws"], a["R"], a["N"], a["nnz"], a["max_row"], a["L"],
                                  a["ldb"], a["ldo"], a["pcount"], a["scale_on"], a["code"], None)


def _stats(lib, **kw):
    a = dict(indptr=P, indices=P, data=P, scale=P, stats=P, ws=P, R=4, N=5, nnz=3, max_row=0, pcount=1.0, scale_on=1, code=2)
    a.update(kw)
    return lib.vcy_csr_lognorm_stats(a["indptr"], a["indices"], a["data"], a["scale"], a["stats"], a["ws"], a["R"], a["N"], a["nnz"], a["max_row"], a["pcount"],
                                   a["scale_on"], a["code"], None)


@pytest.mark.parametrize("bad", [dict(L=0), dict(L=-3), dict(code=0), dict(code=1), dict(code=7), dict(indptr=None), dict(indices=None),
                                 dict(data=None), dict(scale=None), dict(B=None), dict(out=None), dict(scale_on=2), dict(scale_on=-1),
                                 dict(R=0), dict(N=0), dict(nnz=-1), dict(ldb=1), dict(ldo=1), dict(pcount=0.0), dict(pcount=-1.0),
                                 dict(nnz=10 ** 6, ws=None), dict(nnz=10 ** 6, ws=None, max_row=5000), dict(max_row=-1)])
def test_spmm_refuses_bad_arguments_without_a_device(L, bad):
    assert _spmm(L, **bad) == -1, bad
    assert L.vcy_last_error()


@pytest.mark.parametrize("bad", [dict(code=0), dict(code=9), dict(indptr=None), dict(indices=None), dict(data=None), dict(scale=None),
                                 dict(stats=None), dict(scale_on=2), dict(scale_on=-1), dict(R=0), dict(N=0), dict(nnz=-1), dict(pcount=0.0),
                                 dict(nnz=10 ** 6, ws=None), dict(nnz=10 ** 6, ws=None, max_row=5000), dict(max_row=-1)])
def test_stats_refuses_bad_arguments_without_a_device(L, bad):
    assert _stats(L, **bad) == -1, bad
    assert L.vcy_last_error()


def test_chunk_and_workspace_queries(L):
    chunk = int(L.vcy_csr_spmm_chunk())
    assert chunk >= 64 and chunk % 64 == 0
    # no row can be longer than a chunk: nothing to add up afterwards, no workspace
    assert L.vcy_csr_spmm_workspace_bytes(0, 50) == 0 and L.vcy_csr_spmm_workspace_bytes(chunk, 50) == 0
    # one slot of L doubles for every multiple of the chunk length below nnz (a further chunk follows a full chunk, which holds one)
    for nnz in (chunk + 1, 2 * chunk, 2 * chunk + 1, 10 * chunk + 3):
        assert L.vcy_csr_spmm_workspace_bytes(nnz, 50) == ((nnz - 1) // chunk + 1) * 50 * 8
    assert L.vcy_csr_spmm_workspace_bytes(5 * chunk, 0) == 0


@pytest.mark.parametrize("C,G,density,block_nnz", [(1, 5, 1.0, 1 << 20), (37, 130, 0.2, 1 << 20), (37, 130, 0.2, 50), (300, 53, 0.3, 700),
                                                   (40, 9, 0.0, 16), (64, 64, 0.5, 1)])
def test_transpose_csr_index_plumbing_on_the_host(C, G, density, block_nnz):
    """The cursor arithmetic across row blocks, empty rows / genes, a block size below one row's length: scipy's transpose."""
    import scipy.sparse as sp
    import velocyto_amd
    from velocyto_amd import ops
    rng = np.random.default_rng(C * 1000 + G)
    dense = (rng.random((C, G)) < density) * rng.integers(1, 65536, (C, G))
    if C > 2:
        dense[C // 2] = 0                                                 # an empty cell
    if G > 2:
        dense[:, G // 3] = 0                                              # an empty gene
    a = sp.csr_matrix(dense.astype(np.int64))
    a.sort_indices()
    dat = torch.from_numpy(a.data.astype(np.uint16).view(np.int16))
    ptr, idx, val = ops.transpose_csr(torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(a.indices.astype(np.int32)), dat, G,
                                      block_nnz=block_nnz)
    t = sp.csr_matrix(a.T)
    t.sort_indices()
    assert ptr.dtype == torch.int64 and idx.dtype == torch.int32 and val.dtype == torch.int16
    assert np.array_equal(ptr.numpy(), t.indptr) and np.array_equal(idx.numpy(), t.indices)
    assert np.array_equal(val.numpy().view(np.uint16), t.data.astype(np.uint16))
