"""CPU-side checks of the device t-SNE (no GPU needed): argument validation of its C entry points, the parameter errors
DeviceTSNE raises before it touches the device (scikit-learn's), and perform_TSNE's backend keyword with its unchanged default."""
import types

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    import velocyto_amd
    velocyto_amd.build()
    from velocyto_amd import _lib
    return _lib.lib()


def test_tsne_entry_points_refuse_null_pointers(L):
    assert L.vcy_tsne_perplexity(None, None, None, 10, 5, 30.0, None) == -1
    assert b"null pointer" in L.vcy_last_error()
    assert L.vcy_tsne_gradient(None, None, None, None, None, None, None, 10, 2, 1, None) == -1
    assert b"null pointer" in L.vcy_last_error()
    assert L.vcy_tsne_step(None, None, None, None, None, None, None, None, None, 10, 2, 0.5, 50.0, 0.01, 1, None) == -1
    assert b"null pointer" in L.vcy_last_error()
    assert L.vcy_tsne_workspace_bytes(1000, 2) > 0
    assert L.vcy_tsne_workspace_bytes(1000, 4) == 0 and L.vcy_tsne_workspace_bytes(1, 2) == 0
    # both trees: N = 10, n_components = 2, angle 0.5; the parameters are (depth,) = (2,) and (leaf_size, max_depth) = (8, 24)
    for tree, par in (("tree", (2,)), ("atree", (8, 24))):
        calls = {"keys": (3, (10, *par)),
                 "repulsion": (7, (10, *par, 0.5)),
                 "gradient": (9, (10, 2, *par, 0.5, 1)),
                 "step": (11, (10, 2, *par, 0.5, 0.5, 50.0, 0.01, 1))}
        for what, (n_pointers, rest) in calls.items():
            assert getattr(L, f"vcy_tsne_{tree}_{what}")(*[None] * n_pointers, *rest, None) == -1, (tree, what)
            assert b"null pointer" in L.vcy_last_error(), (tree, what)
    assert L.vcy_tsne_tree_workspace_bytes(10, 2) > 0
    assert L.vcy_tsne_atree_workspace_bytes(10, 8, 24) > 0


@pytest.mark.parametrize("kw,n,exc,msg", [
    (dict(perplexity=40.0), 40, ValueError, r"perplexity \(40.0\) must be less than n_samples \(40\)"),
    (dict(n_components=4), 100, ValueError, "inferior to 4"),
    (dict(n_components=0), 100, ValueError, "n_components"),
    (dict(max_iter=100), 100, ValueError, "max_iter"),
    (dict(init="pca"), 100, NotImplementedError, "pca"),
    (dict(init=np.zeros((99, 2))), 100, ValueError, "init has shape"),
])
def test_device_tsne_parameter_errors_come_before_the_device(kw, n, exc, msg):
    from velocyto_amd.tsne import DeviceTSNE
    X = np.random.default_rng(0).normal(size=(n, 5))
    with pytest.raises(exc, match=msg):
        DeviceTSNE(**kw).fit_transform(X)


def test_perform_tsne_backend_keyword():
    from velocyto_amd.preprocess import PreprocessMixin
    sklearn_manifold = pytest.importorskip("sklearn.manifold")
    X = np.random.default_rng(1).normal(size=(60, 6))
    with pytest.raises(ValueError, match="backend"):
        PreprocessMixin.perform_TSNE(types.SimpleNamespace(pcs=X), backend="cuda")
    # the default is still scikit-learn's TSNE, unchanged
    obj = types.SimpleNamespace(pcs=X)
    np.random.seed(3)
    PreprocessMixin.perform_TSNE(obj, perplexity=10, max_iter=250)
    np.random.seed(3)
    ref = sklearn_manifold.TSNE(n_components=2, perplexity=10, angle=0.5, init="random", max_iter=250).fit_transform(X)
    assert np.array_equal(obj.ts, ref)
