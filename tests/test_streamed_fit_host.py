"""StreamedFit without a GPU: the walk plan of every fit_gammas mode, argument validation, and the ABI row of the fused moments."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = {torch.float32: 4, torch.float64: 8}           # vcy_gene_select_passes: one walk per 8-bit digit of the key
NO_OFFSET_FIXED = dict(fit_offset=False, fixperc_q=True)
# (arguments, select phases): the rows of the plan table in streamed_fit's docstring
PLAN = [
    (dict(weighted=False), 0),
    (dict(weighted=False, fit_offset=False), 0),
    (dict(weighted=False, limit_gamma=True), 0),                         # unweighted fits know no limit_gamma
    (dict(weighted=False, fixperc_q=True), 0),                           # fixperc_q is ignored with fit_offset=True
    (dict(weighted=False, **NO_OFFSET_FIXED), 2),
    *[(dict(weights=w), 1) for w in ("sum", "prod", "maxmin", "maxmin_weighted")],
    *[(dict(weights=w, limit_gamma=True), 2) for w in ("sum", "prod", "maxmin", "maxmin_weighted")],
    *[(dict(weights=w, **NO_OFFSET_FIXED), 2) for w in ("sum", "prod", "maxmin", "maxmin_weighted")],
    *[(dict(weights=w, fit_offset=False), 1) for w in ("sum", "maxmin")],
    *[(dict(weights=w, fixperc_q=True), 1) for w in ("prod", "maxmin_weighted")],
    *[(dict(weights=w, **opt), 2) for w in ("maxmin_diag", "maxmin_double")
      for opt in ({}, dict(limit_gamma=True), NO_OFFSET_FIXED, dict(fit_offset=False), dict(fit_offset=False, limit_gamma=True))],
]


@pytest.fixture(scope="module")
def sf():
    import velocyto_amd
    velocyto_amd.build()
    from velocyto_amd import streamed_fit
    return streamed_fit


@pytest.mark.parametrize("dt", list(P))
@pytest.mark.parametrize("kw,phases", PLAN, ids=[str(i) for i in range(len(PLAN))])
def test_n_walks_of_every_row_of_the_plan(sf, kw, phases, dt):
    fit = sf.StreamedFit(200, 1200, dt, "cpu", **kw)
    assert fit.n_walks == phases * P[dt] + 1, kw
    assert fit.passes == P[dt] and fit.walk == 0 and fit.n_fit_cells == 1200


def test_the_default_is_the_default_fit(sf):
    fit = sf.StreamedFit(200, 1200, torch.float32, "cpu")
    assert (fit.weighted, fit.weights, fit.fit_offset, fit.fixperc_q, fit.limit_gamma, fit.perc, fit.power) == (True, "maxmin_diag", True, False, False,
                                                                                                         [2.0, 98.0], 15.0)
    assert not fit.need_up and not fit.need_qf and fit.n_walks == 9


def test_argument_validation(sf):
    mk = lambda **kw: sf.StreamedFit(200, 1200, torch.float32, "cpu", **kw)
    for bad in ("maxmin_diagonal", "", None, 3):
        with pytest.raises(ValueError, match=re.escape(f"weights={bad!r} is not supported")):
            mk(weights=bad)
    for arr in (np.ones((200, 1200)), torch.ones(2, 2)):
        with pytest.raises(ValueError, match="never sees a whole"):
            mk(weights=arr)
    mk(weighted=False, weights="anything")                                # as in the facade: not looked at without weighted
    for n in (0, 1201, -1):
        with pytest.raises(ValueError, match="n_fit_cells"):
            mk(n_fit_cells=n)
    with pytest.raises(ValueError, match="n_total"):
        sf.StreamedFit(200, 0, torch.float32, "cpu")
    with pytest.raises(ValueError, match="two percentiles"):
        mk(maxmin_perc=(2, 50, 98))
    fit = mk(weighted=False)
    with pytest.raises(RuntimeError, match="0 of 1 walks done"):
        fit.result()


def test_the_scaled_routes_re_export_the_driver(sf):
    from velocyto_amd import atlas, sharded
    assert atlas.StreamedFit is sf.StreamedFit and sharded.StreamedFit is sf.StreamedFit


def test_the_fused_moments_row_is_in_header_table_and_guide():
    from velocyto_amd import _lib
    name = "vcy_fit_weighted_moments_fused"
    hdr = open(os.path.join(ROOT, "include", "velocyto_hip.h")).read()
    m = re.search(r"int " + name + r"\(([^;]*)\);", hdr)
    assert m, "not declared in velocyto_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["Y", "X", "fused_mode", "S", "U", "pa", "pb", "pc", "pd", "sa", "sb", "power", "cell_mask",
                                                           "moments", "workspace", "C", "G", "ld", "dtype", "stream"]
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params)
    assert hasattr(_lib.lib(), name)
    assert _lib.lib().vcy_abi_version() == 4                               # a pure addition
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"`{name}(Y, X, fused_mode, S, U, pa, pb, pc, pd, sa, sb, power, cell_mask, moments, ws, C, G, ld, dtype, stream)`" in guide


def test_fused_moments_validate_their_arguments_without_a_gpu():
    from velocyto_amd import _lib
    L = _lib.lib()
    import ctypes
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ok = dict(mode=0, U=p, pc=p, C=4, G=1, ld=1, dtype=0)
    def call(**kw):
        a = dict(ok, **kw)
        return L.vcy_fit_weighted_moments_fused(p, p, a["mode"], p, a["U"], p, p, a["pc"], a["pc"], a["pc"], a["pc"], 15.0, None, p, p, a["C"], a["G"],
                                                a["ld"], a["dtype"], None)
    for bad in (dict(mode=4), dict(mode=-1), dict(U=None), dict(mode=3, pc=None), dict(C=0), dict(G=0), dict(ld=0), dict(dtype=9)):
        assert call(**bad) != 0, bad
