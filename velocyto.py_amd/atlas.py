"""The hot path at atlas scale: knn_imputation -> fit_slope -> velocity chain -> colDeltaCor on SPARSE count layers,
streamed over cell blocks, cells sharded over ranks with NOTHING of cell-count size replicated in dense form.

BASELINE.json configs[4] / SURVEY.md section 8(e), last row: 1M cells x 30k genes, CSR input at ~8 % density.  The reference
cannot run this size: it loads every layer as a dense float64 (G, C) array (analysis.py:59-61; 240 GB per layer) and pools
with a dense x sparse product (neighbors.py:416-423).  The arithmetic below is the reference's, stage by stage, with the
same kernels as the resident path (bench.py `Pipeline`); what changes is where the rows live:

  counts   CSR per rank for its own cells (ops.CsrCounts) plus the COUNT-ROW HALO: the rows of every cell whose pooled
           vector the rank will need (its cells' sampled embedding neighbours) and of those cells' kNN neighbours.  A count
           row is ~12 KB (2400 non-zeros x 5 B) where a pooled row is 120 KB, so ranks exchange count rows ONCE per dataset
           (HaloPlan.fetch_ragged) and afterwards pool every row of e = Sx_sz they read themselves: no dense row ever
           crosses a link, e is sharded by construction, pcs / size factors travel as small vectors.
  A        vcy_knn_pool_csr merges the k + 1 sparse rows of a cell into a dense f32 row (LDS slab per wave), block by block.
  B        fit_slope moments of the rank's own cells, summed over blocks, all-reduced (3 G doubles).  AtlasPath(fit="maxmin_diag"):
           velocyto's default weighted fit instead - its per-gene percentiles from an exact select streamed over the blocks
           (ops.StreamedGeneQuantiles: integer histograms, all-reduced), then the weighted moments (10 G doubles) and the boxed solve.
           fit_gammas' fit_offset / fixperc_q / limit_gamma / steady_state_bool ride on the same walks: their conditional percentiles
           from the masked select (ops.StreamedMaskedGeneQuantiles), the moments over the steady-state cells.
  C + D    per block: e rows = [block | sampled neighbours outside the block], pooled on the spot when the matrices are not
           resident; vcy_coldeltacor_partial_fused on the block with renumbered neighbour lists.

One block that holds all of a rank's cells = the resident mode (Sx, Ux kept between the passes; the layout 8 x 288 GB
affords at 1M cells); smaller blocks trade a second pooling pass for O(block) memory, which lets ONE GPU walk a dataset
whose dense matrices exceed its HBM.  Results do not depend on the block size or on the number of ranks (tests).
"""
from __future__ import annotations

import math
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import distributed as D
from . import ops
from .streamed_fit import StreamedFit, check_weights

KEY_CHUNK = 4096          # cells per deterministic block of the synthetic generator and of the sampling keys
PRUNE_FROM = 100_000      # cells from which the kNN search in the PCA space is projection-pruned (AtlasPath(knn="auto"))


def _keyed_uniform(rows0: int, rows1: int, ncol: int, seed: int, dev) -> torch.Tensor:
    """float64 uniforms for global rows rows0..rows1-1, identical on every rank and for every sharding: row r comes from the
    generator of its KEY_CHUNK-row chunk."""
    out = torch.empty((rows1 - rows0, ncol), dtype=torch.float64, device=dev)
    for ch in range(rows0 // KEY_CHUNK, (rows1 - 1) // KEY_CHUNK + 1):
        gen = torch.Generator(device=dev).manual_seed(int(seed) * 1000003 + ch)
        blk = torch.rand((KEY_CHUNK, ncol), generator=gen, device=dev, dtype=torch.float64)
        a, b = max(rows0, ch * KEY_CHUNK), min(rows1, (ch + 1) * KEY_CHUNK)
        out[a - rows0:b - rows0] = blk[a - ch * KEY_CHUNK:b - ch * KEY_CHUNK]
    return out


def sample_neighbors(emb_full: torch.Tensor, c0: int, c1: int, n_neighbors: int, sampled_fraction: float,
                     sampling_probs=(0.5, 0.1), seed: int = 15071990) -> torch.Tensor:
    """estimate_transition_prob's neighbour subsample (analysis.py:1547-1572) for cells c0..c1-1: the n_neighbors + 1
    nearest cells in the embedding (query excluded), of which int(sampled_fraction * (n_neighbors + 1)) are drawn without
    replacement with probabilities falling linearly from sampling_probs[0] to [1] with the rank (Efraimidis-Spirakis keys;
    the reference draws with numpy's legacy stream on the host - replayed exactly by ops.choice_stream_host in the facade;
    at atlas scale the draw is keyed by the global cell number so that it does not depend on the sharding).  Rows are
    returned sorted by neighbour number (a pair's value does not depend on its column)."""
    dev = emb_full.device
    n1 = n_neighbors + 1
    idx, _ = ops.knn_search(emb_full, n1, include_self=False, q0=c0, Q=c1 - c0)
    p = torch.linspace(sampling_probs[0], sampling_probs[1], n1, device=dev, dtype=torch.float64)
    p = p / p.sum()
    m = int(sampled_fraction * n1)
    out = torch.empty((c1 - c0, m), dtype=torch.int32, device=dev)
    step = 16384
    for s in range(c0, c1, step):
        e = min(c1, s + step)
        keys = torch.log(_keyed_uniform(s, e, n1, seed, dev)) / p[None, :]
        sel = torch.topk(keys, m, dim=1).indices
        out[s - c0:e - c0] = torch.sort(torch.gather(idx[s - c0:e - c0], 1, sel), dim=1).values
    return out.contiguous()


class AtlasPath:
    """One rank's share of the path.  The rank owns the cells c0 .. c0 + cS.C - 1 of a dataset of C_total cells whose labels
    follow a space-filling curve of the embedding, e.g. ops.hilbert_order (so that blocks and shards are spatially coherent:
    a block's sampled neighbours mostly lie inside it and the halos stay small; any labelling gives the same numbers)."""

    def __init__(self, cS: ops.CsrCounts, cU: ops.CsrCounts, fS: torch.Tensor, fU: torch.Tensor, pcs: torch.Tensor, embedding: torch.Tensor, *,
                 c0: int = 0, C_total: Optional[int] = None, k: int = 30, n_neighbors: int = 500, sampled_fraction: float = 0.5,
                 sampling_probs=(0.5, 0.1), block_cells: int = 0, dtype=torch.float32, psc: float = 1e-10, seed: int = 15071990,
                 knn: str = "auto", fit: str = "slope", shift: bool = False, sigma_corr: float = 0.05, expression_scaling: bool = True,
                 scaling_penalty: float = 1.0, balanced: bool = False, b_sight: Optional[int] = None, b_maxl: Optional[int] = None,
                 group_constraint=None, fit_offset: bool = True, fixperc_q: bool = False, limit_gamma: bool = False, steady_state_bool=None,
                 weighted: bool = True, weights="maxmin_diag", maxmin_perc=(2, 98), maxmin_weighted_pow: float = 15):
        """fit: how stage B fits gamma.  "slope" (the default): gamma = max(0, sum xy / sum xx), unweighted, no offset (fit_slope,
        estimation.py:267-279).  "maxmin_diag" (or "default"): velocyto's default fit_gammas(weights="maxmin_diag", fit_offset=True)
        (analysis.py:1179-1257), the recipe of VelocytoLoom.fit_gammas and ShardedLoom.fit_gammas, with the per-gene percentiles
        taken by a streamed exact select (ops.StreamedGeneQuantiles): 9 walks over the pooled blocks in f32, 17 in f64.
        fit_offset, fixperc_q, limit_gamma, steady_state_bool (fit="maxmin_diag" only; anything but the defaults with fit="slope" is a
        ValueError): VelocytoLoom.fit_gammas' options of these names with weighted=True, weights="maxmin_diag" (analysis.py:1120-1260).
        fit_offset=True: the box fit, with up_gamma = estimation._median_and_up_gamma when limit_gamma (fixperc_q is ignored);
        fit_offset=False, fixperc_q=True: the offset fixed to estimation._fixperc_q, gamma in [0, 20] (limit_gamma is ignored);
        fit_offset=False, fixperc_q=False: no offset, gamma in [1e-8, up_gamma] with limit_gamma, else in [0, 20].
        steady_state_bool: a bool mask over the rank's own cells or over all C cells (None or all-true: all cells).  As in the facade
        the weights' thresholds are taken over all cells; the limit_gamma / fixperc_q percentiles and the moments over the masked
        cells only.  Their conditional percentiles come from the masked streamed select (ops.StreamedMaskedGeneQuantiles) in the
        walks the default fit already makes: the number of walks does not change.  With none of the four given the run is bit for
        bit the default fit's.
        weighted, weights, maxmin_perc, maxmin_weighted_pow (fit="maxmin_diag" only, like the four above): VelocytoLoom.fit_gammas'
        arguments of these names - weights one of "sum", "prod", "maxmin", "maxmin_weighted", "maxmin_diag", "maxmin_double" (anything
        else is the facade's ValueError; the weight mode never travels in fit=), or weighted=False.  The walk plan per mode is
        streamed_fit.StreamedFit's; the non-binary weights are formed inside the moments fold (ops.fit_weighted_moments_fused), never
        as a block-sized matrix.  With the defaults the run is bit for bit the default fit's.
        shift: also calculate_embedding_shift (analysis.py:1670-1733, stage E) with sigma_corr, expression_scaling and scaling_penalty
        as there, block by block while the block is in the staging buffers: run() then leaves tp, delta_embedding, scaling and
        delta_embedding_unscaled of the rank's own cells (see _stage_e); delta_S is never formed.
        balanced: pool over the balanced kNN graph (BalancedKNN, neighbors.py:186-357) instead of the plain one.  b_sight and b_maxl
        default to 8 k and 4 k, the recipe of default_fit_preparation (analysis.py:1942-1977) - NOT knn_imputation's own default of
        the whole dataset, whose (C, C) sight lists a million cells cannot hold.  Every rank searches the sight lists of its own cells,
        the int32 lists are all-gathered (C x (b_sight + 1) x 4 bytes per rank) and balanced on every rank's device
        (ops.balance_knn_positions; its rounds and fallback go to knn_stats).  group_constraint: one label per cell (all C cells, or the
        rank's own): picks stay inside a cell's group.  With balanced=False the path is bit for bit what it is without these."""
        if fit not in ("slope", "maxmin_diag", "default"):
            raise ValueError(f"AtlasPath: unknown fit={fit!r} (\"slope\", \"maxmin_diag\" or \"default\")")
        self.fit = "slope" if fit == "slope" else "maxmin_diag"
        self.fit_offset, self.fixperc_q, self.limit_gamma = bool(fit_offset), bool(fixperc_q), bool(limit_gamma)
        self.weighted, self.weights, self.maxmin_weighted_pow = bool(weighted), weights, float(maxmin_weighted_pow)
        self.maxmin_perc = tuple(float(p) for p in maxmin_perc)
        other_weights = (not self.weighted or not (isinstance(weights, str) and weights == "maxmin_diag") or self.maxmin_perc != (2.0, 98.0)
                         or self.maxmin_weighted_pow != 15.0)
        if self.fit == "slope" and (not self.fit_offset or self.fixperc_q or self.limit_gamma or steady_state_bool is not None or other_weights):
            raise ValueError("AtlasPath: fit_offset, fixperc_q, limit_gamma and steady_state_bool belong to fit=\"maxmin_diag\", and so do "
                             "weighted, weights, maxmin_perc and maxmin_weighted_pow; fit=\"slope\" has no offset, no weights and no "
                             "steady-state cells")
        if self.weighted:
            check_weights(weights)
        self.dev = dev = cS.indptr.device
        self.knn_mode = knn
        self.dtype = ops.resolve_dtype(dtype)
        self.G, self.k, self.psc = cS.G, int(k), float(psc)
        self.rules = None                  # ops.partial_rules_for(...) from the all-reduced whole-matrix facts of the first pass
        self.rank, self.world = D.world()
        self.c0, self.nloc = int(c0), cS.C
        self.c1 = self.c0 + self.nloc
        self.C = int(C_total) if C_total is not None else self.nloc
        assert cU.C == self.nloc and cU.G == self.G and fS.numel() == self.nloc and pcs.shape[0] == self.nloc and embedding.shape[0] == self.nloc
        if self.world > 1:
            assert (self.c0, self.c1) == D.shard_bounds(self.C, self.world, self.rank), "cells must be sharded by distributed.shard_bounds"
        self.block_cells = int(block_cells) if block_cells and block_cells > 0 else self.nloc
        # ---- small replicated vectors: the kNN space and the embedding of ALL cells (C x (P + 2) doubles: 256 MB at 1M cells)
        pcs_full = D.all_gather_rows(pcs.double().contiguous(), self.C)
        emb_full = D.all_gather_rows(embedding.double().contiguous(), self.C)
        # ---- kNN graph of the own cells (analysis.py:1005-1010): nearest-first, self excluded; weights (knn > 0) with diag = 1
        self.knn_stats: Dict[str, float] = {}
        if group_constraint is not None and not balanced:
            raise ValueError("group_constraint is supported only with balanced=True")
        idx, dist_ = self._balanced_knn(pcs_full, b_sight, b_maxl, group_constraint) if balanced else self._knn(pcs_full)
        conn = (dist_ > 0).to(self.dtype)
        wrow = torch.cat([torch.ones((self.nloc, 1), device=dev, dtype=self.dtype), conn], 1)
        wrow = (wrow / wrow.sum(1, keepdim=True)).contiguous()
        grow = torch.cat([torch.arange(self.c0, self.c1, device=dev, dtype=torch.int32)[:, None], idx], 1)               # global cell numbers
        grow, wrow = ops.canonical_graph_rows(grow, wrow)       # pooled in ascending GLOBAL cell number: scipy's order, and independent of the sharding
        # ---- sampled embedding neighbours of the own cells (global numbers)
        self.neigh = sample_neighbors(emb_full, self.c0, self.c1, n_neighbors, sampled_fraction, sampling_probs, seed)
        self.nrndm = int(self.neigh.shape[1])
        self._pcs_full = pcs_full
        self.shift, self.sigma_corr = bool(shift), float(sigma_corr)
        self.expression_scaling, self.scaling_penalty = bool(expression_scaling), float(scaling_penalty)
        self._emb_full = emb_full if self.shift else None       # stage E reads the neighbours' coordinates (C x 2 doubles: 16 MB at 1M cells)
        del emb_full
        # ---- E rows: the rows of e = Sx_sz this rank reads = own cells + sampled neighbours owned elsewhere (e_out, ascending)
        need_e = torch.zeros(self.C, dtype=torch.bool, device=dev)
        need_e[self.neigh.reshape(-1).long()] = True
        need_e[self.c0:self.c1] = True
        plan_e = D.HaloPlan(need_e, self.C)
        self.e_out = plan_e.recv_idx.clone()                                          # global numbers, ascending
        grow_e = torch.cat([grow, plan_e.fetch(grow)], 0)                             # graph rows of the E rows, own first
        wrow_e = torch.cat([wrow, plan_e.fetch(wrow)], 0)
        # ---- K rows: the COUNT rows needed to pool every E row = own + everything the E rows' graph rows name
        need_k = torch.zeros(self.C, dtype=torch.bool, device=dev)
        need_k[grow_e.reshape(-1).long()] = True
        need_k[self.c0:self.c1] = True
        plan_k = D.HaloPlan(need_k, self.C)
        self.k_out = plan_k.recv_idx.clone()
        self.n_count_halo, self.n_e_halo = int(self.k_out.numel()), int(self.e_out.numel())

        def with_halo(c: ops.CsrCounts, f: torch.Tensor):
            lens = c.indptr[1:] - c.indptr[:-1]
            lens_h, idx_h, dat_h = plan_k.fetch_ragged(lens, c.indices, c.data)
            ptr = torch.zeros(self.nloc + lens_h.numel() + 1, dtype=torch.int64, device=dev)
            torch.cumsum(torch.cat([lens, lens_h]), 0, out=ptr[1:])
            return (ops.CsrCounts(ptr, torch.cat([c.indices, idx_h]), torch.cat([c.data, dat_h]), c.G),
                    torch.cat([f.double().contiguous(), plan_k.fetch(f.double().contiguous().reshape(-1, 1)).reshape(-1)]))
        self.cS, self.fS = with_halo(cS, fS)
        self.cU, self.fU = with_halo(cU, fU)
        # graph of the E rows in the row numbering of the local count CSR ([own | k_out])
        self.g_idx = ops.localize_rows(grow_e, self.c0, self.c1, self.k_out)           # (n_E, k + 1) int32
        self.g_w = wrow_e
        self.kp1 = self.k + 1
        self.corr = torch.empty((self.nloc, self.nrndm), dtype=self.dtype, device=dev)
        self.gamma = None
        self.q = self.R2 = None            # fit="maxmin_diag": the offset and the weighted R2 of the fit (float32, like gamma)
        self.fit_thresholds = None         # ... and its per-gene float64 thresholds {"denom_S", "denom_U", "down", "up"} (other weights:
        #     see streamed_fit.StreamedFit - "sum"/"prod" {"p99_S", "p99_U"}, "maxmin"/"maxmin_weighted" {"down_S", "up_S"}, "maxmin_double" both); with
        #     limit_gamma also {"med_S", "p90_S", "med_U", "U_p10_above", "S_med_above", "n_above" (int64: cells with Sx > p90_S),
        #     "up_gamma"}, with fixperc_q {"p1_S", "n_below" (int64: cells with Sx <= p1_S), "q_fixed"} - over the steady-state cells
        self.fit_moments = None            # ... and the all-reduced (10, G) moments they were solved from
        self.select_state_bytes = 0        # ... and the bytes the streamed select held at its peak
        self._ss, self.n_fit_cells = self._steady_state(steady_state_bool)      # uint8 (nloc) or None = all cells; the cells the fit is over
        self._blk = (0, self.nloc)         # the rows of the block _data_pass handed out last
        self._in_buf = None                # the block whose own rows the staging buffers hold
        self.stage_ms = np.zeros(4)
        self.stage_e_ms = 0.0              # shift=True, run(timed=True): milliseconds of stage E (kept out of stage_ms)
        self.tp = self.delta_embedding = self.delta_embedding_unscaled = self.scaling = None
        if self.shift:
            edim = int(self._emb_full.shape[1])
            self.tp = torch.empty((self.nloc, self.nrndm), dtype=self.dtype, device=dev)
            self.delta_embedding = torch.empty((self.nloc, edim), dtype=torch.float64, device=dev)
            self.delta_embedding_unscaled = torch.empty((self.nloc, edim), dtype=torch.float64, device=dev)
            if self.expression_scaling:
                self.scaling = torch.empty(self.nloc, dtype=torch.float64, device=dev)
        self._resident = None
        self._plan = None
        self.peak_block_bytes = 0

    def _steady_state(self, ss) -> Tuple[Optional[torch.Tensor], int]:
        """steady_state_bool as (the uint8 mask of the rank's own cells or None for all cells, the number of masked cells of all ranks)."""
        if ss is None:
            return None, self.C
        m = torch.as_tensor(np.asarray(ss))
        if m.dtype != torch.bool or m.ndim != 1 or m.numel() not in (self.nloc, self.C):
            raise ValueError(f"AtlasPath: steady_state_bool must be a 1-d bool mask over the rank's own {self.nloc} cells or over all {self.C} cells")
        if m.numel() != self.nloc:
            m = m[self.c0:self.c1]
        m = m.to(self.dev)
        n = int(D.all_reduce_sum(m.sum().reshape(1).to(torch.int64)).item())
        if n == 0:
            raise ValueError("AtlasPath: steady_state_bool selects no cell")
        return (None if n == self.C else m.to(torch.uint8).contiguous()), n

    def _knn(self, pcs_full: torch.Tensor):
        """Exact kNN of the own cells among all cells: brute force up to PRUNE_FROM cells, projection-pruned beyond (the
        brute-force search is O(C^2): about 2 s per pass at 1M cells; the pruned one evaluated 10 % of the pairs there, 388 ms,
        and returns the same lists, ops.knn_search_pruned)."""
        if self.knn_mode == "pruned" or (self.knn_mode == "auto" and self.C >= PRUNE_FROM):
            return ops.knn_search_pruned(pcs_full, self.k, q0=self.c0, Q=self.nloc, stats=self.knn_stats)
        return ops.knn_search(pcs_full, self.k, include_self=False, q0=self.c0, Q=self.nloc)

    def _balanced_knn(self, pcs_full: torch.Tensor, b_sight, b_maxl, group_constraint):
        """The balanced graph's rows of the own cells in the form _knn returns: (picks (nloc, k) int32, their distances).  A slot the
        sight could not fill holds the cell itself at distance 0, which the weights (distance > 0) turn into weight 0."""
        k, C = self.k, self.C
        sight = 8 * k if b_sight is None else int(b_sight)
        maxl = 4 * k if b_maxl is None else int(b_maxl)
        K = min(sight + 1, C)                                           # the query included, as BalancedKNN.kneighbors searches
        own = torch.arange(self.c0, self.c1, device=self.dev)
        if self.knn_mode == "pruned" or (self.knn_mode == "auto" and C >= PRUNE_FROM):
            # the pruned search excludes the query: the self column (distance 0) goes in front - the same lists, given no duplicate cells
            idx, dist_ = ops.knn_search_pruned(pcs_full, K - 1, q0=self.c0, Q=self.nloc, stats=self.knn_stats)
            idx = torch.cat([own.to(torch.int32)[:, None], idx], 1)
            dist_ = torch.cat([torch.zeros((self.nloc, 1), dtype=dist_.dtype, device=self.dev), dist_], 1)
        else:
            idx, dist_ = ops.knn_search(pcs_full, K, include_self=True, q0=self.c0, Q=self.nloc)
        groups = None
        if group_constraint is not None:
            groups = (group_constraint if isinstance(group_constraint, torch.Tensor) else torch.as_tensor(np.asarray(group_constraint))
                      ).to(self.dev, torch.int64)
            if groups.numel() == self.nloc and self.nloc != C:
                groups = D.all_gather_rows(groups.contiguous(), C)
            if groups.numel() != C:
                raise ValueError("AtlasPath: group_constraint needs one label per cell (all cells, or the rank's own)")
        lists = D.all_gather_rows(idx.contiguous(), C)
        st: Dict[str, float] = {}
        pos, dsi_new, _ = ops.balance_knn_positions(lists, maxl, k, groups, stats=st)
        del lists
        self.knn_stats.update(balance_rounds=st["rounds"], balance_fell_back=st["fell_back"], b_sight=sight, b_maxl=maxl)
        dsi_own = dsi_new[self.c0:self.c1]
        dist_own = ops.balance_distances(dist_, pos[self.c0:self.c1], dsi_own, own)
        return dsi_own[:, 1:].to(torch.int32).contiguous(), dist_own[:, 1:].contiguous()

    # ------------------------------------------------------------------ pooling of arbitrary E rows
    def _e_rows_of(self, g: torch.Tensor) -> torch.Tensor:
        """E-row numbers ([own | e_out]) of global cell numbers."""
        return ops.localize_rows(g, self.c0, self.c1, self.e_out).long()

    def _pool(self, counts: ops.CsrCounts, scale: torch.Tensor, erows, out: ops.CellMatrix) -> None:
        """out[i, :] = pooled vector of E row erows[i] (a slice = contiguous E rows, or an int64 tensor)."""
        if isinstance(erows, slice):
            gi, gw = self.g_idx[erows], self.g_w[erows]
        else:
            gi, gw = self.g_idx.index_select(0, erows), self.g_w.index_select(0, erows)
        n = int(gi.shape[0])
        if n == 0:
            return
        indptr = torch.arange(0, (n + 1) * self.kp1, self.kp1, device=self.dev, dtype=torch.int64)
        ops.knn_pool_csr(counts, scale, indptr, gi.reshape(-1), gw.reshape(-1), dtype=self.dtype, C_out=n, out=out, validate=False)

    def blocks(self) -> List[Tuple[int, int]]:
        return [(b, min(self.nloc, b + self.block_cells)) for b in range(0, self.nloc, self.block_cells)]

    def _plan_blocks(self) -> None:
        """Per block, once per graph: the e rows it reads outside itself (E-row numbers, ascending global number) and its
        neighbour lists in the numbering of its buffer [block | outside]; and the two buffers every block reuses."""
        self._plan = []
        single = len(self.blocks()) == 1
        max_rows, max_nb = 0, 0
        for (b0, b1) in self.blocks():
            nb_ix = self.neigh[b0:b1]
            if single:
                erows_out = torch.arange(self.nloc, self.nloc + self.n_e_halo, device=self.dev)
                ixs = ops.localize_rows(nb_ix, self.c0, self.c1, self.e_out)
            else:
                g = torch.unique(nb_ix.reshape(-1).long())                           # ascending global numbers
                outside = g[(g < self.c0 + b0) | (g >= self.c0 + b1)]
                erows_out = self._e_rows_of(outside)
                ixs = ops.localize_rows(nb_ix, self.c0 + b0, self.c0 + b1, outside)
            self._plan.append((b0, b1, erows_out, ixs))
            max_rows, max_nb = max(max_rows, (b1 - b0) + int(erows_out.numel())), max(max_nb, b1 - b0)
        self._ebuf = ops.CellMatrix.empty(max_rows, self.G, self.dtype)
        self._ubuf = ops.CellMatrix.empty(max_nb, self.G, self.dtype)
        self.peak_block_bytes = (self._ebuf.t.numel() + self._ubuf.t.numel()) * self._ebuf.t.element_size()

    # ------------------------------------------------------------------ one pass of the path
    def _gather_facts(self, Sx_b: ops.CellMatrix, facts: dict) -> None:
        """The scale facts of e = Sx_sz over ALL cells of ALL ranks, block by block, on the first walk over the data."""
        if self.dtype == torch.float64:       # the f64 sqrt element's domain: max |Sx| of every pooled block - the matrix itself, never
            lo, hi = Sx_b.t.aminmax()         # the staging buffer (its halo rows are not written yet on the first pass); judged after
            m = torch.maximum(lo.abs(), hi.abs()).double().reshape(1)     # the all-reduce below, by every rank alike
            facts["absmax"] = m if facts["absmax"] is None else torch.maximum(facts["absmax"], m)
        st, abs_st = ops.abs_stats(Sx_b), facts["abs_st"]
        facts["abs_st"] = st if abs_st is None else torch.stack([abs_st[0] + st[0], torch.minimum(abs_st[1], st[1]), abs_st[2] + st[2]])

    def _decide_rules(self, facts: dict) -> None:
        # stage D's branch rule is decided ONCE from whole-matrix reductions, all-reduced: identical on every rank and for
        # every block size (a per-block or per-rank decision could differ on borderline data)
        abs_st, absmax = facts["abs_st"], facts["absmax"]
        if abs_st is None:                      # a rank without a block still takes part in the all-reduce: the neutral element
            abs_st = torch.tensor([0.0, float("inf"), 0.0], dtype=torch.float64, device=self._ebuf.t.device)
        stats = D.all_reduce_abs_stats(abs_st)
        if self.dtype == torch.float64:
            D.check_f64_sqrt_domain(torch.zeros(1, dtype=torch.float64, device=self._ebuf.t.device) if absmax is None else absmax)
        self.rules = ops.partial_rules_for(self._ebuf, ops.SQRT, self.psc, stats=stats, cells=self.C, domain_checked=True)

    # ------------------------------------------------------------------ stage B, velocyto's default fit, from streamed blocks
    def _data_pass(self, i_pass: int, n_passes: int, use, ev, timed: bool, tms: List[float]) -> None:
        """Walk number i_pass of n_passes over the rank's blocks: every block is pooled into the staging buffers - unless its rows are
        there already: one block = resident mode, nothing is pooled twice - and handed to use(Sx_b, Ux_b); S and U share the walk.
        The walks alternate their direction, so a walk starts on the block the one before ended on, and the last one runs forwards:
        pass 2 then finds the last block in the buffers, as after fit="slope".  Times: pooling of the first walk -> tms[0] (stage A),
        every later pooling and all use -> tms[1] (stage B)."""
        nblk = len(self._plan)
        order = range(nblk) if (n_passes - 1 - i_pass) % 2 == 0 else range(nblk - 1, -1, -1)
        for bi in order:
            b0, b1 = self._plan[bi][0], self._plan[bi][1]
            nb = b1 - b0
            ev[0].record()
            Sx_b, Ux_b = self._ebuf.rows(0, nb), self._ubuf.rows(0, nb)
            self._blk = (b0, b1)
            if self._in_buf != bi:
                self._pool(self.cS, self.fS, slice(b0, b1), Sx_b)
                self._pool(self.cU, self.fU, slice(b0, b1), Ux_b)
                self._in_buf = bi
            ev[1].record()
            use(Sx_b, Ux_b)
            ev[2].record()
            if timed:
                torch.cuda.synchronize()
                tms[0 if i_pass == 0 else 1] += ev[0].elapsed_time(ev[1]); tms[1] += ev[1].elapsed_time(ev[2])

    def _fit_maxmin_diag(self, ev, timed: bool, tms: List[float]) -> Tuple[torch.Tensor, torch.Tensor]:
        """fit_gammas (analysis.py:1179-1257) over blocks: the walks of streamed_fit.StreamedFit, fed from the staging buffers.  With the
        default weights="maxmin_diag" three phases: (1) percentiles [99.9, 100] of Sx and of Ux -> the denominators of
        VelocytoLoom._maxnorm_denominator; (2) percentiles [2, 98] of Sx/dS + Ux/dU -> the binary weights' thresholds; (3) the weighted
        moments, all-reduced and solved in the box.  Phases 1 and 2 take one walk per 8-bit digit of the key each; limit_gamma /
        fixperc_q ride on the same walks (masked selects over the steady-state cells).  The other weight modes: StreamedFit's plan."""
        facts = {"abs_st": None, "absmax": None}
        fit = StreamedFit(self.G, self.C, self.dtype, self.dev, weighted=self.weighted, weights=self.weights, fit_offset=self.fit_offset,
                          fixperc_q=self.fixperc_q, limit_gamma=self.limit_gamma, maxmin_perc=self.maxmin_perc,
                          maxmin_weighted_pow=self.maxmin_weighted_pow, n_fit_cells=self.n_fit_cells)
        cmask = lambda: None if self._ss is None else self._ss[self._blk[0]:self._blk[1]]      # of the block being used

        def timed_(f):
            ev[0].record()
            out = f()
            ev[1].record()
            if timed:
                torch.cuda.synchronize()
                tms[1] += ev[0].elapsed_time(ev[1])
            return out

        for i_pass in range(fit.n_walks):
            first = i_pass == 0 and self.rules is None

            def use(Sx_b, Ux_b):
                fit.add_block(Sx_b, Ux_b, cell_mask=cmask())
                if first:
                    self._gather_facts(Sx_b, facts)
            self._data_pass(i_pass, fit.n_walks, use, ev, timed, tms)
            if first:
                self._decide_rules(facts)
            timed_(fit.end_walk)
        gamma, q, R2 = timed_(fit.result)
        self.fit_thresholds, self.fit_moments, self.select_state_bytes = fit.thresholds, fit.moments, fit.state_bytes
        self.q, self.R2 = q, R2
        return gamma, q

    # ------------------------------------------------------------------ stage E of one block
    def _stage_e(self, b0: int, b1: int, e_buf: ops.CellMatrix, Ux_b: ops.CellMatrix, gamma: torch.Tensor, q: Optional[torch.Tensor],
                 ixs: torch.Tensor) -> None:
        """calculate_embedding_shift (analysis.py:1670-1733) for the block b0..b1-1 whose correlation rows were just written, while
        e_buf = [block | outside rows] and Ux_b still hold it: transition probabilities and the unscaled shift from the NaN -> 1 copy of
        the rows (:1604-1607; self.corr keeps its NaNs) with the GLOBAL neighbour numbers, the expression scaling from the block's
        local lists with delta_S formed in the kernel's fold (vcy_embedding_scaling_fused)."""
        nb = b1 - b0
        neigh = self.neigh[b0:b1]
        fixed = self.corr[b0:b1].clone()
        ops.corr_fixup(fixed, neigh, cell0=self.c0 + b0, zero_self=True, fix_nan=True, nan_to=1.0)
        tp, wd, de = ops.transition_prob(fixed, neigh, self._emb_full, self.sigma_corr, cell0=self.c0 + b0)
        self.tp[b0:b1] = tp
        self.delta_embedding_unscaled[b0:b1] = de
        if not self.expression_scaling:
            self.delta_embedding[b0:b1] = de
            return
        cos = ops.embedding_scaling_fused(e_buf, Ux_b, gamma, q, ixs, wd, validate=False)
        if cos is None:
            # lists wider than the kernel sorts: the block's delta_S is materialised after all and takes embedding_shift's two-step route
            from .analysis import expression_cos
            dS = ops.velocity_chain(e_buf.rows(0, nb), Ux_b, gamma, q, want=("delta_S",))["delta_S"]
            cos = expression_cos(e_buf, [dS], ixs, [wd])
            del dS
        sc = torch.clamp(cos[0] / self.scaling_penalty, 0, 1)                              # NaN stays NaN, like np.clip
        self.scaling[b0:b1] = sc
        self.delta_embedding[b0:b1] = de * sc[:, None]

    def run(self, timed: bool = False) -> torch.Tensor:
        """One pass of the path; returns the rank's correlation rows.  timed=True adds the stages' milliseconds to stage_ms =
        [A pooling, B fit, A kNN search, D].  With fit="maxmin_diag" stage B includes everything its extra walks over the data
        cost, the re-pooling of the blocks in streamed mode too; only the first walk's pooling counts as stage A.  shift=True: stage E
        of every block follows its stage D (results in tp, delta_embedding, scaling, delta_embedding_unscaled); its milliseconds go to
        stage_e_ms."""
        dev, G = self.dev, self.G
        if self._plan is None:
            self._plan_blocks()
        single = len(self._plan) == 1
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        tA = tB = tD = tK = tE = 0.0
        # ---- A, first half: the exact kNN search of the own cells among all cells (analysis.py:1005).  The graph of a dataset
        #      does not change between passes - the count-row halo was built from it - but the search is part of
        #      knn_imputation and of the metric, so every pass repeats it
        ev[0].record()
        self._knn(self._pcs_full)
        ev[1].record()
        if timed:
            torch.cuda.synchronize()
            tK = ev[0].elapsed_time(ev[1])
        self._in_buf = None
        if self.fit == "slope":
            # ---- pass 1: A (pooling of the own cells) + B (fit_slope moments, estimation.py:267-279), block by block
            mom = torch.zeros((3, G), dtype=torch.float64, device=dev)
            facts = {"abs_st": None, "absmax": None}
            for (b0, b1, erows_out, ixs) in self._plan:
                nb = b1 - b0
                ev[0].record()
                Sx_b, Ux_b = self._ebuf.rows(0, nb), self._ubuf.rows(0, nb)
                self._pool(self.cS, self.fS, slice(b0, b1), Sx_b)
                self._pool(self.cU, self.fU, slice(b0, b1), Ux_b)
                ev[1].record()
                mom += ops.fit_slope_moments(Ux_b, Sx_b)
                ev[2].record()
                if self.rules is None:                    # first pass only
                    self._gather_facts(Sx_b, facts)
                if timed:
                    torch.cuda.synchronize()
                    tA += ev[0].elapsed_time(ev[1]); tB += ev[1].elapsed_time(ev[2])
            if self.rules is None:
                self._decide_rules(facts)
            ev[0].record()
            D.all_reduce_sum(mom)
            gamma = ops.fit_slope_from_moments(mom)
            gamma[~torch.isfinite(gamma)] = 0.0          # fit_gammas' policy for genes without signal (analysis.py:1260); NaN would poison every d[c]
            ev[1].record()
            if timed:
                torch.cuda.synchronize()
                tB += ev[0].elapsed_time(ev[1])
            q = None
        else:                                        # the same stages A + B with velocyto's default fit: 2 x passes + 1 walks over the blocks
            tms = [0.0, 0.0]
            gamma, q = self._fit_maxmin_diag(ev, timed, tms)
            assert self._in_buf == len(self._plan) - 1
            tA += tms[0]; tB += tms[1]
        self.gamma = gamma
        # ---- pass 2: C + D per block.  e rows = [block | sampled neighbours outside the block].  The blocks are walked
        #      backwards: the block pass 1 pooled last is still in the buffers and is not pooled again (one block = resident
        #      mode: nothing is pooled twice, only the halo rows are added)
        for n_done, (b0, b1, erows_out, ixs) in enumerate(reversed(self._plan)):
            nb, n_out = b1 - b0, int(erows_out.numel())
            ev[0].record()
            e_buf, Ux_b = self._ebuf.rows(0, nb + n_out), self._ubuf.rows(0, nb)
            if n_done > 0:
                self._pool(self.cS, self.fS, slice(b0, b1), e_buf.rows(0, nb))
                self._pool(self.cU, self.fU, slice(b0, b1), Ux_b)
            self._pool(self.cS, self.fS, erows_out, e_buf.rows(nb, nb + n_out))
            ev[1].record()
            ops.coldeltacor_partial_fused(e_buf, Ux_b, gamma, q, ixs, ops.SQRT, self.rules, self.psc, cell0=0, u_row0=0,
                                          out=self.corr[b0:b1], validate=False)
            ev[2].record()
            if self.shift:
                self._stage_e(b0, b1, e_buf, Ux_b, gamma, q, ixs)
                ev[3].record()
            if timed:
                torch.cuda.synchronize()
                tA += ev[0].elapsed_time(ev[1]); tD += ev[1].elapsed_time(ev[2])
                if self.shift:
                    tE += ev[2].elapsed_time(ev[3])
        if single:
            self._resident = (self._ebuf, self._ubuf)
        if timed:
            self.stage_ms += np.array([tA, tB, tK, tD])
            self.stage_e_ms += tE
        return self.corr

    def gathered_corr(self) -> torch.Tensor:
        """All cells' correlation rows on every rank (the RCCL all-gather north_star names)."""
        return D.all_gather_rows(self.corr, self.C)

    def gathered_shift(self) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """All cells' (delta_embedding, scaling) on every rank after a run with shift=True; scaling is None without expression_scaling."""
        assert self.shift, "AtlasPath(shift=True) computes the embedding shift"
        return (D.all_gather_rows(self.delta_embedding, self.C),
                None if self.scaling is None else D.all_gather_rows(self.scaling, self.C))


def grid_arrows(embedding, delta_embedding, smooth: float = 0.5, steps: Tuple = (40, 40), n_neighbors: int = 100):
    """calculate_grid_arrows (analysis.py:1735-1816) on gathered atlas results - the embedding of all cells and
    AtlasPath.gathered_shift()[0]: (flow_grid, flow, flow_norm, flow_norm_magnitude, total_p_mass) of analysis.grid_arrows; 40 x 40
    arrows are what one draws for a million cells."""
    from .analysis import grid_arrows as _grid_arrows
    to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return _grid_arrows(to_np(embedding), to_np(delta_embedding), smooth, steps, n_neighbors)


def memory_plan(C: int, G: int, nnz_per_cell: float, world: int, block_cells: int, nrndm: int = 250, k: int = 30, count_bytes: int = 1,
                elem_bytes: int = 4, halo_e: float = 0.1, halo_k: float = 0.25, fit: str = "slope", b_sight: int = 0, fit_offset: bool = True,
                fixperc_q: bool = False, limit_gamma: bool = False) -> Dict[str, float]:
    """Bytes one rank holds (GB).  halo_e / halo_k: E and count-row halos as fractions of the rank's own cells (measured:
    tools/halo_fraction.py, AtlasPath.n_e_halo / n_count_halo).  fit="maxmin_diag" adds the state of the streamed select at its
    peak (phase 1: three ranks - both of percentile 99.9 and the maximum - of Sx and of Ux): per (rank, gene) a 256-bin uint32
    histogram, an 8-byte key prefix and a 4-byte rank; it does not grow with the cell count.  fit_offset / fixperc_q / limit_gamma
    (AtlasPath's) add the masked selects that share phase 1: percentiles [50, 90] of Sx and [50] of Ux with limit_gamma, [1] of Sx
    with fixperc_q - two such ranks per percentile, plus 8 bytes of fraction per percentile and 8 of population.  b_sight > 0 (AtlasPath(balanced=True)) adds
    the gathered int32 sight lists of ALL cells, C x (b_sight + 1) x 4 bytes, held while the graph is balanced."""
    lists = C * (b_sight + 1) * 4 if b_sight > 0 else 0
    select = 0 if fit == "slope" else 2 * 3 * G * (256 * 4 + 8 + 4)
    msel = lambda nq: G * (2 * nq * (256 * 4 + 8 + 4) + nq * 8 + 8)
    if fit != "slope" and limit_gamma and (fit_offset or not fixperc_q):
        select += msel(2) + msel(1)
    elif fit != "slope" and fixperc_q and not fit_offset:
        select += msel(1)
    nloc = math.ceil(C / world)
    ld = ops.padded_ld(G)
    blk = min(block_cells if block_cells > 0 else nloc, nloc)
    csr = 2 * (nloc * (1 + halo_k)) * (nnz_per_cell * (4 + count_bytes) + 8 + 4 * (G // 2048 + 2))
    dense_block = (2 * blk + blk * (halo_e if blk == nloc else 0.6)) * ld * elem_bytes
    gb = lambda x: x / 1e9
    return {"cells_per_rank": nloc, "csr_layers_with_halo_GB": gb(csr), "pcs_embedding_replicated_GB": gb(C * 32 * 8),
            "graph_and_neighbour_lists_GB": gb(nloc * (1 + halo_e) * (k + 1) * 8 + nloc * nrndm * 4), "block_Sx_Ux_GB": gb(dense_block),
            "corr_rows_GB": gb(nloc * nrndm * elem_bytes), "kNN_workspace_GB": gb(8192 * C * 4), "fit_select_histograms_GB": gb(select),
            "balanced_sight_lists_GB": gb(lists),
            "total_GB": gb(csr + C * 32 * 8 + dense_block + nloc * nrndm * (4 + elem_bytes) + 8192 * C * 4 + select + lists)}


# ---------------------------------------------------------------------------------------------------------------------------
# synthetic atlas: the generator of bench.py's dense dataset in block-keyed form, so that any rank can produce
# exactly its own cells; counts are thinned to the requested density and stored CSR
def synth_atlas(C: int, G: int, P: int, dev, density: float = 0.08, c0: int = 0, c1: Optional[int] = None, seed: int = 20180812):
    """Returns (cS, cU, totS, totU, pcs_own, emb_own) for cells c0..c1-1 of a C-cell dataset whose labels already follow
    the Hilbert curve of the embedding.  Identical for every (c0, c1) split."""
    c1 = C if c1 is None else c1
    gen = torch.Generator(device=dev).manual_seed(seed)
    alpha = torch.exp(torch.randn(G, generator=gen, device=dev))
    gam = torch.exp(-0.5 + 0.5 * torch.randn(G, generator=gen, device=dev))
    t_on = torch.rand(G, generator=gen, device=dev) * 0.7
    switching = (torch.rand(G, generator=gen, device=dev) < 0.6).float()
    branch_gene = (torch.rand(G, generator=gen, device=dev) < 0.3).float()
    # latent state of ALL cells (small vectors), embedding, curve order
    t = torch.rand(C, generator=gen, device=dev)
    branch = (torch.rand(C, generator=gen, device=dev) < 0.5).float()
    size = torch.exp(0.3 * torch.randn(C, generator=gen, device=dev))
    wob = torch.randn((C, 2), generator=gen, device=dev, dtype=torch.float64)
    emb = torch.stack([t.double() * 10.0, (branch.double() * 2 - 1) * torch.clamp(t.double() - 0.5, min=0) * 8.0], 1) + 0.35 * wob
    perm = ops.hilbert_order(emb.contiguous()).long()
    t, branch, size, emb = t[perm], branch[perm], size[perm], emb[perm].contiguous()
    noise = torch.randn((C, P - 2), generator=gen, device=dev, dtype=torch.float64)[perm] * 0.05
    pcs = torch.cat([emb, noise], 1).contiguous()

    def rates(s, e):
        tt = t[s:e, None]
        tau = torch.clamp(tt - t_on[None, :], min=0.0) * switching[None, :] + (1 - switching[None, :]) * 1.0
        gate = 1.0 - branch_gene[None, :] * branch[s:e, None] * (tt > 0.5).float()
        u = alpha[None, :] * (1 - torch.exp(-4.0 * tau)) * gate
        sp = (alpha / gam)[None, :] * (1 - torch.exp(-2.0 * gam[None, :] * tau)) * gate
        return 0.3 * size[s:e, None] * u, size[s:e, None] * sp
    # thinning factor for the requested density of the spliced layer, calibrated on the first chunk (deterministic)
    _, lam = rates(0, min(C, KEY_CHUNK))
    lo, hi = 1e-6, 10.0
    for _ in range(40):
        mid = math.sqrt(lo * hi)
        if float((1 - torch.exp(-mid * lam)).mean()) > density:
            hi = mid
        else:
            lo = mid
    thin = math.sqrt(lo * hi)
    ld = ops.padded_ld(G)
    parts = {"S": [], "U": []}
    for ch in range(c0 // KEY_CHUNK, (c1 - 1) // KEY_CHUNK + 1):
        s, e = ch * KEY_CHUNK, min(C, (ch + 1) * KEY_CHUNK)
        g2 = torch.Generator(device=dev).manual_seed(seed * 7919 + ch)
        lu, ls = rates(s, e)
        cu = torch.poisson(thin * lu, generator=g2).clamp_(max=65535)
        cs = torch.poisson(thin * ls, generator=g2).clamp_(max=65535)
        a, b = max(c0, s) - s, min(c1, e) - s
        for name, m in (("S", cs), ("U", cu)):
            d = torch.zeros((b - a, ld), dtype=torch.int16, device=dev)
            d[:, :G] = m[a:b].to(torch.int32).to(torch.int16)
            parts[name].append(ops.CsrCounts.from_dense(ops.CountMatrix(d, G).narrowed()))

    def cat(ps):
        wide = any(p.data.dtype == torch.int16 for p in ps)
        ptr, base = [torch.zeros(1, dtype=torch.int64, device=dev)], 0
        for p in ps:
            ptr.append(p.indptr[1:] + base)
            base += p.nnz
        return ops.CsrCounts(torch.cat(ptr), torch.cat([p.indices for p in ps]),
                             torch.cat([(p.data.to(torch.int16) if wide else p.data) for p in ps]), G)
    cS, cU = cat(parts["S"]), cat(parts["U"])
    return cS, cU, cS.row_sums(), cU.row_sums(), pcs[c0:c1].contiguous(), emb[c0:c1].contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# gene selection from the CSR count layers: velocyto's score_detection_levels / score_cv_vs_mean / score_cluster_expression /
# filter_genes on the rank's shards (cells sharded as in AtlasPath).  The per-gene statistics are exact integers (vcy_csr_gene_stats),
# so their all-reduce gives the one-rank bits whatever the sharding; the host arithmetic behind them is the facade's own
# (preprocess.detection_mask, cv_vs_mean_from_stats, cluster_averages) and runs replicated on identical inputs: every function
# returns numpy arrays that are the same on every rank.
def total_cells(c: ops.CsrCounts) -> int:
    """Cells of the whole dataset: the ranks' shard sizes added."""
    n = torch.tensor([float(c.C)], dtype=torch.float64, device=c.indptr.device)
    D.all_reduce_sum(n)
    return int(round(float(n[0])))


def gene_stats(c: ops.CsrCounts, cell_mask=None) -> np.ndarray:
    """(4, G) float64 [sum, sum of squares, expressing cells, max] per gene over ALL ranks' cells (of the masked ones), on the host."""
    st = ops.csr_gene_stats(c, cell_mask)
    if D.active():
        D.all_reduce_sum(st[:3])
        D.all_reduce_max(st[3])
    return st.cpu().numpy()


def score_detection_levels(cS: ops.CsrCounts, cU: ops.CsrCounts, min_expr_counts: float = 50, min_cells_express: float = 20,
                           min_expr_counts_U: float = 0, min_cells_express_U: float = 0) -> np.ndarray:
    """analysis.py:456-475 on CSR layers: the facade's detection_level_selected."""
    from .preprocess import detection_mask
    return detection_mask(gene_stats(cS), gene_stats(cU), min_expr_counts, min_cells_express, min_expr_counts_U, min_cells_express_U)


def _selected_cells(c: ops.CsrCounts, cell_mask) -> int:
    """Cells of the whole dataset that cell_mask keeps (all of them when it is None): the ranks' numbers added."""
    mask = ops._csr_cell_mask(c, cell_mask)
    n = torch.tensor([c.C if mask is None else int((mask != 0).sum())], dtype=torch.int64, device=c.indptr.device)
    D.all_reduce_sum(n)
    return int(n[0])


def _same_width(c: ops.CsrCounts) -> ops.CsrCounts:
    """The layer with uint16 counts when ANY rank's shard holds them (a shard narrows on its own; the select's passes must agree)."""
    wide = torch.tensor([1.0 if c.code == ops.U16 else 0.0], dtype=torch.float64, device=c.indptr.device)
    D.all_reduce_max(wide)
    if float(wide[0]) == 0.0 or c.code == ops.U16:
        return c
    w = ops.CsrCounts(c.indptr, c.indices, c.data.to(torch.int16), c.G)
    w._slabptr = c._slabptr
    return w


def _gene_percentiles(c: ops.CsrCounts, qs, cell_mask, n_total: int) -> torch.Tensor:
    if n_total == 0:
        raise ValueError("gene_percentiles: no cell is selected")
    c = _same_width(c)
    sel = ops.CsrGeneQuantiles(c.G, qs, n_total, c.code == ops.U16, c.indptr.device)
    while not sel.done:
        sel.add_block(c, cell_mask)
        sel.advance()
    return sel.result()


def gene_percentiles(c: ops.CsrCounts, qs, cell_mask=None) -> np.ndarray:
    """np.percentile(dense layer, qs, axis=cells) -> (len(qs), G) float64 over ALL ranks' cells (of the masked ones), zeros included, on
    the host: ops.CsrGeneQuantiles with the integer histograms all-reduced between the digit passes, so the bits are the one-rank
    bits for any sharding."""
    return _gene_percentiles(c, qs, cell_mask, _selected_cells(c, cell_mask)).cpu().numpy()


def check_winsor_perc(winsor_perc) -> Tuple[float, float]:
    try:
        w = [float(v) for v in winsor_perc]
    except (TypeError, ValueError):
        w = []
    if len(w) != 2 or not (0.0 <= w[0] <= w[1] <= 100.0):
        raise ValueError(f"winsor_perc must be two ascending percentiles in [0, 100], got {winsor_perc!r}")
    return w[0], w[1]


def winsorized_gene_stats(c: ops.CsrCounts, winsor_perc=(1, 99.5), cell_mask=None) -> Tuple[np.ndarray, np.ndarray]:
    """analysis.py:262-267 on a CSR layer: (moments, bounds) on the host - bounds (2, G) = the two per-gene percentiles, moments (4, G) =
    [sum, sum of squares, count(> 0), max] of the counts clipped to them, over ALL ranks' cells (of the masked ones).  The integer parts
    (ops.csr_gene_stats_parts) are all-reduced and folded afterwards (ops.csr_gene_stats_clip): the one-rank bits for any sharding."""
    winsor_perc = check_winsor_perc(winsor_perc)
    n_total = _selected_cells(c, cell_mask)
    q = _gene_percentiles(c, winsor_perc, cell_mask, n_total)
    parts = ops.csr_gene_stats_parts(c, cell_mask, q[0], q[1])
    if D.active():
        D.all_reduce_sum(parts[:5])
        D.all_reduce_max(parts[5])
    return ops.csr_gene_stats_clip(parts, n_total, q[0], q[1]).cpu().numpy(), q.cpu().numpy()


def score_cv_vs_mean(c: ops.CsrCounts, C_total: Optional[int] = None, N: int = 3000, min_expr_cells: int = 2, max_expr_avg: float = 20,
                     min_expr_avg: float = 0, svr_gamma: Optional[float] = None, sort_inverse: bool = False,
                     winsorize: bool = False, winsor_perc=None) -> Tuple[np.ndarray, np.ndarray]:
    """analysis.py:201-345 on a CSR layer: (score, mask) = the facade's (cv_mean_score, cv_mean_selected); the SVR noise model
    (preprocess.DeviceSVR) is fitted on every rank on the same points.  C_total: cells of the whole dataset (all-reduced when None).
    winsor_perc = (lower, upper) switches the winsorisation on, whatever `winsorize` says (the mean and the spread are those of the
    counts clipped to the gene's two percentiles, winsorized_gene_stats); winsorize=True without it still raises NotImplementedError."""
    if winsor_perc is None and winsorize:
        raise NotImplementedError("score_cv_vs_mean(winsorize=True) on CSR layers: name the per-gene percentiles, winsor_perc=(lower, upper) "
                                  "(the reference's default is (1, 99.5)); winsorize alone stays refused on this route")
    from .preprocess import cv_vs_mean_from_stats
    moments = None
    if winsor_perc is not None:
        winsor_perc = check_winsor_perc(winsor_perc)
    C_total = total_cells(c) if C_total is None else int(C_total)
    if winsor_perc is not None:
        if min_expr_cells <= ((100 - winsor_perc[1]) * C_total * 0.01):
            min_expr_cells = int(np.ceil((100 - winsor_perc[1]) * c.G * 0.01)) + 2          # sic: genes, as the reference (analysis.py:248)
        moments = winsorized_gene_stats(c, winsor_perc)[0]
    return cv_vs_mean_from_stats(gene_stats(c), C_total, N=N, min_expr_cells=min_expr_cells, max_expr_avg=max_expr_avg,
                                 min_expr_avg=min_expr_avg, svr_gamma=svr_gamma, sort_inverse=sort_inverse, moments=moments)


def score_cluster_expression(cS: ops.CsrCounts, cU: ops.CsrCounts, cluster_ix, n_clusters: int, min_avg_U: float = 0.02,
                             min_avg_S: float = 0.08, size_limit: int = 40) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """analysis.py:441-454 + estimation.py:369-389 on CSR layers: (U_avgs, S_avgs, mask), the averages (genes, clusters).  cluster_ix:
    the cluster number (0..n_clusters-1) of each of the rank's own cells.  One masked pass per cluster of more than `size_limit`
    cells - it reads that cluster's rows only - and the overall average for the others; cluster sizes are all-reduced."""
    from .preprocess import cluster_averages, cluster_expression_mask
    dev = cS.indptr.device
    ix = torch.as_tensor(np.array(cluster_ix, dtype=np.int64), device=dev)
    if ix.numel() != cS.C or cU.C != cS.C or cU.G != cS.G:
        raise ValueError("score_cluster_expression: cS, cU and cluster_ix must describe the same cells and genes")
    if ix.numel() and (int(ix.min()) < 0 or int(ix.max()) >= n_clusters):
        raise ValueError(f"score_cluster_expression: cluster_ix outside 0..{n_clusters - 1}")
    sizes = torch.bincount(ix, minlength=n_clusters).double()
    D.all_reduce_sum(sizes)
    sizes = [int(round(v)) for v in sizes.cpu().tolist()]
    sums = lambda c, mask=None: gene_stats(c, mask)[0]
    U_avgs, S_avgs = cluster_averages(sizes, total_cells(cS), cS.G, lambda i: (sums(cU, ix == i), sums(cS, ix == i)),
                                      lambda: (sums(cU), sums(cS)), size_limit)
    return U_avgs, S_avgs, cluster_expression_mask(U_avgs, S_avgs, min_avg_U, min_avg_S)


def select_genes(keep, *layers: ops.CsrCounts) -> Tuple[ops.CsrCounts, ...]:
    """filter_genes on CSR layers: every layer cut down to the genes `keep` (bool mask or ascending gene numbers)."""
    return tuple(c.select_genes(keep) for c in layers)


GENE_FILTER_THRESHOLDS = ("min_expr_counts", "min_cells_express", "N", "min_avg_U", "min_avg_S")


def default_gene_thresholds(C_total: int, **given) -> Dict[str, float]:
    """The thresholds of default_gene_filter: the cell-count heuristics of default_filter_and_norm (analysis.py:1909-1918;
    PreprocessMixin._default_thresholds) unless passed."""
    from .preprocess import PreprocessMixin
    unknown = sorted(set(given) - set(GENE_FILTER_THRESHOLDS))
    if unknown:
        raise TypeError(f"default_gene_filter: unknown threshold(s) {unknown}; known: {list(GENE_FILTER_THRESHOLDS)}")
    t = PreprocessMixin._default_thresholds(int(C_total))
    return {**{k: t[k] for k in GENE_FILTER_THRESHOLDS}, **{k: v for k, v in given.items() if v is not None}}


def default_gene_filter(cS: ops.CsrCounts, cU: ops.CsrCounts, cluster_ix=None, n_clusters: int = 0, winsor_perc=None, **thresholds):
    """The gene filters of default_filter_and_norm (analysis.py:1889-1940) on CSR layers, in its order: detection filter -> CV-vs-mean at
    max_expr_avg = 40 -> detection filter on the unspliced layer with the halved thresholds, joined with the per-cluster expression
    filter when clusters are given.  Returns (cS', cU', kept): the selected layers and the int64 gene numbers they hold, into the
    layers as given (to subset the row attributes).  It stops before the normalisations: size_factors(cS'.row_sums(), ...) follows.
    winsor_perc: handed to the CV-vs-mean step (score_cv_vs_mean)."""
    if winsor_perc is not None:
        winsor_perc = check_winsor_perc(winsor_perc)
    C_total = total_cells(cS)
    t = default_gene_thresholds(C_total, **thresholds)
    kept = np.arange(cS.G, dtype=np.int64)

    def cut(mask):
        nonlocal cS, cU, kept
        cS, cU = select_genes(mask, cS, cU)
        kept = kept[mask]
    cut(score_detection_levels(cS, cU, min_expr_counts=t["min_expr_counts"], min_cells_express=t["min_cells_express"]))
    cut(score_cv_vs_mean(cS, C_total, N=t["N"], max_expr_avg=40, winsor_perc=winsor_perc)[1])
    half = lambda x: int(x / 2) + 1
    mask = score_detection_levels(cS, cU, min_expr_counts=0, min_cells_express=0, min_expr_counts_U=half(t["min_expr_counts"]),
                                  min_cells_express_U=half(t["min_cells_express"]))
    if cluster_ix is not None:
        mask = mask & score_cluster_expression(cS, cU, cluster_ix, n_clusters, min_avg_U=t["min_avg_U"], min_avg_S=t["min_avg_S"])[2]
    cut(mask)
    return cS, cU, kept


def size_factors(totS: torch.Tensor, totU: torch.Tensor, C: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """avg_size / cell_size of _normalize_S / _normalize_U (analysis.py:540-549, 570-579) with the mean over ALL cells."""
    sums = torch.stack([totS.sum(), totU.sum()])
    D.all_reduce_sum(sums)
    return (sums[0] / C) / totS.clamp(min=1.0), (sums[1] / C) / totU.clamp(min=1.0)


def pca_from_counts(cS: ops.CsrCounts, fS: torch.Tensor, n_components: int = 30, pcount: float = 1.0):
    """The kNN space of the path from its own input: perform_PCA on S_norm = log2(S_sz + pcount) (analysis.py:549-551, 678-700)
    straight from the rank's CSR counts and size factors (preprocess.DevicePCA.fit_transform_csr; cells sharded as in AtlasPath,
    the per-pass sums all-reduced).  Returns (pcs_own, pca): the scores of the rank's own cells as a contiguous device tensor
    (nloc, n_components) float64 - what AtlasPath(pcs=...) takes - and the fitted DevicePCA (the same on every rank)."""
    from .preprocess import DevicePCA
    pca = DevicePCA(n_components=n_components, svd_solver="subspace")
    pcs = pca.fit_transform_csr(cS, fS, pcount=pcount)
    return pcs.contiguous(), pca


def auto_block_cells(nloc: int, C: int, G: int, dev, elem_bytes: int = 4) -> int:
    """Cells per streamed block chosen from the free HBM: as many as fit beside the CSR layers - a block holds ~2.6 dense
    rows per cell (Sx + the e rows it reads outside itself, Ux) of `elem_bytes` per element; the kNN workspace of 8192 queries x C
    distances and 6 GB of headroom stay free.  On 288 GB: 1M cells x 30k genes walk in three blocks of ~366 000 cells in f32."""
    free = torch.cuda.mem_get_info(dev)[0] - 8192 * C * 4 - (6 << 30)
    return int(max(4096, min(nloc, free * 0.6 // (2.6 * ops.padded_ld(G) * elem_bytes))))


def bench_main(a, dev, rank: int, world: int) -> Optional[dict]:
    """bench.py --workload cfg5: the streamed path on synthetic CSR layers; returns the JSON record on rank 0."""
    C, G = a.cells, a.genes
    c0, c1 = D.shard_bounds(C, world, rank)
    t0 = time.perf_counter()
    cS, cU, totS, totU, pcs, emb = synth_atlas(C, G, a.pca_dims, dev, density=a.density, c0=c0, c1=c1)
    fS, fU = size_factors(totS, totU, C)
    nloc = c1 - c0
    dt_name = getattr(a, "dtype", "f32")                 # bench.py --dtype: f64 = the reference's arithmetic (the default), f32 = production mode
    tdt = torch.float64 if dt_name == "f64" else torch.float32
    block = a.block_cells if a.block_cells > 0 else auto_block_cells(nloc, C, G, dev, 8 if dt_name == "f64" else 4)
    path = AtlasPath(cS, cU, fS, fU, pcs, emb, c0=c0, C_total=C, k=a.k, n_neighbors=a.n_neighbors, sampled_fraction=a.sampled_fraction,
                     block_cells=block, dtype=tdt, knn=getattr(a, "knn", "auto"))
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    for _ in range(a.warmup):
        path.run()

    def barrier():
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        path.run(timed=True)
        if world > 1:
            path.gathered_corr()
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    if a.dump:
        corr_all = path.gathered_corr() if world > 1 else path.corr
        neigh_all = D.all_gather_rows(path.neigh, C)
        if rank == 0:
            np.savez(a.dump, gamma=path.gamma.cpu().numpy(), corr=corr_all.cpu().numpy(), neigh=neigh_all.cpu().numpy())
    if rank != 0:
        return None
    ms = dt / a.steps * 1e3
    st = path.stage_ms / a.steps
    nnz = cS.nnz / max(1, nloc)
    plan_1m = memory_plan(1_000_000, G, nnz, 8, 0, nrndm=path.nrndm, k=a.k, count_bytes=cS.data.element_size(),
                          elem_bytes=8 if dt_name == "f64" else 4, halo_e=path.n_e_halo / nloc, halo_k=path.n_count_halo / nloc)
    return {
        "metric": f"cells/sec through knn_imputation->fit_slope->colDeltaCor, {C} cells x {G} genes (cfg5: CSR layers, streamed blocks)",
        "value": C / (ms * 1e-3), "unit": "cells/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": dt_name, "data": "synthetic",
        "rccl_ranks": dist.get_world_size() if (dist.is_initialized() and dist.get_backend() == "nccl") else 0,
        "config": {"workload": f"cfg5 (BASELINE.json configs[4], scaled to what one run holds): synthetic {C} cells x {G} genes, CSR count layers at "
                               f"{100.0 * cS.nnz / max(1, nloc) / G:.1f} % density ({nnz:.0f} non-zeros per cell, {'uint8' if cS.data.dtype == torch.uint8 else 'uint16'} counts), "
                               f"streamed in blocks of {path.block_cells} cells: knn_imputation(k={a.k}) from CSR -> fit_slope -> velocity chain -> "
                               f"colDeltaCorSqrtpartial(nrndm={path.nrndm})",
                   "cells": C, "genes": G, "k": a.k, "nrndm": path.nrndm, "blocks_per_rank": len(path.blocks()), "block_cells": path.block_cells,
                   "e_sharded": True, "count_row_halo": path.n_count_halo, "e_halo_rows": path.n_e_halo,
                   "knn_search": ({"mode": "exact, projection-pruned", **path.knn_stats} if path.knn_stats else {"mode": "exact, brute force"}),
                   "stage_D_rule": ops.RULE_NAMES.get(path.rules, str(path.rules)),
                   "stage_ms": {"A_knn_search": st[2], "A_pooling_from_csr (own cells + e rows outside the block)": st[0], "B_fit_slope": st[1],
                                "D_coldeltacor": st[3]},
                   "setup_s": setup_s,
                   "resident_bytes": {"csr_layers_with_halo": path.cS.nbytes + path.cU.nbytes, "peak_block_Sx_Ux": path.peak_block_bytes,
                                      "torch_peak_allocated": int(torch.cuda.max_memory_allocated(dev))},
                   "plan_1M_cells_8_ranks_GB": plan_1m},
    }
