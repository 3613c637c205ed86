"""Cell-sharded VelocytoLoom: the analysis chain of ``analysis.VelocytoLoom`` over the GPUs of one node, one process per GPU
(``torch.distributed``; at world size 1 no collective is issued).

Every rank calls the same methods in the same order; the method names, keyword arguments and defaults are the reference's
(analysis.py:26-2342).  A rank owns a block of CELLS:

  * the cells are relabelled along the Hilbert curve of the embedding ``ts`` (``ops.hilbert_order``), so a
    rank's contiguous block of the relabelled order is spatially coherent and most neighbours of its cells are its own; the
    relabelling is internal - ``gather`` returns every attribute in the user's cell order;
  * kNN pooling and stage D read the rows of the cells their graphs reference through a halo (``distributed.HaloPlan``, built
    once per graph); a pooled row sums its neighbours in the order of the user's cell numbers (scipy's order in the facade), so
    pooled rows are bit-equal to the facade's;
  * the per-gene percentiles of ``fit_gammas`` and the per-gene shuffle of the randomised control need every cell of a gene: they
    run on GENE slices (``distributed.GeneSlices``), and the weighted fit is its two halves (moments, all-reduce, solve);
  * normalisation, the velocity chain and stage E are row-local (plus one all-gather of the cell sizes and one max-reduce of
    ``Upred``);
  * stage F: the factors of the Markov chain (O(cells x neighbours)) are assembled from the gathered transition probabilities on
    every rank; each rank owns a range of the chain's targets, and a step is one all-gather of the length-C state followed by the
    factored step of the rank's targets (``vcy_diffuse_step_factored_rows``, the full step's values bit for bit).

No rank allocates a (cells x genes) buffer: it holds its own rows, the halo rows of its graphs and, for the length of one
exchange, its gene slice.  The neighbour sampling of ``estimate_transition_prob`` replays the facade's numpy stream on every rank
(no communication) and keeps the rank's rows.
"""
from __future__ import annotations

import logging
import time
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import distributed as D
from . import ops
from .analysis import VelocytoLoom, embedding_shift, fix_correlations, markov_csr, sampling_plan, stage_d_args
from .ops import CellMatrix
from .streamed_fit import StreamedFit, check_weights

_MATRICES = ("S", "U", "S_sz", "U_sz", "S_norm", "U_norm", "Sx", "Ux", "Sx_sz", "Ux_sz", "Upred", "velocity", "delta_S", "delta_S_rndm",
             "Sx_sz_t")


class ShardedLoom:
    """One rank's share of a VelocytoLoom.  ``ShardedLoom.from_arrays(S, U, pcs, ts)`` takes the filtered (genes, cells) count layers,
    the kNN space and the embedding (every rank the full arrays; each keeps its cells); ``ShardedLoom(loom_path, pcs, ts)`` reads a
    .loom file, each rank only its cells.  (The rank's cells lie along the Hilbert curve, scattered over the file: every rank reads
    the file in blocks of 8 192 cells and keeps its columns, so each reads about the whole file once - host I/O, nothing is
    exchanged.)

    Not covered (NotImplementedError): duplicate cells in the kNN space (a distance of 0: the facade then builds the
    graph through scipy), fit_gammas on anything but the pooled size-normalised matrices or with an array of weights,
    knn_random=False, transform="logratio", hidim="pcs"."""

    def __init__(self, loom_path: Optional[str] = None, pcs=None, ts=None, *, dtype=None, group=None, layers=None) -> None:
        self._dtype = ops.resolve_dtype(dtype)
        self._group = group
        self.rank, self.world = D.world()
        self.dev = ops.require_gpu()
        self._m: Dict[str, CellMatrix] = {}
        self.timings: Dict[str, float] = {}
        self.exchange_bytes: Dict[str, int] = {}
        self.pcs = np.asarray(pcs, dtype=np.float64)
        self.ts = np.asarray(ts, dtype=np.float64)
        C = self.pcs.shape[0]
        self.C = C
        self._user = _run_order(self.ts, self.dev)
        self._inv = torch.empty_like(self._user)
        self._inv[self._user] = torch.arange(C, device=self.dev)
        self.c0, self.c1 = D.shard_bounds(C, self.world, self.rank)
        self.nloc = self.c1 - self.c0
        self._mine = self._user[self.c0:self.c1]                     # user numbers of the rank's cells, in the run's order
        mine_h = self._mine.cpu().numpy()
        if layers is None:
            from .loom_io import layer_shape, read_layer_block
            self.loom_filepath = loom_path
            G, Cf = layer_shape(loom_path, "spliced")
            if Cf != C:
                raise ValueError(f"{loom_path} holds {Cf} cells, pcs {C}")
            layers = {}
            for name in ("spliced", "unspliced"):
                # the rank's cells are scattered over the file (curve order): read blocks of cells, keep the rank's columns
                out = None                                                       # the layer's own dtype (uint16 counts stay counts)
                srt = np.argsort(mine_h, kind="stable")
                cells = mine_h[srt]
                for s in range(0, C, 8192):
                    e = min(C, s + 8192)
                    lo, hi = np.searchsorted(cells, [s, e])
                    if hi > lo:
                        blk = read_layer_block(loom_path, name, s, e)
                        if out is None:
                            out = np.zeros((G, self.nloc), dtype=blk.dtype)
                        out[:, srt[lo:hi]] = blk[:, cells[lo:hi] - s]
                if out is None:
                    out = np.zeros((G, self.nloc), dtype=np.float64)
                layers[name] = out
            S_loc, U_loc = layers["spliced"], layers["unspliced"]
        else:
            S_loc, U_loc = layers
        self.G = int(S_loc.shape[0])
        self._init_layers(S_loc, U_loc)

    @classmethod
    def from_arrays(cls, S, U, pcs, ts, *, dtype=None, group=None) -> "ShardedLoom":
        rank, world = D.world()
        C = np.shape(pcs)[0]
        user = _run_order(np.asarray(ts, dtype=np.float64), ops.require_gpu())
        c0, c1 = D.shard_bounds(C, world, rank)
        mine = user[c0:c1].cpu().numpy()
        S, U = np.asarray(S), np.asarray(U)
        return cls(None, pcs, ts, dtype=dtype, group=group, layers=(S[:, mine], U[:, mine]))

    def _init_layers(self, S_loc: np.ndarray, U_loc: np.ndarray) -> None:
        self._m["S"] = CellMatrix.from_genes_major(np.ascontiguousarray(S_loc), self._dtype)
        self._m["U"] = CellMatrix.from_genes_major(np.ascontiguousarray(U_loc), self._dtype)
        # integer layers are pooled from their counts (ops.knn_pool_counts), as the facade does; the decision is collective
        ok = torch.tensor([1.0 if (ops.CountMatrix.representable(S_loc) and ops.CountMatrix.representable(U_loc)) else 0.0], device=self.dev)
        self._reduce_min(ok)
        self._counts = None
        if float(ok) > 0.5:
            # always uint16 storage: the halo exchange moves rows of the same width on every rank
            self._counts = {n: ops.CountMatrix.from_genes_major(np.ascontiguousarray(a), narrow=False) for n, a in (("S", S_loc), ("U", U_loc))}
        self._sz_scale: Dict[str, torch.Tensor] = {}

    # ------------------------------------------------------------------ collectives
    def _reduce_min(self, t: torch.Tensor) -> torch.Tensor:
        return D.all_reduce_max(t.neg_(), self._group).neg_()

    def _gather_cells(self, v: torch.Tensor) -> torch.Tensor:
        """Per-cell rows of the rank (nloc, ...) -> all cells (C, ...) in the USER's order."""
        full = D.all_gather_rows(v.contiguous(), self.C, group=self._group)
        out = torch.empty_like(full)
        out[self._user] = full
        return out

    def _timed(self, name, t0):
        torch.cuda.synchronize()
        self.timings[name] = self.timings.get(name, 0.0) + time.perf_counter() - t0

    def dev_matrix(self, name: str) -> CellMatrix:
        """The rank's rows of a (genes x cells) attribute, in the run's cell order."""
        try:
            return self._m[name]
        except KeyError:
            raise AttributeError(f"{name} has not been computed yet") from None

    # ------------------------------------------------------------------ a1 normalisation
    def _size_factor(self, M: CellMatrix, target_size):
        cs_loc = ops.row_sums(M)
        cs = self._gather_cells(cs_loc)                               # all cell sizes in the user's order: the facade's mean, bit for bit
        avg = float(cs.mean()) if target_size is None else float(target_size)
        return cs_loc, avg / cs_loc, avg, cs

    def normalize(self, which: str = "both", size: bool = True, log: bool = True, pcount: float = 1, relative_size=None,
                  use_S_size_for_U: bool = False, target_size: Tuple[float, float] = (None, None)) -> None:
        """analysis.py:633-676 for which="both" (S and U): row-local, the target size a mean over all cells."""
        t0 = time.perf_counter()
        if which != "both" or relative_size is not None or use_S_size_for_U:
            raise NotImplementedError("ShardedLoom.normalize covers which='both' without relative_size / use_S_size_for_U")
        for name, tgt, fix in (("S", target_size[0], False), ("U", target_size[1], True)):
            M = self._m[name]
            if size:
                cs_loc, fac, avg, cs = self._size_factor(M, tgt)
                setattr(self, "cell_size" if name == "S" else "Ucell_size", cs.cpu().numpy())
                setattr(self, "avg_size" if name == "S" else "Uavg_size", avg)
            else:
                fac = None
            sz, nm = ops.scale_log(M, fac, True, log, pcount, fix_nonfinite=fix)
            self._m[name + "_sz"] = sz
            if log:
                self._m[name + "_norm"] = nm
            scale = fac if fac is not None else torch.ones(M.C, dtype=torch.float64, device=self.dev)
            finite = torch.tensor([1.0 if bool(torch.isfinite(scale).all()) else 0.0], device=self.dev)
            self._reduce_min(finite)
            if float(finite) > 0.5:
                self._sz_scale[name + "_sz"] = scale
            else:
                self._sz_scale.pop(name + "_sz", None)
        self._timed("normalize", t0)

    # ------------------------------------------------------------------ stage A
    def knn_imputation(self, k: int = None, pca_space: float = True, metric: str = "euclidean", diag: float = 1, n_pca_dims: int = None,
                       maximum: bool = False, size_norm: bool = True, balanced: bool = False, b_sight: int = None, b_maxl: int = None,
                       group_constraint=None, n_jobs: int = 8) -> None:
        """analysis.py:933-1023: each rank searches the neighbours of its own cells, fetches the halo rows its graph references and
        pools its rows with the facade's kernels.

        balanced=True (BalancedKNN, neighbors.py:186-357, with the facade's defaults b_sight = max(8 k, C - 1) and b_maxl =
        max(4 k, C - 1)): each rank searches the sight lists of its own cells, the int32 lists are all-gathered in the user's cell
        numbers (the balancing breaks ties by cell number) and EVERY rank balances the whole graph on its device
        (ops.balance_knn_positions: integer work, the same result everywhere, nothing to broadcast); the distances stay with the rank
        that searched them.  The gathered lists take C x (b_sight + 1) x 4 bytes on every rank: C x C x 4 at the whole-dataset
        default (10 GB at 50 000 cells) - pass b_sight for more cells than that holds.  group_constraint: "clusters" (self.cluster_ix)
        or one label per cell in the user's order.  Rounds and fallback of the balancing: self.knn_stats."""
        t0 = time.perf_counter()
        if not pca_space or metric != "euclidean" or diag == 0 or not size_norm or (group_constraint is not None and not balanced):
            raise NotImplementedError("ShardedLoom.knn_imputation covers the PCA space, the euclidean metric, diag != 0 and size_norm=True "
                                      "(group_constraint with balanced=True only)")
        C = self.C
        if k is None:
            k = int(C * 0.025)
        space = torch.from_numpy(np.ascontiguousarray(self.pcs[:, :n_pca_dims])).to(self.dev)
        space_run = space.index_select(0, self._user).contiguous()
        if balanced:
            cols, vals = self._balanced_rows(space_run, int(k), diag, b_sight, b_maxl, group_constraint)
        else:
            idx, dist = ops.knn_search(space_run, k, include_self=False, q0=self.c0, Q=self.nloc)
            self._refuse_duplicates(bool((dist > 0).all()))
            # the facade's rows (weight_rows_from_sorted_knn) in user numbers: the cell itself and its k neighbours, sorted by user number
            nb_user = self._user[idx.long()].to(torch.int32)
            cols = torch.cat([self._mine.to(torch.int32)[:, None], nb_user], 1)
            vals = torch.ones((self.nloc, k + 1), dtype=torch.float64, device=self.dev)
            vals[:, 0] = float(diag)
            vals = vals * (1.0 / (np.float64(k) + np.float64(diag)))
        self._knn_user = torch.sort(cols[:, 1:], dim=1).values           # (the facade's idx_s, user numbers)
        cols, vals = ops.canonical_graph_rows(cols, vals)
        rows_run = self._inv[cols.long()]                                # run order
        need = torch.zeros(C, dtype=torch.bool, device=self.dev)
        need[rows_run.reshape(-1)] = True
        need[self.c0:self.c1] = True
        plan = D.HaloPlan(need, C, self._group)
        self._pool_plan = plan
        local_cols = plan.localize(rows_run).reshape(-1)
        indptr = torch.arange(0, (self.nloc + 1) * (k + 1), k + 1, device=self.dev, dtype=torch.int64)
        w = vals.reshape(-1).to(self._dtype).contiguous()
        order = ops.hilbert_order(space_run[self.c0:self.c1, :2].contiguous()) if space_run.shape[1] >= 2 else None
        if self._counts is not None and "S_sz" in self._sz_scale and "U_sz" in self._sz_scale:
            bufs, scales = [], []
            for n in ("S", "U"):
                cm = self._counts[n]
                bufs.append(ops.CountMatrix(plan.compact(cm.t), cm.G))
                sc = self._sz_scale[n + "_sz"]
                scales.append(torch.cat([sc, plan.fetch(sc[:, None]).reshape(-1)]) if plan.n_recv else sc)
            Sx, Ux = ops.knn_pool_counts(bufs[0], bufs[1], scales[0], scales[1], indptr, local_cols, w, dtype=self._dtype, maximum=maximum,
                                         C_out=self.nloc, order=order, validate=False)
            halo_bytes = 2 * plan.n_recv * self._counts["S"].ld * 2
        else:
            mats = [CellMatrix(plan.compact(self._m[n].t), self._m[n].G) for n in ("S_sz", "U_sz")]
            Sx, Ux = ops.knn_pool2(mats[0], mats[1], indptr, local_cols, w, maximum=maximum, C_out=self.nloc, order=order, validate=False)
            halo_bytes = 2 * plan.n_recv * self._m["S_sz"].ld * self._m["S_sz"].t.element_size()
        self.exchange_bytes["halo_pool"] = halo_bytes
        for n, m in (("Sx", Sx), ("Ux", Ux), ("Sx_sz", Sx), ("Ux_sz", Ux)):
            self._m[n] = m
        self._timed("knn_imputation", t0)

    def _refuse_duplicates(self, fine: bool) -> None:
        """Collective: every rank raises if any rank found cells at distance 0."""
        pos = torch.tensor([1.0 if fine else 0.0], device=self.dev)
        self._reduce_min(pos)
        if float(pos) < 0.5:
            raise NotImplementedError("knn_imputation: cells at distance 0 (duplicates) need the scipy graph of the facade")

    def _balanced_rows(self, space_run: torch.Tensor, k: int, diag: float, b_sight, b_maxl, group_constraint):
        """The rank's rows of the balanced graph in user numbers: (cols (nloc, k + 1) int32 - the cell itself, then its picks, a slot the
        sight could not fill holding the cell again - and their weights): what (knn > 0), setdiag(diag) and connectivity_to_weights
        (analysis.py:1006-1010) make of BalancedKNN's graph - weight (distance > 0) per pick, diag for the cell, times the reciprocal
        of the row sum; a padded slot has distance 0 and weight 0."""
        C = self.C
        sight = int(np.maximum(int(k * 8), C - 1)) if b_sight is None else int(b_sight)
        maxl = int(np.maximum(int(k * 4), C - 1)) if b_maxl is None else int(b_maxl)
        K = min(sight + 1, C)                                           # the query included, as BalancedKNN.kneighbors searches
        idx, dist = ops.knn_search(space_run, K, include_self=True, q0=self.c0, Q=self.nloc)
        own_first = idx[:, 0] == torch.arange(self.c0, self.c1, device=self.dev, dtype=idx.dtype)
        self._refuse_duplicates(bool(own_first.all()) and bool((dist[:, 1:] > 0).all()))
        lists = self._gather_cells(self._user[idx.long()].to(torch.int32))     # (C, K) int32: user numbers, rows in the user's order
        groups = None
        if group_constraint is not None:
            groups = np.array(self.cluster_ix) if isinstance(group_constraint, str) and group_constraint == "clusters" else np.asarray(group_constraint)
        self.knn_stats = {}
        pos, dsi_new, _ = ops.balance_knn_positions(lists, maxl, k, groups, stats=self.knn_stats)
        del lists
        mine = self._mine
        dsi_own = dsi_new[mine]
        dist_own = ops.balance_distances(dist, pos[mine], dsi_own, mine)
        conn = (dist_own[:, 1:] > 0)
        # 1 / (picks + diag) for every possible number of picks, divided on the host as scipy divides (one IEEE division each)
        scale = torch.from_numpy(1.0 / (np.arange(k + 1, dtype=np.float64) + np.float64(diag))).to(self.dev)
        vals = torch.cat([torch.full((self.nloc, 1), float(diag), dtype=torch.float64, device=self.dev), conn.double()], 1)
        vals = vals * scale[conn.sum(1)][:, None]
        return dsi_own.to(torch.int32), vals

    # ------------------------------------------------------------------ stage B
    def _slices(self) -> D.GeneSlices:
        if getattr(self, "_gs", None) is None:
            self._gs = D.GeneSlices(self.C, self.G, self._user, self._group)
        return self._gs

    def fit_gammas(self, steady_state_bool=None, use_imputed_data: bool = True, use_size_norm: bool = True, fit_offset: bool = True,
                   fixperc_q: bool = False, weighted: bool = True, weights="maxmin_diag", limit_gamma: bool = False, maxmin_perc=[2, 98],
                   maxmin_weighted_pow: float = 15, _route: Optional[str] = None) -> None:
        """analysis.py:1120-1260.  The bare default call: the percentiles on gene slices (exact: the facade's kernel on every cell of a
        gene), the weighted fit as per-rank moments, an all-reduce and the box-constrained solve.  Every other combination of
        steady_state_bool (a bool mask over all C cells in the user's order), fit_offset, fixperc_q, weighted, weights (a string),
        limit_gamma, maxmin_perc and maxmin_weighted_pow: the streamed select (streamed_fit.StreamedFit) with the rank's shard as its
        one block - integer histograms and the moments all-reduced, no gene-slice exchange; the bytes handed to the all-reduces go to
        exchange_bytes["fit_select"].  _route="select" sends the default fit down that path too.  Not covered (NotImplementedError):
        use_imputed_data=False, use_size_norm=False, an array of weights, steady_state_bool as an array of cell indices."""
        t0 = time.perf_counter()
        if not use_imputed_data or not use_size_norm:
            raise NotImplementedError("ShardedLoom.fit_gammas covers the pooled size-normalised matrices (use_imputed_data=True, use_size_norm=True)")
        if isinstance(weights, (np.ndarray, torch.Tensor)) and weighted:
            raise NotImplementedError("ShardedLoom.fit_gammas: an array of weights is not covered (a weight mode by name is)")
        if weighted:
            check_weights(weights)
        if _route not in (None, "select"):
            raise ValueError(f"_route={_route!r} (None or \"select\")")
        ss = None
        if steady_state_bool is not None and np.ndim(steady_state_bool) != 0:
            ss = np.asarray(steady_state_bool)
            if ss.dtype != np.bool_:
                raise NotImplementedError("ShardedLoom.fit_gammas: steady_state_bool as an array of cell indices is not covered (a bool mask is)")
            if ss.shape != (self.C,):
                raise ValueError(f"steady_state_bool must be a boolean mask over the {self.C} cells")
            if not ss.any():
                raise ValueError("steady_state_bool selects no cell")
            if ss.all():
                ss = None
        self.steady_state = np.ones(self.C, dtype=bool) if ss is None else ss       # analysis.py:1159-1162, whichever route follows
        perc = [float(p) for p in maxmin_perc]
        default = (ss is None and fit_offset and not fixperc_q and weighted and weights == "maxmin_diag" and not limit_gamma
                   and perc == [2.0, 98.0] and float(maxmin_weighted_pow) == 15.0)
        if _route == "select" or not default:
            self._fit_gammas_select(ss, fit_offset, fixperc_q, weighted, weights, limit_gamma, perc, maxmin_weighted_pow)
            self._timed("fit_gammas", t0)
            return
        gs = self._slices()
        Sx, Ux = self._m["Sx"], self._m["Ux"]
        b0 = gs.bytes_moved
        sl_S = gs.to_slices(Sx)
        sl_U = gs.to_slices(Ux)
        if gs.gs:
            dS, dU = VelocytoLoom._maxnorm_denominator(sl_S), VelocytoLoom._maxnorm_denominator(sl_U)
            q = ops.gene_quantiles(sl_S, perc, M2=sl_U, scale_a=dS, scale_b=dU)
            per_gene = torch.stack([dS, dU, q[0], q[1]], 1)
        else:
            per_gene = torch.empty((0, 4), dtype=torch.float64, device=self.dev)
        del sl_S, sl_U
        self.exchange_bytes["gene_slices_fit"] = gs.bytes_moved - b0
        th = gs.gather_genes(per_gene)
        dS, dU, down, up = (th[:, i].contiguous() for i in range(4))
        self._fit_thresholds = {"denom_S": dS, "denom_U": dU, "down": down, "up": up}
        mom = ops.fit_weighted_moments(Ux, Sx, 1, M=Sx, M2=Ux, scale_a=dS, scale_b=dU, down=down, up=up)
        D.all_reduce_sum(mom, self._group)
        g, q, R2 = ops.fit_weighted_from_moments(mom, self.C, fit_offset=True, box_q=True, lo_gamma=1e-8, up_gamma_default=20.0)
        g = torch.where(torch.isfinite(g), g, torch.zeros_like(g))                     # :1260
        self._gammas_dev, self._q_dev = g, q
        self.gammas, self.q, self.R2 = g.cpu().numpy(), q.cpu().numpy(), R2.cpu().numpy()
        self._timed("fit_gammas", t0)

    def _fit_gammas_select(self, ss, fit_offset, fixperc_q, weighted, weights, limit_gamma, perc, power) -> None:
        """fit_gammas through StreamedFit: the shard is the one block of every walk."""
        cmask, n_fit = None, self.C
        if ss is not None:
            cmask = torch.from_numpy(ss).to(self.dev)[self._mine].to(torch.uint8).contiguous()      # the rank's cells, in the run's order
            n_fit = int(ss.sum())
        fit = StreamedFit(self.G, self.C, self._dtype, self.dev, weighted=weighted, weights=weights, fit_offset=fit_offset, fixperc_q=fixperc_q,
                          limit_gamma=limit_gamma, maxmin_perc=perc, maxmin_weighted_pow=power, n_fit_cells=n_fit, group=self._group)
        Sx, Ux = self._m["Sx_sz"], self._m["Ux_sz"]
        for _ in range(fit.n_walks):
            fit.add_block(Sx, Ux, cell_mask=cmask)
            fit.end_walk()
        g, q, R2 = fit.result()
        self._fit_thresholds = fit.thresholds
        self.exchange_bytes["fit_select"] = fit.reduced_bytes if D.active() else 0
        self._gammas_dev, self._q_dev = g, q
        self.gammas, self.q, self.R2 = g.cpu().numpy(), q.cpu().numpy(), R2.cpu().numpy()

    # ------------------------------------------------------------------ stage C
    def _gene_max(self, M: CellMatrix) -> torch.Tensor:
        return D.all_reduce_max(ops.gene_quantiles(M, [100])[0].contiguous(), self._group)

    def predict_U(self, which_gamma: str = "gammas", which_S: str = "Sx_sz", which_offset: str = "q") -> None:
        """analysis.py:1321-1346 (row-local)."""
        t0 = time.perf_counter()
        if which_S != "Sx_sz":
            raise NotImplementedError("ShardedLoom.predict_U covers which_S='Sx_sz'")
        self.which_S_for_pred = which_S
        gam = torch.as_tensor(np.asarray(getattr(self, which_gamma), dtype=np.float32))
        q = None if which_offset is None else torch.as_tensor(np.asarray(getattr(self, which_offset), dtype=np.float32))
        self._m["Upred"] = ops.velocity_chain(self._m["Sx_sz"], self._m["Ux_sz"], gam, q, want=("Upred",))["Upred"]
        self._timed("predict_U", t0)

    def calculate_velocity(self, kind: str = "residual", eps: float = None) -> None:
        """analysis.py:1348-1379: Ux_sz - Upred; the eps threshold is Upred's maximum over ALL cells (one max-reduce)."""
        t0 = time.perf_counter()
        if kind != "residual":
            raise NotImplementedError(f"Velocity calculation kind={kind} is not implemented")
        up = self._m["Upred"]
        thr = self._gene_max(up) * float(eps) if eps else None
        self._m["velocity"] = ops.lincomb(self._m["Ux_sz"], up, 1.0, -1.0, zero_below=thr)
        self._timed("calculate_velocity", t0)

    def calculate_shift(self, assumption: str = "constant_velocity", delta_t: float = 1) -> None:
        """analysis.py:1381-1408 for the default assumption (row-local)."""
        t0 = time.perf_counter()
        if assumption != "constant_velocity":
            raise NotImplementedError("ShardedLoom.calculate_shift covers assumption='constant_velocity'")
        self._m["delta_S"] = ops.lincomb(self._m["velocity"], None, float(delta_t))
        self._timed("calculate_shift", t0)

    def extrapolate_cell_at_t(self, delta_t: float = 1, clip: bool = True) -> None:
        """analysis.py:1410-1439 (row-local)."""
        t0 = time.perf_counter()
        if clip:
            self.used_delta_t = delta_t
        self._m["Sx_sz_t"] = ops.lincomb(self._m["Sx_sz"], self._m["delta_S"], 1.0, float(delta_t), clip=clip)
        self._timed("extrapolate_cell_at_t", t0)

    # ------------------------------------------------------------------ stage D
    def estimate_transition_prob(self, hidim: str = "Sx_sz", embed: str = "ts", transform: str = "sqrt", ndims: int = None,
                                 n_sight: int = None, psc: float = None, knn_random: bool = True, sampled_fraction: float = 0.3,
                                 sampling_probs: Tuple[float, float] = (0.5, 0.1), max_dist_embed: float = None, n_jobs: int = 4,
                                 threads: int = None, calculate_randomized: bool = True, random_seed: int = 15071990, **kwargs) -> None:
        """analysis.py:1452-1668 with knn_random=True: the embedding kNN of the rank's cells, the facade's sampling stream replayed
        on every rank, stage D through the halo of e = hidim, the randomised control through the gene slices."""
        t0 = time.perf_counter()
        n_neighbors = kwargs.pop("n_neighbors", None)
        if kwargs:
            logging.warning(f"keyword arguments were passed but could not be interpreted {kwargs}")
        if not knn_random or transform == "logratio" or "pcs" in hidim or hidim != "Sx_sz":
            raise NotImplementedError("ShardedLoom.estimate_transition_prob covers hidim='Sx_sz', knn_random=True and the "
                                      "linear / sqrt / log transforms")
        C = self.C
        n_neighbors, psc, mode, kern = stage_d_args(C, transform, hidim, ndims, n_sight, n_neighbors, psc)
        np.random.seed(random_seed)                                                  # :1529
        self.which_hidim = hidim
        hi, dS = self._m[hidim], self._m["delta_S"]
        embedding = np.asarray(getattr(self, embed), dtype=np.float64)
        self.embedding = embedding
        if kern == ops.SQRT and hi.dtype == torch.float64:
            # judged on the whole matrix, by every rank alike
            D.check_f64_sqrt_domain(hi.t.abs().max() if hi.C else torch.zeros(1, dtype=torch.float64, device=self.dev), self._group)
        stats = D.all_reduce_abs_stats(ops.abs_stats(hi), self._group)
        rules = ops.partial_rules_for(hi, kern, psc, stats=stats, cells=C, literal=bool(getattr(self, "literal_rule", False)),
                                      domain_checked=True)
        gs = self._slices()
        self._m.pop("delta_S_rndm", None)
        if calculate_randomized:
            # the control's value at (c, g) is +- delta_S[pi_g(c), g] over ALL cells: shuffled on the gene slices
            b0 = gs.bytes_moved
            sl = gs.to_slices(dS)
            if gs.gs:
                sl = ops.permute_rows_nsign(sl, random_seed, gene0=gs.g0)
            self._m["delta_S_rndm"] = gs.from_slices(sl)
            del sl
            self.exchange_bytes["gene_slices_control"] = gs.bytes_moved - b0
        dmat, _ = ops.delta_transform(hi, dS, self.used_delta_t, mode, psc)
        dmat_r = ops.delta_transform(hi, self._m["delta_S_rndm"], self.used_delta_t, mode, psc)[0] if calculate_randomized else None
        # embedding kNN of the rank's cells (n_neighbors + 1 nearest, query excluded, :1547-1549) in the run's order -> user numbers
        emb_run = torch.from_numpy(np.ascontiguousarray(embedding)).to(self.dev).index_select(0, self._user).contiguous()
        self._emb_run = emb_run
        knn_ix, _ = ops.knn_search(emb_run, n_neighbors + 1, include_self=False, q0=self.c0, Q=self.nloc)
        knn_user = self._user[knn_ix.long()]
        n_cand = int(knn_ix.shape[1])
        p, size = sampling_plan(sampling_probs, n_cand, sampled_fraction, n_neighbors)
        # the facade's numpy stream, replayed whole on every rank (same RNG state afterwards everywhere); the rank keeps its rows
        t_rep = time.perf_counter()
        sampling_ixs = ops.choice_stream_host(n_cand, size, p, C)
        self.timings["sampling_replay"] = time.perf_counter() - t_rep
        self._sampling_loc = sampling_ixs[self._mine.cpu().numpy()]
        picks = torch.from_numpy(self._sampling_loc).to(self.dev)
        neigh_user = torch.gather(knn_user, 1, picks).contiguous()
        self._neigh_user = neigh_user.to(torch.int32)
        neigh_run = self._inv[neigh_user]
        self._neigh_run = neigh_run.to(torch.int32).contiguous()
        # stage D through the halo of e: own rows first, then the remote rows the lists reference
        need = torch.zeros(C, dtype=torch.bool, device=self.dev)
        need[neigh_run.reshape(-1)] = True
        need[self.c0:self.c1] = True
        plan = D.HaloPlan(need, C, self._group)
        self._d_plan = plan
        e = CellMatrix(plan.compact(hi.t), hi.G)
        self.exchange_bytes["halo_stage_d"] = plan.n_recv * hi.ld * hi.t.element_size()
        self._e = e
        nk = plan.localize(neigh_run)
        self._neigh_k = nk
        order = ops.hilbert_order(emb_run[self.c0:self.c1, :2].contiguous()) if embedding.shape[1] >= 2 else None
        corr = torch.empty((self.nloc, size), dtype=hi.dtype, device=self.dev)
        corr_r = torch.empty((self.nloc, size), dtype=hi.dtype, device=self.dev) if calculate_randomized else None
        if size and self.nloc:
            if calculate_randomized:
                ops.coldeltacor_partial_dual(e, dmat, dmat_r, nk, kern, rules, psc, cell0=0, order=order, out=corr, out_rndm=corr_r,
                                             validate=False)
            else:
                ops.coldeltacor_partial(e, dmat, nk, kern, rules, psc, cell0=0, order=order, out=corr, validate=False)
        self.corr_calc = "knn_random"
        fix_correlations(corr, corr_r, nk)                                                         # :1604-1607
        self._corr, self._corr_random = corr, corr_r
        self._timed("estimate_transition_prob", t0)

    # ------------------------------------------------------------------ stage E
    def calculate_embedding_shift(self, sigma_corr: float = 0.05, expression_scaling: bool = True, scaling_penalty: float = 1.) -> None:
        """analysis.py:1670-1733 in neighbour-list form, rank-local: the transition probabilities of the rank's rows, the expression
        scaling from the rows of hi the stage-D halo already holds."""
        t0 = time.perf_counter()
        e = self._e

        def padded(m):                                               # own rows at the top of an e-sized buffer (the kernel's shape)
            if m.C == e.C:
                return m
            out = CellMatrix(torch.zeros_like(e.t), e.G)
            out.t[:m.C] = m.t
            return out
        dS = padded(self._m["delta_S"]) if expression_scaling else None
        dS_r = padded(self._m["delta_S_rndm"]) if expression_scaling and self._corr_random is not None else None
        res = embedding_shift(e, dS, dS_r, self._neigh_k, self._neigh_run, self._corr, self._corr_random, self._emb_run, sigma_corr,
                              expression_scaling, scaling_penalty, cell0=self.c0)
        self._tp, self._delta_embedding, self._scaling = res[0]
        self._tp_random = self._delta_embedding_random = self._scaling_rndm = None
        if len(res) == 2:
            self._tp_random, self._delta_embedding_random, self._scaling_rndm = res[1]
        self.delta_embedding = self._gather_cells(self._delta_embedding).cpu().numpy()
        if self._scaling is not None:
            self.scaling = self._gather_cells(self._scaling).cpu().numpy()
        self._timed("calculate_embedding_shift", t0)

    # ------------------------------------------------------------------ stage F
    def prepare_markov(self, sigma_D: np.ndarray, sigma_W: np.ndarray, direction: str = "forward", cells_ixs: np.ndarray = None) -> None:
        """analysis.py:1818-1863: the facade's factored chain (its CSR: analysis.markov_csr), assembled on every rank from the gathered
        transition probabilities (cells x neighbours: no (cells, cells) matrix, no (cells, genes) one)."""
        t0 = time.perf_counter()
        if direction not in ("forward", "backwards"):
            raise NotImplementedError(f"{direction} is not an implemented direction")
        if cells_ixs is not None:
            raise NotImplementedError("ShardedLoom.prepare_markov covers all cells (cells_ixs=None)")
        tp = self._gather_cells(self._tp)
        ixs = self._gather_cells(self._neigh_user.to(torch.int64))
        indptr, indices, data = markov_csr(tp, ixs, direction)
        self._tr_dev = ops.prepare_markov_factored(indptr, indices, data, np.asarray(self.embedding, dtype=np.float64), sigma_D, sigma_W,
                                                   compute_dtype=self._dtype)
        self._timed("prepare_markov", t0)

    def run_markov(self, starting_p: np.ndarray = None, n_steps: int = 2500, mode: str = "time_evolution") -> None:
        """analysis.py:1865-1887 (Diffusion.diffuse, modes time_evolution and path_integral): the rank steps the targets of its range
        of positions, the state is all-gathered after every step.  The same numbers as the facade's chain, bit for bit."""
        t0 = time.perf_counter()
        if mode not in ("time_evolution", "path_integral"):
            raise NotImplementedError(f"ShardedLoom.run_markov covers mode='time_evolution' and 'path_integral', not {mode!r}")
        tr = self._tr_dev
        n = tr.n
        if starting_p is None:
            starting_p = np.ones(n) / n
        x0 = np.asarray(starting_p, dtype=np.float64)
        x = torch.from_numpy(x0 / x0.sum()).to(self.dev).contiguous()                  # diffusion.py:95 (Diffusion.diffuse)
        p0, p1 = D.shard_bounds(n, self.world, self.rank)
        cells = tr.target_order()                                                      # cell at each target position
        mine = cells[p0:p1]
        y = torch.zeros(n, dtype=torch.float64, device=self.dev)
        acc = torch.zeros(n, dtype=torch.float64, device=self.dev) if mode == "path_integral" else None
        ws = torch.empty(int(ops._lib.lib().vcy_markov_factored_workspace_bytes(n)), dtype=torch.uint8, device=self.dev)
        gathered = torch.empty(n, dtype=torch.float64, device=self.dev)
        t_ex, bytes_ex = 0.0, 0
        for _ in range(int(n_steps)):
            ops.diffuse_step_rows(tr, x, y, p0, p1, accum=acc, workspace=ws)
            te = time.perf_counter()
            full = D.all_gather_rows(y[mine].contiguous(), n, group=self._group)      # the state by position
            nxt = torch.empty_like(x)
            nxt[cells] = full
            x = nxt
            if D.active():
                torch.cuda.synchronize()
                t_ex += time.perf_counter() - te
                bytes_ex += (n - (p1 - p0)) * 8
        if acc is not None:
            gathered[cells] = D.all_gather_rows(acc[mine].contiguous(), n, group=self._group)
            out = gathered
        else:
            out = x
        self.exchange_bytes["markov_state_per_step"] = (n - (p1 - p0)) * 8 if D.active() else 0
        self.timings["markov_state_gather"] = t_ex
        self.diffused = out.cpu().numpy()
        self._timed("run_markov", t0)

    # ------------------------------------------------------------------ results
    def gather(self, name: str):
        """Any attribute of the chain as a host array in the user's cell order (every rank must call it): the (genes, cells)
        matrices as the facade's attributes hold them, the per-cell results (cells, ...), the neighbour-list results
        ``corrcoef`` / ``corrcoef_random`` / ``transition_prob`` / ``transition_prob_random`` as (values, user cell numbers) pairs
        of (cells, neighbours) arrays, ``embedding_knn_indices`` the sampled lists, ``knn_indices`` the pooling graph's (sorted)."""
        if name in _MATRICES:
            return self._gather_matrix(self.dev_matrix(name))
        if name in ("gammas", "q", "R2", "embedding", "diffused", "delta_embedding", "scaling", "cell_size", "Ucell_size"):
            return getattr(self, name)
        lists = {"corrcoef": "_corr", "corrcoef_random": "_corr_random", "transition_prob": "_tp", "transition_prob_random": "_tp_random"}
        if name in lists:
            v = getattr(self, lists[name])
            if v is None:
                raise AttributeError(name)
            return self._gather_cells(v).double().cpu().numpy(), self._gather_cells(self._neigh_user).cpu().numpy()
        per_cell = {"embedding_knn_indices": "_neigh_user", "knn_indices": "_knn_user", "delta_embedding_random": "_delta_embedding_random",
                    "scaling_rndm": "_scaling_rndm"}
        if name in per_cell:
            v = getattr(self, per_cell[name], None)
            if v is None:
                raise AttributeError(name)
            return self._gather_cells(v).cpu().numpy()
        if name == "sampling_ixs":
            return self._gather_cells(torch.from_numpy(self._sampling_loc).to(self.dev)).cpu().numpy()
        if name == "fit_thresholds":
            return {k: v.cpu().numpy() for k, v in self._fit_thresholds.items()}
        raise AttributeError(name)

    def _gather_matrix(self, M: CellMatrix, block_bytes: int = 256 << 20) -> np.ndarray:
        """(genes, cells) host array of a cells-sharded matrix, moved in blocks of genes (no device buffer of the whole matrix)."""
        out = np.empty((self.G, self.C), dtype=np.float64)
        user = self._user.cpu().numpy()
        gb = max(1, min(self.G, block_bytes // max(1, self.C * M.t.element_size())))
        for g0 in range(0, self.G, gb):
            g1 = min(self.G, g0 + gb)
            full = D.all_gather_rows(M.t[:, g0:g1].contiguous(), self.C, group=self._group)
            out[g0:g1, user] = full.double().cpu().numpy().T
        return out


def _run_order(ts: np.ndarray, dev) -> torch.Tensor:
    """The run's cell order: the user's cell numbers along the Hilbert curve of the embedding (every rank computes the same
    permutation from the same input)."""
    C = ts.shape[0]
    if ts.ndim < 2 or ts.shape[1] < 2:
        return torch.arange(C, device=dev)
    return ops.hilbert_order(torch.from_numpy(np.ascontiguousarray(ts[:, :2])).to(dev)).long().contiguous()

