"""VelocytoLoom.fit_gammas (analysis.py:1120-1260) for pooled matrices that are only ever seen as a sequence of cell blocks.

``StreamedFit`` holds the plan of walks over the blocks and knows nothing about where the blocks come from: AtlasPath hands it the
blocks it pools into its two staging buffers, ShardedLoom its resident shard as one block.  Per walk every block is added once
(any order, any blocking, the cells of all ranks); between walks the integer histograms of the streamed selects
(ops.StreamedGeneQuantiles, ops.StreamedMaskedGeneQuantiles) and, after the last, the fp64 moments are summed over the ranks.
Nothing of (block x genes) size is formed beyond the two buffers a block arrives in: the non-binary weights are evaluated inside
the moments fold (ops.fit_weighted_moments_fused).

Plan, with P = vcy_gene_select_passes(dtype) walks per select phase (4 in f32, 8 in f64):

  mode                             phase 1 (P walks)                      phase 2 (P walks)                moments          walks
  weighted=False, no fixperc_q     -                                      -                                weight_mode 2    1
  "sum", "prod"                    [99] of Sx, [99] of Ux                 only limit_gamma / fixperc_q     fused 0 / 1      P+1 (2P+1)
  "maxmin", "maxmin_weighted"      maxmin_perc of Sx                      only limit_gamma / fixperc_q     weight_mode 1    P+1 (2P+1)
                                                                                                           / fused 2
  "maxmin_diag"                    [99.9, 100] of Sx and of Ux            maxmin_perc of Z                 weight_mode 1    2P+1
  "maxmin_double"                  the same + maxmin_perc of Sx           maxmin_perc of Z                 fused 3          2P+1
  weighted=False, fixperc_q        [1] of Sx (masked)                     the conditional [50]             weight_mode 2    2P+1

Z = Sx/denom_S + Ux/denom_U.  The unconditional percentiles behind limit_gamma ([50, 90] of Sx, [50] of Ux) and fixperc_q ([1] of
Sx) ride in phase 1, the conditional ones (Ux and Sx where Sx > p90; Ux where Sx <= p1), which need only those, in phase 2.  As in
the facade the weights' thresholds are taken over all cells; the limit_gamma / fixperc_q percentiles and the moments over the
steady-state cells (`cell_mask` of add_block).
"""
from __future__ import annotations

import logging
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import distributed as D
from . import ops

WEIGHTS = ("sum", "prod", "maxmin", "maxmin_weighted", "maxmin_diag", "maxmin_double")


def check_weights(weights) -> None:
    """The facade's refusal of an unknown weight mode; an array of weights has no streamed form."""
    if isinstance(weights, (np.ndarray, torch.Tensor)):
        raise ValueError("weights as an array is not supported by the streamed fit: it never sees a whole (cells x genes) matrix")
    if not isinstance(weights, str) or weights not in WEIGHTS:
        raise ValueError(f"weights={weights!r} is not supported")


class StreamedFit:
    """fit = StreamedFit(G, n_total, dtype, device, ...); for every walk of fit.n_walks: fit.add_block(Sx_b, Ux_b, cell_mask) on every
    block, then fit.end_walk(); gamma, q, R2 = fit.result().

    n_total: the cells of all ranks; n_fit_cells: the steady-state cells of all ranks (None = n_total) - the n of the solve.
    cell_mask of add_block: the steady-state cells of the block (uint8 / bool, one per cell) or None = every cell.
    group: the process group the histograms and the moments are summed over.

    thresholds: per-gene float64 (int64 for populations), as the walks produce them -
        "sum", "prod":                 p99_S, p99_U
        "maxmin", "maxmin_weighted":   down_S, up_S                       (maxmin_perc of Sx)
        "maxmin_diag":                 denom_S, denom_U, down, up         (down, up: maxmin_perc of Z)
        "maxmin_double":               denom_S, denom_U, down, up, down_S, up_S
        limit_gamma (weighted):        med_S, p90_S, med_U, U_p10_above, S_med_above, n_above, up_gamma
        fixperc_q without fit_offset:  p1_S, n_below, q_fixed
    moments: the summed (10, G) moments of the solve; state_bytes: the bytes the selects held at their peak; reduced_bytes: the bytes
    this rank handed to all-reduces."""

    def __init__(self, G: int, n_total: int, dtype=None, device=None, weighted: bool = True, weights="maxmin_diag", fit_offset: bool = True,
                 fixperc_q: bool = False, limit_gamma: bool = False, maxmin_perc=(2, 98), maxmin_weighted_pow: float = 15,
                 n_fit_cells: Optional[int] = None, group=None):
        self.weighted = bool(weighted)
        if self.weighted:
            check_weights(weights)
        self.weights = weights if self.weighted else None
        self.G, self.n_total = int(G), int(n_total)
        if self.G <= 0 or self.n_total <= 0:
            raise ValueError(f"StreamedFit: G = {G}, n_total = {n_total}")
        self.n_fit_cells = self.n_total if n_fit_cells is None else int(n_fit_cells)
        if not 0 < self.n_fit_cells <= self.n_total:
            raise ValueError(f"StreamedFit: n_fit_cells = {n_fit_cells} of n_total = {n_total} cells")
        self.dtype = ops.resolve_dtype(dtype)
        self.dev = device
        self.group = group
        self.fit_offset, self.fixperc_q, self.limit_gamma = bool(fit_offset), bool(fixperc_q), bool(limit_gamma)
        self.perc = [float(p) for p in maxmin_perc]
        if len(self.perc) != 2:
            raise ValueError(f"maxmin_perc={maxmin_perc!r}: two percentiles")
        self.power = float(maxmin_weighted_pow)
        # what VelocytoLoom.fit_gammas' branches use: up_gamma with limit_gamma unless the fixed offset takes over; unweighted fits know no limit
        self.need_up = self.weighted and self.limit_gamma and (self.fit_offset or not self.fixperc_q)
        self.need_qf = self.fixperc_q and not self.fit_offset
        self.passes = int(_lib.lib().vcy_gene_select_passes(ops._DT[self.dtype]))
        w = self.weights
        self._has1 = self.weighted or self.need_qf
        self._has2 = w in ("maxmin_diag", "maxmin_double") or self.need_up or self.need_qf
        self.n_walks = (self.passes if self._has1 else 0) + (self.passes if self._has2 else 0) + 1
        self._ends = [self.passes if self._has1 else 0, self.n_walks - 1, self.n_walks]     # the walk after which phase 1, 2, 3 end
        self.walk = 0
        self.thresholds: Dict[str, torch.Tensor] = {}
        self.moments = None
        self.state_bytes = 0
        self.reduced_bytes = 0
        self._sel: List[tuple] = []          # the running phase's selects: (select, kind, arguments)
        self._named: Dict[str, object] = {}
        self._mom = None
        self._began = False
        self._result = None

    # ------------------------------------------------------------------ the selects of a phase
    def _device(self):
        if self.dev is None:
            self.dev = ops.require_gpu()
        return self.dev

    def _plain(self, name: str, qs, of_u: bool = False, two: bool = False) -> None:
        sel = ops.StreamedGeneQuantiles(self.G, qs, self.n_total, self.dtype, self._device(), two=two)
        self._sel.append((sel, "z" if two else "plain", of_u))
        self._named[name] = sel

    def _masked(self, name: str, qs, of_u: bool = False, thr=None, mode: int = 0) -> None:
        sel = ops.StreamedMaskedGeneQuantiles(self.G, qs, self.dtype, self._device())
        self._sel.append((sel, "masked", (of_u, thr, mode)))
        self._named[name] = sel

    def _phase(self) -> int:
        return 1 if self.walk < self._ends[0] else (2 if self.walk < self._ends[1] else 3)

    def _begin(self) -> None:
        """The selects of the phase the next walk belongs to (phase 3, the moments, has none)."""
        self._sel, self._named = [], {}
        w, ph = self.weights, self._phase()
        if ph == 1:
            if w in ("sum", "prod"):
                self._plain("S", [99]); self._plain("U", [99], of_u=True)
            elif w in ("maxmin", "maxmin_weighted"):
                self._plain("S2", self.perc)
            elif w in ("maxmin_diag", "maxmin_double"):
                self._plain("S", [99.9, 100]); self._plain("U", [99.9, 100], of_u=True)
                if w == "maxmin_double":
                    self._plain("S2", self.perc)
            if self.need_up:
                self._masked("xS", [50, 90]); self._masked("xU", [50], of_u=True)
            elif self.need_qf:
                self._masked("xS", [1])
        elif ph == 2:
            th = self.thresholds
            if w in ("maxmin_diag", "maxmin_double"):
                self._plain("Z", self.perc, two=True)
            if self.need_up:                         # y[x > p90] at 10, x[x > p90] at 50
                self._masked("y10", [10], of_u=True, thr=th["p90_S"], mode=1); self._masked("xm", [50], thr=th["p90_S"], mode=1)
            elif self.need_qf:                       # y[x <= p1] at 50
                self._masked("qf", [50], of_u=True, thr=th["p1_S"], mode=2)
        self.state_bytes = max(self.state_bytes, sum(s[0].state_bytes for s in self._sel))
        self._began = True

    def _finish(self, ph: int) -> None:
        """A phase's results -> thresholds."""
        th, nm = self.thresholds, self._named
        row = lambda t, i: t[i].contiguous()
        if ph == 1:
            denom = lambda p: torch.where(p[0] == 0, torch.clamp(p[1], min=0.001), p[0]).contiguous()     # _maxnorm_denominator's rule
            if self.weights in ("sum", "prod"):
                th["p99_S"], th["p99_U"] = row(nm["S"].result(), 0), row(nm["U"].result(), 0)
            elif self.weights in ("maxmin_diag", "maxmin_double"):
                th["denom_S"], th["denom_U"] = denom(nm["S"].result()), denom(nm["U"].result())
            if "S2" in nm:
                q = nm["S2"].result()
                th["down_S"], th["up_S"] = row(q, 0), row(q, 1)
            if self.need_up:
                qx = nm["xS"].result()
                th["med_S"], th["p90_S"], th["med_U"] = row(qx, 0), row(qx, 1), row(nm["xU"].result(), 0)
            elif self.need_qf:
                th["p1_S"] = row(nm["xS"].result(), 0)
        elif ph == 2:
            if "Z" in nm:
                q = nm["Z"].result()
                th["down"], th["up"] = row(q, 0), row(q, 1)
            if self.need_up:                       # estimation._median_and_up_gamma from the streamed percentiles
                y10, xm = nm["y10"].result()[0], nm["xm"].result()[0]
                upg = torch.maximum(torch.full_like(y10, 1.5), y10 / xm)
                th.update(U_p10_above=y10, S_med_above=xm, n_above=nm["y10"].counts(),
                          up_gamma=torch.where(th["med_U"] > th["med_S"], upg, torch.full_like(upg, 1.5)))
            elif self.need_qf:                     # estimation._fixperc_q
                th.update(n_below=nm["qf"].counts(), q_fixed=nm["qf"].result()[0])
        self._sel, self._named = [], {}

    # ------------------------------------------------------------------ the walks
    def add_block(self, Sx_b: ops.CellMatrix, Ux_b: ops.CellMatrix, cell_mask=None) -> None:
        if self.walk >= self.n_walks:
            raise RuntimeError("StreamedFit.add_block: every walk is done")
        if Sx_b.G != self.G or Ux_b.G != self.G or Sx_b.C != Ux_b.C or Sx_b.dtype != self.dtype or Ux_b.dtype != self.dtype:
            raise ValueError(f"StreamedFit.add_block: a block of {Sx_b.C} x {Sx_b.G} / {Ux_b.C} x {Ux_b.G} ({Sx_b.dtype}) for a fit over {self.G} genes ({self.dtype})")
        if not self._began:
            self._begin()
        if Sx_b.C == 0:
            return
        th = self.thresholds
        if self._phase() < 3:
            for sel, kind, arg in self._sel:
                if kind == "plain":
                    sel.add_block(Ux_b if arg else Sx_b)
                elif kind == "z":
                    sel.add_block(Sx_b, M2=Ux_b, scale_a=th["denom_S"], scale_b=th["denom_U"])
                else:
                    of_u, thr, mode = arg
                    if mode:
                        sel.add_block(Ux_b if of_u else Sx_b, mask_src=Sx_b, mask_thr=thr, mask_mode=mode, cell_mask=cell_mask)
                    else:
                        sel.add_block(Ux_b if of_u else Sx_b, cell_mask=cell_mask)
            return
        w = self.weights
        if w is None:
            m = ops.fit_weighted_moments(Ux_b, Sx_b, 2, cell_mask=cell_mask)
        elif w in ("sum", "prod"):
            m = ops.fit_weighted_moments_fused(Ux_b, Sx_b, 0 if w == "sum" else 1, Sx_b, Ux_b, th["p99_S"], th["p99_U"], cell_mask=cell_mask)
        elif w == "maxmin":
            m = ops.fit_weighted_moments(Ux_b, Sx_b, 1, M=Sx_b, down=th["down_S"], up=th["up_S"], cell_mask=cell_mask)
        elif w == "maxmin_weighted":
            m = ops.fit_weighted_moments_fused(Ux_b, Sx_b, 2, Sx_b, None, th["down_S"], th["up_S"], power=self.power, cell_mask=cell_mask)
        elif w == "maxmin_diag":
            m = ops.fit_weighted_moments(Ux_b, Sx_b, 1, M=Sx_b, M2=Ux_b, scale_a=th["denom_S"], scale_b=th["denom_U"], down=th["down"], up=th["up"],
                                         cell_mask=cell_mask)
        else:
            m = ops.fit_weighted_moments_fused(Ux_b, Sx_b, 3, Sx_b, Ux_b, th["down"], th["up"], th["down_S"], th["up_S"], th["denom_S"],
                                               th["denom_U"], cell_mask=cell_mask)
        self._mom = m if self._mom is None else self._mom.add_(m)

    def end_walk(self) -> None:
        """Ends a walk: the all-reduce of what it counted (integer histograms, or the fp64 moments after the last walk); at the end of
        a phase its percentiles become thresholds and the next phase's selects are set up."""
        if self.walk >= self.n_walks:
            raise RuntimeError("StreamedFit.end_walk: every walk is done")
        if not self._began:                         # a rank without a block still takes part in the all-reduces
            self._begin()
        ph = self._phase()
        if ph < 3:
            for sel, _, _ in self._sel:
                self.reduced_bytes += 8 + (sel.hist[:1] if sel.pass_no == 0 else sel.hist).numel() * 4
                sel.advance(self.group)
        else:
            mom = self._mom if self._mom is not None else torch.zeros((10, self.G), dtype=torch.float64, device=self._device())
            self.reduced_bytes += mom.numel() * 8
            D.all_reduce_sum(mom, self.group)
            self.moments, self._mom = mom, None
        self.walk += 1
        if self._phase() != ph:
            self._finish(ph)
            self._began = False
            if self._phase() < 3:
                self._begin()

    def result(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(gamma, q, R2), float32 (G): the solve of VelocytoLoom.fit_gammas' branch from the summed moments, gamma with the reference's
        non-finite -> 0 (analysis.py:1260)."""
        if self.walk < self.n_walks:
            raise RuntimeError(f"StreamedFit.result: {self.walk} of {self.n_walks} walks done")
        if self._result is not None:
            return self._result
        mom, n, th = self.moments, self.n_fit_cells, self.thresholds
        solve = ops.fit_weighted_from_moments
        if self.weighted:                         # the arguments of estimation._weighted_offset_device / VelocytoLoom.fit_gammas per branch
            if self.fit_offset:
                gamma, q, R2 = solve(mom, n, fit_offset=True, box_q=True, lo_gamma=1e-8, up_gamma_default=20.0, up_gamma=th.get("up_gamma"))
            elif self.need_qf:
                gamma, q, R2 = solve(mom, n, fit_offset=False, lo_gamma=0.0, up_gamma_default=20.0, q_fixed=th["q_fixed"])
            elif self.need_up:
                gamma, q, R2 = solve(mom, n, fit_offset=False, lo_gamma=1e-8, up_gamma=th["up_gamma"])
            else:
                gamma, q, R2 = solve(mom, n, fit_offset=False, lo_gamma=0.0, up_gamma_default=20.0)
        else:
            if self.limit_gamma:
                logging.warning("limit_gamma not implemented with this settings")
            if self.fit_offset:                   # _fit1_slope_offset: ordinary least squares with an intercept
                gamma, q, R2 = solve(mom, n, fit_offset=True, box_q=False)
            elif self.need_qf:
                gamma, q, R2 = solve(mom, n, fit_offset=False, lo_gamma=0.0, up_gamma_default=20.0, q_fixed=th["q_fixed"])
            else:                                 # fit_slope: max(0, sum xy / sum xx), no upper bound
                gamma, q, R2 = solve(mom, n, fit_offset=False, lo_gamma=0.0, up_gamma_default=float("inf"))
        gamma = torch.where(torch.isfinite(gamma), gamma, torch.zeros_like(gamma))                    # analysis.py:1260
        self._result = (gamma, q, R2)
        return self._result
