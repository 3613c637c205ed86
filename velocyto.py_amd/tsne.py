"""Device t-SNE: ``sklearn.manifold.TSNE`` (``method="barnes_hut"``) as the reference's ``perform_TSNE`` calls it
(analysis.py:1441-1450), every iteration on the GPU (csrc/tsne.hip).

The same as scikit-learn 1.7 (manifold/_t_sne.py, _utils.pyx, _barnes_hut_tsne.pyx):
  * affinities: the k = min(N - 1, int(3 perplexity + 1)) exact Euclidean neighbours of every point (``ops.knn_search``), the
    distances squared in f64 and rounded to f32, every row summed in neighbour-index order by the perplexity bisection
    (``vcy_tsne_perplexity``), then P + P^T and P / sum(P);
  * the objective at dof = max(n_components - 1, 1) and the optimiser: gains +0.2 / x0.8 (at least 0.01), 250 iterations with P x
    early_exaggeration and momentum 0.5, then momentum 0.8 with a fresh update and fresh gains, the best-error and gradient-norm
    checks every 50 iterations; positions, gains and gradient in f32, the update in f64 as numpy 2 makes it; the ``"random"``
    start is bit-equal to scikit-learn's for the same ``random_state``.
Different:
  * by default (``repulsion="exact"``) the repulsion is summed EXACTLY over all pairs, so ``angle`` is accepted and ignored: the
    result is the angle -> 0 limit of scikit-learn's Barnes-Hut gradient, at O(N^2) work per iteration;
    ``repulsion="tree"`` (n_components == 2) applies scikit-learn's acceptance rule with ``angle`` on a complete quadtree of fixed
    depth rebuilt every iteration (scikit-learn's tree is adaptive, so the two accept different nodes at the same angle), or
    with ``tree_depth="adaptive"`` on a quadtree that, like scikit-learn's, is as deep as the points are dense: a cell is split while
    it holds more than ``leaf_size`` points, down to the 24 bits per axis a float32 position resolves (scikit-learn splits down to
    single points; a leaf that is not accepted is summed point by point here);
  * only the point itself is left out of its own repulsion; scikit-learn's tree also drops points that coincide with it within
    its EPSILON (neighbors/_quad_tree.pyx:413-421), so exact duplicates repel each other here;
  * KL, Z and |grad| are summed in f64 (scikit-learn sums the error in f32);
  * an ndarray ``init`` is rounded to f32 (scikit-learn keeps a float64 start in float64); ``init="pca"`` is not implemented.
"""
from __future__ import annotations

import numbers
from typing import Tuple

import numpy as np
import torch

from . import ops

MACHINE_EPSILON = np.finfo(np.double).eps


def check_random_state(seed):
    """sklearn.utils.check_random_state: None -> numpy's global RandomState, an int -> a new RandomState, a RandomState -> itself."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def _symmetrize(idx: torch.Tensor, cond: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """P = C + C^T, then P / max(sum P, eps) (_joint_probabilities_nn), for C stored as (N, k) neighbour lists: one sort of the
    (row, column) keys.  A key occurs at most twice (once from C, once from C^T), so each sum is one addition and the result does
    not depend on any order; entries that sum to exactly 0 are dropped as scipy's sparse addition drops them.
    Returns CSR (indptr int64, indices int32, values f64) with sorted columns."""
    N, k = idx.shape
    dev = idx.device
    rows = torch.arange(N, device=dev, dtype=torch.int64).repeat_interleave(k)
    cols = idx.reshape(-1).to(torch.int64)
    v = cond.reshape(-1)
    keys, order = torch.sort(torch.cat([rows * N + cols, cols * N + rows]), stable=True)
    vals = torch.cat([v, v])[order]
    n = keys.numel()
    first = torch.ones(n, dtype=torch.bool, device=dev)
    first[1:] = keys[1:] != keys[:-1]
    start = torch.nonzero(first).squeeze(1)
    nxt = (start + 1).clamp(max=n - 1)
    dup = (start + 1 < n) & (keys[nxt] == keys[start])
    data = vals[start] + torch.where(dup, vals[nxt], torch.zeros_like(vals[start]))
    keep = data != 0
    ukeys, data = keys[start][keep], data[keep]
    indptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(ukeys // N, minlength=N), 0)
    data = data / torch.clamp(data.sum(), min=MACHINE_EPSILON)
    return indptr, (ukeys % N).to(torch.int32).contiguous(), data


class DeviceTSNE:
    """``sklearn.manifold.TSNE(method="barnes_hut", metric="euclidean")`` on the device: the same constructor arguments,
    ``fit_transform`` and the fitted attributes ``embedding_``, ``kl_divergence_``, ``n_iter_``, ``learning_rate_``,
    ``n_features_in_`` (see the module docstring for what differs).

    repulsion: ``"exact"`` (the default) sums the repulsion over all pairs, O(N^2) per iteration; ``angle`` is accepted and IGNORED.
    ``"tree"`` (n_components == 2 only) uses scikit-learn's Barnes-Hut acceptance rule with ``angle`` (0 <= angle <= 1) on a quadtree
    of ``tree_depth`` levels (None: ``ops.tsne_tree_depth(N)``), O(N log N); its iteration is the faster one above about 50 000
    points (DESIGN.md section 9 has the measurements).  ``tree_depth="adaptive"`` builds the tree to the depth the density asks for
    instead (cells of more than ``leaf_size`` points are split), so that an iteration costs the same however the points are clumped;
    ``leaf_size`` (None: ``ops.TSNE_ATREE_LEAF_SIZE``) is read in that mode only."""

    _EXPLORATION_MAX_ITER = 250
    _N_ITER_CHECK = 50

    def __init__(self, n_components: int = 2, *, perplexity: float = 30.0, early_exaggeration: float = 12.0, learning_rate="auto",
                 max_iter: int = 1000, n_iter_without_progress: int = 300, min_grad_norm: float = 1e-7, init="random", random_state=None,
                 angle: float = 0.5, repulsion: str = "exact", tree_depth=None, leaf_size=None):
        self.repulsion, self.tree_depth, self.leaf_size = repulsion, tree_depth, leaf_size
        self.n_components, self.perplexity, self.early_exaggeration = n_components, perplexity, early_exaggeration
        self.learning_rate, self.max_iter, self.n_iter_without_progress = learning_rate, max_iter, n_iter_without_progress
        self.min_grad_norm, self.init, self.random_state, self.angle = min_grad_norm, init, random_state, angle

    def _check_params(self, shape) -> None:
        """scikit-learn's parameter validation, _check_params_vs_input and the Barnes-Hut dimension limit - before any device work."""
        if len(shape) != 2:
            raise ValueError(f"Expected 2D array, got array with shape {tuple(shape)}")
        N = shape[0]
        nc = self.n_components
        self._check_repulsion(self.repulsion, nc, self.angle, self.tree_depth, self.leaf_size)
        if not isinstance(nc, numbers.Integral) or isinstance(nc, bool) or nc < 1:
            raise ValueError(f"The 'n_components' parameter of TSNE must be an int in the range [1, inf). Got {nc!r} instead.")
        if not (isinstance(self.perplexity, numbers.Real) and self.perplexity > 0):
            raise ValueError(f"The 'perplexity' parameter of TSNE must be a float in the range (0.0, inf). Got {self.perplexity!r} instead.")
        if not (isinstance(self.early_exaggeration, numbers.Real) and self.early_exaggeration >= 1):
            raise ValueError(f"The 'early_exaggeration' parameter of TSNE must be a float in the range [1, inf). Got {self.early_exaggeration!r} instead.")
        if not (isinstance(self.learning_rate, str) and self.learning_rate == "auto"
                or isinstance(self.learning_rate, numbers.Real) and not isinstance(self.learning_rate, str) and self.learning_rate > 0):
            raise ValueError(f"The 'learning_rate' parameter of TSNE must be 'auto' or a float in the range (0.0, inf). Got {self.learning_rate!r} instead.")
        if not (isinstance(self.max_iter, numbers.Integral) and self.max_iter >= self._EXPLORATION_MAX_ITER):
            raise ValueError(f"The 'max_iter' parameter of TSNE must be an int in the range [250, inf). Got {self.max_iter!r} instead.")
        if isinstance(self.init, str):
            if self.init == "pca":
                raise NotImplementedError("DeviceTSNE: init='pca' is not implemented (the reference passes 'random' or an array)")
            if self.init != "random":
                raise ValueError(f"The 'init' parameter of TSNE must be a str among {{'pca', 'random'}} or an array-like. Got {self.init!r} instead.")
        elif np.shape(self.init) != (N, nc):
            raise ValueError(f"init has shape {np.shape(self.init)}, expected (n_samples, n_components) = ({N}, {nc})")
        if self.perplexity >= N:
            raise ValueError(f"perplexity ({self.perplexity}) must be less than n_samples ({N})")
        if N < 2:
            raise ValueError(f"Found array with {N} sample(s) (shape={tuple(shape)}) while a minimum of 2 is required by TSNE.")
        if nc > 3:
            raise ValueError("'n_components' should be inferior to 4 for the barnes_hut algorithm as it relies on quad-tree or oct-tree.")

    @staticmethod
    def _check_repulsion(repulsion, n_components, angle, tree_depth, leaf_size=None) -> None:
        if repulsion not in ("exact", "tree"):
            raise ValueError(f"The 'repulsion' parameter of DeviceTSNE must be 'exact' or 'tree'. Got {repulsion!r} instead.")
        if repulsion == "tree":
            if n_components != 2:
                raise NotImplementedError("DeviceTSNE: repulsion='tree' is implemented for n_components == 2 only")
            if not (isinstance(angle, numbers.Real) and 0.0 <= angle <= 1.0):
                raise ValueError(f"The 'angle' parameter of TSNE must be a float in the range [0.0, 1.0]. Got {angle!r} instead.")
            if isinstance(tree_depth, str):
                if tree_depth != "adaptive":
                    raise ValueError(f"tree_depth must be None, 'adaptive' or an int in the range [1, 11]. Got {tree_depth!r} instead.")
                if leaf_size is not None and not (isinstance(leaf_size, numbers.Integral) and not isinstance(leaf_size, bool) and leaf_size >= 1):
                    raise ValueError(f"leaf_size must be None or an int in the range [1, inf). Got {leaf_size!r} instead.")
            elif tree_depth is not None and not (isinstance(tree_depth, numbers.Integral) and 1 <= tree_depth <= 11):
                raise ValueError(f"tree_depth must be None, 'adaptive' or an int in the range [1, 11]. Got {tree_depth!r} instead.")

    def fit_transform(self, X, y=None) -> np.ndarray:
        """X: (n_samples, n_features) host array or device tensor.  Returns the embedding (n_samples, n_components) float32."""
        if not isinstance(X, torch.Tensor):
            X = np.asarray(X, dtype=np.float64)
        self._check_params(tuple(X.shape))
        N = int(X.shape[0])
        self.n_features_in_ = int(X.shape[1])
        self.learning_rate_ = np.maximum(N / self.early_exaggeration / 4, 50) if isinstance(self.learning_rate, str) else self.learning_rate
        dev = ops.require_gpu()
        X64 = (X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X))).to(dev, torch.float64)
        if not bool(torch.isfinite(X64).all()):
            raise ValueError("Input X contains NaN, infinity or a value too large for dtype('float64').")
        aff = self._affinities(X64)
        Y = torch.from_numpy(self._initial_embedding(N)).to(dev)
        Y = self._tsne(aff["indptr"], aff["indices"], aff["P"], Y)
        self.embedding_ = Y.cpu().numpy()
        return self.embedding_

    def _initial_embedding(self, N: int) -> np.ndarray:
        if isinstance(self.init, str):        # "random": scikit-learn's draw (_t_sne.py:1021-1026), host RNG, same expression
            return 1e-4 * check_random_state(self.random_state).standard_normal(size=(N, self.n_components)).astype(np.float32)
        return np.ascontiguousarray(self.init, dtype=np.float32)

    def _affinities(self, X64: torch.Tensor) -> dict:
        """_joint_probabilities_nn on the device: the neighbours (each row in index order), their f32 squared distances, the
        conditional P and its bisection steps, and the joint P as CSR (indptr int64, indices int32, P f64)."""
        N = X64.shape[0]
        k = min(N - 1, int(3.0 * self.perplexity + 1))
        # centred first: the search's f32 candidate pass measures |x|-relative, distances do not change
        idx, dist = ops.knn_search(X64 - X64.mean(0, keepdim=True), k)
        idx, order = torch.sort(idx, dim=1)                      # distances.sort_indices(): each row in neighbour-index order
        dist = torch.gather(dist, 1, order)
        sqd = (dist * dist).to(torch.float32)                    # distances_nn.data **= 2 (f64), then .astype(np.float32)
        cond, steps = ops.tsne_perplexity(sqd, self.perplexity)
        indptr, indices, P = _symmetrize(idx, cond)
        return dict(idx=idx, sqd=sqd, cond=cond, steps=steps, indptr=indptr, indices=indices, P=P)

    def _tsne(self, indptr: torch.Tensor, indices: torch.Tensor, P: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        """TSNE._tsne: the two phases of the learning schedule; P's values are read as f32 by the kernels, as scikit-learn's
        objective reads them, after P *= early_exaggeration and P /= early_exaggeration in f64."""
        ee = self.early_exaggeration
        P_ex = P * ee
        Y, kl, it = self._gradient_descent(Y, (indptr, indices, P_ex.to(torch.float32)), 0, self._EXPLORATION_MAX_ITER, 0.5,
                                           self._EXPLORATION_MAX_ITER)
        if it < self._EXPLORATION_MAX_ITER or self.max_iter - self._EXPLORATION_MAX_ITER > 0:
            Y, kl, it = self._gradient_descent(Y, (indptr, indices, (P_ex / ee).to(torch.float32)), it + 1, self.max_iter, 0.8,
                                               self.n_iter_without_progress)
        self.n_iter_, self.kl_divergence_ = it, kl
        return Y

    def _repulsion_calls(self, N: int, d: int, repulsion, angle, tree_depth, leaf_size):
        """The repulsion, chosen once for N points in d dimensions, as what the optimiser and the objective call:
        (step(Y, Y_next, csr, update, gains, stats, momentum, lr, min_gain, want), gradient(Y, csr) -> (grad, stats), whether the
        positions and the objective are checked for being finite).  The workspace is made here; a tree's keys are taken per call."""
        self._check_repulsion(repulsion, d, angle, tree_depth, leaf_size)
        if repulsion != "tree":
            ws = ops.tsne_workspace(N, d)
            return (lambda Y, Y_next, csr, update, gains, stats, *opt: ops.tsne_step(Y, Y_next, *csr, update, gains, stats, ws, *opt),
                    lambda Y, csr: ops.tsne_gradient(Y, *csr, compute_error=True, ws=ws), False)
        if isinstance(tree_depth, str):
            leaf = ops.TSNE_ATREE_LEAF_SIZE if leaf_size is None else int(leaf_size)
            ws = ops.tsne_atree_workspace(N, leaf)
            keys = lambda Y: ops.tsne_atree_keys(Y, ws, leaf)[1:]
            return (lambda Y, Y_next, csr, update, gains, stats, *opt:
                    ops.tsne_atree_step(Y, Y_next, *csr, *keys(Y), update, gains, stats, ws, angle, *opt, leaf_size=leaf),
                    lambda Y, csr: ops.tsne_atree_gradient(Y, *csr, *keys(Y), ws, angle, leaf_size=leaf, compute_error=True), True)
        depth = ops.tsne_tree_depth(N) if tree_depth is None else int(tree_depth)
        ws = ops.tsne_tree_workspace(N, depth)
        keys = lambda Y: ops.tsne_tree_keys(Y, ws, depth)[1:]
        return (lambda Y, Y_next, csr, update, gains, stats, *opt:
                ops.tsne_tree_step(Y, Y_next, *csr, *keys(Y), update, gains, stats, ws, depth, angle, *opt),
                lambda Y, csr: ops.tsne_tree_gradient(Y, *csr, *keys(Y), ws, depth, angle, compute_error=True), True)

    def _gradient_descent(self, Y: torch.Tensor, csr, it: int, max_iter: int, momentum: float, n_iter_without_progress: int):
        """_gradient_descent (_t_sne.py:301-444) from positions Y (N, d) f32 on the device: fresh update and gains, one vcy_tsne_step
        per iteration on one stream; the host reads back [Z, KL, |grad|^2] only where scikit-learn computes the error (every 50th
        iteration and the last).  Returns (positions, error, last iteration).
        repulsion="tree": per iteration the keys, their sort and vcy_tsne_tree_step (tree_depth="adaptive": vcy_tsne_atree_step); the
        read at a check also carries whether the new positions are finite, and a fit whose positions are not stops there with a
        FloatingPointError."""
        N, d = Y.shape
        step, _, finite = self._repulsion_calls(N, d, self.repulsion, self.angle, self.tree_depth, self.leaf_size)
        update = torch.zeros((N, d), dtype=torch.float64, device=Y.device)
        gains = torch.ones((N, d), dtype=torch.float32, device=Y.device)
        Y_next = torch.empty_like(Y)
        stats = torch.zeros(4, dtype=torch.float64, device=Y.device)
        lr = float(self.learning_rate_)
        error = best_error = np.finfo(float).max
        best_iter = i = it
        for i in range(it, max_iter):
            check = (i + 1) % self._N_ITER_CHECK == 0
            want = check or i == max_iter - 1
            step(Y, Y_next, csr, update, gains, stats, momentum, lr, 0.01, want)
            Y, Y_next = Y_next, Y
            if want and finite:
                h = torch.cat([stats, torch.isfinite(Y).all().to(torch.float64).reshape(1)]).cpu().numpy()
                if h[4] != 1.0 or not np.all(np.isfinite(h[:3])):
                    raise FloatingPointError(f"DeviceTSNE(repulsion='tree'): non-finite positions or objective at iteration {i}")
                error = float(h[1])
            elif want:
                h = stats.cpu().numpy()
                error = float(h[1])
            if check:
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > n_iter_without_progress:
                    break
                if float(np.sqrt(h[2])) <= self.min_grad_norm:
                    break
        self._gains = gains
        return Y, error, i

    # ------------------------------------------------------------------ helpers for the tests (scipy CSR P, as scikit-learn's)
    @staticmethod
    def _device_args(Y, P):
        dev = ops.require_gpu()
        Yd = torch.from_numpy(np.ascontiguousarray(np.asarray(Y, dtype=np.float32).reshape(P.shape[0], -1))).to(dev)
        csr = (torch.from_numpy(np.asarray(P.indptr, dtype=np.int64)).to(dev), torch.from_numpy(np.asarray(P.indices, dtype=np.int32)).to(dev),
               torch.from_numpy(np.asarray(P.data, dtype=np.float32)).to(dev))
        return Yd, csr

    def _objective(self, Y, P, repulsion: str = "exact", angle: float = 0.5, tree_depth=None, leaf_size=None) -> Tuple[float, np.ndarray]:
        """(KL, grad (N, d) f32) for positions Y and a scipy CSR P (its values read as f32): of _kl_divergence_bh at angle = 0
        (repulsion="exact"), or with the tree repulsion at ``angle`` (repulsion="tree"; tree_depth="adaptive": the adaptive tree)."""
        Yd, csr = self._device_args(Y, P)
        _, gradient, _ = self._repulsion_calls(*Yd.shape, repulsion, angle, tree_depth, leaf_size)
        grad, stats = gradient(Yd, csr)
        return float(stats[1]), grad.cpu().numpy()

    def _descend(self, Y0, P, it: int, max_iter: int, momentum: float, n_iter_without_progress: int = 300):
        """_gradient_descent from Y0 on a scipy CSR P (``learning_rate_`` must be set): (positions, error, last iteration, gains)."""
        Yd, csr = self._device_args(Y0, P)
        Y, err, i = self._gradient_descent(Yd, csr, it, max_iter, momentum, n_iter_without_progress)
        return Y.cpu().numpy(), err, i, self._gains.cpu().numpy()
