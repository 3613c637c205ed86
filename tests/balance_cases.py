"""Cases and plain-numpy references for the balanced kNN selection (neighbors.py:11-183).  No product import.

reference_loop   the reference's greedy loop, restated literally (knn_balance + balance_knn_loop[_constrained])
fixed_point      the same integers as the fixed point of a parallel iteration, with its round count
chain / hub / ... constructed sight lists that reach the edges of both
"""
import numpy as np


def processing_order(dsi):
    """neighbors.py:172-174: in-degree of the sight graph, stable ascending argsort reversed (ties: descending cell number)."""
    n = dsi.shape[0]
    l0 = np.bincount(np.asarray(dsi).ravel(), minlength=n)
    return np.argsort(l0, kind="mergesort")[::-1]


def reference_loop(dsi, dist, maxl, k, groups=None):
    """knn_balance(dsi, dist, maxl, k, constraint=groups): (dist_new, dsi_new, l), float64 / int64 / int64."""
    dsi = np.asarray(dsi, dtype=np.int64)
    n, K = dsi.shape
    assert K >= k, "sight needs to be bigger than k"
    return_distance = dist is not None
    if dist is None:
        dist = np.ones((n, K), dtype=np.float64)
        dist[:, 0] = 0
    lsi = processing_order(dsi)
    dsi_new = -1 * np.ones((n, k + 1), np.int64)            # neighbors.py:38-45
    dist_new = np.zeros((n, k + 1), np.float64)
    l = np.zeros(n, np.int64)
    for el in lsi:                                          # neighbors.py:47-69 / 113-137
        p = 0
        j = 0
        while p < k and j < K:
            m = dsi[el, j]
            if el == m:
                dsi_new[el, 0] = el
                j += 1
                continue
            if groups is not None and groups[el] != groups[m]:
                j += 1
                continue
            if l[m] >= maxl:
                j += 1
                continue
            p += 1
            dsi_new[el, p] = m
            if return_distance:
                dist_new[el, p] = dist[el, j]
            l[m] += 1
            j += 1
        while p < k:                                        # sight exhausted: pad with the cell itself
            p += 1
            dsi_new[el, p] = el
            dist_new[el, p] = dist[el, 0]
    if not return_distance:
        dist_new = np.ones_like(dist_new)
    return dist_new, dsi_new, l


def fixed_point(dsi, dist, maxl, k, groups=None, max_rounds=None):
    """The loop's result as a fixed point.  rank[lsi[i]] = i; s[m] = the maxl-th smallest rank among the cells that take m (n when
    fewer than maxl take it); cell el may take m exactly when rank[el] <= s[m].  A round: every cell, independently, takes the first
    k entries of its list that are not itself, are of its group and are open to it; then every s[m] is recomputed.  Rounds are
    counted until a round changes no selection (that confirming round included).  Returns (dist_new, dsi_new, l, rounds)."""
    dsi = np.asarray(dsi, dtype=np.int64)
    n, K = dsi.shape
    assert K >= k, "sight needs to be bigger than k"
    lsi = processing_order(dsi)
    rank = np.empty(n, np.int64)
    rank[lsi] = np.arange(n)
    me = np.arange(n)[:, None]
    static = dsi != me
    if groups is not None:
        groups = np.asarray(groups)
        static &= groups[dsi] == groups[:, None]
    s = np.full(n, n, np.int64)
    prev, rounds = None, 0
    while True:
        open_ = static & (rank[:, None] <= s[dsi])
        order = np.cumsum(open_, 1)
        take = open_ & (order <= k)
        sel = np.full((n, k), -1, np.int64)                 # positions of the picks, list order
        r, j = np.nonzero(take)
        sel[r, order[r, j] - 1] = j
        rounds += 1
        if prev is not None and np.array_equal(sel, prev):
            break
        if max_rounds is not None and rounds >= max_rounds:
            raise RuntimeError(f"no fixed point after {rounds} rounds")
        prev = sel
        nodes, ranks = dsi[r, j], rank[r]
        o = np.lexsort((ranks, nodes))
        nodes, ranks = nodes[o], ranks[o]
        start = np.searchsorted(nodes, np.arange(n), "left")
        l = np.searchsorted(nodes, np.arange(n), "right") - start
        s = np.full(n, n, np.int64)
        capped = l >= maxl
        s[capped] = ranks[start[capped] + maxl - 1]
    # the loop's output arrays, quirks included
    picked = sel >= 0
    npick = picked.sum(1)
    last = np.where(npick == k, sel[:, k - 1], K)           # the loop reads the entries before its k-th pick, or the whole list
    own = np.where(dsi == me, np.arange(K)[None, :], K).min(1)
    dsi_new = np.empty((n, k + 1), np.int64)
    dsi_new[:, 0] = np.where(own < last, np.arange(n), -1)
    dsi_new[:, 1:] = np.where(picked, np.take_along_axis(dsi, np.maximum(sel, 0), 1), me)
    if dist is None:
        dist_new = np.ones((n, k + 1), np.float64)
    else:
        dist = np.asarray(dist, dtype=np.float64)
        dist_new = np.zeros((n, k + 1), np.float64)
        dist_new[:, 1:] = np.where(picked, np.take_along_axis(dist, np.maximum(sel, 0), 1), dist[:, :1])
    l = np.bincount(dsi_new[:, 1:][picked], minlength=n).astype(np.int64)
    return dist_new, dsi_new, l, rounds


# ------------------------------------------------------------------------------------------------------------ constructed lists
def ascending_dist(n, K, seed=0):
    """Distances that go with any (n, K) lists whose column 0 is the cell: 0 first, then ascending positive values."""
    d = np.sort(np.random.default_rng(seed).random((n, K)) + 0.05, 1)
    d[:, 0] = 0
    return d


def random_lists(n, K, seed, self_at=0):
    """Random sight lists without repeats, K <= n.  self_at: the column that holds the cell itself (None: absent, needs K < n)."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, K), np.int64)
    for c in range(n):
        others = rng.permutation(np.delete(np.arange(n), c))
        if self_at is None:
            out[c] = others[:K]
        else:
            row = list(others[:K - 1])
            row.insert(self_at, c)
            out[c] = row
    return out


def chain(n):
    """n even, k = maxl = 1, K = 3.  Cell c has r = n - 1 - c and the list [c, r - 1, r]; cell n - 1 has [n - 1, 0, 1].  Every cell's
    pick depends on the pick of a cell two ranks earlier, so the rounds grow as n / 2: 31 at n = 64, 99 at n = 200."""
    assert n % 2 == 0 and n >= 4
    c = np.arange(n)
    r = n - 1 - c
    dsi = np.stack([c, r - 1, r], 1)
    dsi[n - 1] = [n - 1, 0, 1]
    return dsi.astype(np.int64)


def hub(n, K, seed=5):
    """Every list starts [el, 0, ...] (cell 0's: [0, 1, ...]): node 0 goes to the first maxl cells in lsi order."""
    dsi = random_lists(n, K, seed)
    for c in range(1, n):
        row = [int(v) for v in dsi[c] if v not in (c, 0)]
        dsi[c] = [c, 0] + row[:K - 2]
    return dsi


def two_groups(n):
    return (np.arange(n) % 2).astype(np.int64)


def own_groups(n):
    return np.arange(n, dtype=np.int64)


def scarce_groups(n, dsi, k):
    """Group 1 is so small that its cells' lists cannot give them k neighbours of their own group; group 0 fills every row."""
    g = np.zeros(n, np.int64)
    g[: max(2, min(k, n // 8))] = 1
    return g


# ------------------------------------------------------------------------------------------------------------ the case lists
def golden_case(g, tag):
    """(dsi, dist, maxl, k, groups) of a golden vector of tests/golden/neighbors.npz (n = 220, k = 9)."""
    if tag == "bal":
        return g["bal_dsi"], g["bal_dist"], 14, 9, None
    if tag == "balc":
        return g["balc_dsi"], g["balc_dist"], 14, 9, g["groups"]
    if tag == "pad":
        return g["bal_dsi"][:, :12], g["bal_dist"][:, :12], 4, 9, None
    assert tag == "nd"                                        # no distances
    return g["bal_dsi"], None, 14, 9, None


WALK_N = (2, 63, 64, 65, 257, 1000)
WALK_K = (1, 9, 63, 64, 65)


def walk_shapes():
    """(n, K, k) at the chunk edges of the list walk: K in {k, k + 1, 63, 64, 65, 128, 129, 241} for every k of WALK_K, each on
    one n of WALK_N with K <= n (taken in turn, so that every n occurs)."""
    out = [(2, 1, 1), (2, 2, 1)]
    i = 0
    for k in WALK_K:
        for K in sorted({k, k + 1, 63, 64, 65, 128, 129, 241}):
            if K < k:
                continue
            fits = [n for n in WALK_N if n >= max(K, 3)]
            out.append((fits[i % len(fits)], K, k))
            i += 1
    return out


def walk_cases():
    """(name, dsi, dist, maxl, k, groups): random lists with the cell itself in column 0, maxl in {1, k, n - 1}."""
    out = []
    for n, K, k in walk_shapes():
        dsi, dist = random_lists(n, K, seed=1000 * k + K), ascending_dist(n, K, seed=K)
        for maxl in sorted({1, k, max(1, n - 1)}):
            out.append((f"n{n}-K{K}-k{k}-maxl{maxl}", dsi, dist, maxl, k, None))
    return out


def constructed_cases():
    """(name, dsi, dist, maxl, k, groups): the hub, the group variants, the cell itself at position 0, 3, K - 1 and absent."""
    n, K, k = 65, 20, 9
    h, d = hub(n, K), ascending_dist(n, K)
    out = [("hub", h, d, 9, k, None), ("two-groups", h, d, 9, k, two_groups(n)), ("own-groups", h, d, 9, k, own_groups(n)),
           ("scarce-group", h, d, 9, k, scarce_groups(n, h, k))]
    for at in (0, 3, 11, None):
        for maxl in (1, 3, 39):
            out.append((f"self-at-{at}-maxl{maxl}", random_lists(40, 12, 3, at), None, maxl, 3, None))
    return out
