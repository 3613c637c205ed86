"""The adaptive-quadtree repulsion of the device t-SNE (csrc/tsne.hip: k_atree_*, vcy_tsne_atree_*) restated
in plain numpy, and the cases its tests share.  tests/test_tsne_atree_oracle.py pins this restatement on the f64 all-pairs sum, on a
recursive build and on scikit-learn's Barnes-Hut gradient (CPU); tests/test_gpu_tsne_atree.py holds the kernels to it.

The algorithm, per evaluation of positions Y (N, 2) f32 at key depth D (1 .. 24), leaf_size and angle:
  box      as the fixed tree's (tsne_tree_cases.box); scale = 2^D / side, or 0 when side is 0;
  keys     ix = min(2^D - 1, floor((y - lo) scale)) in f64, every operation rounded on its own; key = int64 Morton interleave of the
           two D-bit cell numbers, x in the even bits;
  order    stable argsort of the keys;
  nodes    the root (level 0) holds all points; a node of level l with n points is a leaf iff n <= leaf_size or l == D, otherwise
           its children are the non-empty ones of its four level-(l + 1) cells in Morton order; nodes are numbered in depth-first
           preorder and carry skip = the number of the first node after their subtree;
  com      leaf: the f64 sum of its points in sorted order from 0.0; internal: 0.0 + its children's sums in child order;
           com = f32(sum / count);
  walk     per target, depth-first from the root: a node of level l is accepted iff f32((side 2^-l)^2) < f32(angle^2) (dx dx + dy dy)
           in float32 operations against com, and then adds count q and count q^2 (t - com), q = 1 / (1 + d^2); a leaf that is not
           accepted adds its points one by one, the target itself (by index) left out; any other node is opened.
The interaction sums here are f64 (from the f32 positions and centres); the decisions are float32, bit for bit the kernel's.
"""
import numpy as np

from tsne_tree_cases import GAMMA, U, blobs, box, embedding, exact_repulsion, rel_error  # noqa: F401  (shared with the fixed tree's tests)

MAX_DEPTH = 24
DEFAULT_LEAF = 32                 # ops.TSNE_ATREE_LEAF_SIZE


def node_bound(N, leaf_size, D):
    """1 + 4 D floor(N / (leaf_size + 1)): a level has at most floor(N / (leaf_size + 1)) internal nodes, each at most 4 children."""
    return 1 + 4 * D * (N // (leaf_size + 1))


def _spread(x):
    x = x.astype(np.uint64) & np.uint64(0xFFFFFF)
    for s, m in ((16, 0x0000FFFF0000FFFF), (8, 0x00FF00FF00FF00FF), (4, 0x0F0F0F0F0F0F0F0F), (2, 0x3333333333333333), (1, 0x5555555555555555)):
        x = (x | (x << np.uint64(s))) & np.uint64(m)
    return x


def keys(Y, D):
    """(keys (N) int64, lo (2) f64, side, scale)."""
    Y = np.asarray(Y, np.float32)
    lo, side = box(Y)
    scale = float(np.float64(2 ** D) / np.float64(side)) if 0.0 < side < np.inf else 0.0
    t = (Y.astype(np.float64) - lo) * np.float64(scale)
    top = float(2 ** D - 1)
    cell = np.where(t >= 0.0, np.minimum(np.floor(t), top), 0.0).astype(np.int64)
    k = _spread(cell[:, 0]) | (_spread(cell[:, 1]) << np.uint64(1))
    return k.astype(np.int64), lo, side, scale


def build_scan(sk, leaf_size, D):
    """The numbering by flags and one scan, from the sorted keys alone: position i starts the nodes of levels l0(i) .. l1(i), l0 =
    the first level at which the key prefix differs from position i - 1, l1 = min(D, 1 + the deepest level whose cell around i
    holds more than leaf_size points); preorder is the order by (start position, level).
    Returns dict of (nodes) arrays: level, start, count, skip, leaf."""
    sk = np.asarray(sk, np.int64)
    N = len(sk)
    l0 = np.full(N, -1, np.int64)
    l0[0] = 0
    x = sk[1:] ^ sk[:-1]
    nz = np.nonzero(x)[0]
    h = np.frexp(x[nz].astype(np.float64))[1] - 1                       # the highest differing bit (keys < 2^48: exact in f64)
    l0[nz + 1] = D - (h >> 1)
    ub = np.empty((D + 1, N), np.int64)
    deepest = np.full(N, -1, np.int64)
    for l in range(D + 1):
        sh = 2 * (D - l)
        p = sk >> sh
        lb = np.searchsorted(sk, p << sh, side="left")
        ub[l] = np.searchsorted(sk, (p + 1) << sh, side="left")
        deepest[ub[l] - lb > leaf_size] = l                              # the count falls monotonically with the level
    l1 = np.minimum(D, 1 + deepest)
    n_start = np.where(l0 >= 0, np.maximum(l1 - l0 + 1, 0), 0)
    base = np.zeros(N + 1, np.int64)
    base[1:] = np.cumsum(n_start)
    pos = np.repeat(np.arange(N), n_start)
    level = l0[pos] + (np.arange(base[N]) - base[pos])
    end = ub[level, pos]
    count = end - pos
    return dict(level=level.astype(np.int32), start=pos.astype(np.int32), count=count.astype(np.int32), skip=base[end].astype(np.int32),
                leaf=(count <= leaf_size) | (level == D))


def build_recursive(sk, leaf_size, D):
    """The same nodes by the definition: a depth-first recursion that splits a node's range by the next two key bits."""
    sk = np.asarray(sk, np.int64)
    level, start, count, skip, leaf = [], [], [], [], []

    def rec(b, e, l):
        me = len(level)
        is_leaf = e - b <= leaf_size or l == D
        level.append(l), start.append(b), count.append(e - b), skip.append(-1), leaf.append(is_leaf)
        if not is_leaf:
            sh = 2 * (D - l - 1)
            first = (sk[b] >> (sh + 2)) << 2
            cut = b + np.searchsorted(sk[b:e] >> sh, first + np.arange(5), side="left")
            for c in range(4):
                if cut[c + 1] > cut[c]:
                    rec(int(cut[c]), int(cut[c + 1]), l + 1)
        skip[me] = len(level)

    rec(0, len(sk), 0)
    return dict(level=np.asarray(level, np.int32), start=np.asarray(start, np.int32), count=np.asarray(count, np.int32),
                skip=np.asarray(skip, np.int32), leaf=np.asarray(leaf, bool))


def children_of(nodes):
    """(nodes, 4) child numbers in child order, -1 where there is none: the first child is the next node, a sibling its skip."""
    nn = len(nodes["level"])
    ch = np.full((nn, 4), -1, np.int64)
    cur = np.where(nodes["leaf"], -1, np.arange(nn) + 1)
    for c in range(4):
        ok = cur >= 0
        ch[ok, c] = cur[ok]
        nxt = np.full(nn, -1, np.int64)
        nxt[ok] = nodes["skip"][cur[ok]]
        nxt[ok & (nxt >= nodes["skip"])] = -1
        cur = nxt
    assert not (cur >= 0).any()
    return ch


def tree(Y, leaf_size=DEFAULT_LEAF, D=MAX_DEPTH):
    """dict: keys, order (stable), lo, side, scale, D, leaf_size, the node arrays of build_scan, children, sum (nodes, 2) f64 and
    com (nodes, 2) f32."""
    Y = np.asarray(Y, np.float32)
    k, lo, side, scale = keys(Y, D)
    order = np.argsort(k, kind="stable")
    sk = k[order]
    nodes = build_scan(sk, leaf_size, D)
    ch = children_of(nodes)
    nn = len(nodes["level"])
    ys = Y[order].astype(np.float64)
    sums = np.zeros((nn, 2))
    for l in range(D, -1, -1):
        lv = np.nonzero((nodes["level"] == l) & nodes["leaf"])[0]
        for r in range(int(nodes["count"][lv].max(initial=0))):         # the r-th point of every leaf: sequential f64 sums from 0.0
            sel = lv[nodes["count"][lv] > r]
            sums[sel] = sums[sel] + ys[nodes["start"][sel] + r]
        iv = np.nonzero((nodes["level"] == l) & ~nodes["leaf"])[0]
        acc = np.zeros((len(iv), 2))
        for c in range(4):
            has = ch[iv, c] >= 0
            acc[has] = acc[has] + sums[ch[iv[has], c]]
        sums[iv] = acc
    com = (sums / nodes["count"][:, None]).astype(np.float32)
    return dict(keys=k, order=order, lo=lo, side=side, scale=scale, D=D, leaf_size=leaf_size, children=ch, sum=sums, com=com, **nodes)


def repulsion(Y, leaf_size, D, angle, tr=None, chunk=256):
    """The walk of every target.  Returns a dict, everything indexed by the point's original number:
    rep (N, 2), W (N), Z, A (N, 2) = the sums of |force terms|, visits (N, 2) int32 = accepted nodes, directly summed points."""
    Y = np.asarray(Y, np.float32)
    N = Y.shape[0]
    tr = tree(Y, leaf_size, D) if tr is None else tr
    order, side = tr["order"], tr["side"]
    pos = np.empty(N, np.int64)
    pos[order] = np.arange(N)
    ys64 = Y[order].astype(np.float64)
    th2 = np.float32(float(angle) * float(angle))
    w2 = np.asarray([np.float32((np.float64(side) * 2.0 ** -l) ** 2) for l in range(D + 1)], np.float32)
    cnt64 = tr["count"].astype(np.float64)
    nchild = (tr["children"] >= 0).sum(1)
    rep, A, W = np.zeros((N, 2)), np.zeros((N, 2)), np.zeros(N)
    visits = np.zeros((N, 2), np.int64)

    def add(ti, d, mult, n):
        q = 1.0 / (1.0 + (d * d).sum(1))
        w[:] += np.bincount(ti, weights=mult * q, minlength=n)
        for a in range(2):
            f[:, a] += np.bincount(ti, weights=mult * q * q * d[:, a], minlength=n)
            fa[:, a] += np.bincount(ti, weights=mult * q * q * np.abs(d[:, a]), minlength=n)

    for s in range(0, N, chunk):
        T = np.arange(s, min(N, s + chunk))
        n = len(T)
        t32, t64 = Y[T], Y[T].astype(np.float64)
        f, fa, w = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n)
        nacc, ndir = np.zeros(n, np.int64), np.zeros(n, np.int64)
        ti, m = np.arange(n), np.zeros(n, np.int64)
        while len(ti):                                                       # one level of the tree per round
            com = tr["com"][m]
            dx, dy = t32[ti, 0] - com[:, 0], t32[ti, 1] - com[:, 1]            # float32 operations, each rounded on its own
            d2 = dx * dx + dy * dy
            with np.errstate(over="ignore", invalid="ignore"):
                take = w2[tr["level"][m]] < th2 * d2
            assert d2.dtype == np.float32 and (th2 * d2).dtype == np.float32
            if take.any():
                add(ti[take], t64[ti[take]] - com[take].astype(np.float64), cnt64[m[take]], n)
                nacc += np.bincount(ti[take], minlength=n)
            ti, m = ti[~take], m[~take]
            lf = tr["leaf"][m]
            if lf.any():
                tl, ml = ti[lf], m[lf]
                b, c = tr["start"][ml].astype(np.int64), tr["count"][ml].astype(np.int64)
                tj = np.repeat(tl, c)
                j = np.repeat(b, c) + (np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c))
                other = j != pos[T][tj]
                tj, j = tj[other], j[other]
                add(tj, t64[tj] - ys64[j], 1.0, n)
                ndir += np.bincount(tj, minlength=n)
            ti, m = ti[~lf], m[~lf]
            kids = tr["children"][m]
            ti, m = np.repeat(ti, nchild[m]), kids[kids >= 0]
        rep[T], A[T], W[T] = f, fa, w
        visits[T, 0], visits[T, 1] = nacc, ndir
    return dict(rep=rep, A=A, W=W, Z=float(W.sum()), visits=visits.astype(np.int32))


# ---------------------------------------------------------------------------------------------- embeddings
def clumps(N, radius, seed=0):
    """12 clumps of the given radius in a box of side 100: what a fit looks like during early exaggeration."""
    rng = np.random.default_rng([seed, N, 12])
    c = rng.uniform(0.0, 100.0, (12, 2))
    return np.ascontiguousarray(c[np.arange(N) % 12] + radius * rng.standard_normal((N, 2)), dtype=np.float32)


def points(kind, N, seed=0):
    if kind == "clumps3":
        return clumps(N, 1e-3, seed)
    if kind == "clumps5":
        return clumps(N, 1e-5, seed)
    return embedding(kind, N, seed)


# (kind, N, leaf_size (None: N, the root is a leaf), max_depth, angles): what the GPU tests run.  N covers one partly filled wave,
# exactly one wave, one wave and a lane, a workgroup boundary, several workgroups; leaf_size 1, 8, the default (32), one wave of
# points and "everything direct"; N == leaf_size and leaf_size + 1 (the first split); max_depth both ends and 15 / 16 (32 key bits).
ANGLES = (0.0, 0.2, 0.5, 0.8, 1.0)
CASES = (
    [("normal", N, 8, 24, ANGLES) for N in (2, 3, 63, 64, 65, 127, 129)]
    + [("normal", 1000, ls, 24, ANGLES) for ls in (1, 8, 32, 64, None)]
    + [("normal", 5000, 8, 24, (0.2, 0.5, 0.8)), ("normal", 5000, 1, 24, (0.5,))]
    + [("normal", 8, 8, 24, (0.0, 0.5)), ("normal", 9, 8, 24, (0.0, 0.5)), ("normal", 64, 64, 24, (0.0, 1.0)), ("normal", 65, 64, 24, (0.0, 1.0)),
       ("normal", 2, 1, 24, (0.0, 1.0)), ("normal", 129, None, 1, (0.0, 0.5)), ("normal", 32, 32, 24, (0.5,)), ("normal", 33, 32, 24, (0.0, 0.5))]
    + [("normal", 1000, 8, d, (0.0, 0.5, 1.0)) for d in (1, 15, 16)]
    + [("normal", 129, 1, d, (0.0, 1.0)) for d in (1, 15, 16, 24)]
    + [("start", 65, 8, 24, ANGLES), ("start", 1000, 8, 24, (0.0, 0.5)), ("start", 1000, 1, 16, (0.5,))]
    + [("five", 1000, 8, 24, (0.2, 0.8)), ("five", 1000, 1, 24, (0.5,))]
    + [("heavy", 127, 8, 24, ANGLES), ("heavy", 1000, 8, 24, (0.2, 0.8)), ("heavy", 1000, 1, 15, (0.0, 0.5))]
    + [("clusters", 5000, 8, 24, (0.5, 1.0)), ("clusters", 5000, 64, 15, (0.5,))]
    + [("collinear", 129, 8, 24, ANGLES), ("collinear", 1000, 1, 24, (0.5,))]
    + [("dyadic", 1000, ls, d, (0.0, 0.5)) for ls, d in ((1, 24), (8, 16), (8, 2))]
    + [("duplicates", 1000, 1, 24, (0.0, 0.5)), ("duplicates", 64, 1, 24, ANGLES)]
    + [("lone", 65, 8, 24, ANGLES), ("lone", 1000, 8, 24, (0.5,))]
    + [("clumps3", 3000, 8, 24, (0.5,)), ("clumps5", 3000, 8, 24, (0.5,)), ("clumps3", 1000, 1, 24, (0.0, 0.8)), ("clumps3", 3000, 32, 24, (0.2, 0.8))]
)
COINCIDENT = [(N, ls, d) for N in (2, 3, 63, 64, 65, 127, 129, 1000, 5000) for ls, d in ((1, 24), (8, 1), (8, 24), (None, 24))]

_cache = {}


def leaf_of(N, leaf_size):
    return N if leaf_size is None else leaf_size


def case(kind, N, leaf_size, D, angle):
    """(Y, tree, oracle result), computed once per session and read only."""
    ls = leaf_of(N, leaf_size)
    kt = (kind, N, ls, D)
    if kt not in _cache:
        Y = points(kind, N)
        Y.setflags(write=False)
        _cache[kt] = (Y, tree(Y, ls, D))
    Y, tr = _cache[kt]
    ka = kt + (float(angle),)
    if ka not in _cache:
        _cache[ka] = repulsion(Y, ls, D, angle, tr)
    return Y, tr, _cache[ka]


def exact_case(kind, N):
    k = ("exact", kind, N)
    if k not in _cache:
        _cache[k] = exact_repulsion(points(kind, N))
    return _cache[k]


def distinct_cases():
    """(kind, N, leaf_size, D) of CASES, each once."""
    return sorted({(k, N, leaf_of(N, ls), d) for k, N, ls, d, _ in CASES})


# ---------------------------------------------------------------------------------------------- the yardstick: scikit-learn's own error
# || g - g_exact || / || g_exact || of the repulsive gradient, this restatement over scikit-learn 1.7.2's _barnes_hut_tsne.gradient
# (empty P), both against the f64 all-pairs sum: 3000 points, embedding(kind, 3000, seed), D = 24, leaf_size 1 and the default (32),
# angles 0.2, 0.5 and 0.8.  Largest ratio per embedding and seed, measured on the CPU:
#             seed 0    seed 1    seed 2
#   normal    1.086     1.215     1.191
#   five      1.425     1.036     1.613
#   start     0.063     0.081     0.081
# (at leaf_size 32 alone: 1.086, 1.215, 1.191 / 1.374, 1.019, 1.422 / 0.063, 0.081, 0.081; at leaf_size 8: 1.038, 1.187, 1.166 /
# 1.369, 1.024, 1.493 / 0.063, 0.081, 0.080; five's largest is at angle 0.2 and leaf_size 1, where scikit-learn's own error is 7e-4).
# The largest figure of a seed is 1.425, 1.215, 1.613: RATIO_MARGIN is their range, all the margin covers.  The test runs seed 0.
PIN_N, PIN_KINDS, PIN_ANGLES, PIN_LEAVES = 3000, ("normal", "five", "start"), (0.2, 0.5, 0.8), (1, DEFAULT_LEAF)
RATIO_MEASURED = {"normal": (1.086, 1.215, 1.191), "five": (1.425, 1.036, 1.613), "start": (0.063, 0.081, 0.081)}
RATIO_MAX = 1.613
RATIO_MARGIN = 1.613 - 1.215
