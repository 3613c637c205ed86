// t-SNE of the leading PCs (analysis.py:1441-1450: sklearn.manifold.TSNE(n_components, perplexity, angle=theta,
// init=..., max_iter), method="barnes_hut") on the device.  Restated from scikit-learn 1.7's published algorithm:
//   * vcy_tsne_perplexity: _binary_search_perplexity (manifold/_utils.pyx) - one lane per row, the row's neighbours in the
//     caller's order (scikit-learn sorts them by neighbour index), f64 arithmetic on f32 squared distances, its f32
//     constants, at most 100 bisection steps;
//   * vcy_tsne_gradient / vcy_tsne_step: the gradient of _kl_divergence_bh (manifold/_barnes_hut_tsne.pyx:94-242) with the
//     repulsion summed EXACTLY over all pairs (the theta -> 0 limit of the Barnes-Hut tree), and one iteration of
//     _gradient_descent (manifold/_t_sne.py:301-444): gains, momentum, positions.
// Kernels (all deterministic: no atomics, every sum in a fixed order):
//   k_tsne_repulsion<D>  all-pairs repulsion, tiled N^2: a workgroup owns 512 targets (2 per lane) and one contiguous
//                        range of sources (a "split"), streamed through LDS 256 at a time; f32 sums inside a tile, f64 carries
//                        across tiles; per-split, per-target partials of the force and of sum_j w_ij, and per-workgroup
//                        partials of Z.  At dof = 1 a pair costs 8 plain VALU ops + one v_rcp_f32.
//   k_tsne_step<D,STEP>  Z from the partials (every workgroup reduces them in the same order), the attraction over the CSR
//                        rows of P (+ the error terms), the gradient, and with STEP the gains / momentum / position update;
//                        per-workgroup partials of the error and of |grad|^2.
//   k_tsne_stats         KL and |grad|^2 from the partials (one workgroup), at the iterations whose error is asked for.
//   k_tree_*, k_tsne_tree_repulsion    (vcy_tsne_tree_*, D = 2, opt-in) the repulsion by scikit-learn's Barnes-Hut acceptance rule with the
//                        caller's angle on a complete quadtree of fixed depth;
//   k_atree_*, k_tsne_atree_repulsion  (vcy_tsne_atree_*, D = 2, opt-in) the same rule on a quadtree as deep as the points are dense.
// All three fill the same partials, so one tail serves them (tsne_tail: k_tsne_step, k_tsne_stats).  The trees own their build and the
// control flow of their walk, and share: the frame of their keys (TreeFrame, tree_frame, tree_fill_w2), the walk's sums, acceptance, leaf sum
// and stores (TreeAcc, tree_accept, tree_leaf_sweep, tree_walk_store), and on the host TreeTail, tree_check_shared, tree_eval, tree_rep_out.
#include "common.h"
#include <float.h>

// the perplexity search and the update mirror scikit-learn's (separately rounded) numpy / C arithmetic: no implicit
// mul+add fusion; the repulsion writes its fused multiply-adds explicitly
#pragma clang fp contract(off)

namespace vcy {

constexpr int TSNE_TPB = 256;                      // threads per workgroup (every kernel of this file)
constexpr int TSNE_RT = 2;                         // repulsion: targets per lane
constexpr int TSNE_TGT = TSNE_TPB * TSNE_RT;       // repulsion: targets per workgroup
constexpr int TSNE_TILE = 256;                     // repulsion: sources per LDS tile (f32 sums inside, f64 carries across)
constexpr float TSNE_FAR = 1e30f;                  // padding source: d^2 overflows to inf, so w = 0 and the force term is 0 exactly

// ---------------------------------------------------------------- perplexity
// One lane per row.  n_steps[i] = number of bisection steps evaluated when the row met the tolerance, 0 when it used all 100
// without meeting it (NULL: not written).
__global__ __launch_bounds__(TSNE_TPB) void k_tsne_perplexity(const float *__restrict__ sqd, double *__restrict__ P, int *__restrict__ n_steps,
                                                              long long N, int k, float desired_perplexity)
{
    const long long i = (long long)blockIdx.x * TSNE_TPB + threadIdx.x;
    if (i >= N) return;
    const float *d = sqd + i * k;
    double *p = P + i * k;
    const double desired_entropy = log((double)desired_perplexity);
    const double tol = (double)1e-5f, eps = (double)1e-8f;          // PERPLEXITY_TOLERANCE, EPSILON_DBL: f32 constants in _utils.pyx
    double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY;
    int done = 0;
    for (int l = 0; l < 100; ++l) {
        double sum_P = 0.0;
        for (int j = 0; j < k; ++j) {
            const double v = exp(-(double)d[j] * beta);
            p[j] = v;
            sum_P += v;
        }
        if (sum_P == 0.0) sum_P = eps;
        double sum_dP = 0.0;
        for (int j = 0; j < k; ++j) {
            const double v = p[j] / sum_P;
            p[j] = v;
            sum_dP += (double)d[j] * v;
        }
        const double diff = (log(sum_P) + beta * sum_dP) - desired_entropy;
        if (fabs(diff) <= tol) { done = l + 1; break; }
        if (diff > 0.0) {
            beta_min = beta;
            beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
        } else {
            beta_max = beta;
            beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
        }
    }
    if (n_steps) n_steps[i] = done;
}

// ---------------------------------------------------------------- repulsion
// The kernel of the Student-t at dof = max(D - 1, 1): w = (dof / (dof + d^2))^((dof + 1) / 2), and the force weight w^2.
// dof = 1: w = 1 / (1 + d^2); dof = 2: t = 2 / (2 + d^2), w = t^1.5, w^2 = t^3.  The reciprocal is v_rcp_f32
// (__builtin_amdgcn_rcpf): at most 1 ulp from the rounded quotient, exact at 1 and 0.5 (the self term is exactly 1) and
// 0 at +inf (the padding sources).
template <int D> __device__ __forceinline__ void tsne_pair(const float (&t)[D], const float *s, float (&f)[D], float &w)
{
    float dd[D];
#pragma unroll
    for (int a = 0; a < D; ++a) dd[a] = t[a] - s[a];
    if constexpr (D < 3) {
        float d1 = 1.0f;
#pragma unroll
        for (int a = 0; a < D; ++a) d1 = fmaf(dd[a], dd[a], d1);
        const float q = __builtin_amdgcn_rcpf(d1);
        const float q2 = q * q;
#pragma unroll
        for (int a = 0; a < D; ++a) f[a] = fmaf(q2, dd[a], f[a]);
        w += q;
    } else {
        float d2 = 2.0f;
#pragma unroll
        for (int a = 0; a < D; ++a) d2 = fmaf(dd[a], dd[a], d2);
        const float q = 2.0f * __builtin_amdgcn_rcpf(d2);
        const float q3 = q * q * q;
#pragma unroll
        for (int a = 0; a < D; ++a) f[a] = fmaf(q3, dd[a], f[a]);
        w += q * __builtin_sqrtf(q);
    }
}

// grid (target blocks, splits).  part: (S, D + 1, N) f64 - per split the force components and sum_j w_ij (self excluded) of
// every target; zpart (S * target blocks): the workgroup's sum of its targets' sum_j w_ij.
template <int D>
__global__ __launch_bounds__(TSNE_TPB) void k_tsne_repulsion(const float *__restrict__ Y, double *__restrict__ part, double *__restrict__ zpart,
                                                             int N, int src_per_split)
{
    __shared__ float s_y[TSNE_TILE * D];
    __shared__ double s_red[TSNE_TPB / VCY_WAVE];
    const int tid = threadIdx.x, split = blockIdx.y;
    const int s0 = split * src_per_split, s1 = min(N, s0 + src_per_split);
    float ty[TSNE_RT][D];
    int ti[TSNE_RT];
    double F[TSNE_RT][D], W[TSNE_RT];
#pragma unroll
    for (int r = 0; r < TSNE_RT; ++r) {
        ti[r] = blockIdx.x * TSNE_TGT + r * TSNE_TPB + tid;
#pragma unroll
        for (int a = 0; a < D; ++a) { ty[r][a] = ti[r] < N ? Y[(size_t)ti[r] * D + a] : 0.0f; F[r][a] = 0.0; }
        W[r] = 0.0;
    }
    for (int base = s0; base < s1; base += TSNE_TILE) {
        __syncthreads();
        for (int u = tid; u < TSNE_TILE * D; u += TSNE_TPB) s_y[u] = base + u / D < s1 ? Y[(size_t)base * D + u] : TSNE_FAR;
        __syncthreads();
        float f[TSNE_RT][D], w[TSNE_RT];
#pragma unroll
        for (int r = 0; r < TSNE_RT; ++r) {
#pragma unroll
            for (int a = 0; a < D; ++a) f[r][a] = 0.0f;
            w[r] = 0.0f;
        }
#pragma unroll 8
        for (int u = 0; u < TSNE_TILE; ++u) {
            float s[D];
#pragma unroll
            for (int a = 0; a < D; ++a) s[a] = s_y[u * D + a];                 // same address in every lane: LDS broadcast
#pragma unroll
            for (int r = 0; r < TSNE_RT; ++r) tsne_pair<D>(ty[r], s, f[r], w[r]);
        }
#pragma unroll
        for (int r = 0; r < TSNE_RT; ++r) {
#pragma unroll
            for (int a = 0; a < D; ++a) F[r][a] += (double)f[r][a];
            W[r] += (double)w[r];
        }
    }
    double zsum = 0.0;
#pragma unroll
    for (int r = 0; r < TSNE_RT; ++r) {
        if (ti[r] >= N) continue;
        if (ti[r] >= s0 && ti[r] < s1) W[r] -= 1.0;                              // the self term: w_ii = 1 exactly, force 0
#pragma unroll
        for (int a = 0; a < D; ++a) part[((size_t)split * (D + 1) + a) * N + ti[r]] = F[r][a];
        part[((size_t)split * (D + 1) + D) * N + ti[r]] = W[r];
        zsum += W[r];
    }
    zsum = block_sum(zsum, s_red);
    if (tid == 0) zpart[(size_t)split * gridDim.x + blockIdx.x] = zsum;
}

// sum of v[0..n) in a fixed order, valid in every thread of a TSNE_TPB workgroup (the same bits in every workgroup)
__device__ __forceinline__ double tsne_fixed_sum(const double *__restrict__ v, int n, double *s_red)
{
    double acc = 0.0;
    for (int t = threadIdx.x; t < n; t += TSNE_TPB) acc += v[t];
    return block_sum(acc, s_red);
}

// ---------------------------------------------------------------- attraction, gradient, update
// One lane per row i.  grad_i = c (attr_i - rep_i / Z) rounded to f32 as scikit-learn's tot_force and grad *= c are;
// attr_i = sum_k p_k q_ik (y_i - y_j) over the stored entries of row i (f32 terms, f64 sum).
// STEP: _gradient_descent's update for the row's D entries (update f64, gains f32, positions f32 rounded from f64).
template <int D, bool STEP>
__global__ __launch_bounds__(TSNE_TPB) void k_tsne_step(const float *__restrict__ Y, float *__restrict__ Yout, const int64_t *__restrict__ indptr,
                                                        const int32_t *__restrict__ indices, const float *__restrict__ pval,
                                                        const double *__restrict__ part, const double *__restrict__ zpart, int nz, int S,
                                                        float *__restrict__ grad, double *__restrict__ update, float *__restrict__ gains,
                                                        double *__restrict__ blk, double *__restrict__ stats, int N, int compute_error,
                                                        double momentum, double lr, float min_gain)
{
    __shared__ double s_red[TSNE_TPB / VCY_WAVE];
    constexpr int dof = D > 1 ? D - 1 : 1;
    constexpr float fdof = (float)dof, c = 2.0f * (dof + 1.0f) / dof;
    // sum_Q = max(sum_Q, FLOAT64_EPS) - a float constant there
    const double Z = fmax(tsne_fixed_sum(zpart, nz, s_red), (double)(float)DBL_EPSILON);
    const int i = blockIdx.x * TSNE_TPB + threadIdx.x;
    double err = 0.0, g2 = 0.0;
    if (i < N) {
        float yi[D];
        double attr[D], rep[D];
#pragma unroll
        for (int a = 0; a < D; ++a) { yi[a] = Y[(size_t)i * D + a]; attr[a] = 0.0; rep[a] = 0.0; }
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int a = 0; a < D; ++a) rep[a] += part[((size_t)s * (D + 1) + a) * N + i];
        }
        const float tiny = FLT_MIN;
        for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
            const int j = indices[e];
            const float p = pval[e];
            float dd[D], d2 = 0.0f;
#pragma unroll
            for (int a = 0; a < D; ++a) { dd[a] = yi[a] - Y[(size_t)j * D + a]; d2 += dd[a] * dd[a]; }
            float q = fdof / (fdof + d2);
            if (dof != 1) q = q * __builtin_sqrtf(q);
            const float pq = p * q;
#pragma unroll
            for (int a = 0; a < D; ++a) attr[a] += (double)(pq * dd[a]);
            if (compute_error) {
                const float qz = (float)((double)q / Z);
                err += (double)p * log((double)fmaxf(p, tiny) / (double)fmaxf(qz, tiny));
            }
        }
#pragma unroll
        for (int a = 0; a < D; ++a) {
            float g = (float)(attr[a] - rep[a] / Z);
            g = g * c;
            if constexpr (STEP) {
                const size_t o = (size_t)i * D + a;
                double u = update[o];
                float gain = gains[o];
                gain = (u * (double)g < 0.0) ? gain + 0.2f : gain * 0.8f;
                gain = fmaxf(gain, min_gain);
                g = g * gain;
                u = momentum * u - lr * (double)g;
                update[o] = u;
                gains[o] = gain;
                Yout[o] = (float)((double)yi[a] + u);
            } else {
                grad[(size_t)i * D + a] = g;
            }
            g2 += (double)g * (double)g;
        }
    }
    err = block_sum(err, s_red);
    g2 = block_sum(g2, s_red);
    if (threadIdx.x == 0) { blk[blockIdx.x] = err; blk[gridDim.x + blockIdx.x] = g2; }
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[0] = Z;
}

// stats[1] = KL (sum of the error terms), stats[2] = |grad|^2 (after the gains when stepping)
__global__ __launch_bounds__(TSNE_TPB) void k_tsne_stats(const double *__restrict__ blk, int nb, double *__restrict__ stats)
{
    __shared__ double s_red[TSNE_TPB / VCY_WAVE];
    const double err = tsne_fixed_sum(blk, nb, s_red);
    const double g2 = tsne_fixed_sum(blk + nb, nb, s_red);
    if (threadIdx.x == 0) { stats[1] = err; stats[2] = g2; }
}

// ---------------------------------------------------------------- host side
// Source splits of the repulsion: enough workgroups to fill the chip (~2048) but at least 1024 sources per split.
struct TsnePlan {
    int tb, S, per, nb;
    size_t part_off, zpart_off, blk_off, bytes;
};
static TsnePlan tsne_plan(int64_t N, int D)
{
    TsnePlan p;
    p.tb = (int)((N + TSNE_TGT - 1) / TSNE_TGT);
    int64_t S = (2048 + p.tb - 1) / p.tb;
    const int64_t smax = (N + 1023) / 1024;
    if (S > smax) S = smax;
    if (S < 1) S = 1;
    p.per = (int)(((N + S - 1) / S + TSNE_TILE - 1) / TSNE_TILE * TSNE_TILE);
    p.S = (int)((N + p.per - 1) / p.per);
    p.nb = (int)((N + TSNE_TPB - 1) / TSNE_TPB);
    p.part_off = 0;
    p.zpart_off = p.part_off + sizeof(double) * (size_t)p.S * (D + 1) * (size_t)N;
    p.blk_off = p.zpart_off + sizeof(double) * (size_t)p.S * p.tb;
    p.bytes = p.blk_off + sizeof(double) * 2 * (size_t)p.nb;
    return p;
}

// What a gradient (step false: grad is written) or an iteration (step true: Yout, update, gains) is asked for, whichever repulsion it uses.
struct TsneArgs {
    const float *Y;
    float *Yout;
    const int64_t *indptr; const int32_t *indices; const float *pval;      // P as CSR
    float *grad;
    double *update; float *gains;
    double *stats;
    int compute_error;
    double momentum, lr, min_gain;
    bool step;
};

// null pointers and aliasing, before anything else is looked at; `rest`: the entry point's other pointers are all there
static int tsne_args_check(const TsneArgs &a, bool rest, const char *who)
{
    const bool out = a.step ? a.Yout && a.update && a.gains : a.grad != nullptr;
    if (!(a.Y && a.indptr && a.indices && a.pval && a.stats && out && rest)) return fail(VCY_ERR_INVALID, "%s: null pointer", who);
    if (a.step && a.Y == a.Yout) return fail(VCY_ERR_INVALID, "%s: Y_out must not alias Y (the attraction reads every row's old position)", who);
    return VCY_OK;
}

// the tail of every evaluation, on the repulsion's partials (S splits of part, nz entries of zpart)
template <int D>
static int tsne_tail(const TsneArgs &a, const double *part, const double *zpart, int nz, int S, double *blk, int nb, int N, hipStream_t s)
{
    const auto step = a.step ? k_tsne_step<D, true> : k_tsne_step<D, false>;
    hipLaunchKernelGGL(step, dim3(nb), dim3(TSNE_TPB), 0, s, a.Y, a.Yout, a.indptr, a.indices, a.pval, part, zpart, nz, S, a.grad, a.update,
                       a.gains, blk, a.stats, N, a.compute_error, a.momentum, a.lr, (float)a.min_gain);
    VCY_LAUNCH_CHECK();
    if (a.compute_error) {
        hipLaunchKernelGGL(k_tsne_stats, dim3(1), dim3(TSNE_TPB), 0, s, blk, nb, a.stats);
        VCY_LAUNCH_CHECK();
    }
    return VCY_OK;
}

template <int D> static int tsne_launch(const TsneArgs &a, void *workspace, int64_t N, hipStream_t s)
{
    const TsnePlan p = tsne_plan(N, D);
    char *w = (char *)workspace;
    double *part = (double *)(w + p.part_off), *zpart = (double *)(w + p.zpart_off), *blk = (double *)(w + p.blk_off);
    hipLaunchKernelGGL(k_tsne_repulsion<D>, dim3(p.tb, p.S), dim3(TSNE_TPB), 0, s, a.Y, part, zpart, (int)N, p.per);
    VCY_LAUNCH_CHECK();
    return tsne_tail<D>(a, part, zpart, p.S * p.tb, p.S, blk, p.nb, (int)N, s);
}

static int tsne_entry(const TsneArgs &a, void *workspace, int64_t N, int D, const char *who, hipStream_t s)
{
    const int rc = tsne_args_check(a, workspace != nullptr, who);
    if (rc != VCY_OK) return rc;
    if (!(N >= 2 && N < (1ll << 30))) return fail(VCY_ERR_INVALID, "%s: N out of range", who);
    switch (D) {
    case 1: return tsne_launch<1>(a, workspace, N, s);
    case 2: return tsne_launch<2>(a, workspace, N, s);
    case 3: return tsne_launch<3>(a, workspace, N, s);
    default: return fail(VCY_ERR_INVALID, "%s: n_components must be 1, 2 or 3", who);
    }
}

// ---------------------------------------------------------------- tree repulsion (D = 2)
// scikit-learn's Barnes-Hut acceptance rule (max_width^2 / dist^2 < angle^2, per target) on a complete quadtree of `depth`
// levels below the root, rebuilt at every evaluation; DESIGN.md section 9 has the contract.  Per evaluation:
//   k_tree_box, k_tree_keys   the bounding box (min / max: order-free), and every point's Morton key of its leaf cell
//                             (f64, separately rounded; clamped before the integer conversion)
//   [the caller sorts the keys: order = stable argsort, plumbing]
//   k_tree_start, k_tree_gather  start[cell] = first sorted position of the cell (binary search), positions in sorted order
//   k_tree_up<LEAF>           f64 sums of the leaf cells (points in sorted order) and of 4 levels above them per launch
//                             (children 0, 1, 2, 3 in that order): no atomics
//   k_tree_finalize           node record {count, com.x, com.y} in place of the f64 sums (count comes from start[])
//   k_tsne_tree_repulsion     one wave per 64 consecutive sorted targets, one wave-uniform depth-first walk of the implicit tree
// Workspace: TreeHead (128 bytes) | box partials | nodes 16 bytes x (4^(depth+1) - 1) / 3, level l at (4^l - 1) / 3 in Morton
// order | start int32 x (4^depth + 1) | sorted positions | part (3, N) f64 | zpart | blk: what k_tsne_step reads.
constexpr int TREE_MAX_DEPTH = 11;
constexpr int TREE_BOX_BLOCKS = 256;               // workgroups of the min / max pass
constexpr int TREE_RUN = 256;                      // f32 terms added between two f64 carries (as TSNE_TILE in the exact kernel)

struct TreeFrame {                                 // the frame either tree's keys are taken in
    double lo[2], side, scale;                     // box corner, larger extent, 2^depth / side (0 when side is 0 or not finite)
};
struct TreeHead {
    TreeFrame fr;
    float w2[TREE_MAX_DEPTH + 1];                  // f32((side 2^-l)^2)
    float pad[12];
};
static_assert(sizeof(TreeHead) == 128, "TreeHead");

static size_t tree_align(size_t b) { return (b + 127) / 128 * 128; }

// What the workspace of either tree ends in, from the first byte after the tree's own regions: sorted positions | part (3, N) f64 |
// zpart | blk, and the grids that go with them (nbx: workgroups of the box pass, tb: of the walk = entries of zpart, nb: of k_tsne_step).
struct TreeTail {
    int nbx, tb, nb;
    size_t ysort_off, part_off, zpart_off, blk_off, bytes;
};
static TreeTail tree_tail(int64_t N, size_t first)
{
    TreeTail t;
    t.tb = t.nb = (int)((N + TSNE_TPB - 1) / TSNE_TPB);
    t.nbx = t.nb < TREE_BOX_BLOCKS ? t.nb : TREE_BOX_BLOCKS;
    t.ysort_off = first;
    t.part_off = t.ysort_off + tree_align(sizeof(float2) * (size_t)N);
    t.zpart_off = t.part_off + tree_align(sizeof(double) * 3 * (size_t)N);
    t.blk_off = t.zpart_off + tree_align(sizeof(double) * (size_t)t.tb);
    t.bytes = t.blk_off + tree_align(sizeof(double) * 2 * (size_t)t.nb);
    return t;
}

struct TreePlan {
    int L;
    int64_t cells, nodes;
    size_t boxp_off, node_off, start_off;
    TreeTail t;
};
static TreePlan tree_plan(int64_t N, int L)
{
    TreePlan p;
    p.L = L;
    p.cells = 1ll << (2 * L);
    p.nodes = ((1ll << (2 * L + 2)) - 1) / 3;
    p.boxp_off = sizeof(TreeHead);
    p.node_off = p.boxp_off + tree_align(sizeof(float4) * TREE_BOX_BLOCKS);
    p.start_off = p.node_off + tree_align(16 * (size_t)p.nodes);
    p.t = tree_tail(N, p.start_off + tree_align(sizeof(int) * (size_t)(p.cells + 1)));
    return p;
}

__device__ __forceinline__ unsigned tree_level_offset(int l) { return 0x55555555u & ((1u << (2 * l)) - 1u); }   // (4^l - 1) / 3
__device__ __forceinline__ unsigned tree_spread(unsigned x)
{
    x &= 0xffffu;
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    return (x | (x << 1)) & 0x55555555u;
}

// (min x, min y, max x, max y) over the workgroup, valid in every thread; fminf / fmaxf drop a NaN operand
__device__ __forceinline__ float4 tree_block_box(float4 b, float4 *s_box)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        b.x = fminf(b.x, __shfl_xor(b.x, off, 64));
        b.y = fminf(b.y, __shfl_xor(b.y, off, 64));
        b.z = fmaxf(b.z, __shfl_xor(b.z, off, 64));
        b.w = fmaxf(b.w, __shfl_xor(b.w, off, 64));
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_box[threadIdx.x >> 6] = b;
    __syncthreads();
    b = s_box[0];
    for (int i = 1; i < TSNE_TPB / VCY_WAVE; ++i) {
        b.x = fminf(b.x, s_box[i].x);
        b.y = fminf(b.y, s_box[i].y);
        b.z = fmaxf(b.z, s_box[i].z);
        b.w = fmaxf(b.w, s_box[i].w);
    }
    return b;
}

__global__ __launch_bounds__(TSNE_TPB) void k_tree_box(const float2 *__restrict__ Y, float4 *__restrict__ boxp, int N)
{
    __shared__ float4 s_box[TSNE_TPB / VCY_WAVE];
    float4 b = make_float4(INFINITY, INFINITY, -INFINITY, -INFINITY);
    for (int i = blockIdx.x * TSNE_TPB + threadIdx.x; i < N; i += gridDim.x * TSNE_TPB) {
        const float2 y = Y[i];
        b.x = fminf(b.x, y.x);
        b.y = fminf(b.y, y.y);
        b.z = fmaxf(b.z, y.x);
        b.w = fmaxf(b.w, y.y);
    }
    b = tree_block_box(b, s_box);
    if (threadIdx.x == 0) boxp[blockIdx.x] = b;
}

// cell coordinate min(2^L - 1, floor((y - lo) scale)), clamped before the conversion; NaN and negative products give 0
__device__ __forceinline__ unsigned tree_cell(float y, double lo, double scale, int L)
{
    const double t = __dmul_rn(__dsub_rn((double)y, lo), scale);
    const double top = (double)((1 << L) - 1);
    if (!(t >= 0.0)) return 0u;
    return t >= top ? (unsigned)((1 << L) - 1) : (unsigned)(int)floor(t);
}

// the frame of `bits` key bits per axis from the box partials: every workgroup reduces them to the same box
__device__ __forceinline__ TreeFrame tree_frame(const float4 *__restrict__ boxp, int nbx, int bits, float4 *s_box)
{
    float4 b = (int)threadIdx.x < nbx ? boxp[threadIdx.x] : make_float4(INFINITY, INFINITY, -INFINITY, -INFINITY);
    b = tree_block_box(b, s_box);
    TreeFrame f;
    f.lo[0] = (double)b.x; f.lo[1] = (double)b.y;
    f.side = fmax(__dsub_rn((double)b.z, f.lo[0]), __dsub_rn((double)b.w, f.lo[1]));
    f.scale = (f.side > 0.0 && f.side < INFINITY) ? __ddiv_rn((double)(1 << bits), f.side) : 0.0;
    return f;
}

// w2[l] = f32((side 2^-l)^2), l = 0 .. levels
__device__ __forceinline__ void tree_fill_w2(float *__restrict__ w2, double side, int levels)
{
    for (int l = 0; l <= levels; ++l) {
        const double s = __dmul_rn(side, 1.0 / (double)(1 << l));
        w2[l] = (float)__dmul_rn(s, s);
    }
}

__global__ __launch_bounds__(TSNE_TPB) void k_tree_keys(const float2 *__restrict__ Y, const float4 *__restrict__ boxp, int nbx,
                                                        TreeHead *__restrict__ head, int32_t *__restrict__ keys, int N, int L)
{
    __shared__ float4 s_box[TSNE_TPB / VCY_WAVE];
    const TreeFrame f = tree_frame(boxp, nbx, L, s_box);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        head->fr = f;
        tree_fill_w2(head->w2, f.side, TREE_MAX_DEPTH);
        for (int l = 0; l < 12; ++l) head->pad[l] = 0.0f;
    }
    const int i = blockIdx.x * TSNE_TPB + threadIdx.x;
    if (i < N) {
        const float2 y = Y[i];
        keys[i] = (int32_t)(tree_spread(tree_cell(y.x, f.lo[0], f.scale, L)) | (tree_spread(tree_cell(y.y, f.lo[1], f.scale, L)) << 1));
    }
}

// start[c] = number of sorted keys below c, c = 0 .. cells: in [0, N] whatever the keys hold
__global__ __launch_bounds__(TSNE_TPB) void k_tree_start(const int32_t *__restrict__ skeys, int *__restrict__ start, int N, unsigned cells)
{
    const unsigned c = blockIdx.x * TSNE_TPB + threadIdx.x;
    if (c > cells) return;
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((long long)skeys[mid] < (long long)c) lo = mid + 1; else hi = mid;
    }
    start[c] = lo;
}

__global__ __launch_bounds__(TSNE_TPB) void k_tree_gather(const float2 *__restrict__ Y, const int64_t *__restrict__ order, float2 *__restrict__ ysort, int N)
{
    const int i = blockIdx.x * TSNE_TPB + threadIdx.x;
    if (i >= N) return;
    const int64_t o = order[i];
    ysort[i] = Y[(uint64_t)o < (uint64_t)N ? o : 0];
}

// Levels l0, l0 - 1, .., l0 - 4 (down to the root): thread t of a workgroup owns node 256 block + t of level l0, then the
// first 64, 16, 4, 1 threads own the workgroup's nodes one, two, three, four levels up.
template <bool LEAF>
__global__ __launch_bounds__(TSNE_TPB) void k_tree_up(double2 *nsum, const int *__restrict__ start, const float2 *__restrict__ ysort, int N, int l0)
{
    const unsigned base = blockIdx.x * TSNE_TPB, m = base + threadIdx.x;
    if (m < (1u << (2 * l0))) {
        double sx = 0.0, sy = 0.0;
        if constexpr (LEAF) {
            const int b = max(start[m], 0), e = min(start[m + 1], N);
#pragma unroll 8
            for (int j = b; j < e; ++j) {                              // the loads run ahead, the sums stay in order
                const float2 y = ysort[j];
                sx += (double)y.x;
                sy += (double)y.y;
            }
        } else {
            const double2 *ch = nsum + tree_level_offset(l0 + 1) + 4u * m;
            for (int c = 0; c < 4; ++c) { sx += ch[c].x; sy += ch[c].y; }
        }
        nsum[tree_level_offset(l0) + m] = make_double2(sx, sy);
    }
    for (int s = 1; s <= 4 && l0 - s >= 0; ++s) {
        __syncthreads();                                               // the children were written by this workgroup
        const int l = l0 - s;
        const unsigned mm = (base >> (2 * s)) + threadIdx.x;
        if (threadIdx.x < (unsigned)(TSNE_TPB >> (2 * s)) && mm < (1u << (2 * l))) {
            const double2 *ch = nsum + tree_level_offset(l + 1) + 4u * mm;
            double sx = 0.0, sy = 0.0;
            for (int c = 0; c < 4; ++c) { sx += ch[c].x; sy += ch[c].y; }
            nsum[tree_level_offset(l) + mm] = make_double2(sx, sy);
        }
    }
}

// in place: {sum x, sum y} f64 -> {count, com.x, com.y, 0}; an empty node (or a range that runs backwards) gets count 0, com 0
__global__ __launch_bounds__(TSNE_TPB) void k_tree_finalize(void *nodes, const int *__restrict__ start, int L, unsigned nn)
{
    const unsigned idx = blockIdx.x * TSNE_TPB + threadIdx.x;
    if (idx >= nn) return;
    int l = 0;
    while (l < L && tree_level_offset(l + 1) <= idx) ++l;
    const unsigned m = idx - tree_level_offset(l);
    const int sh = 2 * (L - l);
    const int cnt = start[(m + 1u) << sh] - start[m << sh];
    const double2 s = ((const double2 *)nodes)[idx];
    int4 r = make_int4(0, 0, 0, 0);
    if (cnt > 0) {
        r.x = cnt;
        r.y = __float_as_int((float)__ddiv_rn(s.x, (double)cnt));
        r.z = __float_as_int((float)__ddiv_rn(s.y, (double)cnt));
    }
    ((int4 *)nodes)[idx] = r;
}

// What the walks of both trees share.  A lane's sums: f32 of at most TREE_RUN terms (run counts them), carried into f64; the visit counts
struct TreeAcc {
    double F[2] = {0.0, 0.0}, W = 0.0;
    float f[2] = {0.0f, 0.0f}, w = 0.0f;
    int run = 0, n_acc = 0, n_dir = 0;
    __device__ __forceinline__ void carry()
    {
        F[0] += (double)f[0]; F[1] += (double)f[1]; W += (double)w;
        f[0] = f[1] = w = 0.0f;
        run = 0;
    }
};

// scikit-learn's rule for target t and a node of cnt points around (cx, cy) of squared width *w2 (read by active lanes only): the lane
// takes the node when *w2 < th2 d^2 (separately rounded), and then adds the pair arithmetic of tsne_pair<2> with a multiplicity
__device__ __forceinline__ bool tree_accept(TreeAcc &a, const float (&t)[2], float cx, float cy, int cnt, const float *w2, float th2, bool active)
{
    const float dx = __fsub_rn(t[0], cx), dy = __fsub_rn(t[1], cy);
    const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
    const bool take = active && *w2 < __fmul_rn(th2, d2);
    if (take) {
        const float q = __builtin_amdgcn_rcpf(fmaf(dy, dy, fmaf(dx, dx, 1.0f)));
        const float cq = (float)cnt * q, cq2 = cq * q;
        a.f[0] = fmaf(cq2, dx, a.f[0]);
        a.f[1] = fmaf(cq2, dy, a.f[1]);
        a.w += cq;
        ++a.n_acc;
    }
    return take;
}

// The points [b, e) of the sorted order one by one, for the lanes with `open` (p: the lane's own position, left out): 64 points per
// load, one per lane (every lane of the wave is here: the caller's branch is uniform), then broadcast one by one.
__device__ __forceinline__ void tree_leaf_sweep(TreeAcc &a, const float (&t)[2], const float2 *__restrict__ ysort, int b, int e, int p, bool open)
{
    for (int c0 = b; c0 < e; c0 += VCY_WAVE) {
        const int n = min(e - c0, VCY_WAVE), mine = c0 + (int)(threadIdx.x & 63);
        if (a.run + n > TREE_RUN) a.carry();
        const float2 sp = mine < e ? ysort[mine] : make_float2(0.0f, 0.0f);
        for (int u = 0; u < n; ++u) {
            const float s[2] = {readlane_t(sp.x, u), readlane_t(sp.y, u)};
            if (open && c0 + u != p) tsne_pair<2>(t, s, a.f, a.w);
        }
        a.run += n;
    }
    if (open && e > b) a.n_dir += (e - b) - (p >= b && p < e ? 1 : 0);
}

// the last carry, then the lane's sums at its point's own index (part), its visit counts, and the workgroup's share of Z (zpart)
template <bool VISITS>
__device__ __forceinline__ void tree_walk_store(TreeAcc &a, bool valid, int p, const int64_t *__restrict__ order, double *__restrict__ part,
                                                double *__restrict__ zpart, int32_t *__restrict__ visits, int N, double *s_red)
{
    a.carry();
    if (valid) {
        const int64_t o64 = order[p];
        const size_t o = (uint64_t)o64 < (uint64_t)N ? (size_t)o64 : 0;
        part[o] = a.F[0];
        part[(size_t)N + o] = a.F[1];
        part[2 * (size_t)N + o] = a.W;
        if constexpr (VISITS) { visits[2 * o] = a.n_acc; visits[2 * o + 1] = a.n_dir; }
    }
    const double zsum = block_sum(valid ? a.W : 0.0, s_red);
    if (threadIdx.x == 0) zpart[blockIdx.x] = zsum;
}

// One wave per 64 consecutive targets of the sorted order.  (l, m) is wave-uniform and moves in depth-first order: down to
// (l + 1, 4 m) while any lane wants to open, else on to the next sibling, climbing while m & 3 == 3.  acc is the level at
// which the lane accepted an ancestor of the current node (64: none, -1: no target): the lane sits out until the walk is back
// at that level or above.  The node index only grows, and the loop carries the pyramid's node count as its trip bound.
template <bool VISITS>
__global__ __launch_bounds__(TSNE_TPB) void k_tsne_tree_repulsion(const int4 *__restrict__ node, const int *__restrict__ start,
                                                                  const float2 *__restrict__ ysort, const int64_t *__restrict__ order,
                                                                  const TreeHead *__restrict__ head, double *__restrict__ part,
                                                                  double *__restrict__ zpart, int32_t *__restrict__ visits, int N, int L,
                                                                  float th2)
{
    __shared__ double s_red[TSNE_TPB / VCY_WAVE];
    const int p = blockIdx.x * TSNE_TPB + threadIdx.x;
    const bool valid = p < N;
    const float2 tp = valid ? ysort[p] : make_float2(0.0f, 0.0f);
    const float t[2] = {tp.x, tp.y};
    int acc = valid ? 64 : -1;
    TreeAcc a;
    const unsigned nn = tree_level_offset(L + 1);
    int l = 0;
    unsigned m = 0;
    for (unsigned trip = 0; trip < nn; ++trip) {
        const int4 nd = node[tree_level_offset(l) + m];
        const int cnt = __builtin_amdgcn_readfirstlane(nd.x);
        bool descend = false;
        if (cnt > 0) {
            if (acc >= l) acc = 64;
            const bool active = acc == 64;
            if (a.run + 1 > TREE_RUN) a.carry();
            const bool take = tree_accept(a, t, __int_as_float(nd.y), __int_as_float(nd.z), cnt, head->w2 + l, th2, active);
            if (take) acc = l;
            ++a.run;
            const bool open = active && !take;
            const bool any_open = __ballot(open) != 0ull;
            if (l < L) {
                descend = any_open;
            } else if (any_open) {                                     // a leaf somebody does not accept: its points one by one
                const int b = max(__builtin_amdgcn_readfirstlane(start[m]), 0), e = min(__builtin_amdgcn_readfirstlane(start[m + 1]), N);
                tree_leaf_sweep(a, t, ysort, b, e, p, open);
            }
        }
        if (descend) {
            ++l;
            m <<= 2;
        } else {
            while (l > 0 && (m & 3u) == 3u) { m >>= 2; --l; }
            if (l == 0) break;
            ++m;
        }
    }
    tree_walk_store<VISITS>(a, valid, p, order, part, zpart, visits, N, s_red);
}

// rep (N, 3) = force x, y and W of every point from part (3, N); Z = the sum of zpart in k_tsne_step's order
__global__ __launch_bounds__(TSNE_TPB) void k_tree_rep_out(const double *__restrict__ part, const double *__restrict__ zpart, int nz,
                                                           double *__restrict__ rep, double *__restrict__ Z, int N)
{
    __shared__ double s_red[TSNE_TPB / VCY_WAVE];
    if (blockIdx.x == 0) {
        const double z = tsne_fixed_sum(zpart, nz, s_red);
        if (threadIdx.x == 0) Z[0] = z;
    }
    const int i = blockIdx.x * TSNE_TPB + threadIdx.x;
    if (i < N)
        for (int a = 0; a < 3; ++a) rep[(size_t)i * 3 + a] = part[(size_t)a * N + i];
}

// what both trees are refused for alike; each adds the checks of its own parameters
static int tree_check_shared(int64_t N, int n_components, double angle, const char *who)
{
    if (n_components != 2) return fail(VCY_ERR_UNSUPPORTED, "%s: the tree repulsion covers n_components == 2 only", who);
    if (!(N >= 2 && N < (1ll << 30))) return fail(VCY_ERR_INVALID, "%s: N out of range", who);
    if (!(angle >= 0.0 && angle <= 1.0)) return fail(VCY_ERR_INVALID, "%s: angle must be in [0, 1]", who);
    return VCY_OK;
}

// the end of either tree's _repulsion entry point: rep and Z from the partials its walk left in the workspace
static int tree_rep_out(const TreeTail &t, void *workspace, double *rep, double *Z, int64_t N, hipStream_t s)
{
    const char *w = (const char *)workspace;
    hipLaunchKernelGGL(k_tree_rep_out, dim3(t.nb), dim3(TSNE_TPB), 0, s, (const double *)(w + t.part_off), (const double *)(w + t.zpart_off), t.tb,
                       rep, Z, (int)N);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

// build + traversal: part, zpart of the workspace are what k_tsne_step<2, .> reads with one split
static int tree_repulsion_launch(const float *Y, const int64_t *order, const int32_t *skeys, int32_t *visits, void *workspace, const TreePlan &p,
                                 int64_t N, double angle, hipStream_t s)
{
    char *w = (char *)workspace;
    const int n = (int)N, L = p.L;
    int *start = (int *)(w + p.start_off);
    float2 *ysort = (float2 *)(w + p.t.ysort_off);
    void *nodes = w + p.node_off;
    hipLaunchKernelGGL(k_tree_start, dim3((unsigned)((p.cells + 1 + TSNE_TPB - 1) / TSNE_TPB)), dim3(TSNE_TPB), 0, s, skeys, start, n, (unsigned)p.cells);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tree_gather, dim3(p.t.nb), dim3(TSNE_TPB), 0, s, (const float2 *)Y, order, ysort, n);
    VCY_LAUNCH_CHECK();
    for (int l0 = L; l0 >= 0; l0 -= 5) {
        const unsigned g = (unsigned)(((1ll << (2 * l0)) + TSNE_TPB - 1) / TSNE_TPB);
        const auto up = l0 == L ? k_tree_up<true> : k_tree_up<false>;
        hipLaunchKernelGGL(up, dim3(g), dim3(TSNE_TPB), 0, s, (double2 *)nodes, start, ysort, n, l0);
        VCY_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_tree_finalize, dim3((unsigned)((p.nodes + TSNE_TPB - 1) / TSNE_TPB)), dim3(TSNE_TPB), 0, s, nodes, start, L, (unsigned)p.nodes);
    VCY_LAUNCH_CHECK();
    const float th2 = (float)(angle * angle);
    double *part = (double *)(w + p.t.part_off), *zpart = (double *)(w + p.t.zpart_off);
    const auto walk = visits ? k_tsne_tree_repulsion<true> : k_tsne_tree_repulsion<false>;
    hipLaunchKernelGGL(walk, dim3(p.t.tb), dim3(TSNE_TPB), 0, s, (const int4 *)nodes, start, ysort, order, (const TreeHead *)w, part, zpart, visits, n, L, th2);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

static int tree_check(int64_t N, int n_components, int depth, double angle, const char *who)
{
    const int rc = tree_check_shared(N, n_components, angle, who);
    if (rc != VCY_OK) return rc;
    if (depth < 1 || depth > TREE_MAX_DEPTH) return fail(VCY_ERR_INVALID, "%s: depth must be 1 .. 11", who);
    return VCY_OK;
}

// ---------------------------------------------------------------- adaptive tree repulsion (D = 2, opt-in)
// The same box, acceptance rule and pair arithmetic on a quadtree whose depth follows the density (vcy_tsne_atree_*; DESIGN.md
// section 9): int64 Morton keys of `depth` (1 .. 24) bits per axis; a node of level l with n points is a leaf iff n <= leaf_size or
// l == depth, otherwise its children are its non-empty level-(l + 1) cells; nodes in depth-first preorder, each with `skip` = the
// first node after its subtree.  Built from the sorted keys without a launch per level:
//   k_atree_keys    the box, the head and every point's key
//   [the caller sorts the keys]
//   k_atree_flag    position i starts the nodes of levels l0(i) .. l1(i): l0 = first level at which the key prefix differs from
//                   position i - 1, l1 = min(depth, 1 + deepest level whose cell around i holds > leaf_size points) (a binary search
//                   over levels, each probe two binary searches in the keys); also the positions in sorted order
//   k_atree_scan1 / k_atree_scan2   exclusive scan of the per-position node counts: preorder = order by (start position, level)
//   k_atree_emit    node records {start, count, level, skip, com, leaf}; skip = the number of the first node starting at the node's end
//   k_atree_com     per level, deepest first: f64 sums (a leaf's points in sorted order, an internal node's children in child order)
//                   and com = f32(sum / count): no atomics
//   k_tsne_atree_repulsion   one wave per 64 consecutive sorted targets, the node number wave-uniform
// Workspace: ATreeHead (256 bytes) | box partials | node records 32 bytes x cap | node sums 16 bytes x cap | per-position node
// count and levels | scan | chunk offsets | sorted positions | part (3, N) f64 | zpart | blk.  cap = 1 + 4 depth floor(N / (leaf_size + 1)).
constexpr int ATREE_MAX_DEPTH = 24;
constexpr int ATREE_SCAN_ITEMS = 8;                                    // positions per thread of the scan
constexpr int ATREE_SCAN_CHUNK = TSNE_TPB * ATREE_SCAN_ITEMS;
constexpr int ATREE_GRID = 2048;                                       // workgroups of the kernels that loop over the nodes (their number is on the device)

struct ATreeHead {
    TreeFrame fr;
    float w2[ATREE_MAX_DEPTH + 1];                 // f32((side 2^-l)^2)
    int n_nodes;                                   // nodes of this evaluation (<= cap)
    int depth, leaf_size;
    int pad[28];
};
static_assert(sizeof(ATreeHead) == 256, "ATreeHead");

struct ATreeNode {                                 // 32 bytes: one scalar load
    int start, count, level, skip;                 // range [start, start + count) of the sorted order
    float cx, cy;                                  // centre of mass
    int leaf, pad;
};
static_assert(sizeof(ATreeNode) == 32, "ATreeNode");

struct ATreePlan {
    int D, leaf, nchunk;
    int64_t cap;
    size_t boxp_off, node_off, nsum_off, flag_off, scan_off, chunk_off;
    TreeTail t;
};
static int64_t atree_cap(int64_t N, int leaf, int D) { return 1 + 4 * (int64_t)D * (N / ((int64_t)leaf + 1)); }
static ATreePlan atree_plan(int64_t N, int leaf, int D)
{
    ATreePlan p;
    p.D = D;
    p.leaf = leaf;
    p.cap = atree_cap(N, leaf, D);
    p.nchunk = (int)((N + ATREE_SCAN_CHUNK - 1) / ATREE_SCAN_CHUNK);
    p.boxp_off = sizeof(ATreeHead);
    p.node_off = p.boxp_off + tree_align(sizeof(float4) * TREE_BOX_BLOCKS);
    p.nsum_off = p.node_off + tree_align(sizeof(ATreeNode) * (size_t)p.cap);
    p.flag_off = p.nsum_off + tree_align(sizeof(double2) * (size_t)p.cap);
    p.scan_off = p.flag_off + tree_align(sizeof(int) * (size_t)N);
    p.chunk_off = p.scan_off + tree_align(sizeof(int) * (size_t)(N + 1));
    p.t = tree_tail(N, p.chunk_off + tree_align(sizeof(int) * (size_t)(p.nchunk + 1)));
    return p;
}

__device__ __forceinline__ unsigned long long atree_spread(unsigned x)
{
    unsigned long long v = x & 0xffffffu;
    v = (v | (v << 16)) & 0x0000ffff0000ffffull;
    v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
    v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    return (v | (v << 1)) & 0x5555555555555555ull;
}

__global__ __launch_bounds__(TSNE_TPB) void k_atree_keys(const float2 *__restrict__ Y, const float4 *__restrict__ boxp, int nbx,
                                                         ATreeHead *__restrict__ head, int64_t *__restrict__ keys, int N, int D, int leaf)
{
    __shared__ float4 s_box[TSNE_TPB / VCY_WAVE];
    const TreeFrame f = tree_frame(boxp, nbx, D, s_box);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        head->fr = f;
        tree_fill_w2(head->w2, f.side, ATREE_MAX_DEPTH);
        head->n_nodes = 0; head->depth = D; head->leaf_size = leaf;
        for (int l = 0; l < 28; ++l) head->pad[l] = 0;
    }
    const int i = blockIdx.x * TSNE_TPB + threadIdx.x;
    if (i < N) {
        const float2 y = Y[i];
        keys[i] = (int64_t)(atree_spread(tree_cell(y.x, f.lo[0], f.scale, D)) | (atree_spread(tree_cell(y.y, f.lo[1], f.scale, D)) << 1));
    }
}

// first position in [lo, hi) whose key is >= k (hi when there is none): in [lo, hi] whatever the keys hold
__device__ __forceinline__ int atree_lower(const int64_t *__restrict__ sk, int lo, int hi, int64_t k)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (sk[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// flag[i] = nodes starting at position i | l0 << 8 | l1 << 16 (0: none); ysort = positions in sorted order
__global__ __launch_bounds__(TSNE_TPB) void k_atree_flag(const int64_t *__restrict__ sk, const float2 *__restrict__ Y,
                                                         const int64_t *__restrict__ order, int *__restrict__ flag, float2 *__restrict__ ysort,
                                                         int N, int D, int leaf)
{
    const int i = blockIdx.x * TSNE_TPB + threadIdx.x;
    if (i >= N) return;
    const int64_t o = order[i];
    ysort[i] = Y[(uint64_t)o < (uint64_t)N ? o : 0];
    const int64_t k = sk[i];
    int l0 = 0;
    if (i > 0) {
        const unsigned long long x = (unsigned long long)(k ^ sk[i - 1]);
        if (x == 0ull) { flag[i] = 0; return; }                        // a repeated key starts no node
        l0 = D - ((63 - __clzll((long long)x)) >> 1);
    }
    // the deepest level in 0 .. D whose cell around i holds more than `leaf` points (-1: not even the root)
    int a = -1, b = D;
    while (a < b) {
        const int l = a + ((b - a + 1) >> 1), sh = 2 * (D - l);
        const int64_t c0 = (k >> sh) << sh;
        const int first = atree_lower(sk, 0, i, c0), last = atree_lower(sk, i + 1, N, c0 + ((int64_t)1 << sh));
        if (last - first > leaf) a = l; else b = l - 1;
    }
    const int l1 = min(D, a + 1);
    l0 = min(max(l0, 0), D + 1);                                       // keys beyond 2 D bits (not this library's) start no node
    const int n = max(l1 - l0 + 1, 0);
    flag[i] = n ? (n | (l0 << 8) | (l1 << 16)) : 0;
}

// scan[i] = the node counts of the chunk's positions before i; chunk[c] = the chunk's total
__global__ __launch_bounds__(TSNE_TPB) void k_atree_scan1(const int *__restrict__ flag, int *__restrict__ scan, int *__restrict__ chunk, int N)
{
    __shared__ int s_w[TSNE_TPB / VCY_WAVE];
    const int base = blockIdx.x * ATREE_SCAN_CHUNK + threadIdx.x * ATREE_SCAN_ITEMS;
    int v[ATREE_SCAN_ITEMS], tot = 0;
#pragma unroll
    for (int r = 0; r < ATREE_SCAN_ITEMS; ++r) {
        v[r] = base + r < N ? (flag[base + r] & 0xff) : 0;
        tot += v[r];
    }
    int inc = tot;                                                     // inclusive scan over the wave, then over the 4 waves
#pragma unroll
    for (int off = 1; off < VCY_WAVE; off <<= 1) {
        const int o = __shfl_up(inc, off, VCY_WAVE);
        if ((int)(threadIdx.x & 63) >= off) inc += o;
    }
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
    __syncthreads();
    int before = inc - tot;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += s_w[w];
#pragma unroll
    for (int r = 0; r < ATREE_SCAN_ITEMS; ++r) {
        if (base + r < N) scan[base + r] = before;
        before += v[r];
    }
    if (threadIdx.x == TSNE_TPB - 1) chunk[blockIdx.x] = before;
}

// one workgroup: chunk[c] <- the totals of the chunks before c, chunk[nchunk] and head->n_nodes <- the number of nodes (<= cap)
__global__ __launch_bounds__(TSNE_TPB) void k_atree_scan2(int *__restrict__ chunk, int nchunk, ATreeHead *__restrict__ head, int *__restrict__ scan,
                                                          int N, long long cap)
{
    __shared__ int s_w[TSNE_TPB / VCY_WAVE];
    long long carry = 0;
    for (int c0 = 0; c0 < nchunk; c0 += TSNE_TPB) {
        const int c = c0 + threadIdx.x;
        const int v = c < nchunk ? chunk[c] : 0;
        int inc = v;
#pragma unroll
        for (int off = 1; off < VCY_WAVE; off <<= 1) {
            const int o = __shfl_up(inc, off, VCY_WAVE);
            if ((int)(threadIdx.x & 63) >= off) inc += o;
        }
        __syncthreads();
        if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
        __syncthreads();
        long long before = carry + inc - v;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += s_w[w];
        if (c < nchunk) chunk[c] = (int)(before < cap ? before : cap);
        carry += (long long)s_w[0] + s_w[1] + s_w[2] + s_w[3];
    }
    if (threadIdx.x == 0) {
        const int nn = (int)(carry < cap ? carry : cap);
        chunk[nchunk] = nn;
        scan[N] = 0;
        head->n_nodes = nn;
    }
}

__device__ __forceinline__ int atree_number(const int *__restrict__ scan, const int *__restrict__ chunk, int pos)
{
    return scan[pos] + chunk[pos / ATREE_SCAN_CHUNK];                  // pos == N: scan[N] = 0, chunk[nchunk] = the total when N fills its chunks,
}                                                                      // and otherwise the callers pass `nn` for it

// the records of the nodes that start at position i, levels l0 .. l1: the ends are nested, each searched inside the one before
__global__ __launch_bounds__(TSNE_TPB) void k_atree_emit(const int64_t *__restrict__ sk, const int *__restrict__ flag, const int *__restrict__ scan,
                                                         const int *__restrict__ chunk, int nchunk, ATreeNode *__restrict__ node, int N, int D,
                                                         int leaf, long long cap)
{
    const int i = blockIdx.x * TSNE_TPB + threadIdx.x;
    if (i >= N) return;
    const int fl = flag[i], n = fl & 0xff;
    if (!n) return;
    const int l0 = (fl >> 8) & 0xff, nn = chunk[nchunk];
    const int64_t k = sk[i];
    const int first = atree_number(scan, chunk, i);
    int end = N;
    for (int r = 0; r < n; ++r) {
        const int l = l0 + r, sh = 2 * (D - l);
        end = atree_lower(sk, i + 1, end, ((k >> sh) << sh) + ((int64_t)1 << sh));
        const long long idx = (long long)first + r;
        if (idx >= cap || idx >= nn) return;
        ATreeNode nd;
        nd.start = i;
        nd.count = end - i;
        nd.level = l;
        nd.skip = end >= N ? nn : min(max(atree_number(scan, chunk, end), (int)idx + 1), nn);
        nd.cx = nd.cy = 0.0f;
        nd.leaf = (nd.count <= leaf || l >= D) ? 1 : 0;
        nd.pad = 0;
        node[idx] = nd;
    }
}

// the nodes of level l (launched for l = depth .. 0): sum and com; the children are the next node and then each one's skip
__global__ __launch_bounds__(TSNE_TPB) void k_atree_com(ATreeNode *node, double2 *nsum, const float2 *__restrict__ ysort,
                                                        const ATreeHead *__restrict__ head, int N, int l)
{
    const int nn = head->n_nodes;
    for (int idx = blockIdx.x * TSNE_TPB + threadIdx.x; idx < nn; idx += gridDim.x * TSNE_TPB) {
        const ATreeNode nd = node[idx];
        if (nd.level != l) continue;
        double sx = 0.0, sy = 0.0;
        if (nd.leaf) {
            const int b = max(nd.start, 0), e = min(nd.start + nd.count, N);
#pragma unroll 4
            for (int j = b; j < e; ++j) {
                const float2 y = ysort[j];
                sx += (double)y.x;
                sy += (double)y.y;
            }
        } else {
            const int stop = min(nd.skip, nn);
            int c = idx + 1;
            for (int t = 0; t < 4 && c < stop; ++t) {
                const double2 s = nsum[c];
                sx += s.x;
                sy += s.y;
                c = max(node[c].skip, c + 1);
            }
        }
        nsum[idx] = make_double2(sx, sy);
        node[idx].cx = (float)__ddiv_rn(sx, (double)nd.count);
        node[idx].cy = (float)__ddiv_rn(sy, (double)nd.count);
    }
}

// One wave per 64 consecutive targets of the sorted order; the node number i is wave-uniform and only grows.  `until` is the
// skip of the node the lane accepted last: the lane sits out while i < until (a lane without a target: always).  A node that no
// lane wants to open is left for its skip, an internal node that some lane opens for i + 1, a leaf that some lane does not accept
// is summed point by point by those lanes.  The loop carries the node count as its trip bound.
template <bool VISITS>
__global__ __launch_bounds__(TSNE_TPB) void k_tsne_atree_repulsion(const ATreeNode *__restrict__ node, const float2 *__restrict__ ysort,
                                                                   const int64_t *__restrict__ order, const ATreeHead *__restrict__ head,
                                                                   double *__restrict__ part, double *__restrict__ zpart,
                                                                   int32_t *__restrict__ visits, int N, float th2)
{
    __shared__ double s_red[TSNE_TPB / VCY_WAVE];
    const int p = blockIdx.x * TSNE_TPB + threadIdx.x;
    const bool valid = p < N;
    const float2 tp = valid ? ysort[p] : make_float2(0.0f, 0.0f);
    const float t[2] = {tp.x, tp.y};
    int until = valid ? 0 : 0x7fffffff;
    TreeAcc a;
    const int nn = __builtin_amdgcn_readfirstlane(head->n_nodes);
    int i = 0;
    for (int trip = 0; trip < nn && i < nn; ++trip) {
        i = __builtin_amdgcn_readfirstlane(i);
        const ATreeNode nd = node[i];
        const int cnt = __builtin_amdgcn_readfirstlane(nd.count), lvl = min(max(__builtin_amdgcn_readfirstlane(nd.level), 0), ATREE_MAX_DEPTH);
        const int skip = max(__builtin_amdgcn_readfirstlane(nd.skip), i + 1), leaf = __builtin_amdgcn_readfirstlane(nd.leaf);
        const bool active = i >= until;
        if (a.run + 1 > TREE_RUN) a.carry();
        const bool take = tree_accept(a, t, nd.cx, nd.cy, cnt, head->w2 + lvl, th2, active);
        if (take) until = skip;
        ++a.run;
        const bool open = active && !take;
        const bool any_open = __ballot(open) != 0ull;
        if (leaf && any_open) {
            const int b = max(__builtin_amdgcn_readfirstlane(nd.start), 0), e = min(b + max(cnt, 0), N);
            tree_leaf_sweep(a, t, ysort, b, e, p, open);
        }
        i = (!leaf && any_open) ? i + 1 : skip;
    }
    tree_walk_store<VISITS>(a, valid, p, order, part, zpart, visits, N, s_red);
}

// build + traversal: part, zpart of the workspace are what k_tsne_step<2, .> reads with one split
static int tree_repulsion_launch(const float *Y, const int64_t *order, const int64_t *skeys, int32_t *visits, void *workspace, const ATreePlan &p,
                                 int64_t N, double angle, hipStream_t s)
{
    char *w = (char *)workspace;
    const int n = (int)N, D = p.D;
    ATreeHead *head = (ATreeHead *)w;
    ATreeNode *node = (ATreeNode *)(w + p.node_off);
    double2 *nsum = (double2 *)(w + p.nsum_off);
    int *flag = (int *)(w + p.flag_off), *scan = (int *)(w + p.scan_off), *chunk = (int *)(w + p.chunk_off);
    float2 *ysort = (float2 *)(w + p.t.ysort_off);
    hipLaunchKernelGGL(k_atree_flag, dim3(p.t.nb), dim3(TSNE_TPB), 0, s, skeys, (const float2 *)Y, order, flag, ysort, n, D, p.leaf);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_atree_scan1, dim3(p.nchunk), dim3(TSNE_TPB), 0, s, flag, scan, chunk, n);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_atree_scan2, dim3(1), dim3(TSNE_TPB), 0, s, chunk, p.nchunk, head, scan, n, (long long)p.cap);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_atree_emit, dim3(p.t.nb), dim3(TSNE_TPB), 0, s, skeys, flag, scan, chunk, p.nchunk, node, n, D, p.leaf, (long long)p.cap);
    VCY_LAUNCH_CHECK();
    const int64_t want = (p.cap + TSNE_TPB - 1) / TSNE_TPB;
    const unsigned g = (unsigned)(want < ATREE_GRID ? want : ATREE_GRID);
    for (int l = D; l >= 0; --l) {
        hipLaunchKernelGGL(k_atree_com, dim3(g), dim3(TSNE_TPB), 0, s, node, nsum, ysort, head, n, l);
        VCY_LAUNCH_CHECK();
    }
    const float th2 = (float)(angle * angle);
    double *part = (double *)(w + p.t.part_off), *zpart = (double *)(w + p.t.zpart_off);
    const auto walk = visits ? k_tsne_atree_repulsion<true> : k_tsne_atree_repulsion<false>;
    hipLaunchKernelGGL(walk, dim3(p.t.tb), dim3(TSNE_TPB), 0, s, node, ysort, order, head, part, zpart, visits, n, th2);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

// the node numbers are int32: N, leaf_size and depth whose bound 1 + 4 depth floor(N / (leaf_size + 1)) does not fit are out of range
static bool atree_in_range(int64_t N, int leaf, int depth)
{
    return N >= 2 && N < (1ll << 30) && leaf >= 1 && depth >= 1 && depth <= ATREE_MAX_DEPTH && atree_cap(N, leaf, depth) < (1ll << 31);
}

static int atree_check(int64_t N, int n_components, int leaf, int depth, double angle, const char *who)
{
    const int rc = tree_check_shared(N, n_components, angle, who);
    if (rc != VCY_OK) return rc;
    if (leaf < 1) return fail(VCY_ERR_INVALID, "%s: leaf_size must be >= 1", who);
    if (depth < 1 || depth > ATREE_MAX_DEPTH) return fail(VCY_ERR_INVALID, "%s: max_depth must be 1 .. 24", who);
    if (!atree_in_range(N, leaf, depth)) return fail(VCY_ERR_INVALID, "%s: the node bound of N, leaf_size and max_depth exceeds 2^31", who);
    return VCY_OK;
}

// both trees' _gradient and _step after the checks: the build and walk of the plan's tree, then the tail on the one split they leave
template <class Plan, class Key>
static int tree_eval(const TsneArgs &a, const int64_t *order, const Key *skeys, void *workspace, const Plan &p, int64_t N, double angle,
                     hipStream_t s)
{
    const int rc = tree_repulsion_launch(a.Y, order, skeys, nullptr, workspace, p, N, angle, s);
    if (rc != VCY_OK) return rc;
    char *w = (char *)workspace;
    return tsne_tail<2>(a, (const double *)(w + p.t.part_off), (const double *)(w + p.t.zpart_off), p.t.tb, 1, (double *)(w + p.t.blk_off),
                        p.t.nb, (int)N, s);
}

static int tree_entry(const TsneArgs &a, const int64_t *order, const int32_t *skeys, void *workspace, int64_t N, int n_components, int depth,
                      double angle, const char *who, hipStream_t s)
{
    int rc = tsne_args_check(a, order && skeys && workspace, who);
    if (rc == VCY_OK) rc = tree_check(N, n_components, depth, angle, who);
    return rc != VCY_OK ? rc : tree_eval(a, order, skeys, workspace, tree_plan(N, depth), N, angle, s);
}

static int atree_entry(const TsneArgs &a, const int64_t *order, const int64_t *skeys, void *workspace, int64_t N, int n_components, int leaf,
                       int depth, double angle, const char *who, hipStream_t s)
{
    int rc = tsne_args_check(a, order && skeys && workspace, who);
    if (rc == VCY_OK) rc = atree_check(N, n_components, leaf, depth, angle, who);
    return rc != VCY_OK ? rc : tree_eval(a, order, skeys, workspace, atree_plan(N, leaf, depth), N, angle, s);
}

}  // namespace vcy

using namespace vcy;

extern "C" int vcy_tsne_perplexity(const float *sqd, double *P, int32_t *n_steps, int64_t N, int64_t k, double perplexity, vcy_stream stream)
{
    VCY_REQUIRE(sqd && P, "tsne_perplexity: null pointer");
    VCY_REQUIRE(N >= 1 && N < (1ll << 31) && k >= 1 && k < (1ll << 20) && N * k < (1ll << 40), "tsne_perplexity: sizes out of range");
    VCY_REQUIRE(perplexity > 0.0, "tsne_perplexity: perplexity must be > 0");
    hipLaunchKernelGGL(k_tsne_perplexity, dim3((unsigned)((N + TSNE_TPB - 1) / TSNE_TPB)), dim3(TSNE_TPB), 0, (hipStream_t)stream, sqd, P,
                       (int *)n_steps, (long long)N, (int)k, (float)perplexity);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" size_t vcy_tsne_workspace_bytes(int64_t N, int n_components)
{
    if (N < 2 || n_components < 1 || n_components > 3) return 0;
    return tsne_plan(N, n_components).bytes;
}

extern "C" int vcy_tsne_gradient(const float *Y, const int64_t *indptr, const int32_t *indices, const float *pval, float *grad, double *stats,
                                 void *workspace, int64_t N, int n_components, int compute_error, vcy_stream stream)
{
    const TsneArgs a = {Y, nullptr, indptr, indices, pval, grad, nullptr, nullptr, stats, compute_error, 0.0, 0.0, 0.0, false};
    return tsne_entry(a, workspace, N, n_components, "tsne_gradient", (hipStream_t)stream);
}

extern "C" int vcy_tsne_step(const float *Y, float *Y_out, const int64_t *indptr, const int32_t *indices, const float *pval, double *update,
                             float *gains, double *stats, void *workspace, int64_t N, int n_components, double momentum, double learning_rate,
                             double min_gain, int compute_error, vcy_stream stream)
{
    const TsneArgs a = {Y, Y_out, indptr, indices, pval, nullptr, update, gains, stats, compute_error, momentum, learning_rate, min_gain, true};
    return tsne_entry(a, workspace, N, n_components, "tsne_step", (hipStream_t)stream);
}

extern "C" int vcy_tsne_tree_depth(int64_t N)
{
    int L = 1;                                                         // at most 4 points per leaf on average (measured: DESIGN.md section 9)
    while (L < TREE_MAX_DEPTH && (4ll << (2 * L)) < N) ++L;
    return L;
}

extern "C" size_t vcy_tsne_tree_workspace_bytes(int64_t N, int depth)
{
    if (N < 2 || N >= (1ll << 30) || depth < 1 || depth > TREE_MAX_DEPTH) return 0;
    return tree_plan(N, depth).t.bytes;
}

extern "C" int vcy_tsne_tree_keys(const float *Y, int32_t *keys, void *workspace, int64_t N, int depth, vcy_stream stream)
{
    VCY_REQUIRE(Y && keys && workspace, "tsne_tree_keys: null pointer");
    const int rc = tree_check(N, 2, depth, 0.0, "tsne_tree_keys");
    if (rc != VCY_OK) return rc;
    const TreePlan p = tree_plan(N, depth);
    char *w = (char *)workspace;
    float4 *boxp = (float4 *)(w + p.boxp_off);
    hipLaunchKernelGGL(k_tree_box, dim3(p.t.nbx), dim3(TSNE_TPB), 0, (hipStream_t)stream, (const float2 *)Y, boxp, (int)N);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tree_keys, dim3(p.t.nb), dim3(TSNE_TPB), 0, (hipStream_t)stream, (const float2 *)Y, boxp, p.t.nbx, (TreeHead *)w, keys, (int)N, depth);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_tsne_tree_repulsion(const float *Y, const int64_t *order, const int32_t *sorted_keys, double *rep, double *Z, int32_t *visits,
                                       void *workspace, int64_t N, int depth, double angle, vcy_stream stream)
{
    VCY_REQUIRE(Y && order && sorted_keys && rep && Z && workspace, "tsne_tree_repulsion: null pointer");
    const int rc = tree_check(N, 2, depth, angle, "tsne_tree_repulsion");
    if (rc != VCY_OK) return rc;
    const TreePlan p = tree_plan(N, depth);
    const int rc2 = tree_repulsion_launch(Y, order, sorted_keys, visits, workspace, p, N, angle, (hipStream_t)stream);
    return rc2 != VCY_OK ? rc2 : tree_rep_out(p.t, workspace, rep, Z, N, (hipStream_t)stream);
}

extern "C" int vcy_tsne_tree_gradient(const float *Y, const int64_t *indptr, const int32_t *indices, const float *pval, const int64_t *order,
                                      const int32_t *sorted_keys, float *grad, double *stats, void *workspace, int64_t N, int n_components,
                                      int depth, double angle, int compute_error, vcy_stream stream)
{
    const TsneArgs a = {Y, nullptr, indptr, indices, pval, grad, nullptr, nullptr, stats, compute_error, 0.0, 0.0, 0.0, false};
    return tree_entry(a, order, sorted_keys, workspace, N, n_components, depth, angle, "tsne_tree_gradient", (hipStream_t)stream);
}

extern "C" int vcy_tsne_tree_step(const float *Y, float *Y_out, const int64_t *indptr, const int32_t *indices, const float *pval,
                                  const int64_t *order, const int32_t *sorted_keys, double *update, float *gains, double *stats, void *workspace,
                                  int64_t N, int n_components, int depth, double angle, double momentum, double learning_rate, double min_gain,
                                  int compute_error, vcy_stream stream)
{
    const TsneArgs a = {Y, Y_out, indptr, indices, pval, nullptr, update, gains, stats, compute_error, momentum, learning_rate, min_gain, true};
    return tree_entry(a, order, sorted_keys, workspace, N, n_components, depth, angle, "tsne_tree_step", (hipStream_t)stream);
}

extern "C" size_t vcy_tsne_atree_workspace_bytes(int64_t N, int leaf_size, int max_depth)
{
    if (!atree_in_range(N, leaf_size, max_depth)) return 0;
    return atree_plan(N, leaf_size, max_depth).t.bytes;
}

extern "C" int vcy_tsne_atree_keys(const float *Y, int64_t *keys, void *workspace, int64_t N, int leaf_size, int max_depth, vcy_stream stream)
{
    VCY_REQUIRE(Y && keys && workspace, "tsne_atree_keys: null pointer");
    const int rc = atree_check(N, 2, leaf_size, max_depth, 0.0, "tsne_atree_keys");
    if (rc != VCY_OK) return rc;
    const ATreePlan p = atree_plan(N, leaf_size, max_depth);
    char *w = (char *)workspace;
    float4 *boxp = (float4 *)(w + p.boxp_off);
    hipLaunchKernelGGL(k_tree_box, dim3(p.t.nbx), dim3(TSNE_TPB), 0, (hipStream_t)stream, (const float2 *)Y, boxp, (int)N);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_atree_keys, dim3(p.t.nb), dim3(TSNE_TPB), 0, (hipStream_t)stream, (const float2 *)Y, boxp, p.t.nbx, (ATreeHead *)w, keys, (int)N,
                       max_depth, leaf_size);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_tsne_atree_repulsion(const float *Y, const int64_t *order, const int64_t *sorted_keys, double *rep, double *Z, int32_t *visits,
                                        void *workspace, int64_t N, int leaf_size, int max_depth, double angle, vcy_stream stream)
{
    VCY_REQUIRE(Y && order && sorted_keys && rep && Z && workspace, "tsne_atree_repulsion: null pointer");
    const int rc = atree_check(N, 2, leaf_size, max_depth, angle, "tsne_atree_repulsion");
    if (rc != VCY_OK) return rc;
    const ATreePlan p = atree_plan(N, leaf_size, max_depth);
    const int rc2 = tree_repulsion_launch(Y, order, sorted_keys, visits, workspace, p, N, angle, (hipStream_t)stream);
    return rc2 != VCY_OK ? rc2 : tree_rep_out(p.t, workspace, rep, Z, N, (hipStream_t)stream);
}

extern "C" int vcy_tsne_atree_gradient(const float *Y, const int64_t *indptr, const int32_t *indices, const float *pval, const int64_t *order,
                                       const int64_t *sorted_keys, float *grad, double *stats, void *workspace, int64_t N, int n_components,
                                       int leaf_size, int max_depth, double angle, int compute_error, vcy_stream stream)
{
    const TsneArgs a = {Y, nullptr, indptr, indices, pval, grad, nullptr, nullptr, stats, compute_error, 0.0, 0.0, 0.0, false};
    return atree_entry(a, order, sorted_keys, workspace, N, n_components, leaf_size, max_depth, angle, "tsne_atree_gradient", (hipStream_t)stream);
}

extern "C" int vcy_tsne_atree_step(const float *Y, float *Y_out, const int64_t *indptr, const int32_t *indices, const float *pval,
                                   const int64_t *order, const int64_t *sorted_keys, double *update, float *gains, double *stats, void *workspace,
                                   int64_t N, int n_components, int leaf_size, int max_depth, double angle, double momentum, double learning_rate,
                                   double min_gain, int compute_error, vcy_stream stream)
{
    const TsneArgs a = {Y, Y_out, indptr, indices, pval, nullptr, update, gains, stats, compute_error, momentum, learning_rate, min_gain, true};
    return atree_entry(a, order, sorted_keys, workspace, N, n_components, leaf_size, max_depth, angle, "tsne_atree_step", (hipStream_t)stream);
}
