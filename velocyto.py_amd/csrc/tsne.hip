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

template <int D>
static int tsne_launch(const float *Y, float *Yout, const int64_t *indptr, const int32_t *indices, const float *pval, float *grad,
                       double *update, float *gains, double *stats, void *workspace, int64_t N, int compute_error, double momentum,
                       double lr, double min_gain, bool step, hipStream_t s)
{
    const TsnePlan p = tsne_plan(N, D);
    char *w = (char *)workspace;
    double *part = (double *)(w + p.part_off), *zpart = (double *)(w + p.zpart_off), *blk = (double *)(w + p.blk_off);
    const int n = (int)N, nz = p.S * p.tb;
    hipLaunchKernelGGL(k_tsne_repulsion<D>, dim3(p.tb, p.S), dim3(TSNE_TPB), 0, s, Y, part, zpart, n, p.per);
    VCY_LAUNCH_CHECK();
    if (step)
        hipLaunchKernelGGL((k_tsne_step<D, true>), dim3(p.nb), dim3(TSNE_TPB), 0, s, Y, Yout, indptr, indices, pval, part, zpart, nz, p.S,
                           grad, update, gains, blk, stats, n, compute_error, momentum, lr, (float)min_gain);
    else
        hipLaunchKernelGGL((k_tsne_step<D, false>), dim3(p.nb), dim3(TSNE_TPB), 0, s, Y, Yout, indptr, indices, pval, part, zpart, nz, p.S,
                           grad, update, gains, blk, stats, n, compute_error, momentum, lr, (float)min_gain);
    VCY_LAUNCH_CHECK();
    if (compute_error) {
        hipLaunchKernelGGL(k_tsne_stats, dim3(1), dim3(TSNE_TPB), 0, s, blk, p.nb, stats);
        VCY_LAUNCH_CHECK();
    }
    return VCY_OK;
}

static int tsne_dispatch(const float *Y, float *Yout, const int64_t *indptr, const int32_t *indices, const float *pval, float *grad,
                         double *update, float *gains, double *stats, void *workspace, int64_t N, int D, int compute_error,
                         double momentum, double lr, double min_gain, bool step, hipStream_t s)
{
    switch (D) {
    case 1: return tsne_launch<1>(Y, Yout, indptr, indices, pval, grad, update, gains, stats, workspace, N, compute_error, momentum, lr, min_gain, step, s);
    case 2: return tsne_launch<2>(Y, Yout, indptr, indices, pval, grad, update, gains, stats, workspace, N, compute_error, momentum, lr, min_gain, step, s);
    default: return tsne_launch<3>(Y, Yout, indptr, indices, pval, grad, update, gains, stats, workspace, N, compute_error, momentum, lr, min_gain, step, s);
    }
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
    VCY_REQUIRE(Y && indptr && indices && pval && grad && stats && workspace, "tsne_gradient: null pointer");
    VCY_REQUIRE(N >= 2 && N < (1ll << 30), "tsne_gradient: N out of range");
    VCY_REQUIRE(n_components >= 1 && n_components <= 3, "tsne_gradient: n_components must be 1, 2 or 3");
    return tsne_dispatch(Y, nullptr, indptr, indices, pval, grad, nullptr, nullptr, stats, workspace, N, n_components, compute_error, 0.0, 0.0,
                         0.0, false, (hipStream_t)stream);
}

extern "C" int vcy_tsne_step(const float *Y, float *Y_out, const int64_t *indptr, const int32_t *indices, const float *pval, double *update,
                             float *gains, double *stats, void *workspace, int64_t N, int n_components, double momentum, double learning_rate,
                             double min_gain, int compute_error, vcy_stream stream)
{
    VCY_REQUIRE(Y && Y_out && indptr && indices && pval && update && gains && stats && workspace, "tsne_step: null pointer");
    VCY_REQUIRE(Y != Y_out, "tsne_step: Y_out must not alias Y (the attraction reads every row's old position)");
    VCY_REQUIRE(N >= 2 && N < (1ll << 30), "tsne_step: N out of range");
    VCY_REQUIRE(n_components >= 1 && n_components <= 3, "tsne_step: n_components must be 1, 2 or 3");
    return tsne_dispatch(Y, Y_out, indptr, indices, pval, nullptr, update, gains, stats, workspace, N, n_components, compute_error, momentum,
                         learning_rate, min_gain, true, (hipStream_t)stream);
}
