// misc.hip -- the small streaming kernels around the four hot stages:
//   normalisation pre-step (analysis.py:535-631), the dmat transform of estimate_transition_prob
//   on a stored delta_S (analysis.py:1538, 1575-1601), the randomised control's permute_rows_nsign
//   (:2407-2420), the diag/NaN fix-ups (:1604-1612), the transition-probability / embedding-shift
//   step in neighbour-list form (stage E, :1670-1733) and the weight variants of fit_gammas
//   (:1182-1219).  Stage F, the Markov chain of prepare_markov / run_markov, is markov.hip.
#include <math.h>
#include "common.h"

namespace vcy {

// ---------------------------------------------------------------- a1: normalisation
// cell_size[c] = sum_g M[c,g]  (S.sum(0) in the reference's layout): one wave per cell row.
template <typename T>
__global__ __launch_bounds__(256) void k_row_sums(const T *__restrict__ M, double *__restrict__ out, int64_t C, int G, int64_t ld)
{
    using V = typename Vec<T>::type;
    constexpr int N = Vec<T>::N;
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (c >= C) return;
    const T *row = M + c * ld;
    double s = 0.0;
    const int nvec = G / N;
    for (int v = lane; v < nvec; v += 64) {
        const V x = reinterpret_cast<const V *>(row)[v];
        const T *xp = reinterpret_cast<const T *>(&x);
#pragma unroll
        for (int k = 0; k < N; ++k) s += (double)xp[k];
    }
    for (int g = nvec * N + lane; g < G; g += 64) s += (double)row[g];
    s = wave_sum(s);
    if (lane == 0) out[c] = s;
}

// out_sz[c,g] = factor[c] * M[c,g] (non-finite -> 0 when fix != 0, analysis.py:580);
// out_norm[c,g] = log2(out_sz + pcount) (analysis.py:551); either output may be NULL.
template <typename T>
__global__ __launch_bounds__(256) void k_scale_log(const T *__restrict__ M, const double *__restrict__ factor, T *__restrict__ out_sz,
                                                    T *__restrict__ out_norm, int64_t C, int G, int64_t ld, double pcount, int fix)
{
    const int64_t total = C * ld;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = t / ld;
        const int g = (int)(t - c * ld);
        T v = T(0), l = T(0);
        if (g < G) {
            double x = (factor ? factor[c] : 1.0) * (double)M[t];
            if (fix && !isfinite(x)) x = 0.0;
            v = (T)x;
            l = (T)log2(x + pcount);
        }
        if (out_sz) out_sz[t] = v;
        if (out_norm) out_norm[t] = l;
    }
}

// ---------------------------------------------------------------- dmat from a stored delta_S
template <typename T>
__global__ __launch_bounds__(256) void k_delta_transform(const T *__restrict__ hi, const T *__restrict__ dS, T *__restrict__ dmat,
                                                          T *__restrict__ e_out, int64_t C, int G, int64_t ld, T used_dt, int mode, T psc)
{
    // mode 0 linear, 1 sqrt, 2 log10 (sign(D) f(|D|+psc), D = (hi + dt*dS) - hi); 3 logratio:
    // e_out = log2(hi + psc), dmat = log2(|hi + dt*dS| + psc) - e_out   (analysis.py:1583-1584)
    const int64_t total = C * ld;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int g = (int)(t % ld);
        T d = T(0), eo = T(0);
        if (g < G) {
            const T h = hi[t];
            const T ht = h + used_dt * dS[t];
            if (mode == 3) {
                eo = (T)log2((double)(h + psc));
                d = (T)log2((double)(fabs(ht) + psc)) - eo;
            } else {
                const T D = ht - h;
                if (mode == 0) d = D;
                else {
                    const double a = (double)fabs(D) + (double)psc;
                    const T f = (T)(mode == 1 ? sqrt(a) : log10(a));
                    d = D > T(0) ? f : (D < T(0) ? -f : T(0) * f);
                }
            }
        }
        dmat[t] = d;
        if (e_out) e_out[t] = eo;
    }
}

// ---------------------------------------------------------------- randomised control: permute_rows_nsign (analysis.py:2407-2420)
// Per gene, the values shuffled across the cells and multiplied by random signs.  The reference draws both from numba's private
// Mersenne twister, gene after gene; here every gene gets its own pseudo-random PERMUTATION of [0, C) as a function that is evaluated
// where it is needed - a 5-round Feistel network over the 2 * hb >= log2(C) bits of the cell number, keyed by (seed, gene), walked
// until it lands below C (a permutation of [0, 4^hb) restricted to the cycle-walk over a subset is a permutation of the subset) - so
// the shuffle is one gather, out[c, g] = +- in[pi_g(c), g], with no sort, no keys in memory and no gene-major copy.  Statistical
// parity with the reference (uniform, independent per gene), not the same random numbers.
__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t perm_key(uint32_t seed_lo, uint32_t seed_hi, int64_t g) { return mix32(seed_lo ^ mix32((uint32_t)g * 0x9e3779b9u + seed_hi)); }
__device__ __forceinline__ uint32_t perm_cell(uint32_t c, uint32_t key, int hb, uint32_t C)
{
    const uint32_t mask = (1u << hb) - 1u;
    uint32_t x = c;
    do {
        uint32_t L = x >> hb, R = x & mask;
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const uint32_t t = L ^ (mix32(R + key + (uint32_t)r * 0x85ebca6bu) & mask);
            L = R;
            R = t;
        }
        x = (L << hb) | R;
    } while (x >= C);
    return x;
}
__device__ __forceinline__ uint32_t perm_sign(uint32_t c, uint32_t key) { return mix32(key ^ (c * 0xc2b2ae35u + 0x27d4eb2fu)) >> 31; }

template <typename T, int CPT>
__global__ __launch_bounds__(256) void k_permute_rows_nsign(const T *__restrict__ in, T *__restrict__ out, int C, int G, int64_t ld,
                                                             uint32_t seed_lo, uint32_t seed_hi, int hb, int64_t gene0)
{
    const int g = blockIdx.x * 256 + threadIdx.x;            // lanes = consecutive genes: coalesced stores, one sector per gathered value
    if (g >= ld) return;
    const int c0 = blockIdx.y * CPT;
    if (g >= G) {                                             // padding columns of the cell-major layout stay zero
        for (int c = c0; c < min(C, c0 + CPT); ++c) out[(int64_t)c * ld + g] = T(0);
        return;
    }
    const uint32_t key = perm_key(seed_lo, seed_hi, gene0 + g);
    T v[CPT];
    uint32_t sg[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int c = min(c0 + i, C - 1);
        v[i] = in[(int64_t)perm_cell((uint32_t)c, key, hb, (uint32_t)C) * ld + g];
        sg[i] = perm_sign((uint32_t)c, key);
    }
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        if (c0 + i < C) out[(int64_t)(c0 + i) * ld + g] = sg[i] ? -v[i] : v[i];
}

// The same shuffle on a GENE-MAJOR copy (G, C): a gene's values are contiguous, so the gather stays inside one 4 C-byte row that
// lives in L2 - the cell-major gather above moves a 64-byte sector per 4-byte value (96 GB for a 6 GB matrix, 33 ms); two tiled
// transposes and this kernel move 36 GB.  Lanes = consecutive cells of one gene.
template <typename T, int CPT>
__global__ __launch_bounds__(256) void k_permute_within_gene_rows(const T *__restrict__ in, T *__restrict__ out, int C, uint32_t seed_lo,
                                                                   uint32_t seed_hi, int hb, int64_t gene0)
{
    const int g = blockIdx.y;
    const uint32_t key = perm_key(seed_lo, seed_hi, gene0 + g);
    const T *row = in + (int64_t)g * C;
    T *orow = out + (int64_t)g * C;
    const int c0 = blockIdx.x * 256 * CPT + threadIdx.x;
    T v[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int c = min(c0 + i * 256, C - 1);
        const T x = row[perm_cell((uint32_t)c, key, hb, (uint32_t)C)];
        v[i] = perm_sign((uint32_t)c, key) ? -x : x;
    }
#pragma unroll
    for (int i = 0; i < CPT; ++i)
        if (c0 + i * 256 < C) orow[c0 + i * 256] = v[i];
}

// np.fill_diagonal(corrcoef, 0); corrcoef[isnan] = nan_to   (analysis.py:1604-1606) on the compact form
template <typename T>
__global__ void k_corr_fixup(T *__restrict__ vals, const int32_t *__restrict__ ixs, int64_t cell0, int64_t total, int nrndm,
                             int zero_self, int fix_nan, T nan_to, int *__restrict__ nan_count)
{
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = cell0 + t / nrndm;
        T v = vals[t];
        if (zero_self && ixs[t] == c) v = T(0);
        else if (v != v) {
            if (nan_count) atomicAdd(nan_count, 1);
            if (fix_nan) v = nan_to;
        }
        vals[t] = v;
    }
}

// ---------------------------------------------------------------- stage E: transition probabilities
// One wave per cell over its neighbour list (n entries):
//   p_n = exp(corr[c,n]/sigma) / sum_n exp(corr/sigma)                 (analysis.py:1697-1698)
//   u_n = (emb[i_n] - emb[c]) / |emb[i_n] - emb[c]|, 0 on the diagonal  (:1704-1708; 0/0 = NaN otherwise)
//   delta_embedding[c] = sum_n p_n u_n - (1/n) sum_n u_n               (:1710-1712)
//   wdiff[c,n] = p_n - 1/n        (weights of the expression-scaling pooling, :1716)
// The softmax of stage E to the last few bits (tests/test_gpu_markov_kernels.py holds tp to 4 ulps of a long-double reference).
// exp(c / sigma): q = c / sigma is half an ulp of up to 1 / sigma off, which exp() turns into |q| 2^-53 of relative error (250 ulps at
// corr = 1, sigma_corr = 0.005).  c - q sigma is exact in one fma, and exp(q + d) = exp(q) (1 + d): the kernel carries (e, d).
__device__ __forceinline__ double exp_quot(double c, double sigma, double &d)
{
    const double q = c / sigma;
    d = fma(-q, sigma, c) / sigma;
    return exp(q);
}
// (hi, lo) += (b, bl): hi + b with its rounding error (Knuth) and the partner's low part gathered in lo; symmetric in the two operands
__device__ __forceinline__ void two_sum(double &hi, double &lo, double b, double bl)
{
    const double s = hi + b, bb = s - hi;
    const double err = (hi - (s - bb)) + (b - bb);
    hi = s;
    lo = (lo + bl) + err;
}
// e (1 + d) / (zh + zl) rounded once: the quotient e / zh, its exact remainder, and the first-order terms of d and zl
__device__ __forceinline__ double softmax_quot(double e, double d, double zh, double zl)
{
    const double p0 = e / zh;
    return p0 + (fma(-p0, zh, e) + p0 * fma(d, zh, -zl)) / zh;
}

template <typename T>
__global__ __launch_bounds__(256) void k_transition_prob(const T *__restrict__ corr, const int32_t *__restrict__ ixs,
                                                          const double *__restrict__ emb, int edim, T *__restrict__ tp, T *__restrict__ wdiff,
                                                          double *__restrict__ delta_emb, int64_t cell0, int64_t C_out, int n, double sigma)
{
    const int lane = threadIdx.x & 63;
    const int64_t cl = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (cl >= C_out) return;
    const int64_t c = cell0 + cl;
    const T *crow = corr + cl * n;
    const int32_t *irow = ixs + cl * n;
    double z = 0.0, zl = 0.0;          // the normaliser enters every p: a (hi, lo) pair that keeps the sum's rounding errors
    for (int k = lane; k < n; k += 64) { double d; const double e = exp_quot((double)crow[k], sigma, d); two_sum(z, zl, e, e * d); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) two_sum(z, zl, __shfl_xor(z, off, 64), __shfl_xor(zl, off, 64));   // the same pair in every lane
    double acc[4] = {0, 0, 0, 0};   // edim <= 4
    for (int k = lane; k < n; k += 64) {
        double d;
        const double e = exp_quot((double)crow[k], sigma, d);
        const double p = softmax_quot(e, d, z, zl);
        const int i = irow[k];
        if (tp) tp[cl * n + k] = (T)p;
        if (wdiff) wdiff[cl * n + k] = (T)(p - 1.0 / n);
        double nrm = 0.0, dv[4];
        for (int a = 0; a < edim; ++a) { dv[a] = emb[(int64_t)i * edim + a] - emb[c * edim + a]; nrm += dv[a] * dv[a]; }
        nrm = sqrt(nrm);
        for (int a = 0; a < edim; ++a) {
            const double u = (i == c) ? 0.0 : dv[a] / nrm;
            acc[a] += (p - 1.0 / n) * u;
        }
    }
    for (int a = 0; a < edim; ++a) {
        const double s = wave_sum(acc[a]);
        if (lane == 0) delta_emb[cl * edim + a] = s;
    }
}

// cos_proj[c] = sum_g a[c,g] b[c,g] / sqrt(sum_g b[c,g]^2)   (analysis.py:1717), one wave per cell
template <typename T>
__global__ __launch_bounds__(256) void k_row_cosproj(const T *__restrict__ A, const T *__restrict__ B, double *__restrict__ out, int64_t C,
                                                      int G, int64_t ld)
{
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (c >= C) return;
    const T *a = A + c * ld, *b = B + c * ld;
    double sab = 0, sbb = 0;
    for (int g = lane; g < G; g += 64) { const double x = a[g], y = b[g]; sab = fma(x, y, sab); sbb = fma(y, y, sbb); }
    sab = wave_sum(sab); sbb = wave_sum(sbb);
    if (lane == 0) out[c] = sab / sqrt(sbb);
}

// ---------------------------------------------------------------- fit_gammas weight variants
// The non-default W constructions of VelocytoLoom.fit_gammas (analysis.py:1182-1192, 1208-1219),
// written densely so that vcy_fit_weighted(weight_mode 0) can consume them:
//   mode 0 "sum"            W = S/pa + U/pb                              (pa, pb = 99th percentiles)
//   mode 1 "prod"           W = (S/pa) * (U/pb)
//   mode 2 "maxmin_weighted" R = (clip(S, pa, pb) - pa) / (pb - pa);  W = 0.5 (R^pw + (1-R)^pw)
//   mode 3 "maxmin_double"  W = [Z<=pa | Z>=pb] + [S<=pc | S>=pd],  Z = S/sa + U/sb
template <typename T>
__global__ __launch_bounds__(256) void k_gamma_weights(const T *__restrict__ S, const T *__restrict__ U, T *__restrict__ W,
                                                        const double *__restrict__ pa, const double *__restrict__ pb,
                                                        const double *__restrict__ pc, const double *__restrict__ pd,
                                                        const double *__restrict__ sa, const double *__restrict__ sb, int64_t C, int G,
                                                        int64_t ld, int mode, double pw)
{
    const int64_t total = C * ld;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int g = (int)(t % ld);
        T w = T(0);
        if (g < G) {
            const bool dbl = mode == 3;          // U may be NULL in mode 2; pc, pd, sa, sb belong to mode 3
            w = gamma_weight_element<T>(mode, S[t], mode != 2 ? U[t] : T(0), pa[g], pb[g], dbl ? pc[g] : 0.0, dbl ? pd[g] : 0.0,
                                        dbl ? (T)sa[g] : T(1), dbl ? (T)sb[g] : T(1), pw);
        }
        W[t] = w;
    }
}

static inline int grid_for(int64_t total) { const int64_t b = (total + 255) / 256; return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b)); }
}  // namespace vcy

using namespace vcy;

extern "C" int vcy_row_sums(const void *M, double *out, int64_t C, int64_t G, int64_t ld, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(M && out && C > 0 && G > 0 && ld >= G, "row_sums: bad arguments");
    const unsigned blocks = (unsigned)((C + 3) / 4);
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_row_sums<float>, dim3(blocks), dim3(256), 0, as_stream(stream), (const float *)M, out, C, (int)G, ld);
    else if (dtype == VCY_F64) hipLaunchKernelGGL(k_row_sums<double>, dim3(blocks), dim3(256), 0, as_stream(stream), (const double *)M, out, C, (int)G, ld);
    else return fail(VCY_ERR_INVALID, "%s: bad dtype", "row_sums");
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_scale_log(const void *M, const double *factor, void *out_sz, void *out_norm, int64_t C, int64_t G, int64_t ld,
                             double pcount, int fix_nonfinite, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(M && (out_sz || out_norm) && C > 0 && G > 0 && ld >= G, "scale_log: bad arguments");
    const int blocks = grid_for(C * ld);
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_scale_log<float>, dim3(blocks), dim3(256), 0, as_stream(stream), (const float *)M, factor, (float *)out_sz, (float *)out_norm, C, (int)G, ld, pcount, fix_nonfinite);
    else if (dtype == VCY_F64) hipLaunchKernelGGL(k_scale_log<double>, dim3(blocks), dim3(256), 0, as_stream(stream), (const double *)M, factor, (double *)out_sz, (double *)out_norm, C, (int)G, ld, pcount, fix_nonfinite);
    else return fail(VCY_ERR_INVALID, "%s: bad dtype", "scale_log");
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_delta_transform(const void *hi_dim, const void *delta_S, void *dmat, void *e_out, int64_t C, int64_t G, int64_t ld,
                                   double used_dt, int mode, double psc, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(hi_dim && delta_S && dmat && C > 0 && G > 0 && ld >= G, "delta_transform: bad arguments");
    VCY_REQUIRE(mode >= 0 && mode <= 3 && (mode != 3 || e_out), "delta_transform: bad mode (3 = logratio needs e_out)");
    const int blocks = grid_for(C * ld);
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_delta_transform<float>, dim3(blocks), dim3(256), 0, as_stream(stream), (const float *)hi_dim, (const float *)delta_S, (float *)dmat, (float *)e_out, C, (int)G, ld, (float)used_dt, mode, (float)psc);
    else if (dtype == VCY_F64) hipLaunchKernelGGL(k_delta_transform<double>, dim3(blocks), dim3(256), 0, as_stream(stream), (const double *)hi_dim, (const double *)delta_S, (double *)dmat, (double *)e_out, C, (int)G, ld, used_dt, mode, psc);
    else return fail(VCY_ERR_INVALID, "%s: bad dtype", "delta_transform");
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" size_t vcy_permute_rows_nsign_workspace_bytes(int64_t C, int64_t G, int dtype)
{
    if (C <= 0 || G <= 0) return 0;
    return (size_t)C * (size_t)G * (dtype == VCY_F64 ? 8 : 4);
}

static int permute_rows_nsign(const void *in, void *out, void *workspace_a, void *workspace_b, int64_t C, int64_t G, int64_t ld,
                              int64_t gene0, uint64_t seed, int dtype, vcy_stream stream)
{
    VCY_REQUIRE((workspace_a == nullptr) == (workspace_b == nullptr) && (!workspace_a || (workspace_a != workspace_b && workspace_a != in && workspace_b != in &&
                workspace_a != out && workspace_b != out)), "permute_rows_nsign: the two scratch buffers go together and are distinct from in / out");
    VCY_REQUIRE(in && out && in != out && C > 0 && G > 0 && ld >= G && C < (1ll << 30) && G < 65536ll * 256, "permute_rows_nsign: bad arguments");
    VCY_REQUIRE(dtype == VCY_F32 || dtype == VCY_F64, "permute_rows_nsign: bad dtype");
    int hb = 1;
    while ((1ll << (2 * hb)) < C) ++hb;                      // 4^hb >= C: at most 4 walks per cell on average, 1.3 at 50 000
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    hipStream_t st = as_stream(stream);
    if (workspace_a && G <= 65535) {                          // gene-major route: transpose, shuffle inside the rows, transpose back
        void *A = workspace_a, *B = workspace_b;
        int rc = vcy_transpose(in, A, C, G, ld, C, dtype, dtype, stream);
        if (rc) return rc;
        constexpr int CPT = 4;
        const dim3 grid((unsigned)((C + 256 * CPT - 1) / (256 * CPT)), (unsigned)G);
        if (dtype == VCY_F32) hipLaunchKernelGGL((k_permute_within_gene_rows<float, CPT>), grid, dim3(256), 0, st, (const float *)A, (float *)B, (int)C, lo, hi, hb, gene0);
        else hipLaunchKernelGGL((k_permute_within_gene_rows<double, CPT>), grid, dim3(256), 0, st, (const double *)A, (double *)B, (int)C, lo, hi, hb, gene0);
        VCY_LAUNCH_CHECK();
        return vcy_transpose(B, out, G, C, C, ld, dtype, dtype, stream);
    }
    constexpr int CPT = 8;
    const dim3 grid((unsigned)((ld + 255) / 256), (unsigned)((C + CPT - 1) / CPT));
    if (dtype == VCY_F32) hipLaunchKernelGGL((k_permute_rows_nsign<float, CPT>), grid, dim3(256), 0, st, (const float *)in, (float *)out, (int)C, (int)G, ld, lo, hi, hb, gene0);
    else hipLaunchKernelGGL((k_permute_rows_nsign<double, CPT>), grid, dim3(256), 0, st, (const double *)in, (double *)out, (int)C, (int)G, ld, lo, hi, hb, gene0);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_permute_rows_nsign(const void *in, void *out, void *workspace_a, void *workspace_b, int64_t C, int64_t G, int64_t ld,
                                      uint64_t seed, int dtype, vcy_stream stream)
{
    return permute_rows_nsign(in, out, workspace_a, workspace_b, C, G, ld, 0, seed, dtype, stream);
}

extern "C" int vcy_permute_rows_nsign_genes(const void *in, void *out, void *workspace_a, void *workspace_b, int64_t C, int64_t G, int64_t ld,
                                            int64_t gene0, uint64_t seed, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(gene0 >= 0 && gene0 + G <= 65536ll * 256, "permute_rows_nsign_genes: bad gene offset");
    return permute_rows_nsign(in, out, workspace_a, workspace_b, C, G, ld, gene0, seed, dtype, stream);
}

extern "C" int vcy_corr_fixup(void *vals, const int32_t *ixs, int64_t cell0, int64_t C_out, int64_t nrndm, int zero_self, int fix_nan,
                              double nan_to, int *nan_count, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(vals && ixs && C_out > 0 && nrndm > 0, "corr_fixup: bad arguments");
    const int64_t total = C_out * nrndm;
    const int blocks = grid_for(total);
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_corr_fixup<float>, dim3(blocks), dim3(256), 0, as_stream(stream), (float *)vals, ixs, cell0, total, (int)nrndm, zero_self, fix_nan, (float)nan_to, nan_count);
    else if (dtype == VCY_F64) hipLaunchKernelGGL(k_corr_fixup<double>, dim3(blocks), dim3(256), 0, as_stream(stream), (double *)vals, ixs, cell0, total, (int)nrndm, zero_self, fix_nan, nan_to, nan_count);
    else return fail(VCY_ERR_INVALID, "%s: bad dtype", "corr_fixup");
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_transition_prob(const void *corr, const int32_t *ixs, const double *embedding, int edim, void *tp, void *wdiff,
                                   double *delta_embedding, int64_t cell0, int64_t C_out, int64_t n, double sigma_corr, int dtype,
                                   vcy_stream stream)
{
    VCY_REQUIRE(corr && ixs && embedding && delta_embedding && C_out > 0 && n > 0 && edim > 0 && edim <= 4 && sigma_corr > 0, "transition_prob: bad arguments");
    const unsigned blocks = (unsigned)((C_out + 3) / 4);
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_transition_prob<float>, dim3(blocks), dim3(256), 0, as_stream(stream), (const float *)corr, ixs, embedding, edim, (float *)tp, (float *)wdiff, delta_embedding, cell0, C_out, (int)n, sigma_corr);
    else if (dtype == VCY_F64) hipLaunchKernelGGL(k_transition_prob<double>, dim3(blocks), dim3(256), 0, as_stream(stream), (const double *)corr, ixs, embedding, edim, (double *)tp, (double *)wdiff, delta_embedding, cell0, C_out, (int)n, sigma_corr);
    else return fail(VCY_ERR_INVALID, "%s: bad dtype", "transition_prob");
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_row_cosproj(const void *A, const void *B, double *out, int64_t C, int64_t G, int64_t ld, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(A && B && out && C > 0 && G > 0 && ld >= G, "row_cosproj: bad arguments");
    const unsigned blocks = (unsigned)((C + 3) / 4);
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_row_cosproj<float>, dim3(blocks), dim3(256), 0, as_stream(stream), (const float *)A, (const float *)B, out, C, (int)G, ld);
    else if (dtype == VCY_F64) hipLaunchKernelGGL(k_row_cosproj<double>, dim3(blocks), dim3(256), 0, as_stream(stream), (const double *)A, (const double *)B, out, C, (int)G, ld);
    else return fail(VCY_ERR_INVALID, "%s: bad dtype", "row_cosproj");
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_gamma_weights(const void *S, const void *U, void *W, const double *pa, const double *pb, const double *pc,
                                 const double *pd, const double *sa, const double *sb, int64_t C, int64_t G, int64_t ld, int mode,
                                 double power, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(S && W && pa && pb && C > 0 && G > 0 && ld >= G && mode >= 0 && mode <= 3, "gamma_weights: bad arguments");
    VCY_REQUIRE(mode == 2 || U, "gamma_weights: U needed");
    VCY_REQUIRE(mode != 3 || (pc && pd && sa && sb), "gamma_weights: maxmin_double needs pc, pd, sa, sb");
    const int blocks = grid_for(C * ld);
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_gamma_weights<float>, dim3(blocks), dim3(256), 0, as_stream(stream), (const float *)S, (const float *)U, (float *)W, pa, pb, pc, pd, sa, sb, C, (int)G, ld, mode, power);
    else if (dtype == VCY_F64) hipLaunchKernelGGL(k_gamma_weights<double>, dim3(blocks), dim3(256), 0, as_stream(stream), (const double *)S, (const double *)U, (double *)W, pa, pb, pc, pd, sa, sb, C, (int)G, ld, mode, power);
    else return fail(VCY_ERR_INVALID, "%s: bad dtype", "gamma_weights");
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}
