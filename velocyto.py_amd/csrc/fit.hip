// fit.hip -- stage B: per-gene gamma fits and the per-gene order statistics behind their weights.
//
// Reference: estimation.fit_slope* / _fit1_slope* (estimation.py:173-366) loop over genes in
// Python and call scipy optimisers on each gene's (C,) vectors; VelocytoLoom.fit_gammas
// (analysis.py:1179-1219) builds the weights from np.percentile(axis=1).
// Here a gene is a COLUMN of the cells-major matrices.  One streaming pass accumulates all
// per-gene moments (fp64) for a block of cells per workgroup, lanes mapped to adjacent genes so
// every load is a coalesced row segment; a second tiny kernel reduces the per-block partials in
// a fixed order (deterministic, no atomics) and solves each gene's least-squares problem in
// closed form -- the problems the reference hands to nnls / Brent / L-BFGS-B are 1- or
// 2-parameter convex quadratics over a box.  HBM-bound: 2 * G * s bytes per cell (plain fit).
#include <math.h>
#include <algorithm>
#include "common.h"

namespace vcy {

constexpr int FIT_CB = 32;        // cell blocks (partials per gene)
constexpr int FIT_NMOM = 10;      // Sx Sy Sxx Sxy Syy | Sw Swx Swy Swxx Swxy

// ---------------------------------------------------------------- plain fit_slope moments
// thread = one 16-byte gene vector; block = 256 threads; grid = (gene tiles, FIT_CB).
template <typename T>
__global__ __launch_bounds__(256) void k_moments_plain(const T *__restrict__ Y, const T *__restrict__ X, double *__restrict__ part,
                                                        int C, int G, int64_t ld)
{
    using V = typename Vec<T>::type;
    constexpr int N = Vec<T>::N;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;   // vector index along genes
    const int g = v * N;
    if (g >= G) return;
    const int cb = blockIdx.y;
    const int per = (C + FIT_CB - 1) / FIT_CB;
    const int c0 = cb * per, c1 = min(C, c0 + per);
    double sxx[N], sxy[N], syy[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { sxx[k] = 0; sxy[k] = 0; syy[k] = 0; }
    int c = c0;
    for (; c + 3 < c1; c += 4) {
        V xv[4], yv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            xv[u] = reinterpret_cast<const V *>(X + (int64_t)(c + u) * ld)[v];
            yv[u] = reinterpret_cast<const V *>(Y + (int64_t)(c + u) * ld)[v];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const T *xp = reinterpret_cast<const T *>(&xv[u]);
            const T *yp = reinterpret_cast<const T *>(&yv[u]);
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const double x = xp[k], y = yp[k];
                sxx[k] = fma(x, x, sxx[k]); sxy[k] = fma(x, y, sxy[k]); syy[k] = fma(y, y, syy[k]);
            }
        }
    }
    for (; c < c1; ++c) {
        const V xv = reinterpret_cast<const V *>(X + (int64_t)c * ld)[v];
        const V yv = reinterpret_cast<const V *>(Y + (int64_t)c * ld)[v];
        const T *xp = reinterpret_cast<const T *>(&xv);
        const T *yp = reinterpret_cast<const T *>(&yv);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double x = xp[k], y = yp[k];
            sxx[k] = fma(x, x, sxx[k]); sxy[k] = fma(x, y, sxy[k]); syy[k] = fma(y, y, syy[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (g + k < G) {
            double *p = part + ((int64_t)cb * 3) * G + g + k;
            p[0] = sxx[k]; p[(int64_t)G] = sxy[k]; p[2 * (int64_t)G] = syy[k];
        }
    }
}

// fixed-order reduction of the FIT_CB per-block partials -> moments (3, G)
__global__ void k_fit_slope_reduce(const double *__restrict__ part, double *__restrict__ mom, int G)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double sxx = 0, sxy = 0, syy = 0;
    for (int cb = 0; cb < FIT_CB; ++cb) {
        const double *p = part + ((int64_t)cb * 3) * G + g;
        sxx += p[0]; sxy += p[(int64_t)G]; syy += p[2 * (int64_t)G];
    }
    mom[g] = sxx; mom[(int64_t)G + g] = sxy; mom[2 * (int64_t)G + g] = syy;
}

// estimation.py:173-188: not any(x) -> NaN; not any(y) -> 0; else nnls == max(0, <x,y>/<x,x>).
__global__ void k_fit_slope_final(const double *__restrict__ mom, float *__restrict__ gamma, int G)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const double sxx = mom[g], sxy = mom[(int64_t)G + g], syy = mom[2 * (int64_t)G + g];
    double m;
    if (!(sxx > 0)) m = NAN;
    else if (!(syy > 0)) m = 0.0;
    else { m = sxy / sxx; if (m < 0) m = 0; }
    gamma[g] = (float)m;
}

// ---------------------------------------------------------------- weighted moments
// Z value used by the "maxmin*" weights (analysis.py:1203-1206): evaluated in T so that the
// thresholds (k_gene_quantiles) and the weights (here) see bit-identical numbers.
template <typename T> __device__ __forceinline__ T zvalue(T m, T m2, T a, T b, bool two)
{
    return two ? (m / a + m2 / b) : m;   // true divisions, like Sx/denom_Sx + Ux/denom_Ux
}

// CM: cells with cmask[c] == 0 add nothing and are not read (the steady-state cells of fit_gammas); the kept cells are summed in
// the order the unmasked kernel sums them, so an all-ones mask gives its moments bit for bit.
// WMODE 3..6: the fused weights, gamma_weight_element's modes 0..3 ("sum", "prod", "maxmin_weighted", "maxmin_double") evaluated in
// the fold - no dense W.  The arguments then carry that function's: M = S, M2 = U (not read in mode 2), down = pa, up = pb,
// scale_a = sa, scale_b = sb, and pc, pd, pw.
constexpr int WMODE_FUSED = 3;
template <typename T, int WMODE, bool CM>
__device__ __forceinline__ void moments_weighted_body(const T *__restrict__ Y, const T *__restrict__ X, const T *__restrict__ W,
                                                      const T *__restrict__ M, const T *__restrict__ M2,
                                                      const double *__restrict__ scale_a, const double *__restrict__ scale_b,
                                                      const double *__restrict__ down, const double *__restrict__ up,
                                                      double *__restrict__ part, int C, int G, int64_t ld,
                                                      const unsigned char *__restrict__ cmask, const double *__restrict__ pc = nullptr,
                                                      const double *__restrict__ pd = nullptr, double pw = 0.0)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;   // lane <-> gene: coalesced 4/8-byte row segments
    if (g >= G) return;
    const int cb = blockIdx.y;
    const int per = (C + FIT_CB - 1) / FIT_CB;
    const int c0 = cb * per, c1 = min(C, c0 + per);
    const bool two = (WMODE == 1) && scale_a != nullptr;
    T den_a = T(1), den_b = T(1);
    double dn = 0, upv = 0;        // thresholds stay fp64: compared against (double)z like the reference's X <= down
    if (WMODE == 1) {
        if (two) { den_a = (T)scale_a[g]; den_b = (T)scale_b[g]; }
        dn = down[g]; upv = up[g];
    }
    constexpr int FM = WMODE - WMODE_FUSED;      // the fused weight's mode and its per-gene values
    double fpc = 0, fpd = 0;
    if (WMODE >= WMODE_FUSED) {
        dn = down[g]; upv = up[g];
        if (FM == 3) { fpc = pc[g]; fpd = pd[g]; den_a = (T)scale_a[g]; den_b = (T)scale_b[g]; }
    }
    double sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0, sw = 0, swx = 0, swy = 0, swxx = 0, swxy = 0;
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {
        if (CM && cmask[c] == 0) continue;   // the same for every lane: the row is skipped whole
        const int64_t o = (int64_t)c * ld + g;
        const double x = X[o], y = Y[o];
        double w;
        if (WMODE == 0) w = W[o];
        else if (WMODE == 1) {
            const double z = (double)zvalue<T>(M[o], two ? M2[o] : T(0), den_a, den_b, two);
            w = (z <= dn || z >= upv) ? 1.0 : 0.0;
        } else if (WMODE >= WMODE_FUSED) {
            w = (double)gamma_weight_element<T>(FM, M[o], FM != 2 ? M2[o] : T(0), dn, upv, fpc, fpd, den_a, den_b, pw);
        } else w = 1.0;
        sx += x; sy += y; sxx = fma(x, x, sxx); sxy = fma(x, y, sxy); syy = fma(y, y, syy);
        const double wx = w * x;
        sw += w; swx += wx; swy = fma(w, y, swy); swxx = fma(wx, x, swxx); swxy = fma(wx, y, swxy);
    }
    double *p = part + ((int64_t)cb * FIT_NMOM) * G + g;
    const int64_t s = G;
    p[0] = sx; p[s] = sy; p[2 * s] = sxx; p[3 * s] = sxy; p[4 * s] = syy;
    p[5 * s] = sw; p[6 * s] = swx; p[7 * s] = swy; p[8 * s] = swxx; p[9 * s] = swxy;
}

template <typename T, int WMODE>
__global__ __launch_bounds__(256) void k_moments_weighted(const T *__restrict__ Y, const T *__restrict__ X, const T *__restrict__ W,
                                                           const T *__restrict__ M, const T *__restrict__ M2,
                                                           const double *__restrict__ scale_a, const double *__restrict__ scale_b,
                                                           const double *__restrict__ down, const double *__restrict__ up,
                                                           double *__restrict__ part, int C, int G, int64_t ld)
{
    moments_weighted_body<T, WMODE, false>(Y, X, W, M, M2, scale_a, scale_b, down, up, part, C, G, ld, nullptr);
}

template <typename T, int WMODE>
__global__ __launch_bounds__(256) void k_moments_weighted_masked(const T *__restrict__ Y, const T *__restrict__ X, const T *__restrict__ W,
                                                                  const T *__restrict__ M, const T *__restrict__ M2,
                                                                  const double *__restrict__ scale_a, const double *__restrict__ scale_b,
                                                                  const double *__restrict__ down, const double *__restrict__ up,
                                                                  double *__restrict__ part, int C, int G, int64_t ld,
                                                                  const unsigned char *__restrict__ cmask)
{
    moments_weighted_body<T, WMODE, true>(Y, X, W, M, M2, scale_a, scale_b, down, up, part, C, G, ld, cmask);
}

template <typename T, int FM, bool CM>
__global__ __launch_bounds__(256) void k_moments_fused(const T *__restrict__ Y, const T *__restrict__ X, const T *__restrict__ S,
                                                        const T *__restrict__ U, const double *__restrict__ pa, const double *__restrict__ pb,
                                                        const double *__restrict__ pc, const double *__restrict__ pd,
                                                        const double *__restrict__ sa, const double *__restrict__ sb, double pw,
                                                        double *__restrict__ part, int C, int G, int64_t ld,
                                                        const unsigned char *__restrict__ cmask)
{
    moments_weighted_body<T, WMODE_FUSED + FM, CM>(Y, X, nullptr, S, U, sa, sb, pa, pb, part, C, G, ld, cmask, pc, pd, pw);
}

// Exact minimiser of  sum w (x m + q - y)^2  over [lo_m,hi_m] x [lo_q,hi_q] from the weighted
// moments: interior stationary point if feasible, else the best clipped edge minimum (convex).
__device__ inline void box_wls2(double sw, double sx, double sy, double sxx, double sxy, double lo_m, double hi_m,
                                double lo_q, double hi_q, double &m_out, double &q_out)
{
    auto f = [&](double m, double q) { return m * m * sxx + q * q * sw + 2 * m * q * sx - 2 * m * sxy - 2 * q * sy; };
    const double det = sxx * sw - sx * sx;
    if (det > 0) {
        const double m = (sxy * sw - sx * sy) / det, q = (sxx * sy - sx * sxy) / det;
        if (m >= lo_m && m <= hi_m && q >= lo_q && q <= hi_q) { m_out = m; q_out = q; return; }
    }
    double best = INFINITY;
    const double qs[2] = {lo_q, hi_q}, ms[2] = {lo_m, hi_m};
    for (int t = 0; t < 2; ++t) {
        const double q = qs[t];
        double m = sxx > 0 ? (sxy - q * sx) / sxx : lo_m;
        m = fmin(fmax(m, lo_m), hi_m);
        const double v = f(m, q);
        if (v < best) { best = v; m_out = m; q_out = q; }
    }
    for (int t = 0; t < 2; ++t) {
        const double m = ms[t];
        double q = sw > 0 ? (sy - m * sx) / sw : lo_q;
        q = fmin(fmax(q, lo_q), hi_q);
        const double v = f(m, q);
        if (v < best) { best = v; m_out = m; q_out = q; }
    }
}

// fit_offset=1, box_q=1 : _fit1_slope_weighted_offset (estimation.py:212-241), bounds
//                          gamma in [lo_gamma, up_gamma], q in [0, 2*sum(yw)/sum(w)]
// fit_offset=1, box_q=0 : _fit1_slope_offset (estimation.py:244-264) unconstrained OLS with intercept
// fit_offset=0          : _fit1_slope_weighted (estimation.py:191-209) / fixperc_q branches: gamma in
//                          [lo_gamma, up_gamma] with the offset fixed to q_fixed[g]
// R2 (estimation.py:323-331, 355-363) is unweighted, -1e16 when non-finite.
// The solve of one gene from its ten reduced moments over n cells (shared by the one-pass and the two-step forms below).
__device__ __forceinline__ void fit_weighted_solve(const double *mo, double n, int g, int fit_offset, int box_q, double lo_gamma,
                                                   double up_gamma_default, const double *__restrict__ up_gamma,
                                                   const double *__restrict__ q_fixed, float *__restrict__ gamma, float *__restrict__ qout,
                                                   float *__restrict__ R2)
{
    const double sx = mo[0], sy = mo[1], sxx = mo[2], sxy = mo[3], syy = mo[4];
    const double sw = mo[5], swx = mo[6], swy = mo[7], swxx = mo[8], swxy = mo[9];
    const double hi = up_gamma ? up_gamma[g] : up_gamma_default;
    double m, q;
    if (!(sxx > 0)) { m = NAN; q = 0.0; }
    else if (!(syy > 0)) { m = 0.0; q = 0.0; }
    else if (fit_offset) {
        if (box_q) box_wls2(sw, swx, swy, swxx, swxy, lo_gamma, hi, 0.0, 2.0 * swy / sw, m, q);
        else {
            const double det = swxx * sw - swx * swx;
            m = (swxy * sw - swx * swy) / det;
            q = (swy - m * swx) / sw;
        }
    } else {
        q = q_fixed ? q_fixed[g] : 0.0;
        m = swxx > 0 ? (swxy - q * swx) / swxx : lo_gamma;
        m = fmin(fmax(m, lo_gamma), hi);
    }
    gamma[g] = (float)m;
    if (qout) qout[g] = (float)q;
    if (R2) {
        // the reference evaluates R2 with the optimiser's fp64 (m, q), before the float32 store (estimation.py:351-359)
        const double ssres = m * m * sxx + n * q * q + syy + 2 * m * q * sx - 2 * m * sxy - 2 * q * sy;
        const double sstot = syy - sy * sy / n;
        const double r2 = 1.0 - ssres / sstot;
        R2[g] = isfinite(r2) ? (float)r2 : -1e16f;
    }
}

// the per-block partials summed in block order, then solved
__device__ __forceinline__ void fold_partials(const double *__restrict__ part, int G, int g, double *mo)
{
    for (int k = 0; k < FIT_NMOM; ++k) mo[k] = 0;
    for (int cb = 0; cb < FIT_CB; ++cb)
        for (int k = 0; k < FIT_NMOM; ++k) mo[k] += part[((int64_t)cb * FIT_NMOM + k) * G + g];
}

__global__ void k_fit_weighted_final(const double *__restrict__ part, int fit_offset, int box_q, double lo_gamma,
                                     double up_gamma_default, const double *__restrict__ up_gamma, const double *__restrict__ q_fixed,
                                     float *__restrict__ gamma, float *__restrict__ qout, float *__restrict__ R2, int C, int G)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double mo[FIT_NMOM];
    fold_partials(part, G, g, mo);
    fit_weighted_solve(mo, (double)C, g, fit_offset, box_q, lo_gamma, up_gamma_default, up_gamma, q_fixed, gamma, qout, R2);
}

// two-step form (cell-sharded fits): the folded moments (FIT_NMOM, G) of a block of cells ...
__global__ void k_fit_weighted_fold(const double *__restrict__ part, double *__restrict__ mom, int G)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double mo[FIT_NMOM];
    fold_partials(part, G, g, mo);
    for (int k = 0; k < FIT_NMOM; ++k) mom[(int64_t)k * G + g] = mo[k];
}

// ... and the solve from moments summed over all blocks (n = the number of cells they cover)
__global__ void k_fit_weighted_from_moments(const double *__restrict__ mom, double n, int fit_offset, int box_q, double lo_gamma,
                                            double up_gamma_default, const double *__restrict__ up_gamma, const double *__restrict__ q_fixed,
                                            float *__restrict__ gamma, float *__restrict__ qout, float *__restrict__ R2, int G)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double mo[FIT_NMOM];
    for (int k = 0; k < FIT_NMOM; ++k) mo[k] = mom[(int64_t)k * G + g];
    fit_weighted_solve(mo, n, g, fit_offset, box_q, lo_gamma, up_gamma_default, up_gamma, q_fixed, gamma, qout, R2);
}

// ---------------------------------------------------------------- per-gene order statistics
// Step 1: gene-major key matrix Z (G, C): 64x64 LDS tile transpose of zvalue(M, M2).
// Optional mask (conditional percentiles of estimation.py:200-202, 222, 229-231, 255):
//   mask_mode 1 keeps cells with mask_src[c,g] >  mask_thr[g]   (y[x > percentile(x, 90)])
//   mask_mode 2 keeps cells with mask_src[c,g] <= mask_thr[g]   (y[x <= percentile(x, 1)])
// masked-out entries become +inf, sort last, and are not counted by k_gene_quantiles.
template <typename T>
__global__ __launch_bounds__(256) void k_build_z(const T *__restrict__ M, const T *__restrict__ M2, const double *__restrict__ scale_a,
                                                  const double *__restrict__ scale_b, const T *__restrict__ mask_src,
                                                  const double *__restrict__ mask_thr, int mask_mode, T *__restrict__ Z, int C, int G,
                                                  int64_t ld)
{
    __shared__ T tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c0 = blockIdx.y * 64, g0 = blockIdx.x * 64;
    const bool two = scale_a != nullptr;
    const int g = g0 + tx;
    T den_a = T(1), den_b = T(1);
    if (two && g < G) { den_a = (T)scale_a[g]; den_b = (T)scale_b[g]; }
    for (int j = ty; j < 64; j += 4) {
        const int c = c0 + j;
        T z = T(0);
        if (c < C && g < G) {
            const int64_t o = (int64_t)c * ld + g;
            z = zvalue<T>(M[o], two ? M2[o] : T(0), den_a, den_b, two);
            if (mask_mode) {
                const double mv = (double)mask_src[o], th = mask_thr[g];
                const bool keep = mask_mode == 1 ? (mv > th) : (mv <= th);
                if (!keep) z = (T)INFINITY;
            }
        }
        tile[j][tx] = z;
    }
    __syncthreads();
    for (int j = ty; j < 64; j += 4) {
        const int gg = g0 + j, cc = c0 + tx;
        if (gg < G && cc < C) Z[(int64_t)gg * C + cc] = tile[tx][j];
    }
}

struct QArgs { double q[16]; };   // percentiles travel as kernel arguments (no host->device copy)

template <typename T> struct Key;
template <> struct Key<float> {
    using U = uint32_t;
    static __device__ __forceinline__ U enc(float f) { U u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
    static __device__ __forceinline__ float dec(U u) { u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u; return __uint_as_float(u); }
};
template <> struct Key<double> {
    using U = uint64_t;
    static __device__ __forceinline__ U enc(double f) { U u = (U)__double_as_longlong(f); return (u >> 63) ? ~u : (u | 0x8000000000000000ull); }
    static __device__ __forceinline__ double dec(U u) { u = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u; return __longlong_as_double((long long)u); }
};

// lerp_numpy (common.h): numpy's _lerp between two order statistics, shared by every percentile kernel of the library.

// One histogram increment per matching lane.  Expression rows are mostly exact zeros and a row's values share a few exponents, so the
// lanes of a wave mostly ask for the SAME bin - and LDS atomics on one address serialise, 64 deep when a whole wave holds zeros (the 2nd
// percentile of a 60 %-zero matrix cost twice the 98th).  The lanes that share the first matching lane's digit are therefore folded
// into one atomic carrying their count (VCY_QPEEL rounds of it); only the lanes left over add one each.
#ifndef VCY_QPEEL
#define VCY_QPEEL 1
#endif
__device__ __forceinline__ void hist_add(unsigned *hist, unsigned bin, bool match)
{
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int round = 0; round < VCY_QPEEL; ++round) {
        const unsigned long long m = __ballot(match);
        if (m == 0) return;
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
        const unsigned lead_bin = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);
        const bool same = match && bin == lead_bin;
        const unsigned long long ms = __ballot(same);
        if (lane == leader) atomicAdd(&hist[lead_bin], (unsigned)__popcll(ms));
        match = match && !same;
    }
    if (match) atomicAdd(&hist[bin], 1u);
}

// Step 2: one workgroup per gene: MSB-first 8-bit radix select of rank `r` over the gene's C keys
// (sizeof(key) passes, 256-bin LDS histogram; the row is L2-resident after the first pass), then one
// more pass for the next order statistic (count <= v, min > v).  numpy.percentile's default
// 'linear' rule: h = (C-1) q/100, lo = floor(h), t = h - lo,
//   t < 0.5 ? v[lo] + (v[lo+1]-v[lo]) t : v[lo+1] - (v[lo+1]-v[lo]) (1-t)      (numpy _lerp)
template <typename T>
__global__ __launch_bounds__(256) void k_gene_quantiles(const T *__restrict__ Z, QArgs qa, int nq,
                                                         double *__restrict__ out, int C, int G, int masked)
{
    using U = typename Key<T>::U;
    constexpr int PASSES = sizeof(U);
    __shared__ unsigned hist[256];
    __shared__ U s_prefix;
    __shared__ unsigned s_rank;
    __shared__ unsigned s_cnt_le;
    __shared__ unsigned long long s_min_gt;
    const int g = blockIdx.x, tid = threadIdx.x;
    const T *row = Z + (int64_t)g * C;
    int nvalid = C;
    if (masked) {   // entries removed by the mask were stored as +inf
        if (tid == 0) s_cnt_le = 0;
        __syncthreads();
        unsigned cnt = 0;
        for (int c = tid; c < C; c += 256) cnt += (row[c] < (T)INFINITY) ? 1u : 0u;
        cnt = wave_sum(cnt);
        if ((tid & 63) == 0) atomicAdd(&s_cnt_le, cnt);
        __syncthreads();
        nvalid = (int)s_cnt_le;
        __syncthreads();
    }
    for (int qi = 0; qi < nq; ++qi) {
        if (nvalid == 0) { if (tid == 0) out[(int64_t)qi * G + g] = NAN; continue; }
        const double h = __dmul_rn((double)(nvalid - 1), qa.q[qi] / 100.0);   // numpy: (n-1) * (q/100)
        const int lo = (int)floor(h);
        const double t = h - lo;
        U prefix = 0;
        unsigned rank = (unsigned)lo;   // 0-based rank among elements matching the prefix so far
        for (int pass = 0; pass < PASSES; ++pass) {
            const int shift = 8 * (PASSES - 1 - pass);
            hist[tid] = 0;
            __syncthreads();
            for (int c = tid; c < C; c += 256) {
                const U k = Key<T>::enc(row[c]);
                const bool match = (pass == 0) || ((k >> ((shift + 8) & (8 * PASSES - 1))) == (prefix >> ((shift + 8) & (8 * PASSES - 1))));
                hist_add(hist, (unsigned)((k >> shift) & 0xff), match);
            }
            __syncthreads();
            if (tid < 64) {   // one wave scans the 256 bins: 4 bins per lane
                unsigned h0 = hist[tid * 4], h1 = hist[tid * 4 + 1], h2 = hist[tid * 4 + 2], h3 = hist[tid * 4 + 3];
                unsigned tot = h0 + h1 + h2 + h3, incl = tot;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    unsigned o = __shfl_up(incl, off, 64);
                    if (tid >= off) incl += o;
                }
                const unsigned excl = incl - tot;
                if (rank >= excl && rank < incl) {   // exactly one lane
                    unsigned r = rank - excl;
                    int d;
                    if (r < h0) d = 0;
                    else if ((r -= h0) < h1) d = 1;
                    else if ((r -= h1) < h2) d = 2;
                    else { r -= h2; d = 3; }
                    s_prefix = prefix | ((U)(tid * 4 + d) << shift);
                    s_rank = r;
                }
            }
            __syncthreads();
            prefix = s_prefix;
            rank = s_rank;
        }
        const T vlo = Key<T>::dec(prefix);
        // next order statistic
        if (tid == 0) { s_cnt_le = 0; s_min_gt = ~0ull; }
        __syncthreads();
        unsigned cnt = 0;
        unsigned long long mg = ~0ull;
        for (int c = tid; c < C; c += 256) {
            const U k = Key<T>::enc(row[c]);
            if (k <= prefix) ++cnt;
            else if ((unsigned long long)k < mg) mg = (unsigned long long)k;
        }
        cnt = wave_sum(cnt);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(mg, off, 64);
            mg = o < mg ? o : mg;
        }
        if ((tid & 63) == 0) { atomicAdd(&s_cnt_le, cnt); atomicMin(&s_min_gt, mg); }
        __syncthreads();
        if (tid == 0) {
            T vhi = vlo;
            if (lo + 1 < nvalid && s_cnt_le < (unsigned)(lo + 2)) vhi = Key<T>::dec((U)s_min_gt);
            out[(int64_t)qi * G + g] = lerp_numpy((double)vlo, (double)vhi, t);
        }
        __syncthreads();
    }
}

// Step 2, register-resident (round 3): the same selection with the gene's C keys held in the REGISTERS of a 1024-thread workgroup
// (NPT keys per thread, C <= 1024 NPT).  k_gene_quantiles re-reads the 200 KB row of a gene from memory on every radix pass - ten
// passes for two percentiles, and 2048 co-resident rows are 400 MB, far beyond L2: 60 GB of re-reads for a 6 GB matrix, 17 ms at
// 50 000 x 30 000.  Here the row is read ONCE (coalesced: thread t takes elements t, t + 1024, ...), every pass walks registers;
// histograms, scans and the interpolation are the ones of k_gene_quantiles, so the results are the same to the bit.
template <typename T, int NPT>
__global__ __launch_bounds__(1024) void k_gene_quantiles_reg(const T *__restrict__ Z, QArgs qa, int nq,
                                                              double *__restrict__ out, int C, int G, int masked)
{
    using U = typename Key<T>::U;
    constexpr int PASSES = sizeof(U);
    constexpr U KMAX = ~(U)0;                                // padding key: sorts last, never reaches a rank < nvalid
    constexpr int COPIES = 32, CSTRIDE = 257;                // lane l counts in copy l % 32; copy c starts at bank c, so equal digits of
    __shared__ unsigned hcopy[COPIES * CSTRIDE];             // different lanes fall in different banks (two lanes per word at worst)
    __shared__ unsigned hist[256];                           // the copies folded
    __shared__ unsigned hist0[256];                          // ... of the first digit: the same for every percentile
    __shared__ U s_prefix;
    __shared__ unsigned s_rank;
    __shared__ unsigned s_cnt_le;
    __shared__ unsigned long long s_min_gt;
    const int g = blockIdx.x, tid = threadIdx.x;
    const T *row = Z + (int64_t)g * C;
    U key[NPT];
    unsigned nfin = 0;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        // branch-free (a load inside a branch makes hipcc wait for it inside the branch: NPT serialised round trips)
        const int c = tid + 1024 * i;
        const T v = row[c < C ? c : C - 1];
        key[i] = c < C ? Key<T>::enc(v) : KMAX;
        nfin += (c < C && v < (T)INFINITY) ? 1u : 0u;
    }
    for (int i = tid; i < COPIES * CSTRIDE; i += 1024) hcopy[i] = 0;
    if (tid < 256) hist[tid] = 0;
    if (tid == 0) s_cnt_le = 0;
    __syncthreads();
    int nvalid = C;
    if (masked) {   // entries removed by the mask were stored as +inf
        const unsigned cnt = wave_sum(nfin);
        if ((tid & 63) == 0) atomicAdd(&s_cnt_le, cnt);
        __syncthreads();
        nvalid = (int)s_cnt_le;
        __syncthreads();
    }
    unsigned *mine = hcopy + (tid & (COPIES - 1)) * CSTRIDE;
    for (int qi = 0; qi < nq; ++qi) {
        if (nvalid == 0) { if (tid == 0) out[(int64_t)qi * G + g] = NAN; continue; }
        const double h = __dmul_rn((double)(nvalid - 1), qa.q[qi] / 100.0);   // numpy: (n-1) * (q/100)
        const int lo = (int)floor(h);
        const double t = h - lo;
        U prefix = 0;
        unsigned rank = (unsigned)lo;
        // (the pass loop stays rolled: unrolled, hipcc hoists every key's digit of every pass out of the percentile loop -
        // PASSES x NPT more live registers, kilobytes of scratch)
#pragma unroll 1
        for (int pass = 0; pass < PASSES; ++pass) {
            const int shift = 8 * (PASSES - 1 - pass);
            const bool counted = pass == 0 && qi > 0;      // the first digit's histogram is kept from the first percentile
            if (!counted) {
#pragma unroll
                for (int i = 0; i < NPT; ++i) {
                    // (padding keys are counted too: they sit above every real key, and the rank looked for is below the real count)
                    const U k = key[i];
                    const bool match = (pass == 0) || ((k >> ((shift + 8) & (8 * PASSES - 1))) == (prefix >> ((shift + 8) & (8 * PASSES - 1))));
                    if (match) atomicAdd(&mine[(unsigned)((k >> shift) & 0xff)], 1u);
                }
                __syncthreads();
                {   // fold the copies (and leave them zero for the next pass): thread = (bin, quarter of the copies)
                    const int bin = tid & 255, part = tid >> 8;
                    unsigned sum = 0;
#pragma unroll
                    for (int c = 0; c < COPIES / 4; ++c) {
                        unsigned *w = hcopy + (part * (COPIES / 4) + c) * CSTRIDE + bin;
                        sum += *w;
                        *w = 0;
                    }
                    if (sum) atomicAdd(&hist[bin], sum);
                }
                __syncthreads();
            }
            if (tid < 64) {   // one wave scans the 256 bins: 4 bins per lane
                const unsigned *hsrc = counted ? hist0 : hist;
                unsigned h0 = hsrc[tid * 4], h1 = hsrc[tid * 4 + 1], h2 = hsrc[tid * 4 + 2], h3 = hsrc[tid * 4 + 3];
                if (!counted) {
                    if (pass == 0) { hist0[tid * 4] = h0; hist0[tid * 4 + 1] = h1; hist0[tid * 4 + 2] = h2; hist0[tid * 4 + 3] = h3; }
                    hist[tid * 4] = 0; hist[tid * 4 + 1] = 0; hist[tid * 4 + 2] = 0; hist[tid * 4 + 3] = 0;
                }
                unsigned tot = h0 + h1 + h2 + h3, incl = tot;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    unsigned o = __shfl_up(incl, off, 64);
                    if (tid >= off) incl += o;
                }
                const unsigned excl = incl - tot;
                if (rank >= excl && rank < incl) {   // exactly one lane
                    unsigned r = rank - excl;
                    int d;
                    if (r < h0) d = 0;
                    else if ((r -= h0) < h1) d = 1;
                    else if ((r -= h1) < h2) d = 2;
                    else { r -= h2; d = 3; }
                    s_prefix = prefix | ((U)(tid * 4 + d) << shift);
                    s_rank = r;
                }
            }
            __syncthreads();
            prefix = s_prefix;
            rank = s_rank;
        }
        const T vlo = Key<T>::dec(prefix);
        // next order statistic
        if (tid == 0) { s_cnt_le = 0; s_min_gt = ~0ull; }
        __syncthreads();
        unsigned cnt = 0;
        unsigned long long mg = ~0ull;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const U k = key[i];   // a padding key can only be counted when the answer is NaN anyway, or be the minimum when it is not used
            if (k <= prefix) ++cnt;
            else if ((unsigned long long)k < mg) mg = (unsigned long long)k;
        }
        cnt = wave_sum(cnt);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(mg, off, 64);
            mg = o < mg ? o : mg;
        }
        if ((tid & 63) == 0) { atomicAdd(&s_cnt_le, cnt); atomicMin(&s_min_gt, mg); }
        __syncthreads();
        if (tid == 0) {
            T vhi = vlo;
            if (lo + 1 < nvalid && s_cnt_le < (unsigned)(lo + 2)) vhi = Key<T>::dec((U)s_min_gt);
            out[(int64_t)qi * G + g] = lerp_numpy((double)vlo, (double)vhi, t);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- streamed per-gene order statistics
// The same exact selection for a matrix that is only ever seen as a sequence of cell blocks (the atlas path): memory O(genes).
// A TARGET is one rank of one gene's sorted column; per (target, gene) the state is the key prefix fixed so far and the rank
// left among the keys that share it.  One digit pass over the data = k_select_count on every block (adds the block's counts
// of the current 8-bit digit, per target restricted to the keys matching its prefix, into a global (targets, G, 256)
// histogram of integers), then k_select_advance (scans a histogram, fixes the digit, updates the rank).  sizeof(key)
// passes: 4 over f32 data, 8 over f64.  The counts are integers, so neither the blocking, the order of the blocks, the
// order of the atomics nor a sum over ranks changes a bit of the result.  Both ranks of a percentile (lo, lo + 1) are
// targets of the same passes; k_select_finish interpolates like k_gene_quantiles (lerp_numpy).
//
// k_select_count: a workgroup of 16 waves takes a slab of 64 genes x a range of at most SEL_MAXCELLS cells.  Lane <-> gene
// (a wave reads one 256/512-byte row segment per cell), waves interleave the cells.  The slab's histograms live in LDS as
// [target][bin pair][gene], two 16-bit counters to the word (a range never holds 2^16 cells), gene stride 65: the lanes of a
// counting wave (64 genes, one bin each) and the lanes of a flushing wave (64 bin pairs of one gene) both fall in 64
// different banks.  LDS adds are the native ds_add_u32; a wave's lanes never share a word, waves may.  Up to 4 targets per
// launch: 4 x 33 280 B of the CU's 160 KiB.  Non-empty counters are flushed with device-scope integer atomics, a wave's
// going to consecutive bins of one gene.  In the first pass every target has the same (empty) prefix: target 0 is counted
// alone and k_select_advance reads its histogram for all.
constexpr int SEL_GENES = 64, SEL_GSTRIDE = 65, SEL_WAVES = 16, SEL_MAXT = 4, SEL_MAXCELLS = 32768, SEL_MAXTARGETS = 16;
constexpr size_t SEL_LDS_PER_TARGET = (size_t)128 * SEL_GSTRIDE * sizeof(unsigned);

//
// MK (the masked select, vcy_gene_mselect_*): which cells count for a gene.  0: all (the instances of vcy_gene_select_*, whose
// code the parameter leaves as it was).  1: the cells with cell_mask[c] != 0 (NULL = all).  2 and 3: of those, the cells with
// v > mask_thr[g] (mask_mode 1) or v <= mask_thr[g] (mask_mode 2), compared in fp64 as k_build_z compares - a NaN threshold keeps
// nothing -, where v is M[c,g] itself (2: the block is read once) or mask_src[c,g] (3).  A row the cell mask removes is not read.
// The mask never widens the LDS counters' range: a range still holds at most SEL_MAXCELLS cells.
template <typename T, int NT, bool TWO, int MK = 0>
__global__ __launch_bounds__(64 * SEL_WAVES) void k_select_count(const T *__restrict__ M, const T *__restrict__ M2,
                                                                  const double *__restrict__ scale_a, const double *__restrict__ scale_b,
                                                                  const uint64_t *__restrict__ prefix, unsigned *__restrict__ hist, int pass,
                                                                  int C, int per, int G, int64_t ld, const T *__restrict__ mask_src = nullptr,
                                                                  const double *__restrict__ mask_thr = nullptr,
                                                                  const unsigned char *__restrict__ cell_mask = nullptr, int mask_mode = 0)
{
    static_assert(MK == 0 || !TWO, "the masked select takes one matrix");
    using U = typename Key<T>::U;
    constexpr int PASSES = sizeof(U);
    constexpr int UNR = 8;                                         // cells a wave has in flight: their loads are issued before the first is used
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned *cnt = reinterpret_cast<unsigned *>(smem);            // [NT][128][SEL_GSTRIDE]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = blockIdx.x * SEL_GENES, g = g0 + lane;
    const int c0 = blockIdx.y * per, c1 = min(C, c0 + per);
    for (int i = tid; i < NT * 128 * SEL_GSTRIDE; i += 64 * SEL_WAVES) cnt[i] = 0;
    __syncthreads();
    const int shift = 8 * (PASSES - 1 - pass);
    if (g < G) {
        U pf[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) pf[t] = pass == 0 ? (U)0 : (U)(prefix[(int64_t)t * G + g] >> (shift + 8));
        T den_a = T(1), den_b = T(1);
        if (TWO) { den_a = (T)scale_a[g]; den_b = (T)scale_b[g]; }
        double thr = 0.0;
        if (MK >= 2) thr = mask_thr[g];
        for (int cb = c0 + wave; cb < c1; cb += SEL_WAVES * UNR) {
            T m[UNR], m2[UNR];
            unsigned on = (1u << UNR) - 1;                             // MK != 0: bit u = the cell mask keeps cell u's row
            if constexpr (MK != 0) {
                // the UNR mask bytes first, so the row loads below wait for them once and not one after the other; a wave's lanes
                // share the cells, so the bits go to a scalar register and the branches on them are uniform
                if (cell_mask != nullptr) {
                    on = 0;
#pragma unroll
                    for (int u = 0; u < UNR; ++u) on |= (cell_mask[min(cb + u * SEL_WAVES, c1 - 1)] != 0 ? 1u : 0u) << u;
                    on = (unsigned)__builtin_amdgcn_readfirstlane((int)on);
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                // branch-free: a cell beyond the range re-reads the range's last row (inside the block) and is dropped below
                const int c = min(cb + u * SEL_WAVES, c1 - 1);
                const int64_t o = (int64_t)c * ld + g;
                if constexpr (MK == 0) {
                    m[u] = M[o];
                    m2[u] = TWO ? M2[o] : T(0);
                } else {
                    m[u] = T(0); m2[u] = T(0);                         // m2: the mask's source when it is not M
                    if ((on >> u) & 1u) {
                        m[u] = M[o];
                        if (MK == 3) m2[u] = mask_src[o];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (cb + u * SEL_WAVES >= c1) break;
                if constexpr (MK != 0) {
                    bool keep = (on >> u) & 1u;
                    if (MK >= 2) {
                        const double mv = (double)(MK == 2 ? m[u] : m2[u]);
                        keep = keep && (mask_mode == 1 ? (mv > thr) : (mv <= thr));
                    }
                    if (!keep) continue;
                }
                const U k = Key<T>::enc(MK == 0 ? zvalue<T>(m[u], m2[u], den_a, den_b, TWO) : m[u]);
                const unsigned d = (unsigned)((k >> shift) & 0xff);
                const U hi = pass == 0 ? (U)0 : (U)(k >> ((shift + 8) & (8 * PASSES - 1)));
                const unsigned inc = 1u << ((d & 1) * 16);
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (hi == pf[t]) atomicAdd(&cnt[(t * 128 + (int)(d >> 1)) * SEL_GSTRIDE + lane], inc);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < NT * SEL_GENES * 128; i += 64 * SEL_WAVES) {
        const int bp = i & 127, gl = (i >> 7) & (SEL_GENES - 1), t = i >> 13;
        const unsigned v = cnt[(t * 128 + bp) * SEL_GSTRIDE + gl];
        if (v != 0 && g0 + gl < G) {
            unsigned *h = hist + ((int64_t)t * G + (g0 + gl)) * 256 + 2 * bp;
            if (v & 0xffffu) atomicAdd(h, v & 0xffffu);
            if (v >> 16) atomicAdd(h + 1, v >> 16);
        }
    }
}

// One wave per (target, gene): scan the 256 bins (4 per lane, as k_gene_quantiles does), fix the digit that holds the rank.
// A rank beyond the histogram's total (cells missing from the pass) selects nothing and leaves the state as it was.
__global__ __launch_bounds__(256) void k_select_advance(uint64_t *__restrict__ prefix, unsigned *__restrict__ rank,
                                                         const unsigned *__restrict__ hist, int shift, int shared_hist, int NT, int G)
{
    const int lane = threadIdx.x & 63;
    const int64_t tg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tg >= (int64_t)NT * G) return;
    const unsigned *h = hist + (shared_hist ? tg % G : tg) * 256 + lane * 4;
    const unsigned h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];
    const unsigned tot = h0 + h1 + h2 + h3;
    unsigned incl = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    const unsigned excl = incl - tot, rk = rank[tg];
    if (rk >= excl && rk < incl) {   // at most one lane
        unsigned r = rk - excl;
        int d;
        if (r < h0) d = 0;
        else if ((r -= h0) < h1) d = 1;
        else if ((r -= h1) < h2) d = 2;
        else { r -= h2; d = 3; }
        prefix[tg] |= (uint64_t)(lane * 4 + d) << shift;
        rank[tg] = r;
    }
}

struct SelArgs { double t[16]; int ilo[16], ihi[16]; };   // per percentile: interpolation fraction, targets of v[lo] and v[lo + 1]

template <typename T>
__global__ void k_select_finish(const uint64_t *__restrict__ prefix, SelArgs sa, int nq, double *__restrict__ out, int G)
{
    using U = typename Key<T>::U;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    for (int qi = 0; qi < nq; ++qi) {
        const T vlo = Key<T>::dec((U)prefix[(int64_t)sa.ilo[qi] * G + g]), vhi = Key<T>::dec((U)prefix[(int64_t)sa.ihi[qi] * G + g]);
        out[(int64_t)qi * G + g] = lerp_numpy((double)vlo, (double)vhi, sa.t[qi]);
    }
}

// ---- the masked select: a gene's population n_g is known only after pass 0, whose one histogram counts every kept cell.
// State: (2 nq, G) uint64 prefixes, (nq, G) fp64 fractions, (G) int64 populations, (2 nq, G) uint32 ranks; targets 2 qi and
// 2 qi + 1 are the ranks lo and hi of percentile qi.  Until pass 0 ends the fraction's slot holds the percentile itself.
__global__ void k_mselect_begin(uint64_t *__restrict__ prefix, double *__restrict__ frac, int64_t *__restrict__ pop,
                                unsigned *__restrict__ rank, QArgs qa, int nq, int G)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    pop[g] = 0;
    for (int qi = 0; qi < nq; ++qi) {
        frac[(int64_t)qi * G + g] = qa.q[qi];
        for (int s = 0; s < 2; ++s) { prefix[(int64_t)(2 * qi + s) * G + g] = 0; rank[(int64_t)(2 * qi + s) * G + g] = 0xffffffffu; }
    }
}

// End of pass 0, one wave per (percentile, gene): the histogram's total is n_g; both ranks and the fraction follow with the
// arithmetic of k_gene_quantiles, and the first digit of both is fixed from the same scan (k_select_advance's).  n_g == 0 leaves
// the ranks beyond every later histogram, so nothing is ever selected, and k_mselect_finish writes NaN.
__global__ __launch_bounds__(256) void k_mselect_advance0(uint64_t *__restrict__ prefix, double *__restrict__ frac,
                                                           int64_t *__restrict__ pop, unsigned *__restrict__ rank,
                                                           const unsigned *__restrict__ hist, int shift, int nq, int G)
{
    const int lane = threadIdx.x & 63;
    const int64_t qg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qg >= (int64_t)nq * G) return;
    const int qi = (int)(qg / G), g = (int)(qg % G);
    const unsigned *h = hist + (int64_t)g * 256 + lane * 4;
    const unsigned h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];
    const unsigned tot = h0 + h1 + h2 + h3;
    unsigned incl = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    const unsigned excl = incl - tot;
    const unsigned n = (unsigned)__shfl((int)incl, 63, 64);
    const double q = frac[qg];
    if (qi == 0 && lane == 0) pop[g] = (int64_t)n;
    if (n == 0) {
        if (lane == 0) frac[qg] = 0.0;
        return;
    }
    const double hh = __dmul_rn((double)(n - 1), q / 100.0);   // numpy: (n-1) * (q/100)
    const unsigned lo = (unsigned)floor(hh), hi = min(lo + 1, n - 1);
    if (lane == 0) frac[qg] = hh - (double)lo;
    const unsigned rks[2] = {lo, hi};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const unsigned rk = rks[s];
        if (rk >= excl && rk < incl) {   // exactly one lane
            unsigned r = rk - excl;
            int d;
            if (r < h0) d = 0;
            else if ((r -= h0) < h1) d = 1;
            else if ((r -= h1) < h2) d = 2;
            else { r -= h2; d = 3; }
            const int64_t tg = (int64_t)(2 * qi + s) * G + g;
            prefix[tg] = (uint64_t)(lane * 4 + d) << shift;
            rank[tg] = r;
        }
    }
}

template <typename T>
__global__ void k_mselect_finish(const uint64_t *__restrict__ prefix, const double *__restrict__ frac, const int64_t *__restrict__ pop,
                                 int nq, double *__restrict__ out, int64_t *__restrict__ counts, int G)
{
    using U = typename Key<T>::U;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int64_t n = pop[g];
    if (counts) counts[g] = n;
    for (int qi = 0; qi < nq; ++qi) {
        const T vlo = Key<T>::dec((U)prefix[(int64_t)(2 * qi) * G + g]), vhi = Key<T>::dec((U)prefix[(int64_t)(2 * qi + 1) * G + g]);
        out[(int64_t)qi * G + g] = n > 0 ? lerp_numpy((double)vlo, (double)vhi, frac[(int64_t)qi * G + g]) : (double)NAN;
    }
}

}  // namespace vcy

using namespace vcy;

extern "C" size_t vcy_fit_workspace_bytes(int64_t G) { return (size_t)FIT_CB * FIT_NMOM * (size_t)G * sizeof(double); }

extern "C" int vcy_fit_slope_moments(const void *Y, const void *X, double *moments, void *workspace, int64_t C, int64_t G,
                                     int64_t ld, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(Y && X && moments && workspace, "fit_slope_moments: null pointer");
    VCY_REQUIRE(C > 0 && G > 0 && ld >= G, "fit_slope_moments: bad shape");
    VCY_REQUIRE(dtype == VCY_F32 || dtype == VCY_F64, "fit_slope_moments: bad dtype");
    const int N = dtype == VCY_F32 ? 4 : 2;
    VCY_REQUIRE(ld % N == 0, "fit_slope_moments: ld must keep rows 16-byte aligned");
    hipStream_t st = as_stream(stream);
    const int nvec = (int)((G + N - 1) / N);
    dim3 grid((unsigned)((nvec + 255) / 256), FIT_CB);
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_moments_plain<float>, grid, dim3(256), 0, st, (const float *)Y, (const float *)X, (double *)workspace, (int)C, (int)G, ld);
    else hipLaunchKernelGGL(k_moments_plain<double>, grid, dim3(256), 0, st, (const double *)Y, (const double *)X, (double *)workspace, (int)C, (int)G, ld);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fit_slope_reduce, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, (const double *)workspace, moments, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_fit_slope_from_moments(const double *moments, float *gamma, int64_t G, vcy_stream stream)
{
    VCY_REQUIRE(moments && gamma && G > 0, "fit_slope_from_moments: bad arguments");
    hipLaunchKernelGGL(k_fit_slope_final, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, as_stream(stream), moments, gamma, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_fit_slope(const void *Y, const void *X, float *gamma, void *workspace, int64_t C, int64_t G, int64_t ld,
                             int dtype, vcy_stream stream)
{
    VCY_REQUIRE(Y && X && gamma && workspace, "fit_slope: null pointer");
    // partials use FIT_CB*3*G doubles of the FIT_CB*FIT_NMOM*G workspace; the reduced moments sit behind them
    double *mom = (double *)workspace + (size_t)FIT_CB * 3 * (size_t)G;
    int rc = vcy_fit_slope_moments(Y, X, mom, workspace, C, G, ld, dtype, stream);
    if (rc) return rc;
    return vcy_fit_slope_from_moments(mom, gamma, G, stream);
}

static int fit_weighted_partials(const void *Y, const void *X, int weight_mode, const void *W, const void *M, const void *M2,
                                 const double *scale_a, const double *scale_b, const double *down, const double *up, void *workspace,
                                 int64_t C, int64_t G, int64_t ld, int dtype, hipStream_t st, const unsigned char *cmask = nullptr)
{
    VCY_REQUIRE(C > 0 && G > 0 && ld >= G, "fit_weighted: bad shape");
    VCY_REQUIRE(dtype == VCY_F32 || dtype == VCY_F64, "fit_weighted: bad dtype");
    VCY_REQUIRE(weight_mode >= 0 && weight_mode <= 2, "fit_weighted: bad weight_mode");
    VCY_REQUIRE(weight_mode != 0 || W, "fit_weighted: weight_mode 0 needs W");
    VCY_REQUIRE(weight_mode != 1 || (M && down && up), "fit_weighted: weight_mode 1 needs M, down, up");
    VCY_REQUIRE(weight_mode != 1 || ((scale_a == nullptr) == (scale_b == nullptr) && (scale_a == nullptr || M2)), "fit_weighted: scale_a/scale_b/M2 go together");
    dim3 grid((unsigned)((G + 255) / 256), FIT_CB);
#define VCY_LAUNCH_W(T, MODE)                                                                                                  \
    if (cmask)                                                                                                                 \
        hipLaunchKernelGGL((k_moments_weighted_masked<T, MODE>), grid, dim3(256), 0, st, (const T *)Y, (const T *)X, (const T *)W,     \
                           (const T *)M, (const T *)M2, scale_a, scale_b, down, up, (double *)workspace, (int)C, (int)G, ld, cmask);  \
    else                                                                                                                       \
        hipLaunchKernelGGL((k_moments_weighted<T, MODE>), grid, dim3(256), 0, st, (const T *)Y, (const T *)X, (const T *)W, (const T *)M, \
                           (const T *)M2, scale_a, scale_b, down, up, (double *)workspace, (int)C, (int)G, ld)
    if (dtype == VCY_F32) {
        if (weight_mode == 0) { VCY_LAUNCH_W(float, 0); } else if (weight_mode == 1) { VCY_LAUNCH_W(float, 1); } else { VCY_LAUNCH_W(float, 2); }
    } else {
        if (weight_mode == 0) { VCY_LAUNCH_W(double, 0); } else if (weight_mode == 1) { VCY_LAUNCH_W(double, 1); } else { VCY_LAUNCH_W(double, 2); }
    }
#undef VCY_LAUNCH_W
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_fit_weighted(const void *Y, const void *X, int weight_mode, const void *W, const void *M, const void *M2,
                                const double *scale_a, const double *scale_b, const double *down, const double *up,
                                int fit_offset, int box_q, double lo_gamma, double up_gamma_default, const double *up_gamma,
                                const double *q_fixed, float *gamma, float *q, float *R2, void *workspace, int64_t C, int64_t G,
                                int64_t ld, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(Y && X && gamma && workspace, "fit_weighted: null pointer");
    hipStream_t st = as_stream(stream);
    int rc = fit_weighted_partials(Y, X, weight_mode, W, M, M2, scale_a, scale_b, down, up, workspace, C, G, ld, dtype, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_fit_weighted_final, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, (const double *)workspace, fit_offset,
                       box_q, lo_gamma, up_gamma_default, up_gamma, q_fixed, gamma, q, R2, (int)C, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_fit_weighted_moments(const void *Y, const void *X, int weight_mode, const void *W, const void *M, const void *M2,
                                        const double *scale_a, const double *scale_b, const double *down, const double *up, double *moments,
                                        void *workspace, int64_t C, int64_t G, int64_t ld, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(Y && X && moments && workspace, "fit_weighted_moments: null pointer");
    hipStream_t st = as_stream(stream);
    int rc = fit_weighted_partials(Y, X, weight_mode, W, M, M2, scale_a, scale_b, down, up, workspace, C, G, ld, dtype, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_fit_weighted_fold, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, (const double *)workspace, moments, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_fit_weighted_moments_masked(const void *Y, const void *X, int weight_mode, const void *W, const void *M, const void *M2,
                                               const double *scale_a, const double *scale_b, const double *down, const double *up,
                                               const unsigned char *cell_mask, double *moments, void *workspace, int64_t C, int64_t G,
                                               int64_t ld, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(Y && X && moments && workspace && cell_mask, "fit_weighted_moments_masked: null pointer");
    hipStream_t st = as_stream(stream);
    int rc = fit_weighted_partials(Y, X, weight_mode, W, M, M2, scale_a, scale_b, down, up, workspace, C, G, ld, dtype, st, cell_mask);
    if (rc) return rc;
    hipLaunchKernelGGL(k_fit_weighted_fold, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, (const double *)workspace, moments, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

template <typename T>
static void fit_fused_launch(const void *Y, const void *X, int fm, const void *S, const void *U, const double *pa, const double *pb,
                             const double *pc, const double *pd, const double *sa, const double *sb, double pw, const unsigned char *cmask,
                             void *workspace, int64_t C, int64_t G, int64_t ld, hipStream_t st)
{
    dim3 grid((unsigned)((G + 255) / 256), FIT_CB);
#define VCY_LAUNCH_F(FM, CM)                                                                                                          \
    hipLaunchKernelGGL((k_moments_fused<T, FM, CM>), grid, dim3(256), 0, st, (const T *)Y, (const T *)X, (const T *)S, (const T *)U, pa, pb, \
                       pc, pd, sa, sb, pw, (double *)workspace, (int)C, (int)G, ld, cmask)
#define VCY_LAUNCH_FM(FM) do { if (cmask) { VCY_LAUNCH_F(FM, true); } else { VCY_LAUNCH_F(FM, false); } } while (0)
    if (fm == 0) VCY_LAUNCH_FM(0); else if (fm == 1) VCY_LAUNCH_FM(1); else if (fm == 2) VCY_LAUNCH_FM(2); else VCY_LAUNCH_FM(3);
#undef VCY_LAUNCH_FM
#undef VCY_LAUNCH_F
}

extern "C" int vcy_fit_weighted_moments_fused(const void *Y, const void *X, int fused_mode, const void *S, const void *U, const double *pa,
                                              const double *pb, const double *pc, const double *pd, const double *sa, const double *sb,
                                              double power, const unsigned char *cell_mask, double *moments, void *workspace, int64_t C,
                                              int64_t G, int64_t ld, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(Y && X && S && pa && pb && moments && workspace, "fit_weighted_moments_fused: null pointer");
    VCY_REQUIRE(C > 0 && G > 0 && ld >= G, "fit_weighted_moments_fused: bad shape");
    VCY_REQUIRE(dtype == VCY_F32 || dtype == VCY_F64, "fit_weighted_moments_fused: bad dtype");
    VCY_REQUIRE(fused_mode >= 0 && fused_mode <= 3, "fit_weighted_moments_fused: bad fused_mode");
    VCY_REQUIRE(fused_mode == 2 || U, "fit_weighted_moments_fused: U needed");
    VCY_REQUIRE(fused_mode != 3 || (pc && pd && sa && sb), "fit_weighted_moments_fused: maxmin_double needs pc, pd, sa, sb");
    hipStream_t st = as_stream(stream);
    if (dtype == VCY_F32) fit_fused_launch<float>(Y, X, fused_mode, S, U, pa, pb, pc, pd, sa, sb, power, cell_mask, workspace, C, G, ld, st);
    else fit_fused_launch<double>(Y, X, fused_mode, S, U, pa, pb, pc, pd, sa, sb, power, cell_mask, workspace, C, G, ld, st);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fit_weighted_fold, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, (const double *)workspace, moments, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_fit_weighted_from_moments(const double *moments, int64_t n_cells, int fit_offset, int box_q, double lo_gamma,
                                             double up_gamma_default, const double *up_gamma, const double *q_fixed, float *gamma, float *q,
                                             float *R2, int64_t G, vcy_stream stream)
{
    VCY_REQUIRE(moments && gamma && G > 0 && n_cells > 0, "fit_weighted_from_moments: bad arguments");
    hipLaunchKernelGGL(k_fit_weighted_from_moments, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, as_stream(stream), moments, (double)n_cells,
                       fit_offset, box_q, lo_gamma, up_gamma_default, up_gamma, q_fixed, gamma, q, R2, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

// (5, G) fp64 per-gene raw moments over cells [sum x, sum y, sum xx, sum xy, sum yy]: the ingredients of the paired
// row correlation of filter_genes_by_phase_portrait (analysis.py:1285-1288) and of any unweighted per-gene fit.
__global__ void k_gene_moments_reduce(const double *__restrict__ part, double *__restrict__ mom, int G)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    for (int k = 0; k < 5; ++k) {
        double s = 0.0;
        for (int cb = 0; cb < FIT_CB; ++cb) s += part[((int64_t)cb * FIT_NMOM + k) * G + g];
        mom[(int64_t)k * G + g] = s;
    }
}

extern "C" int vcy_gene_moments(const void *Y, const void *X, double *moments, void *workspace, int64_t C, int64_t G, int64_t ld,
                                int dtype, vcy_stream stream)
{
    VCY_REQUIRE(Y && X && moments && workspace && C > 0 && G > 0 && ld >= G, "gene_moments: bad arguments");
    VCY_REQUIRE(dtype == VCY_F32 || dtype == VCY_F64, "gene_moments: bad dtype");
    hipStream_t st = as_stream(stream);
    dim3 grid((unsigned)((G + 255) / 256), FIT_CB);
    if (dtype == VCY_F32)
        hipLaunchKernelGGL((k_moments_weighted<float, 2>), grid, dim3(256), 0, st, (const float *)Y, (const float *)X, (const float *)nullptr, (const float *)nullptr,
                           (const float *)nullptr, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, (double *)workspace, (int)C, (int)G, ld);
    else
        hipLaunchKernelGGL((k_moments_weighted<double, 2>), grid, dim3(256), 0, st, (const double *)Y, (const double *)X, (const double *)nullptr, (const double *)nullptr,
                           (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, (double *)workspace, (int)C, (int)G, ld);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gene_moments_reduce, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, (const double *)workspace, moments, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" size_t vcy_quantile_workspace_bytes(int64_t C, int64_t G) { return (size_t)C * (size_t)G * sizeof(double); }

extern "C" int vcy_gene_quantiles(const void *M, const void *M2, const double *scale_a, const double *scale_b, const void *mask_src,
                                  const double *mask_thr, int mask_mode, const double *qs_host, int nq, double *out, void *workspace,
                                  int64_t C, int64_t G, int64_t ld, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(mask_mode >= 0 && mask_mode <= 2 && (mask_mode == 0 || (mask_src && mask_thr)), "gene_quantiles: bad mask arguments");
    VCY_REQUIRE(M && qs_host && out && workspace && nq > 0 && nq <= 16, "gene_quantiles: bad arguments");
    VCY_REQUIRE(C > 0 && G > 0 && ld >= G, "gene_quantiles: bad shape");
    VCY_REQUIRE((scale_a == nullptr) == (scale_b == nullptr) && (scale_a == nullptr || M2), "gene_quantiles: scale_a/scale_b/M2 go together");
    VCY_REQUIRE(dtype == VCY_F32 || dtype == VCY_F64, "gene_quantiles: bad dtype");
    hipStream_t st = as_stream(stream);
    QArgs qs_dev;
    for (int i = 0; i < 16; ++i) qs_dev.q[i] = i < nq ? qs_host[i] : 0.0;
    for (int i = 0; i < nq; ++i) VCY_REQUIRE(qs_host[i] >= 0.0 && qs_host[i] <= 100.0, "gene_quantiles: percentile outside [0,100]");
    void *Z = workspace;   // gene-major key matrix (G, C) of dtype
    dim3 gridz((unsigned)((G + 63) / 64), (unsigned)((C + 63) / 64));
    if (dtype == VCY_F32) {
        hipLaunchKernelGGL(k_build_z<float>, gridz, dim3(256), 0, st, (const float *)M, (const float *)M2, scale_a, scale_b, (const float *)mask_src, mask_thr, mask_mode, (float *)Z, (int)C, (int)G, ld);
        VCY_LAUNCH_CHECK();
        // the gene's keys in the registers of 1024 threads when they fit (C <= 65 536 in f32), else the row is re-read per pass
        const bool reg = env_int("VCY_QUANTILES_REG", 1) == 1;
#define VCY_QREG(TT, NPT) hipLaunchKernelGGL((k_gene_quantiles_reg<TT, NPT>), dim3((unsigned)G), dim3(1024), 0, st, (const TT *)Z, qs_dev, nq, out, (int)C, (int)G, mask_mode != 0)
        if (reg && C <= 1024 * 16) VCY_QREG(float, 16);
        else if (reg && C <= 1024 * 32) VCY_QREG(float, 32);
        else if (reg && C <= 1024 * 48) VCY_QREG(float, 48);
        else if (reg && C <= 1024 * 56) VCY_QREG(float, 56);
        else if (reg && C <= 1024 * 64) VCY_QREG(float, 64);
        else hipLaunchKernelGGL(k_gene_quantiles<float>, dim3((unsigned)G), dim3(256), 0, st, (const float *)Z, qs_dev, nq, out, (int)C, (int)G, mask_mode != 0);
    } else {
        hipLaunchKernelGGL(k_build_z<double>, gridz, dim3(256), 0, st, (const double *)M, (const double *)M2, scale_a, scale_b, (const double *)mask_src, mask_thr, mask_mode, (double *)Z, (int)C, (int)G, ld);
        VCY_LAUNCH_CHECK();
        const bool reg = env_int("VCY_QUANTILES_REG", 1) == 1;          // f64 keys take two registers each: up to 32 768 cells
        if (reg && C <= 1024 * 8) VCY_QREG(double, 8);
        else if (reg && C <= 1024 * 16) VCY_QREG(double, 16);
        else if (reg && C <= 1024 * 24) VCY_QREG(double, 24);
        else if (reg && C <= 1024 * 32) VCY_QREG(double, 32);
        else if (reg && C <= 1024 * 40) VCY_QREG(double, 40);
        else if (reg && C <= 1024 * 50) VCY_QREG(double, 50);          // 100 of the 128 VGPRs a 1024-thread workgroup may use hold keys
        else hipLaunchKernelGGL(k_gene_quantiles<double>, dim3((unsigned)G), dim3(256), 0, st, (const double *)Z, qs_dev, nq, out, (int)C, (int)G, mask_mode != 0);
    }
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

// ---- streamed order statistics: the state is (ntargets, G) uint64 prefixes followed by (ntargets, G) uint32 ranks
extern "C" int vcy_gene_select_digit_bits(void) { return 8; }
extern "C" int vcy_gene_select_passes(int dtype) { return dtype == VCY_F32 ? 4 : (dtype == VCY_F64 ? 8 : 0); }
extern "C" size_t vcy_gene_select_state_bytes(int64_t G, int ntargets) { return (size_t)ntargets * (size_t)G * (sizeof(uint64_t) + sizeof(unsigned)); }
extern "C" size_t vcy_gene_select_hist_bytes(int64_t G, int ntargets) { return (size_t)ntargets * (size_t)G * 256 * sizeof(unsigned); }

static int select_args_ok(const void *state, const void *hist, int ntargets, int64_t G, int dtype)
{
    VCY_REQUIRE(state && hist, "gene_select: null pointer");
    VCY_REQUIRE(ntargets > 0 && ntargets <= SEL_MAXTARGETS, "gene_select: ntargets outside [1,16]");
    VCY_REQUIRE(G > 0 && G <= INT32_MAX / 2, "gene_select: bad gene count");
    VCY_REQUIRE(dtype == VCY_F32 || dtype == VCY_F64, "gene_select: bad dtype");
    return VCY_OK;
}

extern "C" int vcy_gene_select_begin(void *state, void *hist, const int64_t *ranks_host, int ntargets, int64_t n_total, int64_t G,
                                     int dtype, vcy_stream stream)
{
    int rc = select_args_ok(state, hist, ntargets, G, dtype);
    if (rc) return rc;
    VCY_REQUIRE(ranks_host, "gene_select_begin: null pointer");
    // the counters are 32-bit (and are summed over ranks as int32): every count is at most the total cell number
    VCY_REQUIRE(n_total > 0 && n_total <= INT32_MAX, "gene_select_begin: the total cell number must be in [1, 2^31 - 1] (32-bit counts)");
    for (int t = 0; t < ntargets; ++t) VCY_REQUIRE(ranks_host[t] >= 0 && ranks_host[t] < n_total, "gene_select_begin: rank outside [0, n_total)");
    hipStream_t st = as_stream(stream);
    uint64_t *prefix = (uint64_t *)state;
    unsigned *rank = (unsigned *)(prefix + (size_t)ntargets * G);
    VCY_CHECK_HIP(hipMemsetAsync(prefix, 0, (size_t)ntargets * G * sizeof(uint64_t), st));
    VCY_CHECK_HIP(hipMemsetAsync(hist, 0, vcy_gene_select_hist_bytes(G, ntargets), st));
    for (int t = 0; t < ntargets; ++t)      // hipMemsetD32Async: one 32-bit pattern per target row, no host buffer to keep alive
        VCY_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(rank + (size_t)t * G), (int)ranks_host[t], (size_t)G, st));
    return VCY_OK;
}

struct SelMask { const void *src; const double *thr; const unsigned char *cells; int mode, mk; };   // mk: k_select_count's MK

template <typename T>
static int select_count_launch(const void *M, const void *M2, const double *scale_a, const double *scale_b, const uint64_t *prefix,
                               unsigned *hist, int pass, int nt, int64_t C, int64_t G, int64_t ld, hipStream_t st,
                               const SelMask &mask = SelMask{nullptr, nullptr, nullptr, 0, 0})
{
    DevInfo di;
    int rc = device_info(&di);
    if (rc) return rc;
    const int64_t slabs = (G + SEL_GENES - 1) / SEL_GENES;
    // cell ranges: short enough for the 16-bit LDS counters, and enough of them that the grid covers the CUs four times over
    int64_t nsplit = std::max<int64_t>((C + SEL_MAXCELLS - 1) / SEL_MAXCELLS, (4 * (int64_t)di.cus + slabs - 1) / slabs);
    nsplit = std::min<int64_t>(std::max<int64_t>(nsplit, 1), (C + 63) / 64);      // ... but no range below 64 cells (the flush is per range)
    const int64_t per = (C + nsplit - 1) / nsplit;
    VCY_REQUIRE(per <= SEL_MAXCELLS, "gene_select_count_block: cell range too long");
    const dim3 grid((unsigned)slabs, (unsigned)((C + per - 1) / per));
    VCY_REQUIRE(grid.y <= 65535, "gene_select_count_block: block of cells too large for one launch");
    const size_t lds = (size_t)nt * SEL_LDS_PER_TARGET;
#define VCY_SEL(NT)                                                                                                              \
    {                                                                                                                            \
        auto kern = M2 ? k_select_count<T, NT, true> : k_select_count<T, NT, false>;                                             \
        rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds);                                                      \
        if (rc) return rc;                                                                                                       \
        hipLaunchKernelGGL(kern, grid, dim3(64 * SEL_WAVES), lds, st, (const T *)M, (const T *)M2, scale_a, scale_b, prefix, hist, pass, \
                           (int)C, (int)per, (int)G, ld, (const T *)nullptr, (const double *)nullptr, (const unsigned char *)nullptr, 0); \
    }
#define VCY_MSEL(NT, MK)                                                                                                         \
    {                                                                                                                            \
        auto kern = k_select_count<T, NT, false, MK>;                                                                            \
        rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds);                                                      \
        if (rc) return rc;                                                                                                       \
        hipLaunchKernelGGL(kern, grid, dim3(64 * SEL_WAVES), lds, st, (const T *)M, (const T *)nullptr, (const double *)nullptr,  \
                           (const double *)nullptr, prefix, hist, pass, (int)C, (int)per, (int)G, ld, (const T *)mask.src, mask.thr, \
                           mask.cells, mask.mode);                                                                               \
    }
#define VCY_MSEL_NT(MK) { if (nt == 1) VCY_MSEL(1, MK) else if (nt == 2) VCY_MSEL(2, MK) else if (nt == 3) VCY_MSEL(3, MK) else VCY_MSEL(4, MK) }
    if (mask.mk == 1) VCY_MSEL_NT(1)
    else if (mask.mk == 2) VCY_MSEL_NT(2)
    else if (mask.mk == 3) VCY_MSEL_NT(3)
    else if (nt == 1) VCY_SEL(1) else if (nt == 2) VCY_SEL(2) else if (nt == 3) VCY_SEL(3) else VCY_SEL(4)
#undef VCY_MSEL_NT
#undef VCY_MSEL
#undef VCY_SEL
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_gene_select_count_block(const void *M, const void *M2, const double *scale_a, const double *scale_b, const void *state,
                                           void *hist, int pass, int ntargets, int64_t C, int64_t G, int64_t ld, int dtype,
                                           vcy_stream stream)
{
    int rc = select_args_ok(state, hist, ntargets, G, dtype);
    if (rc) return rc;
    VCY_REQUIRE(M, "gene_select_count_block: null pointer");
    VCY_REQUIRE(C > 0 && C <= INT32_MAX && ld >= G, "gene_select_count_block: bad shape");
    VCY_REQUIRE((scale_a == nullptr) == (scale_b == nullptr) && (scale_a == nullptr) == (M2 == nullptr), "gene_select_count_block: scale_a/scale_b/M2 go together");
    VCY_REQUIRE(pass >= 0 && pass < vcy_gene_select_passes(dtype), "gene_select_count_block: pass outside [0, passes)");
    hipStream_t st = as_stream(stream);
    const uint64_t *prefix = (const uint64_t *)state;
    // first pass: one histogram for all targets; later: groups of up to SEL_MAXT targets (each group reads the block once)
    const int n = pass == 0 ? 1 : ntargets;
    for (int t0 = 0; t0 < n; t0 += SEL_MAXT) {
        const int nt = std::min(SEL_MAXT, n - t0);
        unsigned *h = (unsigned *)hist + (size_t)t0 * G * 256;
        rc = dtype == VCY_F32 ? select_count_launch<float>(M, M2, scale_a, scale_b, prefix + (size_t)t0 * G, h, pass, nt, C, G, ld, st)
                              : select_count_launch<double>(M, M2, scale_a, scale_b, prefix + (size_t)t0 * G, h, pass, nt, C, G, ld, st);
        if (rc) return rc;
    }
    return VCY_OK;
}

extern "C" int vcy_gene_select_advance(void *state, void *hist, int pass, int ntargets, int64_t G, int dtype, vcy_stream stream)
{
    int rc = select_args_ok(state, hist, ntargets, G, dtype);
    if (rc) return rc;
    const int passes = vcy_gene_select_passes(dtype);
    VCY_REQUIRE(pass >= 0 && pass < passes, "gene_select_advance: pass outside [0, passes)");
    hipStream_t st = as_stream(stream);
    uint64_t *prefix = (uint64_t *)state;
    unsigned *rank = (unsigned *)(prefix + (size_t)ntargets * G);
    const int64_t tg = (int64_t)ntargets * G;
    hipLaunchKernelGGL(k_select_advance, dim3((unsigned)((tg + 3) / 4)), dim3(256), 0, st, prefix, rank, (const unsigned *)hist,
                       8 * (passes - 1 - pass), pass == 0 ? 1 : 0, ntargets, (int)G);
    VCY_LAUNCH_CHECK();
    VCY_CHECK_HIP(hipMemsetAsync(hist, 0, vcy_gene_select_hist_bytes(G, pass == 0 ? 1 : ntargets), st));
    return VCY_OK;
}

extern "C" int vcy_gene_select_finish(const void *state, const int *lo_target, const int *hi_target, const double *t_host, int nq,
                                      int ntargets, double *out, int64_t G, int dtype, vcy_stream stream)
{
    int rc = select_args_ok(state, state, ntargets, G, dtype);
    if (rc) return rc;
    VCY_REQUIRE(lo_target && hi_target && t_host && out && nq > 0 && nq <= 16, "gene_select_finish: bad arguments");
    SelArgs sa;
    for (int i = 0; i < 16; ++i) {
        const bool in = i < nq;
        if (in) VCY_REQUIRE(lo_target[i] >= 0 && lo_target[i] < ntargets && hi_target[i] >= 0 && hi_target[i] < ntargets &&
                            t_host[i] >= 0.0 && t_host[i] < 1.0, "gene_select_finish: target or fraction out of range");
        sa.t[i] = in ? t_host[i] : 0.0; sa.ilo[i] = in ? lo_target[i] : 0; sa.ihi[i] = in ? hi_target[i] : 0;
    }
    hipStream_t st = as_stream(stream);
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_select_finish<float>, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, (const uint64_t *)state, sa, nq, out, (int)G);
    else hipLaunchKernelGGL(k_select_finish<double>, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, (const uint64_t *)state, sa, nq, out, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

// ---- masked streamed order statistics (state layout: k_mselect_begin)
struct MselState { uint64_t *prefix; double *frac; int64_t *pop; unsigned *rank; };
static MselState msel_state(const void *state, int nq, int64_t G)
{
    MselState s;
    s.prefix = (uint64_t *)state;
    s.frac = (double *)(s.prefix + (size_t)2 * nq * G);
    s.pop = (int64_t *)(s.frac + (size_t)nq * G);
    s.rank = (unsigned *)(s.pop + (size_t)G);
    return s;
}

extern "C" size_t vcy_gene_mselect_state_bytes(int64_t G, int nq)
{
    return (size_t)G * ((size_t)2 * nq * (sizeof(uint64_t) + sizeof(unsigned)) + (size_t)nq * sizeof(double) + sizeof(int64_t));
}

static int mselect_args_ok(const void *state, const void *hist, int nq, int64_t G, int dtype)
{
    VCY_REQUIRE(nq > 0 && 2 * nq <= SEL_MAXTARGETS, "gene_mselect: nq outside [1,8]");
    return select_args_ok(state, hist, 2 * nq, G, dtype);
}

extern "C" int vcy_gene_mselect_begin(void *state, void *hist, const double *qs_host, int nq, int64_t G, int dtype, vcy_stream stream)
{
    int rc = mselect_args_ok(state, hist, nq, G, dtype);
    if (rc) return rc;
    VCY_REQUIRE(qs_host, "gene_mselect_begin: null pointer");
    QArgs qa;
    for (int i = 0; i < 16; ++i) qa.q[i] = i < nq ? qs_host[i] : 0.0;
    for (int i = 0; i < nq; ++i) VCY_REQUIRE(qs_host[i] >= 0.0 && qs_host[i] <= 100.0, "gene_mselect_begin: percentile outside [0,100]");
    hipStream_t st = as_stream(stream);
    const MselState s = msel_state(state, nq, G);
    hipLaunchKernelGGL(k_mselect_begin, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, s.prefix, s.frac, s.pop, s.rank, qa, nq, (int)G);
    VCY_LAUNCH_CHECK();
    VCY_CHECK_HIP(hipMemsetAsync(hist, 0, vcy_gene_select_hist_bytes(G, 2 * nq), st));
    return VCY_OK;
}

extern "C" int vcy_gene_mselect_count_block(const void *M, const void *mask_src, const double *mask_thr, int mask_mode,
                                            const unsigned char *cell_mask, const void *state, void *hist, int pass, int nq, int64_t C,
                                            int64_t G, int64_t ld, int dtype, vcy_stream stream)
{
    int rc = mselect_args_ok(state, hist, nq, G, dtype);
    if (rc) return rc;
    VCY_REQUIRE(M, "gene_mselect_count_block: null pointer");
    VCY_REQUIRE(C > 0 && C <= INT32_MAX && ld >= G, "gene_mselect_count_block: bad shape");
    VCY_REQUIRE(mask_mode >= 0 && mask_mode <= 2 && (mask_mode == 0 || (mask_src && mask_thr)), "gene_mselect_count_block: bad mask arguments");
    VCY_REQUIRE(pass >= 0 && pass < vcy_gene_select_passes(dtype), "gene_mselect_count_block: pass outside [0, passes)");
    hipStream_t st = as_stream(stream);
    const SelMask mask{mask_src, mask_thr, cell_mask, mask_mode, mask_mode == 0 ? 1 : (mask_src == M ? 2 : 3)};
    const uint64_t *prefix = (const uint64_t *)state;
    const int n = pass == 0 ? 1 : 2 * nq;      // pass 0: one histogram, whose total is the gene's population
    for (int t0 = 0; t0 < n; t0 += SEL_MAXT) {
        const int nt = std::min(SEL_MAXT, n - t0);
        unsigned *h = (unsigned *)hist + (size_t)t0 * G * 256;
        rc = dtype == VCY_F32 ? select_count_launch<float>(M, nullptr, nullptr, nullptr, prefix + (size_t)t0 * G, h, pass, nt, C, G, ld, st, mask)
                              : select_count_launch<double>(M, nullptr, nullptr, nullptr, prefix + (size_t)t0 * G, h, pass, nt, C, G, ld, st, mask);
        if (rc) return rc;
    }
    return VCY_OK;
}

extern "C" int vcy_gene_mselect_advance(void *state, void *hist, int pass, int nq, int64_t G, int dtype, vcy_stream stream)
{
    int rc = mselect_args_ok(state, hist, nq, G, dtype);
    if (rc) return rc;
    const int passes = vcy_gene_select_passes(dtype);
    VCY_REQUIRE(pass >= 0 && pass < passes, "gene_mselect_advance: pass outside [0, passes)");
    hipStream_t st = as_stream(stream);
    const MselState s = msel_state(state, nq, G);
    const int shift = 8 * (passes - 1 - pass);
    if (pass == 0) {
        const int64_t qg = (int64_t)nq * G;
        hipLaunchKernelGGL(k_mselect_advance0, dim3((unsigned)((qg + 3) / 4)), dim3(256), 0, st, s.prefix, s.frac, s.pop, s.rank,
                           (const unsigned *)hist, shift, nq, (int)G);
    } else {
        const int64_t tg = (int64_t)2 * nq * G;
        hipLaunchKernelGGL(k_select_advance, dim3((unsigned)((tg + 3) / 4)), dim3(256), 0, st, s.prefix, s.rank, (const unsigned *)hist, shift,
                           0, 2 * nq, (int)G);
    }
    VCY_LAUNCH_CHECK();
    VCY_CHECK_HIP(hipMemsetAsync(hist, 0, vcy_gene_select_hist_bytes(G, pass == 0 ? 1 : 2 * nq), st));
    return VCY_OK;
}

extern "C" int vcy_gene_mselect_finish(const void *state, int nq, double *out, int64_t *counts, int64_t G, int dtype, vcy_stream stream)
{
    int rc = mselect_args_ok(state, state, nq, G, dtype);
    if (rc) return rc;
    VCY_REQUIRE(out, "gene_mselect_finish: null pointer");
    hipStream_t st = as_stream(stream);
    const MselState s = msel_state(state, nq, G);
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_mselect_finish<float>, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, s.prefix, s.frac, s.pop, nq, out, counts, (int)G);
    else hipLaunchKernelGGL(k_mselect_finish<double>, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, s.prefix, s.frac, s.pop, nq, out, counts, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}
