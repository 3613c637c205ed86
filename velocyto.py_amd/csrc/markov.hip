// markov.hip -- stage F, the Markov chain of prepare_markov / run_markov:
//   the step of Diffusion.diffuse (diffusion.py:93-105) on a dense or a CSC matrix, prepare_markov
//   (analysis.py:1818-1863) in dense and in factored form, and the step of the factored chain: a sparse
//   product plus a discrete Gauss transform evaluated on the fly, over all sources or over the chunks
//   near the targets (culled), for all targets or a range of them (cell-sharded chains).
#include <math.h>
#include "common.h"

namespace vcy {

// ---------------------------------------------------------------- stage F: Markov step  y = x . T
// dense row-major T (n, n): y[j] = sum_i x[i] T[i,j]; lanes over j (coalesced rows), rows split over
// blockIdx.y with a deterministic two-stage reduction through `part` (gridDim.y, n).
template <typename T>
__global__ __launch_bounds__(256) void k_vecmat_dense(const T *__restrict__ Tm, const double *__restrict__ x, double *__restrict__ part, int n)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int per = (n + gridDim.y - 1) / gridDim.y;
    const int i0 = blockIdx.y * per, i1 = min(n, i0 + per);
    double acc = 0.0;
    for (int i = i0; i < i1; ++i) acc = fma(x[i], (double)Tm[(int64_t)i * n + j], acc);
    part[(int64_t)blockIdx.y * n + j] = acc;
}
// the same sums with 16-byte loads: a thread owns Vec<T>::N adjacent columns (n % N == 0 keeps every row 16-byte aligned) and
// keeps 8 rows in flight; each column still accumulates its rows in ascending order, so the result is bit-identical to
// k_vecmat_dense.  One step streams the whole matrix once: this is the HBM-bound kernel of run_markov.
template <typename T>
__global__ __launch_bounds__(256) void k_vecmat_dense_vec(const T *__restrict__ Tm, const double *__restrict__ x, double *__restrict__ part, int n)
{
    constexpr int N = Vec<T>::N;
    typedef T V __attribute__((ext_vector_type(N)));
    const int j = (blockIdx.x * blockDim.x + threadIdx.x) * N;
    if (j >= n) return;
    const int per = (n + gridDim.y - 1) / gridDim.y;
    const int i0 = blockIdx.y * per, i1 = min(n, i0 + per);
    double acc[N];
#pragma unroll
    for (int c = 0; c < N; ++c) acc[c] = 0.0;
    const T *p = Tm + (int64_t)i0 * n + j;
    int i = i0;
    for (; i + 8 <= i1; i += 8, p += (int64_t)8 * n) {
        V v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load((const V *)(p + (int64_t)u * n));
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double xi = x[i + u];
#pragma unroll
            for (int c = 0; c < N; ++c) acc[c] = fma(xi, (double)v[u][c], acc[c]);
        }
    }
    for (; i < i1; ++i, p += n) {
        const V v = *(const V *)p;
        const double xi = x[i];
#pragma unroll
        for (int c = 0; c < N; ++c) acc[c] = fma(xi, (double)v[c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < N; ++c) part[(int64_t)blockIdx.y * n + j + c] = acc[c];
}
__global__ void k_vecmat_reduce(const double *__restrict__ part, double *__restrict__ y, double *__restrict__ accum, int n, int nparts)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int p = 0; p < nparts; ++p) s += part[(int64_t)p * n + j];
    y[j] = s;
    if (accum) accum[j] += s;     // path_integral: result = result + x   (diffusion.py:99)
}
// CSC form (column gather): y[j] = sum_p val[p] x[row[p]], one wave per column
template <typename T>
__global__ __launch_bounds__(256) void k_vecmat_csc(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowidx, const T *__restrict__ val,
                                                     const double *__restrict__ x, double *__restrict__ y, double *__restrict__ accum, int n)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= n) return;
    double acc = 0.0;
    for (int64_t p = colptr[j] + lane; p < colptr[j + 1]; p += 64) acc = fma((double)val[p], x[rowidx[p]], acc);
    acc = wave_sum(acc);
    if (lane == 0) { y[j] = acc; if (accum) accum[j] += acc; }
}

// ---------------------------------------------------------------- prepare_markov (analysis.py:1818-1863)
// One workgroup per row c of the dense (n, n) Markov matrix.  P arrives as CSR (the transition
// probabilities, or their transpose for direction="backwards"); emb is (n, edim) fp64.
//   t[c,j]  = P[c,j] * K(dist(c,j); sigma_D);  t[c,c] = max_j t[c,j];  t /= sum_j t      (:1853-1857)
//   kw[c,j] = K(dist(c,j); sigma_W) / sum_j K                                         (:1859-1860)
//   tr      = 0.8 t + 0.2 kw, rows renormalised                                        (:1861-1862)
// K(x; s) = exp(-x^2 / (2 s^2)) / sqrt(2 pi s^2)   (gaussian_kernel, :2449-2451)
__device__ __forceinline__ double gauss_k(double x, double s) { return exp(-(x * x) / (2.0 * s * s)) / sqrt(2.0 * 3.14159265358979323846 * s * s); }

template <typename T>
__global__ __launch_bounds__(256) void k_prepare_markov(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                         const double *__restrict__ pval, const double *__restrict__ emb, int edim,
                                                         T *__restrict__ tr, int n, double sigma_D, double sigma_W)
{
    __shared__ double red[8];
    __shared__ double s_vals[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    double ec[4];
    for (int a = 0; a < edim; ++a) ec[a] = emb[(int64_t)c * edim + a];
    auto dist_to = [&](int j) {
        double d2 = 0.0;
        for (int a = 0; a < edim; ++a) { const double df = emb[(int64_t)j * edim + a] - ec[a]; d2 += df * df; }
        return sqrt(d2);
    };
    // dense noise kernel row sum
    double kw = 0.0;
    for (int j = tid; j < n; j += 256) kw += gauss_k(dist_to(j), sigma_W);
    kw = block_sum(kw, red);
    // sparse part: max and sum of P * K_D over the stored entries (zeros elsewhere -> max >= 0)
    const int64_t p0 = indptr[c], p1 = indptr[c + 1];
    double mx = 0.0, sm = 0.0;
    for (int64_t p = p0 + tid; p < p1; p += 256) {
        const int j = indices[p];
        const double v = pval[p] * gauss_k(dist_to(j), sigma_D);
        mx = fmax(mx, v);
        if (j != c) sm += v;
    }
    mx = wave_max(mx);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    sm = block_sum(sm, red) + mx;      // diagonal := row maximum
    T *row = tr + (int64_t)c * n;
    for (int j = tid; j < n; j += 256) row[j] = (T)(0.2 * gauss_k(dist_to(j), sigma_W) / kw);
    __syncthreads();
    for (int64_t p = p0 + tid; p < p1; p += 256) {
        const int j = indices[p];
        if (j != c) row[j] = (T)((double)row[j] + 0.8 * (pval[p] * gauss_k(dist_to(j), sigma_D)) / sm);
    }
    if (tid == 0) row[c] = (T)((double)row[c] + 0.8 * mx / sm);
    __syncthreads();
    double tot = 0.0;
    for (int j = tid; j < n; j += 256) tot += (double)row[j];
    tot = block_sum(tot, red);
    for (int j = tid; j < n; j += 256) row[j] = (T)((double)row[j] / tot);
    (void)s_vals;
}

// ---------------------------------------------------------------- the same chain in factored form
// tr[c,j] = (0.2 K_W(c,j) / kw[c] + s[c,j]) / tot[c]: a Gaussian of the embedding distance plus a sparse matrix s with the
// pattern of P and a diagonal.  Nothing in it needs n^2 memory: a step x <- x . tr is
//     y[j] = sum_c (x[c] / tot[c]) s[c,j]  +  sum_c u[c] exp2(-|es[c] - es[j]|^2),     u[c] = 0.2 g x[c] / (tot[c] kw[c]),
// es = embedding * sqrt(log2(e) / (2 sigma_W^2)), g = 1 / sqrt(2 pi sigma_W^2): a sparse product (k_vecmat_csc) and a discrete
// Gauss transform evaluated on the fly - n^2 exp2 per step (VALU-bound, 0.5 ms at 50 000 cells in f32) instead of n^2 matrix
// elements from HBM (1.6 ms from f32, 3.0 ms from f64 storage), and no 10-20 GB matrix.
// k_prepare_markov_factored: one workgroup per row c, same reductions as k_prepare_markov; sval in the CSR order of P
// (0 where P stores the diagonal), sdiag = 0.8 max / sm, kw, tot.
__global__ __launch_bounds__(256) void k_prepare_markov_factored(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                  const double *__restrict__ pval, const double *__restrict__ emb, int edim,
                                                                  double *__restrict__ sval, double *__restrict__ sdiag, double *__restrict__ kw_out,
                                                                  double *__restrict__ tot_out, int n, double sigma_D, double sigma_W)
{
    __shared__ double red[8];
    const int c = blockIdx.x, tid = threadIdx.x;
    double ec[4];
    for (int a = 0; a < edim; ++a) ec[a] = emb[(int64_t)c * edim + a];
    auto dist_to = [&](int j) {
        double d2 = 0.0;
        for (int a = 0; a < edim; ++a) { const double df = emb[(int64_t)j * edim + a] - ec[a]; d2 += df * df; }
        return sqrt(d2);
    };
    double kw = 0.0;
    for (int j = tid; j < n; j += 256) kw += gauss_k(dist_to(j), sigma_W);
    kw = block_sum(kw, red);
    const int64_t p0 = indptr[c], p1 = indptr[c + 1];
    double mx = 0.0, sm = 0.0;
    for (int64_t p = p0 + tid; p < p1; p += 256) {
        const int j = indices[p];
        const double v = pval[p] * gauss_k(dist_to(j), sigma_D);
        mx = fmax(mx, v);
        if (j != c) sm += v;
    }
    mx = wave_max(mx);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    sm = block_sum(sm, red) + mx;      // diagonal := row maximum
    double tot = 0.0;
    for (int j = tid; j < n; j += 256) tot += 0.2 * gauss_k(dist_to(j), sigma_W) / kw;
    for (int64_t p = p0 + tid; p < p1; p += 256) {
        const int j = indices[p];
        const double v = j != c ? 0.8 * (pval[p] * gauss_k(dist_to(j), sigma_D)) / sm : 0.0;
        sval[p] = v;
        tot += v;
    }
    tot = block_sum(tot, red) + 0.8 * mx / sm;
    if (tid == 0) { sdiag[c] = 0.8 * mx / sm; kw_out[c] = kw; tot_out[c] = tot; }
}

template <typename CT>
__global__ void k_markov_scale_coords(const double *__restrict__ emb, CT *__restrict__ es, int64_t total, double scale)
{
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t < total) es[t] = (CT)(emb[t] * scale);
}
template <typename CT>
__global__ void k_markov_scale_x(const double *__restrict__ x, const double *__restrict__ tot, const double *__restrict__ kw, double *__restrict__ v,
                                 CT *__restrict__ u, int n, double coef, const int32_t *__restrict__ rank)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double vc = x[c] / tot[c];
    v[c] = vc;
    u[rank ? rank[c] : c] = (CT)(coef * vc / kw[c]);          // rank: the cell's position in the spatially sorted order of the culled transform
}

__device__ __forceinline__ float exp2_neg(float d2) { return __builtin_amdgcn_exp2f(-d2); }
// f64: 2^(-d2) for d2 >= 0 without the library's general exp2 (range checks, denormal paths: ~45 instructions).
// Round 4-5 form: -d2 = k + r with k = rint(-d2), 2^r by the degree-13 Taylor
// polynomial of exp(r ln 2) on |r| <= 1/2, scaled by v_ldexp_f64 - 17 f64 instructions, 17 of the 22 of a (target, source) pair.
// Round 6 form (exp2_neg_tab): -d2 = (64 i + j) / 64 + r with |r| <= 2^-7,
//     2^(-d2) = 2^i  x  T[j]  x  2^r,        T[j] = 2^(j / 64) correctly rounded (64 doubles in LDS: entry j sits in bank pair j, so the 64
//                                            lanes of a read hit different banks or the same word - never a conflict),
//     2^r - 1 = r (c1 + r (c2 + r (c3 + r (c4 + r c5))))    Taylor of exp(r ln 2), truncation 3.5e-17 at |r| = 2^-7,
// the integer 64 i + j read out of the low word of fma(x, 64, 1.5 x 2^52) (no v_rndne, no conversion), 2^i applied by v_ldexp_f64 (the argument is
// clamped to -1000: below 2^-1000 the reference's exp() has long underflowed any sum it could enter): fmax, fma, sub, fma, four fma + a
// multiply, fma, ldexp = 11 f64 instructions and three 32-bit ones (22 % off a step of the full transform, 2.00 -> 1.56 ms at 50 000 cells), within
// 1 ulp of exp2() (tests/test_gpu_ops.py::test_f64_exp2_element_accuracy).  A NaN distance (a NaN or infinite coordinate) is dropped by the
// clamp - and does not need to survive it: such a cell's own normalisation kw[c] is NaN (it sums the same distances), so u[c] is NaN and
// fma(u[c], finite, .) poisons every target exactly as the dense chain does.
// (the table sits in LDS: every kernel that evaluates exp2_neg_tab fills it - 64 threads - before its first barrier.  Entry j of this 64-entry
// form is entry 4 j of c_exp2_tab256 below, both correctly rounded: one table in the source, read with a stride of 4)
__device__ __forceinline__ double exp2_neg_tab(double d2, const double *__restrict__ T)
{
    constexpr double MAGIC = 6755399441055744.0;                    // 1.5 x 2^52: the low word of x 64 + MAGIC is rint(64 x) in two's complement
    const double x = fmax(-d2, -1000.0);
    const double s = fma(x, 64.0, MAGIC);
    const int k = __double2loint(s);                                // 64 i + j
    const double r = fma(s - MAGIC, -0.015625, x);                  // exact, |r| <= 2^-7
    double q = 0.0013333558146428443;                               // ln2^5 / 5!
    q = fma(q, r, 0.009618129107628477);
    q = fma(q, r, 0.05550410866482158);
    q = fma(q, r, 0.2402265069591007);
    q = fma(q, r, 0.6931471805599453);
    q *= r;                                                         // 2^r - 1
    const double t = T[k & 63];
    const double w = fma(t, q, t);                                  // 2^(j / 64 + r) in [0.99, 2.02)
    return ldexp(w, k >> 6);                                        // (one v_ldexp_f64: the integer add on the exponent field cost two moves beside it)
}
// The same with a 256-entry table (2 KB: up to four lanes per bank pair) and a degree-4 polynomial on |r| <= 2^-9 (truncation 3.8e-17): one fma fewer.
// Measured (profiles/r06_markov_exp2.txt): the culled transform (one target per thread) gains 6 % - 0.610 -> 0.571 ms per step -, the full transform
// (two targets per thread: twice the table reads per wave-instruction of arithmetic) loses 5 % to bank conflicts: the culled kernel takes this form,
// the full one the 64-entry form.
__constant__ double c_exp2_tab256[256] = {                           // 2^(j / 256), j = 0 .. 255, correctly rounded (50-digit decimal arithmetic)
    0x1.0000000000000p+0, 0x1.00b1afa5abcbfp+0, 0x1.0163da9fb3335p+0, 0x1.02168143b0281p+0,
    0x1.02c9a3e778061p+0, 0x1.037d42e11bbccp+0, 0x1.04315e86e7f85p+0, 0x1.04e5f72f654b1p+0,
    0x1.059b0d3158574p+0, 0x1.0650a0e3c1f89p+0, 0x1.0706b29ddf6dep+0, 0x1.07bd42b72a836p+0,
    0x1.0874518759bc8p+0, 0x1.092bdf66607e0p+0, 0x1.09e3ecac6f383p+0, 0x1.0a9c79b1f3919p+0,
    0x1.0b5586cf9890fp+0, 0x1.0c0f145e46c85p+0, 0x1.0cc922b7247f7p+0, 0x1.0d83b23395decp+0,
    0x1.0e3ec32d3d1a2p+0, 0x1.0efa55fdfa9c5p+0, 0x1.0fb66affed31bp+0, 0x1.1073028d7233ep+0,
    0x1.11301d0125b51p+0, 0x1.11edbab5e2ab6p+0, 0x1.12abdc06c31ccp+0, 0x1.136a814f204abp+0,
    0x1.1429aaea92de0p+0, 0x1.14e95934f312ep+0, 0x1.15a98c8a58e51p+0, 0x1.166a45471c3c2p+0,
    0x1.172b83c7d517bp+0, 0x1.17ed48695bbc0p+0, 0x1.18af9388c8deap+0, 0x1.1972658375d2fp+0,
    0x1.1a35beb6fcb75p+0, 0x1.1af99f8138a1cp+0, 0x1.1bbe084045cd4p+0, 0x1.1c82f95281c6bp+0,
    0x1.1d4873168b9aap+0, 0x1.1e0e75eb44027p+0, 0x1.1ed5022fcd91dp+0, 0x1.1f9c18438ce4dp+0,
    0x1.2063b88628cd6p+0, 0x1.212be3578a819p+0, 0x1.21f49917ddc96p+0, 0x1.22bdda27912d1p+0,
    0x1.2387a6e756238p+0, 0x1.2451ffb82140ap+0, 0x1.251ce4fb2a63fp+0, 0x1.25e85711ece75p+0,
    0x1.26b4565e27cddp+0, 0x1.2780e341ddf29p+0, 0x1.284dfe1f56381p+0, 0x1.291ba7591bb70p+0,
    0x1.29e9df51fdee1p+0, 0x1.2ab8a66d10f13p+0, 0x1.2b87fd0dad990p+0, 0x1.2c57e39771b2fp+0,
    0x1.2d285a6e4030bp+0, 0x1.2df961f641589p+0, 0x1.2ecafa93e2f56p+0, 0x1.2f9d24abd886bp+0,
    0x1.306fe0a31b715p+0, 0x1.31432edeeb2fdp+0, 0x1.32170fc4cd831p+0, 0x1.32eb83ba8ea32p+0,
    0x1.33c08b26416ffp+0, 0x1.3496266e3fa2dp+0, 0x1.356c55f929ff1p+0, 0x1.36431a2de883bp+0,
    0x1.371a7373aa9cbp+0, 0x1.37f26231e754ap+0, 0x1.38cae6d05d866p+0, 0x1.39a401b7140efp+0,
    0x1.3a7db34e59ff7p+0, 0x1.3b57fbfec6cf4p+0, 0x1.3c32dc313a8e5p+0, 0x1.3d0e544ede173p+0,
    0x1.3dea64c123422p+0, 0x1.3ec70df1c5175p+0, 0x1.3fa4504ac801cp+0, 0x1.40822c367a024p+0,
    0x1.4160a21f72e2ap+0, 0x1.423fb2709468ap+0, 0x1.431f5d950a897p+0, 0x1.43ffa3f84b9d4p+0,
    0x1.44e086061892dp+0, 0x1.45c2042a7d232p+0, 0x1.46a41ed1d0057p+0, 0x1.4786d668b3237p+0,
    0x1.486a2b5c13cd0p+0, 0x1.494e1e192aed2p+0, 0x1.4a32af0d7d3dep+0, 0x1.4b17dea6db7d7p+0,
    0x1.4bfdad5362a27p+0, 0x1.4ce41b817c114p+0, 0x1.4dcb299fddd0dp+0, 0x1.4eb2d81d8abffp+0,
    0x1.4f9b2769d2ca7p+0, 0x1.508417f4531eep+0, 0x1.516daa2cf6642p+0, 0x1.5257de83f4eefp+0,
    0x1.5342b569d4f82p+0, 0x1.542e2f4f6ad27p+0, 0x1.551a4ca5d920fp+0, 0x1.56070dde910d2p+0,
    0x1.56f4736b527dap+0, 0x1.57e27dbe2c4cfp+0, 0x1.58d12d497c7fdp+0, 0x1.59c0827ff07ccp+0,
    0x1.5ab07dd485429p+0, 0x1.5ba11fba87a03p+0, 0x1.5c9268a5946b7p+0, 0x1.5d84590998b93p+0,
    0x1.5e76f15ad2148p+0, 0x1.5f6a320dceb71p+0, 0x1.605e1b976dc09p+0, 0x1.6152ae6cdf6f4p+0,
    0x1.6247eb03a5585p+0, 0x1.633dd1d1929fdp+0, 0x1.6434634ccc320p+0, 0x1.652b9febc8fb7p+0,
    0x1.6623882552225p+0, 0x1.671c1c70833f6p+0, 0x1.68155d44ca973p+0, 0x1.690f4b19e9538p+0,
    0x1.6a09e667f3bcdp+0, 0x1.6b052fa75173ep+0, 0x1.6c012750bdabfp+0, 0x1.6cfdcddd47645p+0,
    0x1.6dfb23c651a2fp+0, 0x1.6ef9298593ae5p+0, 0x1.6ff7df9519484p+0, 0x1.70f7466f42e87p+0,
    0x1.71f75e8ec5f74p+0, 0x1.72f8286ead08ap+0, 0x1.73f9a48a58174p+0, 0x1.74fbd35d7cbfdp+0,
    0x1.75feb564267c9p+0, 0x1.77024b1ab6e09p+0, 0x1.780694fde5d3fp+0, 0x1.790b938ac1cf6p+0,
    0x1.7a11473eb0187p+0, 0x1.7b17b0976cfdbp+0, 0x1.7c1ed0130c132p+0, 0x1.7d26a62ff86f0p+0,
    0x1.7e2f336cf4e62p+0, 0x1.7f3878491c491p+0, 0x1.80427543e1a12p+0, 0x1.814d2add106d9p+0,
    0x1.82589994cce13p+0, 0x1.8364c1eb941f7p+0, 0x1.8471a4623c7adp+0, 0x1.857f4179f5b21p+0,
    0x1.868d99b4492edp+0, 0x1.879cad931a436p+0, 0x1.88ac7d98a6699p+0, 0x1.89bd0a478580fp+0,
    0x1.8ace5422aa0dbp+0, 0x1.8be05bad61778p+0, 0x1.8cf3216b5448cp+0, 0x1.8e06a5e0866d9p+0,
    0x1.8f1ae99157736p+0, 0x1.902fed0282c8ap+0, 0x1.9145b0b91ffc6p+0, 0x1.925c353aa2fe2p+0,
    0x1.93737b0cdc5e5p+0, 0x1.948b82b5f98e5p+0, 0x1.95a44cbc8520fp+0, 0x1.96bdd9a7670b3p+0,
    0x1.97d829fde4e50p+0, 0x1.98f33e47a22a2p+0, 0x1.9a0f170ca07bap+0, 0x1.9b2bb4d53fe0dp+0,
    0x1.9c49182a3f090p+0, 0x1.9d674194bb8d5p+0, 0x1.9e86319e32323p+0, 0x1.9fa5e8d07f29ep+0,
    0x1.a0c667b5de565p+0, 0x1.a1e7aed8eb8bbp+0, 0x1.a309bec4a2d33p+0, 0x1.a42c980460ad8p+0,
    0x1.a5503b23e255dp+0, 0x1.a674a8af46052p+0, 0x1.a799e1330b358p+0, 0x1.a8bfe53c12e59p+0,
    0x1.a9e6b5579fdbfp+0, 0x1.ab0e521356ebap+0, 0x1.ac36bbfd3f37ap+0, 0x1.ad5ff3a3c2774p+0,
    0x1.ae89f995ad3adp+0, 0x1.afb4ce622f2ffp+0, 0x1.b0e07298db666p+0, 0x1.b20ce6c9a8952p+0,
    0x1.b33a2b84f15fbp+0, 0x1.b468415b749b1p+0, 0x1.b59728de5593ap+0, 0x1.b6c6e29f1c52ap+0,
    0x1.b7f76f2fb5e47p+0, 0x1.b928cf22749e4p+0, 0x1.ba5b030a1064ap+0, 0x1.bb8e0b79a6f1fp+0,
    0x1.bcc1e904bc1d2p+0, 0x1.bdf69c3f3a207p+0, 0x1.bf2c25bd71e09p+0, 0x1.c06286141b33dp+0,
    0x1.c199bdd85529cp+0, 0x1.c2d1cd9fa652cp+0, 0x1.c40ab5fffd07ap+0, 0x1.c544778fafb22p+0,
    0x1.c67f12e57d14bp+0, 0x1.c7ba88988c933p+0, 0x1.c8f6d9406e7b5p+0, 0x1.ca3405751c4dbp+0,
    0x1.cb720dcef9069p+0, 0x1.ccb0f2e6d1675p+0, 0x1.cdf0b555dc3fap+0, 0x1.cf3155b5bab74p+0,
    0x1.d072d4a07897cp+0, 0x1.d1b532b08c968p+0, 0x1.d2f87080d89f2p+0, 0x1.d43c8eacaa1d6p+0,
    0x1.d5818dcfba487p+0, 0x1.d6c76e862e6d3p+0, 0x1.d80e316c98398p+0, 0x1.d955d71ff6075p+0,
    0x1.da9e603db3285p+0, 0x1.dbe7cd63a8315p+0, 0x1.dd321f301b460p+0, 0x1.de7d5641c0658p+0,
    0x1.dfc97337b9b5fp+0, 0x1.e11676b197d17p+0, 0x1.e264614f5a129p+0, 0x1.e3b333b16ee12p+0,
    0x1.e502ee78b3ff6p+0, 0x1.e653924676d76p+0, 0x1.e7a51fbc74c83p+0, 0x1.e8f7977cdb740p+0,
    0x1.ea4afa2a490dap+0, 0x1.eb9f4867cca6ep+0, 0x1.ecf482d8e67f1p+0, 0x1.ee4aaa2188510p+0,
    0x1.efa1bee615a27p+0, 0x1.f0f9c1cb6412ap+0, 0x1.f252b376bba97p+0, 0x1.f3ac948dd7274p+0,
    0x1.f50765b6e4540p+0, 0x1.f6632798844f8p+0, 0x1.f7bfdad9cbe14p+0, 0x1.f91d802243c89p+0,
    0x1.fa7c1819e90d8p+0, 0x1.fbdba3692d514p+0, 0x1.fd3c22b8f71f1p+0, 0x1.fe9d96b2a23d9p+0,
};
__device__ __forceinline__ double exp2_neg_tab256(double d2, const double *__restrict__ T)
{
    constexpr double MAGIC = 6755399441055744.0;
    const double x = fmax(-d2, -1000.0);
    const double s = fma(x, 256.0, MAGIC);
    const int k = __double2loint(s);
    const double r = fma(s - MAGIC, -0.00390625, x);                // |r| <= 2^-9
    double q = 0.009618129107628477;                                // ln2^4 / 4!
    q = fma(q, r, 0.05550410866482158);
    q = fma(q, r, 0.2402265069591007);
    q = fma(q, r, 0.6931471805599453);
    q *= r;
    const double t = T[k & 255];
    return ldexp(fma(t, q, t), k >> 8);
}
template <int TAB> __device__ __forceinline__ float exp2_neg_any(float d2, const double *) { return exp2_neg(d2); }
template <int TAB> __device__ __forceinline__ double exp2_neg_any(double d2, const double *T) { return TAB == 64 ? exp2_neg_tab(d2, T) : exp2_neg_tab256(d2, T); }

// The sparse half of a step, y[j] = sum_p scsc[p] v[rowidx[p]] over column j (k_vecmat_csc), riding in the Gauss-transform launch: the two
// halves are independent, and a loop of thousands of steps is bound by the number of launches as soon as the kernels are small
// (13 us per kernel whatever it does at 10 000 cells).  The first `rows` rows of the grid (blockIdx.y) do it, four columns per workgroup.
struct SparseHalf {
    const int64_t *colptr;
    const int32_t *rowidx;
    const double *scsc, *v;
    double *y;
    int n, rows;                                                // rows = 0: no sparse half in this launch
};
__device__ __forceinline__ void sparse_half(const SparseHalf &sp)
{
    const int lane = threadIdx.x & 63;
    const int64_t j = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (j >= sp.n) return;
    double acc = 0.0;
    for (int64_t p = sp.colptr[j] + lane; p < sp.colptr[j + 1]; p += 64) acc = fma(sp.scsc[p], sp.v[sp.rowidx[p]], acc);
    acc = wave_sum(acc);
    if (lane == 0) sp.y[j] = acc;
}

// The Gauss transform, part[by][j] = sum over a workgroup's sources c of u[c] exp2(-|es[c] - es[j]|^2), in two kernels that differ in the
// sources they walk.  What they share: a thread owns JPT targets, j0 + 256 t (the loads clamped at n - 1, the store guarded); the source index
// is uniform over the block (scalar loads); 8 terms are folded in CT before they are added to the fp64 accumulator.  TAB is the table form of
// the fp64 element and tab its table in LDS (the f32 element uses neither).
template <typename CT, int EDIM, int JPT>
__device__ __forceinline__ void gt_targets(const CT *__restrict__ es, int n, int j0, CT (&ej)[JPT][EDIM], double (&acc)[JPT])
{
#pragma unroll
    for (int t = 0; t < JPT; ++t) {
        const int j = min(j0 + t * 256, n - 1);
#pragma unroll
        for (int a = 0; a < EDIM; ++a) ej[t][a] = es[(int64_t)j * EDIM + a];
        acc[t] = 0.0;
    }
}
template <int TAB, typename CT, int EDIM, int JPT>
__device__ __forceinline__ void gt_term(const CT *__restrict__ es, const CT *__restrict__ u, const double *tab, const CT (&ej)[JPT][EDIM], int c, CT (&fold)[JPT])
{
    CT ec[EDIM];
#pragma unroll
    for (int a = 0; a < EDIM; ++a) ec[a] = es[(int64_t)c * EDIM + a];
    const CT uc = u[c];
#pragma unroll
    for (int t = 0; t < JPT; ++t) {
        CT d2 = CT(0);
#pragma unroll
        for (int a = 0; a < EDIM; ++a) { const CT df = ej[t][a] - ec[a]; d2 = fma(df, df, d2); }
        fold[t] = fma(uc, exp2_neg_any<TAB>(d2, tab), fold[t]);
    }
}
// acc += the terms of the sources [c, c1): in eights, then the tail.  An empty tail adds nothing; a fold of zeros would leave acc as it is too
// (acc starts at +0, and a sum with a +0 in it is never -0), so the guard serves both kernels.
template <int TAB, typename CT, int EDIM, int JPT>
__device__ __forceinline__ void gt_add_range(const CT *__restrict__ es, const CT *__restrict__ u, const double *tab, const CT (&ej)[JPT][EDIM], int c, int c1,
                                             double (&acc)[JPT])
{
    for (; c + 8 <= c1; c += 8) {
        CT fold[JPT];
#pragma unroll
        for (int t = 0; t < JPT; ++t) fold[t] = CT(0);
#pragma unroll
        for (int q = 0; q < 8; ++q) gt_term<TAB>(es, u, tab, ej, c + q, fold);
#pragma unroll
        for (int t = 0; t < JPT; ++t) acc[t] += (double)fold[t];
    }
    if (c < c1) {
        CT fold[JPT];
#pragma unroll
        for (int t = 0; t < JPT; ++t) fold[t] = CT(0);
        for (; c < c1; ++c) gt_term<TAB>(es, u, tab, ej, c, fold);
#pragma unroll
        for (int t = 0; t < JPT; ++t) acc[t] += (double)fold[t];
    }
}
template <int JPT>
__device__ __forceinline__ void gt_store(double *__restrict__ part, int by, int n, int j0, const double (&acc)[JPT])
{
#pragma unroll
    for (int t = 0; t < JPT; ++t)
        if (j0 + t * 256 < n) part[(int64_t)by * n + j0 + t * 256] = acc[t];
}

// All sources, split evenly over blockIdx.y.  bx0: first target block (target-range steps).
template <typename CT, int EDIM, int JPT>
__global__ __launch_bounds__(256) void k_gauss_transform(const CT *__restrict__ es, const CT *__restrict__ u, double *__restrict__ part, int n,
                                                          int nparts, SparseHalf sp, int bx0)
{
    __shared__ double s_tab[64];
    if ((int)blockIdx.y < sp.rows) { sparse_half(sp); return; }
    if (sizeof(CT) == 8) {                                      // the fp64 instance's table of 2^(j / 64) (exp2_neg_tab)
        if (threadIdx.x < 64) s_tab[threadIdx.x] = c_exp2_tab256[4 * threadIdx.x];
        __syncthreads();
    }
    const int by = (int)blockIdx.y - sp.rows;
    const int j0 = (bx0 + (int)blockIdx.x) * 256 * JPT + threadIdx.x;
    CT ej[JPT][EDIM];
    double acc[JPT];
    gt_targets(es, n, j0, ej, acc);
    const int per = (n + nparts - 1) / nparts;
    gt_add_range<64>(es, u, s_tab, ej, by * per, min(n, by * per + per), acc);
    gt_store(part, by, n, j0, acc);
}
// The same transform for a kernel that is NARROW against the extent of the embedding (prepare_markov is typically called with sigma_W
// of a grid step): terms below 2^-cut of their weight are left out.  Cells are visited in a spatially sorted order (Hilbert curve of
// the embedding, made by the caller), so 256 consecutive targets and 32 consecutive sources both fill small boxes; a workgroup
// skips every chunk of 32 sources whose box is farther than sqrt(cut) from its targets' box.  The box tests of 64 chunks are made at
// once, one per lane, and the survivors walked through a ballot mask (one test after the other costs a scalar-load round trip each -
// more than the arithmetic they save).  What is left out per target is below n max(u) 2^-cut: cut = 48 (f32) / 72 (f64) puts it
// under the rounding of the accumulation itself.
constexpr int GT_CHUNK = 32;
template <typename CT, int EDIM>
__global__ void k_gauss_boxes(const CT *__restrict__ pts, int npts, CT *__restrict__ lo, CT *__restrict__ hi, int nbox)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;     // box b = bounding box of GT_CHUNK consecutive points
    if (b >= nbox) return;
    const int p0 = b * GT_CHUNK, p1 = min(npts, p0 + GT_CHUNK);
#pragma unroll
    for (int a = 0; a < EDIM; ++a) {
        CT l = pts[(int64_t)p0 * EDIM + a], h = l;
        for (int q = p0 + 1; q < p1; ++q) { const CT v = pts[(int64_t)q * EDIM + a]; l = fmin(l, v); h = fmax(h, v); }
        lo[(int64_t)b * EDIM + a] = l;
        hi[(int64_t)b * EDIM + a] = h;
    }
}

template <typename CT, int EDIM, int JPT>
__global__ __launch_bounds__(256) void k_gauss_transform_culled(const CT *__restrict__ es, const CT *__restrict__ u, double *__restrict__ part, int n,
                                                                 const CT *__restrict__ clo, const CT *__restrict__ chi, int nchunk, CT cut,
                                                                 int nparts, SparseHalf sp, int bx0)
{
    __shared__ CT red[2][EDIM][4];
    __shared__ double s_tab[256];
    if ((int)blockIdx.y < sp.rows) { sparse_half(sp); return; }
    if (sizeof(CT) == 8) s_tab[threadIdx.x] = c_exp2_tab256[threadIdx.x];                       // 256 threads, published by the barrier below
    const int by = (int)blockIdx.y - sp.rows;
    const int j0 = (bx0 + (int)blockIdx.x) * 256 * JPT + threadIdx.x;
    CT ej[JPT][EDIM];
    double acc[JPT];
    gt_targets(es, n, j0, ej, acc);
    CT tlo[EDIM], thi[EDIM];                                   // the box of this workgroup's targets
#pragma unroll
    for (int a = 0; a < EDIM; ++a) {
        CT l = ej[0][a], h = ej[0][a];
#pragma unroll
        for (int t = 1; t < JPT; ++t) { l = fmin(l, ej[t][a]); h = fmax(h, ej[t][a]); }
        l = -wave_max(-l);
        h = wave_max(h);
        if ((threadIdx.x & 63) == 0) { red[0][a][threadIdx.x >> 6] = l; red[1][a][threadIdx.x >> 6] = h; }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < EDIM; ++a) {
        tlo[a] = fmin(fmin(red[0][a][0], red[0][a][1]), fmin(red[0][a][2], red[0][a][3]));
        thi[a] = fmax(fmax(red[1][a][0], red[1][a][1]), fmax(red[1][a][2], red[1][a][3]));
    }
    // the sources are split over blockIdx.y by chunks (finely: where the data is dense a few workgroups get all the work of a target
    // block, and the launch lasts as long as the busiest of them)
    const int qper = (nchunk + nparts - 1) / nparts;
    const int qa = by * qper, qb = min(nchunk, qa + qper);
    const int lane = threadIdx.x & 63;
    for (int qq = qa; qq < qb; qq += 64) {
        const int mine = qq + lane;                            // every wave makes the same 64 tests and gets the same mask
        bool near = false;
        if (mine < qb) {
            CT d2 = CT(0);
#pragma unroll
            for (int a = 0; a < EDIM; ++a) {
                const CT gap = fmax(fmax(clo[(int64_t)mine * EDIM + a] - thi[a], tlo[a] - chi[(int64_t)mine * EDIM + a]), CT(0));
                d2 = fma(gap, gap, d2);
            }
            near = !(d2 > cut);
        }
        unsigned long long mask = __ballot(near);
        while (mask) {
            const int q = qq + __builtin_ctzll(mask);
            mask &= mask - 1;
            gt_add_range<256>(es, u, s_tab, ej, q * GT_CHUNK, min(n, q * GT_CHUNK + GT_CHUNK), acc);
        }
    }
    gt_store(part, by, n, j0, acc);
}
// y[j] += the folded partials (fixed order); path_integral: accum += y.  Then, what the NEXT step starts with (k_markov_scale_x of
// the new y, saved a launch per step: thousands of steps of a few small kernels are bound by launches): v = y / tot, u = coef v / kw.
template <typename CT>
__global__ void k_gauss_reduce(const double *__restrict__ part, double *__restrict__ y, double *__restrict__ accum, int n, int nparts,
                               const int32_t *__restrict__ order, const double *__restrict__ tot, const double *__restrict__ kw,
                               double *__restrict__ v, CT *__restrict__ u, double coef)
{
    // order (culled transform): the partials are indexed by position in the sorted order; thread = position, so that the nparts reads
    // stay coalesced and only the update of y (and v) is scattered; u is indexed by position too
    const int jj = blockIdx.x * blockDim.x + threadIdx.x;
    if (jj >= n) return;
    const int j = order ? order[jj] : jj;
    double s = 0.0;
    for (int p = 0; p < nparts; ++p) s += part[(int64_t)p * n + jj];
    s += y[j];
    y[j] = s;
    if (accum) accum[j] += s;
    const double vj = s / tot[j];
    v[j] = vj;
    u[jj] = (CT)(coef * vj / kw[j]);
}

// Target-range step (cell-sharded chains): the sparse half and the fold of the targets at positions t0 .. t0 + nt - 1 only (position =
// cell, or the cell's place in `order` for the culled transform), with the arithmetic of sparse_half / k_gauss_reduce; the fold of
// v / u for the next step is left out (the next step starts from the all-gathered state).
__global__ void k_sparse_rows(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowidx, const double *__restrict__ scsc,
                              const double *__restrict__ v, double *__restrict__ y, const int32_t *__restrict__ order, int64_t t0, int64_t nt)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nt) return;
    const int64_t j = order ? (int64_t)order[t0 + i] : t0 + i;
    double acc = 0.0;
    for (int64_t p = colptr[j] + lane; p < colptr[j + 1]; p += 64) acc = fma(scsc[p], v[rowidx[p]], acc);
    acc = wave_sum(acc);
    if (lane == 0) y[j] = acc;
}

__global__ void k_gauss_reduce_rows(const double *__restrict__ part, double *__restrict__ y, double *__restrict__ accum, int n, int nparts,
                                    const int32_t *__restrict__ order, int64_t t0, int64_t nt)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nt) return;
    const int64_t jj = t0 + i;
    const int64_t j = order ? (int64_t)order[jj] : jj;
    double s = 0.0;
    for (int p = 0; p < nparts; ++p) s += part[(int64_t)p * n + jj];
    s += y[j];
    y[j] = s;
    if (accum) accum[j] += s;
}

}  // namespace vcy

using namespace vcy;

extern "C" size_t vcy_diffuse_workspace_bytes(int64_t n) { return (size_t)64 * (size_t)n * sizeof(double); }

extern "C" int vcy_diffuse_step_dense(const void *tr, const double *x, double *y, double *accum, void *workspace, int64_t n, int dtype,
                                      vcy_stream stream)
{
    VCY_REQUIRE(tr && x && y && workspace && n > 0 && x != y, "diffuse_step_dense: bad arguments");
    const int nparts = n >= 4096 ? 64 : (n >= 512 ? 16 : 1);
    dim3 grid((unsigned)((n + 255) / 256), nparts);
    hipStream_t st = as_stream(stream);
    VCY_REQUIRE(dtype == VCY_F32 || dtype == VCY_F64, "diffuse_step_dense: bad dtype");
    const int per_thread = dtype == VCY_F32 ? 4 : 2;
    if (n % per_thread == 0 && ((uintptr_t)tr & 15) == 0 && n >= 1024) {
        dim3 gv((unsigned)((n / per_thread + 255) / 256), nparts);
        if (dtype == VCY_F32) hipLaunchKernelGGL(k_vecmat_dense_vec<float>, gv, dim3(256), 0, st, (const float *)tr, x, (double *)workspace, (int)n);
        else hipLaunchKernelGGL(k_vecmat_dense_vec<double>, gv, dim3(256), 0, st, (const double *)tr, x, (double *)workspace, (int)n);
    }
    else if (dtype == VCY_F32) hipLaunchKernelGGL(k_vecmat_dense<float>, grid, dim3(256), 0, st, (const float *)tr, x, (double *)workspace, (int)n);
    else hipLaunchKernelGGL(k_vecmat_dense<double>, grid, dim3(256), 0, st, (const double *)tr, x, (double *)workspace, (int)n);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vecmat_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double *)workspace, y, accum, (int)n, nparts);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_diffuse_step_csc(const int64_t *colptr, const int32_t *rowidx, const void *val, const double *x, double *y,
                                    double *accum, int64_t n, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(colptr && rowidx && val && x && y && n > 0 && x != y, "diffuse_step_csc: bad arguments");
    const unsigned blocks = (unsigned)((n + 3) / 4);
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_vecmat_csc<float>, dim3(blocks), dim3(256), 0, as_stream(stream), colptr, rowidx, (const float *)val, x, y, accum, (int)n);
    else if (dtype == VCY_F64) hipLaunchKernelGGL(k_vecmat_csc<double>, dim3(blocks), dim3(256), 0, as_stream(stream), colptr, rowidx, (const double *)val, x, y, accum, (int)n);
    else return fail(VCY_ERR_INVALID, "%s: bad dtype", "diffuse_step_csc");
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}
extern "C" int vcy_prepare_markov(const int64_t *indptr, const int32_t *indices, const double *pval, const double *embedding, int edim,
                                  void *tr, int64_t n, double sigma_D, double sigma_W, int dtype, vcy_stream stream)
{
    VCY_REQUIRE(indptr && indices && pval && embedding && tr && n > 0 && edim > 0 && edim <= 4 && sigma_D > 0 && sigma_W > 0, "prepare_markov: bad arguments");
    if (dtype == VCY_F32) hipLaunchKernelGGL(k_prepare_markov<float>, dim3((unsigned)n), dim3(256), 0, as_stream(stream), indptr, indices, pval, embedding, edim, (float *)tr, (int)n, sigma_D, sigma_W);
    else if (dtype == VCY_F64) hipLaunchKernelGGL(k_prepare_markov<double>, dim3((unsigned)n), dim3(256), 0, as_stream(stream), indptr, indices, pval, embedding, edim, (double *)tr, (int)n, sigma_D, sigma_W);
    else return fail(VCY_ERR_INVALID, "%s: bad dtype", "prepare_markov");
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

// ---- factored chain (see k_prepare_markov_factored)
static inline int gauss_parts(int64_t n) { const int64_t bx = (n + 511) / 512; int p = (int)((3072 + bx - 1) / bx); return p < 1 ? 1 : (p > 64 ? 64 : p); }

extern "C" size_t vcy_markov_factored_workspace_bytes(int64_t n) { return (size_t)(64 + 2) * (size_t)(n > 0 ? n : 0) * sizeof(double); }

extern "C" int vcy_prepare_markov_factored(const int64_t *indptr, const int32_t *indices, const double *pval, const double *embedding, int edim,
                                           double *sval, double *sdiag, double *kw, double *tot, void *es, int64_t n, double sigma_D,
                                           double sigma_W, int compute_dtype, vcy_stream stream)
{
    VCY_REQUIRE(indptr && indices && pval && embedding && sval && sdiag && kw && tot && es, "prepare_markov_factored: null pointer");
    VCY_REQUIRE(n > 0 && n < (1ll << 31) && edim > 0 && edim <= 4 && sigma_D > 0 && sigma_W > 0, "prepare_markov_factored: bad arguments");
    VCY_REQUIRE(compute_dtype == VCY_F32 || compute_dtype == VCY_F64, "prepare_markov_factored: bad dtype");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_prepare_markov_factored, dim3((unsigned)n), dim3(256), 0, st, indptr, indices, pval, embedding, edim, sval, sdiag, kw, tot,
                       (int)n, sigma_D, sigma_W);
    VCY_LAUNCH_CHECK();
    const double scale = sqrt(1.4426950408889634 / (2.0 * sigma_W * sigma_W));          // exp(-d^2 / (2 s^2)) = exp2(-(scale d)^2)
    const int64_t total = n * edim;
    if (compute_dtype == VCY_F32) hipLaunchKernelGGL(k_markov_scale_coords<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, embedding, (float *)es, total, scale);
    else hipLaunchKernelGGL(k_markov_scale_coords<double>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, embedding, (double *)es, total, scale);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

static inline int64_t gt_chunks(int64_t n) { return (n + GT_CHUNK - 1) / GT_CHUNK; }

extern "C" size_t vcy_markov_cull_boxes_bytes(int64_t n, int edim, int compute_dtype)
{
    if (n <= 0 || edim <= 0) return 0;
    return (size_t)2 * (size_t)gt_chunks(n) * (size_t)edim * (compute_dtype == VCY_F64 ? 8 : 4);
}

template <typename CT>
static int markov_cull_boxes(const CT *es, CT *boxes, int64_t n, int edim, hipStream_t st)
{
    const int64_t nc = gt_chunks(n);
    CT *clo = boxes, *chi = clo + nc * edim;
#define VCY_GB(ED) hipLaunchKernelGGL((k_gauss_boxes<CT, ED>), dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, es, (int)n, clo, chi, (int)nc)
    switch (edim) { case 1: VCY_GB(1); break; case 2: VCY_GB(2); break; case 3: VCY_GB(3); break; default: VCY_GB(4); break; }
#undef VCY_GB
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_markov_cull_boxes(const void *es_sorted, void *boxes, int64_t n, int edim, int compute_dtype, vcy_stream stream)
{
    VCY_REQUIRE(es_sorted && boxes && n > 0 && n < (1ll << 31) && edim > 0 && edim <= 4, "markov_cull_boxes: bad arguments");
    if (compute_dtype == VCY_F32) return markov_cull_boxes<float>((const float *)es_sorted, (float *)boxes, n, edim, as_stream(stream));
    if (compute_dtype == VCY_F64) return markov_cull_boxes<double>((const double *)es_sorted, (double *)boxes, n, edim, as_stream(stream));
    return fail(VCY_ERR_INVALID, "%s: bad dtype", "markov_cull_boxes");
}

// ---- a step of the factored chain: whole (plain or culled transform) or for a range of targets
// What the three step entries take: es and boxes are of the compute dtype; rank, order and boxes are null for the plain transform.
struct StepArgs {
    const double *x; double *y, *accum;                                                  // state in, state out, path integral (or null)
    const int64_t *colptr; const int32_t *rowidx; const double *scsc, *tot, *kw;         // the factored chain (k_prepare_markov_factored), s in CSC form
    const void *es; const int32_t *rank, *order; const void *boxes;                      // scaled coordinates; the culled transform's order and chunk boxes
    int edim; double sigma_W, cut;
    void *workspace; int64_t n; hipStream_t st;
};
static int check_step(const StepArgs &a, const char *who)
{
    const bool ok = a.x && a.y && a.colptr && a.rowidx && a.scsc && a.tot && a.kw && a.es && a.workspace && a.x != a.y && a.n > 0 && a.n < (1ll << 31) &&
                    a.edim > 0 && a.edim <= 4 && a.sigma_W > 0;
    return ok ? VCY_OK : fail(VCY_ERR_INVALID, "%s: bad arguments", who);
}

// The plan of a step: the workspace split v | u | part and how the Gauss transform is cut into workgroups.
constexpr int JPT_PLAIN = 2, JPT_CULLED = 1;                   // targets per thread (profiles/r06_markov_exp2.txt)
template <typename CT>
struct StepPlan {
    double *v;                                                  // x / tot
    CT *u;                                                      // coef v / kw, in the order of the transform's positions
    double *part;                                               // (nparts, n) partial sums of the transform
    double coef;
    int tpb, nparts;                                            // targets per workgroup (grid x), source parts (grid y)
    const CT *clo, *chi;                                        // culled transform: the boxes of the nc source chunks (null: plain transform)
    int nc;
    CT cut;
};
template <typename CT>
static StepPlan<CT> step_plan(const StepArgs &a)
{
    double *v = (double *)a.workspace;
    const double coef = 0.2 / sqrt(2.0 * 3.14159265358979323846 * a.sigma_W * a.sigma_W);
    if (!a.boxes) return {v, (CT *)(v + a.n), v + 2 * a.n, coef, 256 * JPT_PLAIN, gauss_parts(a.n), nullptr, nullptr, 0, CT(0)};
    const int64_t nc = gt_chunks(a.n);
    const CT *clo = (const CT *)a.boxes;
    return {v, (CT *)(v + a.n), v + 2 * a.n, coef, 256 * JPT_CULLED, (int)(nc < 64 ? nc : 64), clo, clo + nc * a.edim, (int)nc, (CT)a.cut};
}
template <typename CT>
static void markov_scale_x(const StepPlan<CT> &p, const StepArgs &a)        // v = x / tot, u = coef v / kw
{
    hipLaunchKernelGGL(k_markov_scale_x<CT>, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, a.st, a.x, a.tot, a.kw, p.v, p.u, (int)a.n, p.coef, a.rank);
}

// The transform of the target blocks [bx0, bx1) (p.tpb positions each); the first sp.rows rows of the grid do the sparse half.
template <typename CT, int EDIM>
static void launch_gauss(const StepPlan<CT> &p, const StepArgs &a, int bx0, int bx1, const SparseHalf &sp)
{
    const dim3 grid((unsigned)(bx1 - bx0), (unsigned)(sp.rows + p.nparts));
    const CT *es = (const CT *)a.es, *u = p.u;
    if (p.clo)
        hipLaunchKernelGGL((k_gauss_transform_culled<CT, EDIM, JPT_CULLED>), grid, dim3(256), 0, a.st, es, u, p.part, (int)a.n, p.clo, p.chi,
                           p.nc, p.cut, p.nparts, sp, bx0);
    else
        hipLaunchKernelGGL((k_gauss_transform<CT, EDIM, JPT_PLAIN>), grid, dim3(256), 0, a.st, es, u, p.part, (int)a.n, p.nparts, sp, bx0);
}
template <typename CT>
static int gauss_transform(const StepPlan<CT> &p, const StepArgs &a, int bx0, int bx1, const SparseHalf &sp)
{
    const int edim = a.edim;
    switch (edim) {
    case 1: launch_gauss<CT, 1>(p, a, bx0, bx1, sp); break;
    case 2: launch_gauss<CT, 2>(p, a, bx0, bx1, sp); break;
    case 3: launch_gauss<CT, 3>(p, a, bx0, bx1, sp); break;
    default: launch_gauss<CT, 4>(p, a, bx0, bx1, sp); break;
    }
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

template <typename CT>
static int diffuse_step_factored(const StepArgs &a, int prepared)
{
    const StepPlan<CT> p = step_plan<CT>(a);
    if (!prepared) {   // a step that follows another one on the same workspace finds v and u written by its fold
        markov_scale_x(p, a);
        VCY_LAUNCH_CHECK();
    }
    // one launch for both halves of the step: the sparse product in the first rows of the grid, the Gauss transform in the others
    const int64_t gx = (a.n + p.tpb - 1) / p.tpb;
    const SparseHalf sp{a.colptr, a.rowidx, a.scsc, p.v, a.y, (int)a.n, (int)(((a.n + 3) / 4 + gx - 1) / gx)};
    if (const int rc = gauss_transform(p, a, 0, (int)gx, sp)) return rc;
    hipLaunchKernelGGL(k_gauss_reduce<CT>, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, a.st, (const double *)p.part, a.y, a.accum,
                       (int)a.n, p.nparts, a.order, a.tot, a.kw, p.v, p.u, p.coef);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

// Targets t0 .. t1 - 1: the full step's target blocks and source parts, the sparse half and the fold in kernels of their own.
template <typename CT>
static int diffuse_step_factored_rows(const StepArgs &a, int64_t t0, int64_t t1)
{
    if (t1 == t0) return VCY_OK;
    const StepPlan<CT> p = step_plan<CT>(a);
    const int64_t nt = t1 - t0;
    markov_scale_x(p, a);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sparse_rows, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, a.st, a.colptr, a.rowidx, a.scsc, (const double *)p.v, a.y, a.order, t0, nt);
    VCY_LAUNCH_CHECK();
    const SparseHalf sp{a.colptr, a.rowidx, a.scsc, p.v, a.y, (int)a.n, 0};                // rows = 0: the sparse half ran above
    if (const int rc = gauss_transform(p, a, (int)(t0 / p.tpb), (int)((t1 + p.tpb - 1) / p.tpb), sp)) return rc;
    hipLaunchKernelGGL(k_gauss_reduce_rows, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, a.st, (const double *)p.part, a.y, a.accum, (int)a.n, p.nparts,
                       a.order, t0, nt);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_diffuse_step_factored(const double *x, double *y, double *accum, const int64_t *colptr, const int32_t *rowidx, const double *scsc,
                                         const double *tot, const double *kw, const void *es, int edim, double sigma_W, void *workspace, int64_t n,
                                         int prepared, int compute_dtype, vcy_stream stream)
{
    const StepArgs a{x, y, accum, colptr, rowidx, scsc, tot, kw, es, nullptr, nullptr, nullptr, edim, sigma_W, 0.0, workspace, n, as_stream(stream)};
    if (const int rc = check_step(a, "diffuse_step_factored")) return rc;
    if (compute_dtype == VCY_F32) return diffuse_step_factored<float>(a, prepared);
    if (compute_dtype == VCY_F64) return diffuse_step_factored<double>(a, prepared);
    return fail(VCY_ERR_INVALID, "%s: bad dtype", "diffuse_step_factored");
}

extern "C" int vcy_diffuse_step_factored_culled(const double *x, double *y, double *accum, const int64_t *colptr, const int32_t *rowidx,
                                                const double *scsc, const double *tot, const double *kw, const void *es_sorted,
                                                const int32_t *rank, const int32_t *order, const void *boxes, int edim, double sigma_W,
                                                double cut, void *workspace, int64_t n, int prepared, int compute_dtype, vcy_stream stream)
{
    const StepArgs a{x, y, accum, colptr, rowidx, scsc, tot, kw, es_sorted, rank, order, boxes, edim, sigma_W, cut, workspace, n, as_stream(stream)};
    if (const int rc = check_step(a, "diffuse_step_factored_culled")) return rc;
    VCY_REQUIRE(rank && order && boxes && cut > 0, "diffuse_step_factored_culled: bad arguments");
    if (compute_dtype == VCY_F32) return diffuse_step_factored<float>(a, prepared);
    if (compute_dtype == VCY_F64) return diffuse_step_factored<double>(a, prepared);
    return fail(VCY_ERR_INVALID, "%s: bad dtype", "diffuse_step_factored_culled");
}

extern "C" int vcy_diffuse_step_factored_rows(const double *x, double *y, double *accum, const int64_t *colptr, const int32_t *rowidx,
                                              const double *scsc, const double *tot, const double *kw, const void *es, const int32_t *rank,
                                              const int32_t *order, const void *boxes, int edim, double sigma_W, double cut, void *workspace,
                                              int64_t n, int64_t t0, int64_t t1, int compute_dtype, vcy_stream stream)
{
    // without boxes the step is the plain one, whatever rank and order hold
    const StepArgs a{x, y, accum, colptr, rowidx, scsc, tot, kw, es, boxes ? rank : nullptr, boxes ? order : nullptr, boxes, edim, sigma_W, cut, workspace, n, as_stream(stream)};
    if (const int rc = check_step(a, "diffuse_step_factored_rows")) return rc;
    VCY_REQUIRE(0 <= t0 && t0 <= t1 && t1 <= n, "diffuse_step_factored_rows: bad arguments");
    VCY_REQUIRE(!boxes || (rank && order && cut > 0), "diffuse_step_factored_rows: the culled step needs rank, order and cut");
    if (compute_dtype == VCY_F32) return diffuse_step_factored_rows<float>(a, t0, t1);
    if (compute_dtype == VCY_F64) return diffuse_step_factored_rows<double>(a, t0, t1);
    return fail(VCY_ERR_INVALID, "%s: bad dtype", "diffuse_step_factored_rows");
}
