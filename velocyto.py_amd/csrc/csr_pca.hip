// csr_pca.hip -- PCA straight from SPARSE (CSR) count layers: the two thin products of the subspace iteration and the per-gene moments.
//
// Reference: perform_PCA on S_norm = log2(S_sz + pcount) (analysis.py:549-551, 678-700), which the reference forms dense in float64
// (240 GB at 1M cells x 30k genes).  The operand here is never formed: a stored count c of a cell with size factor s stands for
//     x = log2(c * s + pcount) - log2(pcount)            (f64, computed on the fly; 0 where nothing is stored)
// i.e. S_norm up to the constant log2(pcount), which the centring of the PCA removes (preprocess.DevicePCA.fit_transform_csr).
//
// k_csr_lognorm_spmm: out[r, j] = sum over the stored elements p of row r of x(p) * B[indices[p], j], j < L: sparse x thin-dense.
// One kernel for both orientations of the layer: the CSR as stored (rows = cells, s = scale[r]: the projection X Z) and its gene-major
// copy (rows = genes, indices = cell numbers, s = scale[indices[p]]: the contraction X^T Y).
//
// Shape: a WAVE owns a unit = up to SPMM_CHUNK consecutive stored elements of ONE row; lanes run over the L columns (column tiles of 64
// for L > 64).  64 elements at a time are loaded and transformed lane-parallel (one log2 per element, not per element and column), then
// handed out with v_readlane: the element's index is wave-uniform, so a row of B is ONE coalesced load of L doubles, SPMM_FLIGHT of them
// in flight per wave, and every lane adds its column in element order: acc = fma(x, B[i, j], acc).  No cross-lane arithmetic, no atomics.
//
// Skew (a housekeeping gene of the gene-major copy has as many elements as there are cells, most genes a handful, some none): a row longer
// than SPMM_CHUNK is cut into chunks summed by separate waves.  Chunk 0 of every row goes straight to out; chunk c >= 1 goes to a
// workspace slot and k_csr_chunk_fixup adds the slots to out in chunk order.  Every sum therefore has a fixed order: results are
// bit-identical from run to run.  Units need no table: unit w < R is chunk 0 of row w; the further chunks are found from the layer's
// element positions - the FULL chunk c - 1 in front of chunk c covers SPMM_CHUNK consecutive positions, hence exactly one multiple
// m * SPMM_CHUNK, and full chunks are disjoint, so "unit R + m = the chunk that follows the full chunk holding position m * SPMM_CHUNK
// (none if that chunk is not full or nothing follows)" names every further chunk exactly once, m doubles as its workspace slot, and the
// row is one binary search in indptr.
#include "common.h"

namespace vcy {

constexpr int SPMM_CHUNK = 4096;      // stored elements per unit (vcy_csr_spmm_chunk)
constexpr int SPMM_WAVES = 4;         // units per workgroup
constexpr int SPMM_FLIGHT = 8;        // rows of B requested together by a wave

// products and sums rounded one by one as numpy rounds them (no contraction into an fma): v is the same double the dense route logs
template <typename CT> __device__ __forceinline__ double lognorm_x(CT c, double s, double pc, double lpc)
{
    return log2(__dadd_rn(__dmul_rn((double)c, s), pc)) - lpc;
}

// unit w -> (row, [a, b) element positions, slot): slot < 0 = chunk 0, written to out; otherwise the workspace slot of a further chunk.
// Every bound is clamped to [0, nnz]: a malformed indptr yields wrong numbers, never an access outside the arrays.
__device__ __forceinline__ bool resolve_unit(const int64_t *__restrict__ indptr, int64_t R, int64_t nnz, int64_t w, int64_t &row, int64_t &a,
                                             int64_t &b, int64_t &slot)
{
    int64_t s, e;
    if (w < R) {
        row = w;
        s = indptr[w];
        e = indptr[w + 1];
        a = s;
        slot = -1;
    } else {
        const int64_t m = w - R, q = m * SPMM_CHUNK;
        if (q >= nnz) return false;
        int64_t lo = 0, hi = R;                          // first row whose start lies beyond q; the row before it holds q
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (indptr[mid] > q) hi = mid; else lo = mid + 1;
        }
        if (lo < 1) return false;
        row = lo - 1;
        s = indptr[row];
        e = indptr[row + 1];
        a = s + ((q - s) / SPMM_CHUNK + 1) * SPMM_CHUNK;
        if (a >= e) return false;
        slot = m;
    }
    a = max(a, (int64_t)0);
    b = min(min(e, a + SPMM_CHUNK), nnz);
    return true;
}

template <typename CT, bool ON_INDEX>
__global__ __launch_bounds__(64 * SPMM_WAVES) void k_csr_lognorm_spmm(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                      const CT *__restrict__ data, const double *__restrict__ scale,
                                                                      const double *__restrict__ B, double *__restrict__ out,
                                                                      double *__restrict__ ws, int64_t R, int N, int64_t nnz, int L, int64_t ldb,
                                                                      int64_t ldo, int64_t units, double pc, double lpc)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // in an SGPR: all that follows from it is scalar
    const int64_t w = (int64_t)blockIdx.x * SPMM_WAVES + wave;
    int64_t row, a, b, slot;
    if (w >= units || !resolve_unit(indptr, R, nnz, w, row, a, b, slot)) return;       // whole waves leave: there is no barrier below
    double *dst = slot < 0 ? out + row * ldo : ws + slot * L;
    const double srow = ON_INDEX ? 1.0 : scale[row];
    for (int j0 = 0; j0 < L; j0 += 64) {
        const int j = j0 + lane;
        const bool act = j < L;
        const double *Bj = B + min(j, L - 1);             // lanes past the last column read it again: no branch around a load
        double acc = 0.0;
        for (int64_t p0 = a; p0 < b; p0 += 64) {
            const int nb = (int)min((int64_t)64, b - p0);
            int idx = 0;
            double x = 0.0;
            if (lane < nb) {                             // lane t: element p0 + t, transformed once for all columns
                idx = min(max(indices[p0 + lane], 0), N - 1);
                x = lognorm_x(data[p0 + lane], ON_INDEX ? scale[idx] : srow, pc, lpc);
            }
            for (int q = 0; q < nb; q += SPMM_FLIGHT) {
                double bv[SPMM_FLIGHT];
#pragma unroll
                for (int u = 0; u < SPMM_FLIGHT; ++u) {  // the request phase is nothing but loads (past the end: the last row again)
                    const int iq = __builtin_amdgcn_readlane(idx, min(q + u, nb - 1));
                    bv[u] = Bj[(int64_t)iq * ldb];
                }
#pragma unroll
                for (int u = 0; u < SPMM_FLIGHT; ++u)
                    if (q + u < nb) acc = fma(readlane_t(x, q + u), bv[u], acc);
            }
        }
        if (act) dst[j] = acc;
    }
}

// per-row sum of x and of x^2 over the same units: lanes over the elements (lane t takes t, t + 64, ...), then the DPP tree - a fixed order
template <typename CT, bool ON_INDEX>
__global__ __launch_bounds__(64 * SPMM_WAVES) void k_csr_lognorm_stats(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                       const CT *__restrict__ data, const double *__restrict__ scale,
                                                                       double *__restrict__ out, double *__restrict__ ws, int64_t R, int N,
                                                                       int64_t nnz, int64_t units, double pc, double lpc)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // in an SGPR: all that follows from it is scalar
    const int64_t w = (int64_t)blockIdx.x * SPMM_WAVES + wave;
    int64_t row, a, b, slot;
    if (w >= units || !resolve_unit(indptr, R, nnz, w, row, a, b, slot)) return;
    const double srow = ON_INDEX ? 1.0 : scale[row];
    double s1 = 0.0, s2 = 0.0;
    for (int64_t p = a + lane; p < b; p += 64) {
        const int idx = min(max(indices[p], 0), N - 1);
        const double x = lognorm_x(data[p], ON_INDEX ? scale[idx] : srow, pc, lpc);
        s1 += x;
        s2 = fma(x, x, s2);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    double *dst = slot < 0 ? out + row * 2 : ws + slot * 2;
    if (lane == 0) { dst[0] = s1; dst[1] = s2; }
}

// out[r, :] += the workspace slots of the further chunks of row r, in chunk order (one thread per row and column)
__global__ __launch_bounds__(256) void k_csr_chunk_fixup(const int64_t *__restrict__ indptr, double *__restrict__ out, const double *__restrict__ ws,
                                                         int64_t R, int L, int64_t ldo, int64_t slots)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R * L) return;
    const int64_t r = t / L;
    const int j = (int)(t - r * L);
    const int64_t s = indptr[r], len = indptr[r + 1] - s;
    if (len <= SPMM_CHUNK) return;
    double acc = out[r * ldo + j];
    for (int64_t c = 1; c * SPMM_CHUNK < len; ++c) {
        const int64_t m = (s + (c - 1) * SPMM_CHUNK + SPMM_CHUNK - 1) / SPMM_CHUNK;     // the multiple of the chunk length inside chunk c - 1
        if (m >= 0 && m < slots) acc += ws[m * L + j];
    }
    out[r * ldo + j] = acc;
}

// workspace slots = further units.  max_row: the caller's upper bound on the stored elements of any row (0: not known) - when no row exceeds a
// chunk there are no further chunks: no units beyond the rows, no second launch, no workspace (the cell-major layer at atlas scale)
static inline int64_t spmm_slots(int64_t nnz, int64_t max_row = 0)
{
    if (max_row > 0 && max_row <= SPMM_CHUNK) return 0;
    return nnz > SPMM_CHUNK ? (nnz - 1) / SPMM_CHUNK + 1 : 0;
}

}  // namespace vcy

using namespace vcy;

extern "C" int64_t vcy_csr_spmm_chunk(void) { return SPMM_CHUNK; }

extern "C" size_t vcy_csr_spmm_workspace_bytes(int64_t nnz, int64_t L)
{
    if (nnz <= 0 || L <= 0) return 0;
    return (size_t)spmm_slots(nnz) * (size_t)L * sizeof(double);
}

static int csr_common_checks(const int64_t *indptr, const int32_t *indices, const void *data, const double *scale, const void *workspace,
                             int64_t R, int64_t N, int64_t nnz, int64_t max_row, double pcount, int scale_on, int count_dtype, const char *who)
{
    VCY_REQUIRE(indptr && scale, who);
    VCY_REQUIRE(R > 0 && N > 0 && nnz >= 0 && N < (1LL << 31), "csr_lognorm: bad shape (R > 0, 0 < N < 2^31, nnz >= 0)");
    VCY_REQUIRE(nnz == 0 || (indices && data), who);
    VCY_REQUIRE(count_dtype == VCY_U16 || count_dtype == VCY_U8, "csr_lognorm: count_dtype must be VCY_U16 or VCY_U8");
    VCY_REQUIRE(scale_on == VCY_SCALE_ON_ROW || scale_on == VCY_SCALE_ON_INDEX, "csr_lognorm: scale_on must be VCY_SCALE_ON_ROW or VCY_SCALE_ON_INDEX");
    VCY_REQUIRE(pcount > 0.0 && pcount < 1e300, "csr_lognorm: pcount must be positive and finite");
    VCY_REQUIRE(max_row >= 0, "csr_lognorm: max_row must be 0 (not known) or an upper bound on the stored elements of a row");
    VCY_REQUIRE(spmm_slots(nnz, max_row) == 0 || workspace, "csr_lognorm: workspace missing (vcy_csr_spmm_workspace_bytes)");
    VCY_REQUIRE((R + spmm_slots(nnz, max_row) + SPMM_WAVES - 1) / SPMM_WAVES < (1LL << 31), "csr_lognorm: grid too large");
    return VCY_OK;
}

extern "C" int vcy_csr_lognorm_spmm(const int64_t *indptr, const int32_t *indices, const void *data, const double *scale, const double *B,
                                    double *out, void *workspace, int64_t R, int64_t N, int64_t nnz, int64_t max_row, int64_t L, int64_t ldb,
                                    int64_t ldo, double pcount, int scale_on, int count_dtype, vcy_stream stream)
{
    VCY_REQUIRE(L > 0 && L < (1LL << 31), "csr_lognorm_spmm: L must be positive");
    VCY_REQUIRE(B && out, "csr_lognorm_spmm: null pointer");
    if (int rc = csr_common_checks(indptr, indices, data, scale, workspace, R, N, nnz, max_row, pcount, scale_on, count_dtype, "csr_lognorm_spmm: null pointer")) return rc;
    VCY_REQUIRE(ldb >= L && ldo >= L, "csr_lognorm_spmm: ldb and ldo must be at least L");
    VCY_REQUIRE((R * L + 255) / 256 < (1LL << 31), "csr_lognorm_spmm: grid too large");
    const int64_t slots = spmm_slots(nnz, max_row), units = R + slots;
    const unsigned blocks = (unsigned)((units + SPMM_WAVES - 1) / SPMM_WAVES);
    const double lpc = log2(pcount);
    hipStream_t st = as_stream(stream);
#define VCY_SPMM(CT, ON)                                                                                                                        \
    hipLaunchKernelGGL((k_csr_lognorm_spmm<CT, ON>), dim3(blocks), dim3(64 * SPMM_WAVES), 0, st, indptr, indices, (const CT *)data, scale, B, out, \
                       (double *)workspace, R, (int)N, nnz, (int)L, ldb, ldo, units, pcount, lpc)
    if (count_dtype == VCY_U16) { if (scale_on == VCY_SCALE_ON_INDEX) VCY_SPMM(uint16_t, true); else VCY_SPMM(uint16_t, false); }
    else { if (scale_on == VCY_SCALE_ON_INDEX) VCY_SPMM(uint8_t, true); else VCY_SPMM(uint8_t, false); }
#undef VCY_SPMM
    VCY_LAUNCH_CHECK();
    if (slots) {
        hipLaunchKernelGGL(k_csr_chunk_fixup, dim3((unsigned)((R * L + 255) / 256)), dim3(256), 0, st, indptr, out, (const double *)workspace, R, (int)L,
                           ldo, slots);
        VCY_LAUNCH_CHECK();
    }
    return VCY_OK;
}

extern "C" int vcy_csr_lognorm_stats(const int64_t *indptr, const int32_t *indices, const void *data, const double *scale, double *stats,
                                     void *workspace, int64_t R, int64_t N, int64_t nnz, int64_t max_row, double pcount, int scale_on,
                                     int count_dtype, vcy_stream stream)
{
    VCY_REQUIRE(stats, "csr_lognorm_stats: null pointer");
    if (int rc = csr_common_checks(indptr, indices, data, scale, workspace, R, N, nnz, max_row, pcount, scale_on, count_dtype, "csr_lognorm_stats: null pointer")) return rc;
    const int64_t slots = spmm_slots(nnz, max_row), units = R + slots;
    const unsigned blocks = (unsigned)((units + SPMM_WAVES - 1) / SPMM_WAVES);
    const double lpc = log2(pcount);
    hipStream_t st = as_stream(stream);
#define VCY_STATS(CT, ON)                                                                                                                      \
    hipLaunchKernelGGL((k_csr_lognorm_stats<CT, ON>), dim3(blocks), dim3(64 * SPMM_WAVES), 0, st, indptr, indices, (const CT *)data, scale, stats, \
                       (double *)workspace, R, (int)N, nnz, units, pcount, lpc)
    if (count_dtype == VCY_U16) { if (scale_on == VCY_SCALE_ON_INDEX) VCY_STATS(uint16_t, true); else VCY_STATS(uint16_t, false); }
    else { if (scale_on == VCY_SCALE_ON_INDEX) VCY_STATS(uint8_t, true); else VCY_STATS(uint8_t, false); }
#undef VCY_STATS
    VCY_LAUNCH_CHECK();
    if (slots) {
        hipLaunchKernelGGL(k_csr_chunk_fixup, dim3((unsigned)((R * 2 + 255) / 256)), dim3(256), 0, st, indptr, stats, (const double *)workspace, R, 2,
                           (int64_t)2, slots);
        VCY_LAUNCH_CHECK();
    }
    return VCY_OK;
}
