// csr_select.hip -- gene selection on the atlas path: per-gene count statistics straight from the cells-major CSR layer, and the gene
// (column) subset of such a layer.
//
// Reference: score_detection_levels (analysis.py:456-475), score_cv_vs_mean (analysis.py:214-345), score_cluster_expression
// (analysis.py:441-454 + estimation.py:369-389) and filter_genes (analysis.py:441-497) on the raw counts, which the reference holds
// dense.  Here the layer only exists as CSR counts (ops.CsrCounts): rows = cells, indices = gene numbers ascending inside a row.
//
// k_csr_gene_stats: stats (4, G) = [sum x, sum x^2, count(x > 0), max x] per gene over the cells with cell_mask != 0 - the four rows of
// vcy_gene_stats - with no gene-major copy and no dense tile in global memory.  Grid = (cell tiles of GS_CELLS cells) x (gene slabs of
// the pooling kernel's 2048 genes).  The per-row slab table the layer already carries for pooling (vcy_csr_slab_ptr) says where a slab's
// elements start in every row, so a workgroup reads only its slab's segment of each of its rows: rows over waves, lanes over consecutive
// stored elements (coalesced).  The accumulators of the slab live in LDS, 2048 x (8 + 8 + 4 + 4) B = 48 KB per workgroup (three
// workgroups, 24 waves, per CU of 160 KB), updated with LDS integer atomics: ds_add_u64 twice, ds_add_u32, ds_max_u32.  The tile's
// partial goes to the workspace with plain vector stores and k_csr_gene_stats_fold adds the partials per gene (integers again) and
// converts.  No global atomics of any kind.  Rows with cell_mask == 0 are skipped whole (one byte read): a cluster's masked pass costs
// the cluster's elements, not the layer's.
//
// Exactness.  Counts are integers <= 65535.  sum x and sum x^2 are accumulated as unsigned 64-bit integers (x^2 < 2^32, so 2^32 cells
// fit), the count and the maximum as 32-bit integers (a tile has GS_CELLS cells; the fold adds the counts in 64 bits).  Integer
// sums do not depend on the order the atomics land in: the result is bit-identical from run to run and for any cell blocking.  One
// conversion to f64 at the end: sum x <= 2^16 C and the count are exact for every C < 2^37; sum x^2 <= 2^32 C is exact in f64 (< 2^53)
// up to C = 2^21 cells of all-65535 counts, and ONE correct rounding (round to nearest even of the exact integer) beyond.  The dense
// kernel's f64 sums of the same integers are exact below 2^53 as well, so the two agree bit for bit there.
// An explicitly stored zero counts in nothing (sums + 0, no detection, max unchanged): it is skipped.  Genes with nothing stored (and
// every gene when no cell is selected) come out 0, 0, 0, 0.
//
// k_csr_gene_stats_parts / k_csr_gene_stats_clip: the same statistics of the counts clipped to per-gene bounds (the winsorised values of
// score_cv_vs_mean, analysis.py:255-298), described where they stand below.  The element walk all of them share is csr_walk.h's.
//
// k_csr_select_count / k_csr_select_fill: the CSR of the columns with remap[g] >= 0, renumbered remap[g].  A wave per row; 64 stored
// elements at a time, kept elements compacted in order by ballot + prefix count, so the row's element order is preserved (ascending
// output indices for a monotone remap).  Rows are NOT cut into chunks: a row of a cells-major layer holds at most G elements (a few
// thousand at 30k genes), the skew that vcy_csr_spmm_chunk answers belongs to the gene-major copy, which is never a column-subset
// operand.  Two launches with the caller's cumulative sum of row_len between them; the only temporaries are remap (G int32) and
// row_len / indptr_out (C int64).
// Every position is clamped to [0, indptr[C]) on the way in and to the row's output range on the way out: malformed tables yield wrong
// numbers, never an access outside the arrays.
#include "common.h"
#include "csr_walk.h"

namespace vcy {

constexpr int GS_SLAB = 2048;         // genes per workgroup: must be the slab of the table built by vcy_csr_slab_ptr (checked on the host)
constexpr int GS_CELLS = 2048;        // cells per workgroup tile (vcy_csr_gene_stats_block_cells)
constexpr int GS_WAVES = 8;           // waves per workgroup, each on 64 rows of the tile at a time
constexpr int GS_ROWS = 4;            // rows of a wave whose elements are requested together
constexpr int GS_NZ = 3;              // x 64 elements of each row requested up front (a slab's segment of a 30k-gene row at 8 % holds ~160)
constexpr int SEL_WAVES = 4;          // rows per workgroup of the select kernels

template <typename CT>
__global__ __launch_bounds__(64 * GS_WAVES) void k_csr_gene_stats(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                   const CT *__restrict__ data, const int32_t *__restrict__ slabptr,
                                                                   const uint8_t *__restrict__ cell_mask, unsigned long long *__restrict__ p_sum,
                                                                   unsigned long long *__restrict__ p_sq, unsigned *__restrict__ p_cnt,
                                                                   unsigned *__restrict__ p_max, int64_t C, int G, int nslab)
{
    __shared__ unsigned long long a_sum[GS_SLAB], a_sq[GS_SLAB];
    __shared__ unsigned a_cnt[GS_SLAB], a_max[GS_SLAB];
    const int64_t tile = blockIdx.x;
    const int slab = blockIdx.y, g0 = slab * GS_SLAB;
    for (int g = threadIdx.x; g < GS_SLAB; g += 64 * GS_WAVES) { a_sum[g] = 0; a_sq[g] = 0; a_cnt[g] = 0; a_max[g] = 0; }
    __syncthreads();
    const int64_t c0 = tile * GS_CELLS, c1 = min(C, c0 + GS_CELLS), nnz = indptr[C];
    auto add = [&](unsigned g, unsigned x) {
        if (x == 0u || g >= (unsigned)GS_SLAB) return;       // a stored zero counts in nothing; a gene outside the slab: a malformed table
        atomicAdd(&a_sum[g], (unsigned long long)x);
        atomicAdd(&a_sq[g], (unsigned long long)x * x);
        atomicAdd(&a_cnt[g], 1u);
        atomicMax(&a_max[g], x);
    };
    csr_slab_walk<CT, GS_WAVES, GS_ROWS, GS_NZ>(indptr, indices, data, slabptr, cell_mask, c0, c1, nnz, slab, nslab, g0, add);
    __syncthreads();
    const int64_t o = tile * G;
    for (int g = threadIdx.x; g < GS_SLAB && g0 + g < G; g += 64 * GS_WAVES) {
        p_sum[o + g0 + g] = a_sum[g];
        p_sq[o + g0 + g] = a_sq[g];
        p_cnt[o + g0 + g] = a_cnt[g];
        p_max[o + g0 + g] = a_max[g];
    }
}

// stats[:, g] = the tiles' partials of gene g added up (integers: the order is immaterial), converted once.  64 genes per workgroup
// (a wave reads 512 consecutive bytes of a tile's row), the tiles dealt to its GS_FOLD waves, whose four partial results meet in LDS:
// at 1M cells x 30k genes the partials are 352 MB in 489 tiles, which one thread per gene would walk with 469 waves on 256 CUs.
constexpr int GS_FOLD = 4;

__global__ __launch_bounds__(64 * GS_FOLD) void k_csr_gene_stats_fold(const unsigned long long *__restrict__ p_sum, const unsigned long long *__restrict__ p_sq,
                                                                      const unsigned *__restrict__ p_cnt, const unsigned *__restrict__ p_max,
                                                                      double *__restrict__ stats, int64_t tiles, int G)
{
    __shared__ unsigned long long r_sum[GS_FOLD][64], r_sq[GS_FOLD][64], r_cnt[GS_FOLD][64];
    __shared__ unsigned r_max[GS_FOLD][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * 64 + lane;
    unsigned long long s = 0, ss = 0, n = 0;
    unsigned mx = 0;
    if (g < G)
        for (int64_t t = wave; t < tiles; t += GS_FOLD) {
            s += p_sum[t * G + g];
            ss += p_sq[t * G + g];
            n += p_cnt[t * G + g];
            mx = max(mx, p_max[t * G + g]);
        }
    r_sum[wave][lane] = s; r_sq[wave][lane] = ss; r_cnt[wave][lane] = n; r_max[wave][lane] = mx;
    __syncthreads();
    if (wave != 0 || g >= G) return;
#pragma unroll
    for (int w = 1; w < GS_FOLD; ++w) { s += r_sum[w][lane]; ss += r_sq[w][lane]; n += r_cnt[w][lane]; mx = max(mx, r_max[w][lane]); }
    stats[g] = (double)s;
    stats[(int64_t)G + g] = (double)ss;
    stats[2 * (int64_t)G + g] = (double)n;
    stats[3 * (int64_t)G + g] = (double)mx;
}

// ---- the statistics of the counts clipped to per-gene bounds [lo, hi] (score_cv_vs_mean's winsorised values, analysis.py:255-298).
// k_csr_gene_stats_parts keeps, per gene, integers only: n_below = positive counts < lo, n_above = counts > hi, the sum and the sum of
// squares of the others, the number of positive counts and their maximum.  A count is an integer, so x < lo is x <= ceil(lo) - 1 and
// x > hi is x > floor(hi): the two bounds go to LDS as 16-bit integers in one word per gene (clamped to 0..65535, which loses nothing:
// ceil(lo) - 1 >= 65535 puts every count below, floor(hi) < 0 every positive count above).  A count above hi is counted above whatever
// lo says (np.clip's order; lo <= hi is the caller's to keep).  LDS: 2048 x (8 + 4 + 4 x 4 + 4) B = 64 KB, two workgroups per CU; a tile
// of GS_CELLS cells sums at most 2048 x 65535 < 2^27 in 32 bits.  The tiles' partials are added per gene by k_csr_gene_stats_parts_fold
// into parts (6, G) int64 = [n_below, n_above, sum, sum of squares, positive counts, max]: what a cell-sharded caller adds (max: maximises)
// over its ranks.  k_csr_gene_stats_clip then forms the four rows of vcy_gene_stats of the clipped values from them, the implicit and
// stored zeros (z = n_cells - positive counts, each worth lo when lo > 0) included, in a fixed order with every product and sum rounded
// on its own (no fma):  sum = (lo * (n_below + [lo > 0] z) + S1) + hi * n_above,  sum of squares = ((lo * lo) * (...) + S2) + (hi * hi) * n_above.
// Integers in, one expression per gene out: the result does not depend on launch order, cell blocking or sharding.
template <typename CT>
__global__ __launch_bounds__(64 * GS_WAVES) void k_csr_gene_stats_parts(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                         const CT *__restrict__ data, const int32_t *__restrict__ slabptr,
                                                                         const uint8_t *__restrict__ cell_mask, const double *__restrict__ lo,
                                                                         const double *__restrict__ hi, unsigned long long *__restrict__ p_sq,
                                                                         unsigned *__restrict__ p_u32, int64_t C, int G, int nslab, int64_t tiles)
{
    __shared__ unsigned long long a_sq[GS_SLAB];
    __shared__ unsigned a_sum[GS_SLAB], a_below[GS_SLAB], a_above[GS_SLAB], a_cnt[GS_SLAB], a_max[GS_SLAB], a_bnd[GS_SLAB];
    const int64_t tile = blockIdx.x;
    const int slab = blockIdx.y, g0 = slab * GS_SLAB;
    for (int g = threadIdx.x; g < GS_SLAB; g += 64 * GS_WAVES) {
        a_sq[g] = 0; a_sum[g] = 0; a_below[g] = 0; a_above[g] = 0; a_cnt[g] = 0; a_max[g] = 0;
        unsigned jlo = 0u, ihi = 65535u;
        if (lo && g0 + g < G) {
            const double l = ceil(lo[g0 + g]) - 1.0, h = floor(hi[g0 + g]);
            jlo = l >= 65535.0 ? 65535u : (l > 0.0 ? (unsigned)l : 0u);          // a NaN bound clips nothing
            ihi = h >= 65535.0 ? 65535u : (h > 0.0 ? (unsigned)h : (h < 65535.0 ? 0u : 65535u));
        }
        a_bnd[g] = jlo | (ihi << 16);
    }
    __syncthreads();
    const int64_t c0 = tile * GS_CELLS, c1 = min(C, c0 + GS_CELLS), nnz = indptr[C];
    auto add = [&](unsigned g, unsigned x) {
        if (x == 0u || g >= (unsigned)GS_SLAB) return;       // a stored zero is one of the gene's zeros; a gene outside the slab: a malformed table
        const unsigned b = a_bnd[g];
        atomicAdd(&a_cnt[g], 1u);
        atomicMax(&a_max[g], x);
        if (x > (b >> 16)) atomicAdd(&a_above[g], 1u);
        else if (x <= (b & 0xffffu)) atomicAdd(&a_below[g], 1u);
        else {
            atomicAdd(&a_sum[g], x);
            atomicAdd(&a_sq[g], (unsigned long long)x * x);
        }
    };
    csr_slab_walk<CT, GS_WAVES, GS_ROWS, GS_NZ>(indptr, indices, data, slabptr, cell_mask, c0, c1, nnz, slab, nslab, g0, add);
    __syncthreads();
    const int64_t o = tile * G, plane = tiles * G;
    for (int g = threadIdx.x; g < GS_SLAB && g0 + g < G; g += 64 * GS_WAVES) {
        p_sq[o + g0 + g] = a_sq[g];
        p_u32[o + g0 + g] = a_below[g];
        p_u32[plane + o + g0 + g] = a_above[g];
        p_u32[2 * plane + o + g0 + g] = a_sum[g];
        p_u32[3 * plane + o + g0 + g] = a_cnt[g];
        p_u32[4 * plane + o + g0 + g] = a_max[g];
    }
}

// parts[:, g] = the tiles' partials of gene g added up (the maximum: maximised); the layout of k_csr_gene_stats_fold
__global__ __launch_bounds__(64 * GS_FOLD) void k_csr_gene_stats_parts_fold(const unsigned long long *__restrict__ p_sq, const unsigned *__restrict__ p_u32,
                                                                            long long *__restrict__ parts, int64_t tiles, int G)
{
    __shared__ unsigned long long r_v[GS_FOLD][6][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * 64 + lane;
    const int64_t plane = tiles * G;
    unsigned long long v[6] = {0, 0, 0, 0, 0, 0};             // n_below, n_above, sum, sum of squares, positive counts, max
    if (g < G)
        for (int64_t t = wave; t < tiles; t += GS_FOLD) {
            const int64_t o = t * G + g;
            v[0] += p_u32[o];
            v[1] += p_u32[plane + o];
            v[2] += p_u32[2 * plane + o];
            v[3] += p_sq[o];
            v[4] += p_u32[3 * plane + o];
            v[5] = max(v[5], (unsigned long long)p_u32[4 * plane + o]);
        }
#pragma unroll
    for (int k = 0; k < 6; ++k) r_v[wave][k][lane] = v[k];
    __syncthreads();
    if (wave != 0 || g >= G) return;
#pragma unroll
    for (int w = 1; w < GS_FOLD; ++w) {
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] += r_v[w][k][lane];
        v[5] = max(v[5], r_v[w][5][lane]);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) parts[(int64_t)k * G + g] = (long long)v[k];
}

__global__ __launch_bounds__(256) void k_csr_gene_stats_clip(const long long *__restrict__ parts, const double *__restrict__ lo,
                                                             const double *__restrict__ hi, double *__restrict__ stats, long long n_cells, int G)
{
#pragma clang fp contract(off)   // the order and the roundings above are the definition
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int64_t G64 = G;
    const long long n_below = parts[g], n_above = parts[G64 + g], s1 = parts[2 * G64 + g], s2 = parts[3 * G64 + g], p = parts[4 * G64 + g];
    const double mx = (double)parts[5 * G64 + g];
    double s = (double)s1, ss = (double)(unsigned long long)s2, cnt = (double)p, m = mx;
    if (lo && n_cells > 0) {
        const double l = lo[g], h = hi[g];
        const long long z = n_cells - p;
        const double nb = (double)(n_below + (l > 0.0 ? z : 0)), na = (double)n_above;
        s = (l * nb + s) + h * na;                                      // plain operators: the pragma above does not reach into __dmul_rn / __dadd_rn
        ss = ((l * l) * nb + ss) + (h * h) * na;
        cnt = h > 0.0 ? (double)(p + (l > 0.0 ? z : 0)) : 0.0;          // clip(x) > 0: every positive count when hi > 0, the zeros too when lo > 0
        m = fmin(fmax(mx, l), h);                                       // clip is monotone: the largest clipped value is the clipped maximum
    }
    stats[g] = s;
    stats[G64 + g] = ss;
    stats[2 * G64 + g] = cnt;
    stats[3 * G64 + g] = m;
}

// row_len[r] = number of stored elements of row r whose gene is kept
__global__ __launch_bounds__(64 * SEL_WAVES) void k_csr_select_count(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                      const int32_t *__restrict__ remap, int64_t *__restrict__ row_len, int64_t C,
                                                                      int G)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row = (int64_t)blockIdx.x * SEL_WAVES + wave;
    if (row >= C) return;                                 // whole waves leave: there is no barrier below
    const int64_t nnz = indptr[C], a = max(indptr[row], (int64_t)0), b = min(indptr[row + 1], nnz);
    int n = 0;
    for (int64_t p = a + lane; p < b; p += 64) {
        const unsigned g = (unsigned)indices[p];
        n += (g < (unsigned)G && remap[g] >= 0) ? 1 : 0;
    }
    n = wave_sum(n);
    if (lane == 0) row_len[row] = n;
}

template <typename CT>
__global__ __launch_bounds__(64 * SEL_WAVES) void k_csr_select_fill(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                     const CT *__restrict__ data, const int32_t *__restrict__ remap,
                                                                     const int64_t *__restrict__ indptr_out, int32_t *__restrict__ indices_out,
                                                                     CT *__restrict__ data_out, int64_t C, int G)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row = (int64_t)blockIdx.x * SEL_WAVES + wave;
    if (row >= C) return;
    const int64_t nnz = indptr[C], a = max(indptr[row], (int64_t)0), b = min(indptr[row + 1], nnz);
    int64_t o = max(indptr_out[row], (int64_t)0);
    const int64_t o_end = min(indptr_out[row + 1], indptr_out[C]);
    for (int64_t p0 = a; p0 < b; p0 += 64) {              // wave-uniform trip count: the ballot sees all 64 lanes
        const int64_t p = p0 + lane;
        int r = -1;
        CT x = 0;
        if (p < b) {
            const unsigned g = (unsigned)indices[p];
            x = data[p];
            if (g < (unsigned)G) r = remap[g];
        }
        const unsigned long long kept = __ballot(r >= 0);
        const int before = __popcll(kept & ((1ull << lane) - 1ull));       // kept elements in front of this lane's: order preserved
        const int64_t q = o + before;
        if (r >= 0 && q < o_end) {
            indices_out[q] = r;
            data_out[q] = x;
        }
        o += __popcll(kept);
    }
}

static inline int64_t gs_tiles(int64_t C) { return (C + GS_CELLS - 1) / GS_CELLS; }

}  // namespace vcy

using namespace vcy;

extern "C" int64_t vcy_csr_gene_stats_block_cells(void) { return GS_CELLS; }

extern "C" size_t vcy_csr_gene_stats_workspace_bytes(int64_t C, int64_t G)
{
    if (C <= 0 || G <= 0) return 0;
    return (size_t)gs_tiles(C) * (size_t)G * (2 * sizeof(unsigned long long) + 2 * sizeof(unsigned));
}

extern "C" int vcy_csr_gene_stats(const int64_t *indptr, const int32_t *indices, const void *data, const int32_t *slabptr,
                                  const uint8_t *cell_mask, double *stats, void *workspace, int64_t C, int64_t G, int count_dtype,
                                  vcy_stream stream)
{
    VCY_REQUIRE(C >= 0 && G >= 0 && G < (1LL << 31), "csr_gene_stats: bad shape (C >= 0, 0 <= G < 2^31)");
    VCY_REQUIRE(count_dtype == VCY_U16 || count_dtype == VCY_U8, "csr_gene_stats: count_dtype must be VCY_U16 or VCY_U8");
    if (G == 0) return VCY_OK;
    VCY_REQUIRE(stats, "csr_gene_stats: null pointer (stats)");
    VCY_REQUIRE(C == 0 || (indptr && indices && data && slabptr && workspace), "csr_gene_stats: null pointer");
    VCY_REQUIRE(C == 0 || (uintptr_t)workspace % 8 == 0, "csr_gene_stats: workspace must be 8-byte aligned");
    static_assert(GS_SLAB == 2048, "the slab of vcy_csr_slab_ptr");
    VCY_REQUIRE(vcy_csr_slab_genes() == GS_SLAB, "csr_gene_stats: slab size differs from vcy_csr_slab_genes()");
    const int64_t tiles = gs_tiles(C), nslab = (G + GS_SLAB - 1) / GS_SLAB;
    VCY_REQUIRE(tiles < (1LL << 31) && nslab < 65536, "csr_gene_stats: grid too large");
    hipStream_t st = as_stream(stream);
    unsigned long long *p_sum = (unsigned long long *)workspace, *p_sq = p_sum + tiles * G;
    unsigned *p_cnt = (unsigned *)(p_sq + tiles * G), *p_max = p_cnt + tiles * G;
    if (tiles) {
        const dim3 grid((unsigned)tiles, (unsigned)nslab);
        if (count_dtype == VCY_U16)
            hipLaunchKernelGGL(k_csr_gene_stats<uint16_t>, grid, dim3(64 * GS_WAVES), 0, st, indptr, indices, (const uint16_t *)data, slabptr, cell_mask,
                               p_sum, p_sq, p_cnt, p_max, C, (int)G, (int)nslab);
        else
            hipLaunchKernelGGL(k_csr_gene_stats<uint8_t>, grid, dim3(64 * GS_WAVES), 0, st, indptr, indices, (const uint8_t *)data, slabptr, cell_mask,
                               p_sum, p_sq, p_cnt, p_max, C, (int)G, (int)nslab);
        VCY_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_csr_gene_stats_fold, dim3((unsigned)((G + 63) / 64)), dim3(64 * GS_FOLD), 0, st, (const unsigned long long *)p_sum,
                       (const unsigned long long *)p_sq, (const unsigned *)p_cnt, (const unsigned *)p_max, stats, tiles, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" size_t vcy_csr_gene_stats_parts_workspace_bytes(int64_t C, int64_t G)
{
    if (C <= 0 || G <= 0) return 0;
    return (size_t)gs_tiles(C) * (size_t)G * (sizeof(unsigned long long) + 5 * sizeof(unsigned));
}

extern "C" int vcy_csr_gene_stats_parts(const int64_t *indptr, const int32_t *indices, const void *data, const int32_t *slabptr,
                                        const uint8_t *cell_mask, const double *lo, const double *hi, int64_t *parts, void *workspace,
                                        int64_t C, int64_t G, int count_dtype, vcy_stream stream)
{
    VCY_REQUIRE(C >= 0 && G >= 0 && G < (1LL << 31), "csr_gene_stats_parts: bad shape (C >= 0, 0 <= G < 2^31)");
    VCY_REQUIRE(count_dtype == VCY_U16 || count_dtype == VCY_U8, "csr_gene_stats_parts: count_dtype must be VCY_U16 or VCY_U8");
    VCY_REQUIRE((lo == nullptr) == (hi == nullptr), "csr_gene_stats_parts: lo and hi go together");
    if (G == 0) return VCY_OK;
    VCY_REQUIRE(parts, "csr_gene_stats_parts: null pointer (parts)");
    VCY_REQUIRE(C == 0 || (indptr && indices && data && slabptr && workspace), "csr_gene_stats_parts: null pointer");
    VCY_REQUIRE(C == 0 || (uintptr_t)workspace % 8 == 0, "csr_gene_stats_parts: workspace must be 8-byte aligned");
    VCY_REQUIRE(vcy_csr_slab_genes() == GS_SLAB, "csr_gene_stats_parts: slab size differs from vcy_csr_slab_genes()");
    const int64_t tiles = gs_tiles(C), nslab = (G + GS_SLAB - 1) / GS_SLAB;
    VCY_REQUIRE(tiles < (1LL << 31) && nslab < 65536, "csr_gene_stats_parts: grid too large");
    hipStream_t st = as_stream(stream);
    unsigned long long *p_sq = (unsigned long long *)workspace;
    unsigned *p_u32 = (unsigned *)(p_sq + tiles * G);
    if (tiles) {
        const dim3 grid((unsigned)tiles, (unsigned)nslab);
        if (count_dtype == VCY_U16)
            hipLaunchKernelGGL(k_csr_gene_stats_parts<uint16_t>, grid, dim3(64 * GS_WAVES), 0, st, indptr, indices, (const uint16_t *)data, slabptr,
                               cell_mask, lo, hi, p_sq, p_u32, C, (int)G, (int)nslab, tiles);
        else
            hipLaunchKernelGGL(k_csr_gene_stats_parts<uint8_t>, grid, dim3(64 * GS_WAVES), 0, st, indptr, indices, (const uint8_t *)data, slabptr,
                               cell_mask, lo, hi, p_sq, p_u32, C, (int)G, (int)nslab, tiles);
        VCY_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_csr_gene_stats_parts_fold, dim3((unsigned)((G + 63) / 64)), dim3(64 * GS_FOLD), 0, st, (const unsigned long long *)p_sq,
                       (const unsigned *)p_u32, (long long *)parts, tiles, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_csr_gene_stats_clip(const int64_t *parts, const double *lo, const double *hi, int64_t n_cells, double *stats, int64_t G,
                                       vcy_stream stream)
{
    VCY_REQUIRE(G >= 0 && G < (1LL << 31) && n_cells >= 0, "csr_gene_stats_clip: bad shape (0 <= G < 2^31, n_cells >= 0)");
    VCY_REQUIRE((lo == nullptr) == (hi == nullptr), "csr_gene_stats_clip: lo and hi go together");
    if (G == 0) return VCY_OK;
    VCY_REQUIRE(parts && stats, "csr_gene_stats_clip: null pointer");
    hipLaunchKernelGGL(k_csr_gene_stats_clip, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, as_stream(stream), (const long long *)parts, lo, hi, stats,
                       (long long)n_cells, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_csr_select_count(const int64_t *indptr, const int32_t *indices, const int32_t *remap, int64_t *row_len, int64_t C,
                                    int64_t G, vcy_stream stream)
{
    VCY_REQUIRE(C >= 0 && G > 0 && G < (1LL << 31), "csr_select_count: bad shape (C >= 0, 0 < G < 2^31)");
    if (C == 0) return VCY_OK;
    VCY_REQUIRE(indptr && indices && remap && row_len, "csr_select_count: null pointer");
    const int64_t blocks = (C + SEL_WAVES - 1) / SEL_WAVES;
    VCY_REQUIRE(blocks < (1LL << 31), "csr_select_count: grid too large");
    hipLaunchKernelGGL(k_csr_select_count, dim3((unsigned)blocks), dim3(64 * SEL_WAVES), 0, as_stream(stream), indptr, indices, remap, row_len, C, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_csr_select_fill(const int64_t *indptr, const int32_t *indices, const void *data, const int32_t *remap,
                                   const int64_t *indptr_out, int32_t *indices_out, void *data_out, int64_t C, int64_t G, int count_dtype,
                                   vcy_stream stream)
{
    VCY_REQUIRE(C >= 0 && G > 0 && G < (1LL << 31), "csr_select_fill: bad shape (C >= 0, 0 < G < 2^31)");
    VCY_REQUIRE(count_dtype == VCY_U16 || count_dtype == VCY_U8, "csr_select_fill: count_dtype must be VCY_U16 or VCY_U8");
    if (C == 0) return VCY_OK;
    VCY_REQUIRE(indptr && indices && data && remap && indptr_out && indices_out && data_out, "csr_select_fill: null pointer");
    const int64_t blocks = (C + SEL_WAVES - 1) / SEL_WAVES;
    VCY_REQUIRE(blocks < (1LL << 31), "csr_select_fill: grid too large");
    hipStream_t st = as_stream(stream);
    if (count_dtype == VCY_U16)
        hipLaunchKernelGGL(k_csr_select_fill<uint16_t>, dim3((unsigned)blocks), dim3(64 * SEL_WAVES), 0, st, indptr, indices, (const uint16_t *)data, remap,
                           indptr_out, indices_out, (uint16_t *)data_out, C, (int)G);
    else
        hipLaunchKernelGGL(k_csr_select_fill<uint8_t>, dim3((unsigned)blocks), dim3(64 * SEL_WAVES), 0, st, indptr, indices, (const uint8_t *)data, remap,
                           indptr_out, indices_out, (uint8_t *)data_out, C, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}
