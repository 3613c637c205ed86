// csr_quantiles.hip -- exact per-gene order statistics of a cells-major CSR count layer, implicit zeros included: the percentiles
// behind score_cv_vs_mean(winsorize=True) (analysis.py:255-298; np.percentile at analysis.py:264) for a layer that only exists as
// ops.CsrCounts.  No gene-major copy, no dense tile.
//
// The rule.  Over n selected cells gene g has p_g positive stored counts and z_g = n - p_g zeros (cells that store nothing for it, and
// explicitly stored zeros).  The value of rank r (0-based, ascending) is 0 when r < z_g and the (r - z_g)-th smallest positive stored
// count otherwise.  The ranks - at most 32, the same for every gene - are ops.percentile_targets' for n cells.
//
// The select is an MSB-first radix select on 8-bit digits over the positive stored counts: ONE counting walk for a uint8 layer, TWO
// for uint16.  A walk (k_csr_hist) is the tiling of k_csr_gene_stats: grid = (tiles of QH_CELLS cells) x (slabs of 2048 genes), every
// row's slab segment found through vcy_csr_slab_ptr's table and read once, masked-out rows skipped whole after one byte, stored
// zeros skipped.  Walk 0 counts, per gene, the histogram of the first digit (the count itself for uint8, its high byte for uint16)
// into hist[0] (G x 256 uint32).  k_csr_qadvance<0> then scans a gene's 256 bins in one wave, finds p_g, and fixes for every target
// rank either the value 0 or the first digit and the rank left inside that bin; the targets of a gene that share a first digit share
// one histogram of walk 1, and hist[0] is rewritten in place as the gene's digit -> histogram table (256 words; most are "none").
// Walk 1 (uint16 only) counts the low byte of every element whose high byte has a histogram into hist[1 + slot], and
// k_csr_qadvance<1> fixes the low digit.  k_csr_qfinish interpolates with lerp_numpy - the helper of k_gene_quantiles - in f64.
// Nothing is read back to the host between the walks; a cell-sharded caller adds hist[0] (after walk 0) and hist[1:] (after walk 1)
// over its ranks before the advance.
//
// Where the counts land.  A gene's 256-bin table cannot sit in LDS for a whole slab (2048 x 256 x 4 B = 2 MB against 160 KB), and
// 2.4e9 single global integer adds run at the memory-side atomic rate (measured: 122 ms a walk at 1M cells, 23 x the statistics
// pass).  But counts are small: a workgroup keeps the bins 0..QH_SHORT-1 of its slab's genes in LDS as 16-bit counters, two to a
// word (2048 x 8 x 2 B = 32 KB, four workgroups = 32 waves per CU; a tile has at most QH_CELLS <= 65535 rows and a gene appears at
// most once in a row, so a counter cannot carry into its neighbour), adds with ds_add_u32, and at the end adds its non-zero counters
// to the global table with plain global_atomic_add_u32 (vector, no return).  A digit >= QH_SHORT is added to the global table at
// once.  QH_SHORT = 8 and QH_CELLS = 4096 are the measured best of {0, 8, 16} x {4096, 8192} on the synthetic atlas
// (profiles/gene_select_winsor.txt): 16 bins halve the occupancy (64 KB) and cost more than the global adds they save there.
// Every add is an integer add: the histograms, and with them every bit of the result, do not depend on the order of arrival, the
// launch, the cell blocking or the sharding.
// Every index is checked before it is used: a gene outside [0, G), a slot >= ntargets or a position outside [0, nnz) is dropped.
#include "common.h"
#include "csr_walk.h"

namespace vcy {

constexpr int QH_SLAB = 2048;         // genes per workgroup: the slab of vcy_csr_slab_ptr (checked on the host)
#ifndef VCY_QH_CELLS
#define VCY_QH_CELLS 4096
#endif
#ifndef VCY_QH_SHORT
#define VCY_QH_SHORT 8
#endif
constexpr int QH_CELLS = VCY_QH_CELLS;   // cells per workgroup tile (vcy_csr_quantiles_block_cells); at most 65535, see above
constexpr int QH_WAVES = 8;
constexpr int QH_ROWS = 4;
constexpr int QH_NZ = 3;
constexpr int QH_SHORT = VCY_QH_SHORT;   // digits below this are counted in LDS (0: every count goes to the global table at once; measured, profiles/gene_select_winsor.txt)
constexpr int QH_WORDS = QH_SHORT / 2;
constexpr int QH_TAB = QH_SHORT > 0 ? QH_SLAB * QH_WORDS : 1;
constexpr int QH_MAXT = 32;           // distinct target ranks (16 percentiles x 2)
constexpr int QH_MAXQ = 16;
constexpr unsigned QH_NONE = 0xffffffffu;
static_assert(QH_CELLS <= 65535 && QH_SHORT % 2 == 0 && QH_SHORT <= 256, "16-bit counters, two to a word");

struct QRanks { long long r[QH_MAXT]; };
struct QLerp { int lo[QH_MAXQ], hi[QH_MAXQ]; double t[QH_MAXQ]; };

// PASS 0: hist0[g][first digit] += 1.  PASS 1 (uint16): map = hist0 rewritten by k_csr_qadvance<0>; hist1[map[g][high byte]][g][low byte] += 1.
template <typename CT, int PASS>
__global__ __launch_bounds__(64 * QH_WAVES) void k_csr_hist(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                             const CT *__restrict__ data, const int32_t *__restrict__ slabptr,
                                                             const uint8_t *__restrict__ cell_mask, const unsigned *map, unsigned *hist,
                                                             int64_t C, int G, int nslab, unsigned nt)
{
    __shared__ unsigned tab[QH_TAB];
    const int64_t tile = blockIdx.x;
    const int slab = blockIdx.y, g0 = slab * QH_SLAB;
    for (int i = threadIdx.x; i < QH_TAB; i += 64 * QH_WAVES) tab[i] = 0u;
    __syncthreads();
    const int64_t c0 = tile * QH_CELLS, c1 = min(C, c0 + QH_CELLS), nnz = indptr[C];
    auto add = [&](unsigned g, unsigned x) {
        if (x == 0u || g >= (unsigned)QH_SLAB || g0 + (int)g >= G) return;       // a stored zero is a zero; a gene outside the slab: a malformed table
        const unsigned hb = (PASS == 0 || sizeof(CT) == 1) ? 0u : (x >> 8) & 0xffu;
        const unsigned d = (PASS == 0 && sizeof(CT) == 2) ? (x >> 8) & 0xffu : x & 0xffu;
        if (QH_SHORT > 0 && hb == 0u && d < (unsigned)QH_SHORT) {
            atomicAdd(&tab[g * QH_WORDS + (d >> 1)], 1u << ((d & 1u) * 16));
            return;
        }
        const int64_t gg = g0 + (int64_t)g;
        if (PASS == 0) atomicAdd(&hist[gg * 256 + d], 1u);
        else {
            const unsigned s = map[gg * 256 + hb];
            if (s < nt) atomicAdd(&hist[((int64_t)s * G + gg) * 256 + d], 1u);
        }
    };
    csr_slab_walk<CT, QH_WAVES, QH_ROWS, QH_NZ>(indptr, indices, data, slabptr, cell_mask, c0, c1, nnz, slab, nslab, g0, add);
    __syncthreads();
    for (int i = threadIdx.x; QH_SHORT > 0 && i < QH_TAB; i += 64 * QH_WAVES) {      // QH_WORDS lanes = one gene's bins, consecutive bytes
        const unsigned w = tab[i];
        const int64_t gg = g0 + i / (QH_WORDS > 0 ? QH_WORDS : 1);
        if (w == 0u || gg >= G) continue;
        unsigned *dst = hist + gg * 256;
        if (PASS == 1) {
            const unsigned s = map[gg * 256];                                     // the LDS counters hold high byte 0
            if (s >= nt) continue;
            dst = hist + ((int64_t)s * G + gg) * 256;
        }
        const int d = 2 * (i % (QH_WORDS > 0 ? QH_WORDS : 1));
        if (w & 0xffffu) atomicAdd(dst + d, w & 0xffffu);
        if (w >> 16) atomicAdd(dst + d + 1, w >> 16);
    }
}

// inclusive prefix sum of the lanes' totals over the wave (the scan of k_gene_quantiles)
__device__ __forceinline__ unsigned wave_scan_incl(unsigned tot, int lane)
{
    unsigned incl = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    return incl;
}

// the bin of rank r (0-based) in the histogram a wave holds 4 bins per lane: found = does any bin hold it; then digit and the rank left
// inside the bin, the same in every lane
__device__ __forceinline__ bool wave_find_bin(const unsigned h[4], unsigned incl, unsigned r, int lane, unsigned &digit, unsigned &left)
{
    const unsigned tot = h[0] + h[1] + h[2] + h[3], excl = incl - tot;
    unsigned d = 0, rr = 0;
    const bool mine = r >= excl && r < incl;                 // at most one lane
    if (mine) {
        rr = r - excl;
        if (rr < h[0]) d = 0;
        else if ((rr -= h[0]) < h[1]) d = 1;
        else if ((rr -= h[1]) < h[2]) d = 2;
        else { rr -= h[2]; d = 3; }
        d += 4u * lane;
    }
    const unsigned long long m = __ballot(mine);
    if (m == 0) return false;
    const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
    digit = (unsigned)__builtin_amdgcn_readlane((int)d, src);
    left = (unsigned)__builtin_amdgcn_readlane((int)rr, src);
    return true;
}

// One wave per gene.  val (nt, G): the value of every target as far as it is known; left (nt, G): its rank inside the bucket of that
// prefix, QH_NONE once the value is final.
template <int PASS>
__global__ __launch_bounds__(256) void k_csr_qadvance(unsigned *hist, unsigned *__restrict__ val, unsigned *__restrict__ left, QRanks ranks,
                                                       int nt, long long n_cells, int G, int wide)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;                                       // whole waves leave: there is no barrier below
    if (PASS == 0) {
        unsigned *h0 = hist + g * 256;
        unsigned h[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) h[k] = h0[lane * 4 + k];
        const unsigned incl = wave_scan_incl(h[0] + h[1] + h[2] + h[3], lane);
        const long long p = (long long)(unsigned)__builtin_amdgcn_readlane((int)incl, 63), z = n_cells - p;
        unsigned slot[4] = {QH_NONE, QH_NONE, QH_NONE, QH_NONE};
        for (int t = 0; t < nt; ++t) {
            const long long r = ranks.r[t];
            unsigned v = 0u, lf = QH_NONE, digit = 0u, rest = 0u;
            if (r >= z && wave_find_bin(h, incl, (unsigned)(r - z), lane, digit, rest)) {      // otherwise one of the zeros (or a rank past the end: 0)
                v = wide ? digit << 8 : digit;
                if (wide) {
                    lf = rest;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (slot[k] == QH_NONE && (unsigned)(lane * 4 + k) == digit) slot[k] = (unsigned)t;
                }
            }
            if (lane == 0) { val[(int64_t)t * G + g] = v; left[(int64_t)t * G + g] = lf; }
        }
        if (wide)                                             // the gene's digit -> histogram table takes the place of its first histogram
#pragma unroll
            for (int k = 0; k < 4; ++k) h0[lane * 4 + k] = slot[k];
    } else {
        const unsigned *map = hist + g * 256;
        for (int t = 0; t < nt; ++t) {
            const unsigned lf = left[(int64_t)t * G + g];
            if (lf == QH_NONE) continue;                      // wave-uniform
            const unsigned v = val[(int64_t)t * G + g], s = map[(v >> 8) & 0xffu];
            unsigned digit = 0u, rest = 0u;
            if (s < (unsigned)nt) {
                const unsigned *h1 = hist + ((int64_t)(1 + s) * G + g) * 256;
                unsigned h[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) h[k] = h1[lane * 4 + k];
                const unsigned incl = wave_scan_incl(h[0] + h[1] + h[2] + h[3], lane);
                if (!wave_find_bin(h, incl, lf, lane, digit, rest)) digit = 0u;
            }
            if (lane == 0) { val[(int64_t)t * G + g] = (v & 0xff00u) | digit; left[(int64_t)t * G + g] = QH_NONE; }
        }
    }
}

__global__ __launch_bounds__(256) void k_csr_qfinish(const unsigned *__restrict__ val, QLerp q, int nq, double *__restrict__ out, int G)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    for (int i = 0; i < nq; ++i)
        out[(int64_t)i * G + g] = lerp_numpy((double)val[(int64_t)q.lo[i] * G + g], (double)val[(int64_t)q.hi[i] * G + g], q.t[i]);
}

static inline int q_passes(int count_dtype) { return count_dtype == VCY_U16 ? 2 : 1; }

}  // namespace vcy

using namespace vcy;

#define VCY_Q_SHAPE(who)                                                                                                      \
    VCY_REQUIRE(G >= 0 && G < (1LL << 31), who ": bad shape (0 <= G < 2^31)");                                                 \
    VCY_REQUIRE(count_dtype == VCY_U16 || count_dtype == VCY_U8, who ": count_dtype must be VCY_U16 or VCY_U8");               \
    VCY_REQUIRE(ntargets >= 1 && ntargets <= QH_MAXT, who ": ntargets outside [1, 32]")

extern "C" int64_t vcy_csr_quantiles_block_cells(void) { return QH_CELLS; }

extern "C" int vcy_csr_quantiles_passes(int count_dtype) { return count_dtype == VCY_U16 || count_dtype == VCY_U8 ? q_passes(count_dtype) : 0; }

extern "C" size_t vcy_csr_quantiles_state_bytes(int64_t G, int ntargets)
{
    if (G <= 0 || ntargets < 1 || ntargets > QH_MAXT) return 0;
    return (size_t)G * (size_t)ntargets * 2 * sizeof(unsigned);
}

extern "C" size_t vcy_csr_quantiles_hist_bytes(int64_t G, int ntargets, int count_dtype)
{
    if (G <= 0 || ntargets < 1 || ntargets > QH_MAXT) return 0;
    return (size_t)G * 256 * sizeof(unsigned) * (size_t)(1 + (count_dtype == VCY_U16 ? ntargets : 0));
}

extern "C" int vcy_csr_quantiles_begin(void *hist, int ntargets, int64_t G, int count_dtype, vcy_stream stream)
{
    VCY_Q_SHAPE("csr_quantiles_begin");
    if (G == 0) return VCY_OK;
    VCY_REQUIRE(hist, "csr_quantiles_begin: null pointer");
    VCY_CHECK_HIP(hipMemsetAsync(hist, 0, vcy_csr_quantiles_hist_bytes(G, ntargets, count_dtype), as_stream(stream)));
    return VCY_OK;
}

extern "C" int vcy_csr_quantiles_count(const int64_t *indptr, const int32_t *indices, const void *data, const int32_t *slabptr,
                                       const uint8_t *cell_mask, void *hist, int pass, int ntargets, int64_t C, int64_t G, int count_dtype,
                                       vcy_stream stream)
{
    VCY_Q_SHAPE("csr_quantiles_count");
    VCY_REQUIRE(C >= 0, "csr_quantiles_count: bad shape (C >= 0)");
    VCY_REQUIRE(pass >= 0 && pass < q_passes(count_dtype), "csr_quantiles_count: pass outside [0, passes)");
    if (G == 0 || C == 0) return VCY_OK;
    VCY_REQUIRE(indptr && indices && data && slabptr && hist, "csr_quantiles_count: null pointer");
    VCY_REQUIRE(vcy_csr_slab_genes() == QH_SLAB, "csr_quantiles_count: slab size differs from vcy_csr_slab_genes()");
    const int64_t tiles = (C + QH_CELLS - 1) / QH_CELLS, nslab = (G + QH_SLAB - 1) / QH_SLAB;
    VCY_REQUIRE(tiles < (1LL << 31) && nslab < 65536, "csr_quantiles_count: grid too large");
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)tiles, (unsigned)nslab), block(64 * QH_WAVES);
    unsigned *h0 = (unsigned *)hist, *h1 = h0 + G * 256;
    if (count_dtype == VCY_U8)
        hipLaunchKernelGGL((k_csr_hist<uint8_t, 0>), grid, block, 0, st, indptr, indices, (const uint8_t *)data, slabptr, cell_mask, (const unsigned *)nullptr,
                           h0, C, (int)G, (int)nslab, (unsigned)ntargets);
    else if (pass == 0)
        hipLaunchKernelGGL((k_csr_hist<uint16_t, 0>), grid, block, 0, st, indptr, indices, (const uint16_t *)data, slabptr, cell_mask,
                           (const unsigned *)nullptr, h0, C, (int)G, (int)nslab, (unsigned)ntargets);
    else
        hipLaunchKernelGGL((k_csr_hist<uint16_t, 1>), grid, block, 0, st, indptr, indices, (const uint16_t *)data, slabptr, cell_mask, (const unsigned *)h0,
                           h1, C, (int)G, (int)nslab, (unsigned)ntargets);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_csr_quantiles_advance(void *state, void *hist, const int64_t *ranks_host, int pass, int ntargets, int64_t n_cells, int64_t G,
                                         int count_dtype, vcy_stream stream)
{
    VCY_Q_SHAPE("csr_quantiles_advance");
    VCY_REQUIRE(pass >= 0 && pass < q_passes(count_dtype), "csr_quantiles_advance: pass outside [0, passes)");
    VCY_REQUIRE(n_cells >= 1 && n_cells < (1LL << 32), "csr_quantiles_advance: n_cells outside [1, 2^32)");
    VCY_REQUIRE(ranks_host, "csr_quantiles_advance: null pointer (ranks_host)");
    QRanks rk;
    for (int t = 0; t < QH_MAXT; ++t) rk.r[t] = 0;
    for (int t = 0; t < ntargets; ++t) {
        VCY_REQUIRE(ranks_host[t] >= 0 && ranks_host[t] < n_cells, "csr_quantiles_advance: rank outside [0, n_cells)");
        rk.r[t] = ranks_host[t];
    }
    if (G == 0) return VCY_OK;
    VCY_REQUIRE(state && hist, "csr_quantiles_advance: null pointer");
    unsigned *val = (unsigned *)state, *left = val + (int64_t)ntargets * G;
    const dim3 grid((unsigned)((G + 3) / 4));
    if (pass == 0)
        hipLaunchKernelGGL(k_csr_qadvance<0>, grid, dim3(256), 0, as_stream(stream), (unsigned *)hist, val, left, rk, ntargets, (long long)n_cells, (int)G,
                           count_dtype == VCY_U16 ? 1 : 0);
    else
        hipLaunchKernelGGL(k_csr_qadvance<1>, grid, dim3(256), 0, as_stream(stream), (unsigned *)hist, val, left, rk, ntargets, (long long)n_cells, (int)G, 1);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_csr_quantiles_finish(const void *state, const int *lo_target, const int *hi_target, const double *t_host, int nq, int ntargets,
                                        double *out, int64_t G, vcy_stream stream)
{
    VCY_REQUIRE(G >= 0 && G < (1LL << 31), "csr_quantiles_finish: bad shape (0 <= G < 2^31)");
    VCY_REQUIRE(ntargets >= 1 && ntargets <= QH_MAXT && nq >= 1 && nq <= QH_MAXQ, "csr_quantiles_finish: ntargets outside [1, 32] or nq outside [1, 16]");
    VCY_REQUIRE(lo_target && hi_target && t_host, "csr_quantiles_finish: null pointer");
    QLerp q;
    for (int i = 0; i < QH_MAXQ; ++i) { q.lo[i] = 0; q.hi[i] = 0; q.t[i] = 0.0; }
    for (int i = 0; i < nq; ++i) {
        VCY_REQUIRE(lo_target[i] >= 0 && lo_target[i] < ntargets && hi_target[i] >= 0 && hi_target[i] < ntargets, "csr_quantiles_finish: target outside [0, ntargets)");
        VCY_REQUIRE(t_host[i] >= 0.0 && t_host[i] < 1.0, "csr_quantiles_finish: fraction outside [0, 1)");
        q.lo[i] = lo_target[i]; q.hi[i] = hi_target[i]; q.t[i] = t_host[i];
    }
    if (G == 0) return VCY_OK;
    VCY_REQUIRE(state && out, "csr_quantiles_finish: null pointer");
    hipLaunchKernelGGL(k_csr_qfinish, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, as_stream(stream), (const unsigned *)state, q, nq, out, (int)G);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}
