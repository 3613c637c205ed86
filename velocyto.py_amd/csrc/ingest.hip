// ingest.hip -- .loom ingest: a gene-major block of a count layer, in the file's own element type, validated, converted, transposed and
// compacted on the device; and the host loop that fills such a block from the file's chunks.
//
// Reference: VelocytoLoom.__init__ (analysis.py:56-67) loads /layers/spliced, unspliced, ambiguous whole as float64 (genes, cells) and
// sums them per cell.  Here a layer arrives in blocks of cells (loom_io.LayerBlockReader): the tile is (G genes, B cells), row stride
// ldt >= B elements, element type u8 / u16 / u32 / i32 / i64 / f32 / f64 as stored in the file.
//
// k_loom_tile<T, MODE>: grid = (stripes of LT_CELLS = 64 cells) x (slabs of LT_SLAB = 1024 genes), 4 waves.  The tile is read ONCE per
// launch, lane = cell: a wave-load is 64 consecutive cells of one gene row (coalesced along the cells), 16 gene rows of a wave in flight.
// On the way in every element is validated and converted to its uint16 count (`conv`).
//   COUNT: each lane keeps its cell's non-zero count, sum, flags and maximum over the slab; the four waves meet in LDS and the slab's
//          partial per cell goes to the workspace with plain stores.  No LDS tile, no transposition needed.
//   FILL:  the converted 64 x 64 sub-tile goes to LDS as [cell][gene] (pitch 66 halfwords = 33 dwords: the 32 lanes of a store group
//          fall on 32 banks); then a wave takes a cell's row with lane = gene, and the row's non-zeros are compacted in order by ballot +
//          prefix count - genes ascending inside the cell's row - behind the cell's cursor.  The cursor starts at row_start[c] + the
//          non-zeros of the slabs in front (the COUNT launch's partials) and ends at the slab's own partial.  Two LDS images alternate,
//          so there is one barrier per sub-tile.
//   DENSE: the same with 128 genes per sub-tile (pitch 130 halfwords = 65 dwords) and a lane writing genes 2l, 2l + 1 of the cell's row
//          of the cells-major uint16 matrix as one dword (256 B per wave-store), zeros in the padding columns; the COUNT sums as well.
// k_loom_fold adds the slabs' partials per cell (integers: the order is immaterial) and leaves one (flags, max) pair per 256 cells;
// k_loom_result folds those into the result block.  No global atomics of any kind.
//
// conv.  A stored zero (-0.0 included) counts in nothing.  Flags: 1 = an element is not an integer (NaN and +-inf included), 2 = an
// element is negative, 4 = an element exceeds 65535.  A NaN or an infinity sets flag 1 only.  The maximum is over the elements
// clamped to 0 .. 2^62 (NaN: 0).  A non-zero element that is no valid count is carried as 65535, so COUNT and FILL agree on what is
// stored whatever the tile holds; sums and data mean something only when no flag is set.
// Every position is clamped: FILL writes inside [max(row_start[c], 0), min(row_start[c + 1], capacity)) only, whatever the workspace
// holds; DENSE writes rows s .. s + B - 1 < C and columns < ld only.
//
// vcy_loom_block_host: the host side of a block (no device work).  `threads` std::threads take chunks from a shared counter: fetch
// the chunk's stored bytes from the HDF5 library (H5Dget_chunk_storage_size + H5Dread_chunk, handed in as function pointers: this
// library does not link HDF5; both find the chunk through the dataset's index, where H5Dget_chunk_info_by_coord of 1.10 walks the
// index from its start - 8 ms per chunk at 480 000 chunks), inflate (zlib), undo the byte shuffle, and place the chunk's rows, cropped
// to the dataset and to the block, into the tile.
#include "common.h"

#include <atomic>
#include <type_traits>
#include <thread>
#include <vector>
#include <zlib.h>

namespace vcy {

constexpr int LT_CELLS = 64;          // cells per workgroup stripe (lane = cell on the way in)
constexpr int LT_SLAB = 1024;         // genes per workgroup (vcy_loom_tile_slab_genes)
constexpr int LT_WAVES = 4;
constexpr int LT_ROWS = 16;           // gene rows of a wave requested together
constexpr int LT_FOLD = 256;          // cells per workgroup of k_loom_fold

enum { LT_COUNT = 0, LT_FILL = 1, LT_DENSE = 2 };

struct LoomWs {                       // views into the workspace; Bp = stripes * 64 cells, entry [slab * Bp + cell]
    unsigned long long *sum;
    long long *mx;
    int *nnz;
    int *flags;
    long long *blk;                   // [2 * fold blocks]: flags, max per LT_FOLD cells
    int64_t Bp, nslab, nfold;
};

static inline int64_t lt_stripes(int64_t B) { return (B + LT_CELLS - 1) / LT_CELLS; }
static inline int64_t lt_slabs(int64_t G) { return (G + LT_SLAB - 1) / LT_SLAB; }

static inline LoomWs lt_views(void *workspace, int64_t G, int64_t B)
{
    LoomWs w;
    w.Bp = lt_stripes(B) * LT_CELLS;
    w.nslab = lt_slabs(G);
    w.nfold = (w.Bp + LT_FOLD - 1) / LT_FOLD;
    const int64_t n = w.nslab * w.Bp;
    w.sum = (unsigned long long *)workspace;
    w.mx = (long long *)(w.sum + n);
    w.nnz = (int *)(w.mx + n);
    w.flags = w.nnz + n;
    w.blk = (long long *)(w.flags + n);
    return w;
}

// element -> uint16 count; flags and maximum updated
template <typename T> __device__ __forceinline__ unsigned conv(T x, int &flags, long long &mx)
{
    if constexpr (sizeof(T) <= 2) {                                   // u8, u16: every value is a count
        mx = max(mx, (long long)x);
        return (unsigned)x;
    } else if constexpr (std::is_floating_point<T>::value) {
        if (x == (T)0) return 0u;                                     // -0.0 too
        if (!(x == x) || x == (T)INFINITY || x == -(T)INFINITY) { flags |= 1; return 65535u; }
        const bool frac = x != rint(x), neg = x < (T)0, over = x > (T)65535;
        flags |= (frac ? 1 : 0) | (neg ? 2 : 0) | (over ? 4 : 0);
        if (!neg) mx = max(mx, (long long)min(x, (T)4611686018427387904.0));
        return (frac || neg || over) ? 65535u : (unsigned)x;
    } else {
        const bool neg = x < (T)0, over = !neg && (unsigned long long)x > 65535ull;
        flags |= (neg ? 2 : 0) | (over ? 4 : 0);
        if (!neg) mx = max(mx, (long long)x);
        return (neg || over) ? 65535u : (unsigned)x;
    }
}

__device__ __forceinline__ int64_t readlane64(int64_t v, int l)
{
    return ((int64_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)v, l);
}

template <typename T, int MODE>
__global__ __launch_bounds__(64 * LT_WAVES) void k_loom_tile(const T *__restrict__ tile, LoomWs ws, const int64_t *__restrict__ row_start,
                                                              int32_t *__restrict__ indices, uint16_t *__restrict__ data, int64_t capacity,
                                                              uint16_t *__restrict__ dense, int64_t s, int64_t C, int64_t ld, int G, int64_t B,
                                                              int64_t ldt)
{
    constexpr int GT = MODE == LT_DENSE ? 128 : 64;                   // genes per sub-tile
    constexpr int PITCH = GT + 2;                                     // halfwords per cell row of the LDS image: (GT / 2 + 1) dwords, odd
    constexpr int NR = GT / LT_WAVES;                                 // gene rows a wave brings in per sub-tile
    __shared__ alignas(16) uint16_t img[MODE == LT_COUNT ? 1 : 2][MODE == LT_COUNT ? 1 : LT_CELLS * PITCH];
    __shared__ unsigned long long r_sum[LT_WAVES][64];
    __shared__ long long r_mx[LT_WAVES][64];
    __shared__ int r_nnz[LT_WAVES][64], r_flags[LT_WAVES][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c0 = (int64_t)blockIdx.x * LT_CELLS, c = c0 + lane;
    const int slab = blockIdx.y, g0 = slab * LT_SLAB, g1 = g0 + LT_SLAB;             // the grid covers G (DENSE: ld) genes
    const bool in = c < B;
    unsigned long long sum = 0;
    long long mx = 0;
    int nnz = 0, flags = 0;
    // FILL: lane j < 16 of wave w owns the cursor of cell c0 + 16 w + j
    int64_t cur = 0, end = 0;
    if constexpr (MODE == LT_FILL) {
        const int64_t cc = c0 + wave * 16 + (lane & 15);
        if (cc < B) {
            int64_t o = max(row_start[cc], (int64_t)0);
            for (int sl = 0; sl < slab; ++sl) o += max(ws.nnz[(int64_t)sl * ws.Bp + cc], 0);
            cur = o;
            end = min(min(o + max(ws.nnz[(int64_t)slab * ws.Bp + cc], 0), row_start[cc + 1]), capacity);
        }
    }
    int it = 0;
    for (int gs = g0; gs < g1 && gs < (MODE == LT_DENSE ? (int)ld : G); gs += GT, ++it) {
        // in: wave w takes gene rows gs + w, gs + w + 4, ...; LT_ROWS loads per lane before the first is used
#pragma unroll
        for (int h = 0; h < NR; h += LT_ROWS) {
            T x[LT_ROWS];
#pragma unroll
            for (int k = 0; k < LT_ROWS; ++k) {
                const int g = gs + (h + k) * LT_WAVES + wave;
                x[k] = (T)0;
                if (in && g < G) x[k] = tile[(int64_t)g * ldt + c];
            }
#pragma unroll
            for (int k = 0; k < LT_ROWS; ++k) {
                const unsigned v = conv<T>(x[k], flags, mx);
                if constexpr (MODE != LT_FILL) {
                    nnz += v != 0u;
                    sum += v;
                }
                if constexpr (MODE != LT_COUNT) img[it & 1][lane * PITCH + (h + k) * LT_WAVES + wave] = (uint16_t)v;
            }
        }
        if constexpr (MODE == LT_COUNT) continue;
        __syncthreads();              // one barrier per sub-tile: the next one goes to the other image
        if constexpr (MODE == LT_FILL) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const unsigned v = img[it & 1][(wave * 16 + j) * PITCH + lane];
                const unsigned long long kept = __ballot(v != 0u);
                const int before = __popcll(kept & ((1ull << lane) - 1ull));          // kept genes in front of this lane's: ascending order
                const int64_t q = readlane64(cur, j) + before, q_end = readlane64(end, j);
                if (v != 0u && q < q_end) {
                    indices[q] = gs + lane;
                    data[q] = (uint16_t)v;
                }
                if (lane == j) cur += __popcll(kept);
            }
        }
        if constexpr (MODE == LT_DENSE) {
            const int g = gs + 2 * lane;                                               // ld is a multiple of 2 and gs of 128: dword stores
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int cl = wave * 16 + j;
                const unsigned v2 = *reinterpret_cast<const unsigned *>(&img[it & 1][cl * PITCH + 2 * lane]);
                const int64_t row = s + c0 + cl;
                if (c0 + cl < B && row < C && g + 1 < ld) *reinterpret_cast<unsigned *>(dense + row * ld + g) = v2;
            }
        }
    }
    if constexpr (MODE == LT_FILL) return;
    r_sum[wave][lane] = sum; r_mx[wave][lane] = mx; r_nnz[wave][lane] = nnz; r_flags[wave][lane] = flags;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < LT_WAVES; ++w) { sum += r_sum[w][lane]; mx = max(mx, r_mx[w][lane]); nnz += r_nnz[w][lane]; flags |= r_flags[w][lane]; }
    const int64_t o = (int64_t)slab * ws.Bp + c;                                       // c < Bp: the padded cells are written too (zeros)
    ws.sum[o] = sum; ws.mx[o] = mx; ws.nnz[o] = nnz; ws.flags[o] = flags;
}

// per cell: the slabs' partials added up; per workgroup: (flags, max) of its LT_FOLD cells
__global__ __launch_bounds__(LT_FOLD) void k_loom_fold(LoomWs ws, int64_t *__restrict__ nnz_out, int64_t *__restrict__ sums, int64_t B)
{
    __shared__ int s_flags;
    __shared__ long long s_mx;
    if (threadIdx.x == 0) { s_flags = 0; s_mx = 0; }
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * LT_FOLD + threadIdx.x;
    if (c < ws.Bp) {
        unsigned long long sum = 0;
        long long mx = 0, n = 0;
        int flags = 0;
        for (int64_t sl = 0; sl < ws.nslab; ++sl) {
            const int64_t o = sl * ws.Bp + c;
            sum += ws.sum[o]; mx = max(mx, ws.mx[o]); n += ws.nnz[o]; flags |= ws.flags[o];
        }
        if (c < B) {
            if (nnz_out) nnz_out[c] = n;
            if (sums) sums[c] = (int64_t)sum;
        }
        if (flags) atomicOr(&s_flags, flags);                                          // LDS atomics
        if (mx) atomicMax(&s_mx, mx);
    }
    __syncthreads();
    if (threadIdx.x == 0) { ws.blk[2 * blockIdx.x] = s_flags; ws.blk[2 * blockIdx.x + 1] = s_mx; }
}

// result[4] = { any non-integer, any negative, any above 65535, largest value }
__global__ __launch_bounds__(64) void k_loom_result(LoomWs ws, int64_t *__restrict__ result)
{
    long long flags = 0, mx = 0;
    for (int64_t b = threadIdx.x; b < ws.nfold; b += 64) { flags |= ws.blk[2 * b]; mx = max(mx, ws.blk[2 * b + 1]); }
    const bool f1 = __ballot((flags & 1) != 0) != 0, f2 = __ballot((flags & 2) != 0) != 0, f4 = __ballot((flags & 4) != 0) != 0;
    mx = wave_max(mx);
    if (threadIdx.x == 0) { result[0] = f1; result[1] = f2; result[2] = f4; result[3] = mx; }
}

template <int MODE>
static int lt_launch(int elem, dim3 grid, hipStream_t st, const void *tile, LoomWs ws, const int64_t *row_start, int32_t *indices, uint16_t *data,
                     int64_t capacity, uint16_t *dense, int64_t s, int64_t C, int64_t ld, int G, int64_t B, int64_t ldt)
{
#define VCY_LT_CASE(code, T)                                                                                                            \
    case code:                                                                                                                          \
        hipLaunchKernelGGL((k_loom_tile<T, MODE>), grid, dim3(64 * LT_WAVES), 0, st, (const T *)tile, ws, row_start, indices, data, capacity, dense, s, \
                           C, ld, G, B, ldt);                                                                                           \
        break;
    switch (elem) {
        VCY_LT_CASE(VCY_LOOM_U8, uint8_t)
        VCY_LT_CASE(VCY_LOOM_U16, uint16_t)
        VCY_LT_CASE(VCY_LOOM_U32, uint32_t)
        VCY_LT_CASE(VCY_LOOM_I32, int32_t)
        VCY_LT_CASE(VCY_LOOM_I64, int64_t)
        VCY_LT_CASE(VCY_LOOM_F32, float)
        VCY_LT_CASE(VCY_LOOM_F64, double)
    default:
        return fail(VCY_ERR_INVALID, "%s: elem_type must be one of VCY_LOOM_U8 .. VCY_LOOM_F64", "loom_tile");
    }
#undef VCY_LT_CASE
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

static int lt_fold(LoomWs ws, int64_t *nnz, int64_t *sums, int64_t *result, int64_t B, hipStream_t st)
{
    hipLaunchKernelGGL(k_loom_fold, dim3((unsigned)ws.nfold), dim3(LT_FOLD), 0, st, ws, nnz, sums, B);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_loom_result, dim3(1), dim3(64), 0, st, ws, result);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

static inline int lt_elem_size(int elem)
{
    switch (elem) {
    case VCY_LOOM_U8: return 1;
    case VCY_LOOM_U16: return 2;
    case VCY_LOOM_U32: case VCY_LOOM_I32: case VCY_LOOM_F32: return 4;
    case VCY_LOOM_I64: case VCY_LOOM_F64: return 8;
    default: return 0;
    }
}

}  // namespace vcy

using namespace vcy;

#define VCY_LT_SHAPE(who)                                                                                                        \
    VCY_REQUIRE(G > 0 && G < (1LL << 31) - 2 * LT_SLAB && B > 0 && ldt >= B, who ": bad shape (0 < G < 2^31 - 2048, B > 0, ldt >= B)"); \
    VCY_REQUIRE(lt_elem_size(elem_type) > 0, who ": elem_type must be one of VCY_LOOM_U8 .. VCY_LOOM_F64");                         \
    VCY_REQUIRE(tile && workspace, who ": null pointer");                                                                          \
    VCY_REQUIRE((uintptr_t)tile % lt_elem_size(elem_type) == 0 && (uintptr_t)workspace % 8 == 0, who ": misaligned tile or workspace"); \
    VCY_REQUIRE(lt_stripes(B) < (1LL << 31), who ": grid too large")

extern "C" int64_t vcy_loom_tile_slab_genes(void) { return LT_SLAB; }

extern "C" size_t vcy_loom_tile_workspace_bytes(int64_t G, int64_t B)
{
    if (G <= 0 || B <= 0) return 0;
    const int64_t Bp = lt_stripes(B) * LT_CELLS;
    return (size_t)lt_slabs(G) * (size_t)Bp * 24 + (size_t)((Bp + LT_FOLD - 1) / LT_FOLD) * 16;
}

extern "C" int vcy_loom_tile_count(const void *tile, int64_t *nnz, int64_t *sums, int64_t *result, void *workspace, int64_t G, int64_t B,
                                   int64_t ldt, int elem_type, vcy_stream stream)
{
    VCY_LT_SHAPE("loom_tile_count");
    VCY_REQUIRE(nnz && sums && result, "loom_tile_count: null pointer");
    const LoomWs ws = lt_views(workspace, G, B);
    hipStream_t st = as_stream(stream);
    const int rc = lt_launch<LT_COUNT>(elem_type, dim3((unsigned)lt_stripes(B), (unsigned)ws.nslab), st, tile, ws, nullptr, nullptr, nullptr, 0, nullptr,
                                       0, 0, 0, (int)G, B, ldt);
    return rc != VCY_OK ? rc : lt_fold(ws, nnz, sums, result, B, st);
}

extern "C" int vcy_loom_tile_fill(const void *tile, const void *workspace, const int64_t *row_start, int32_t *indices, void *data,
                                  int64_t capacity, int64_t G, int64_t B, int64_t ldt, int elem_type, vcy_stream stream)
{
    VCY_LT_SHAPE("loom_tile_fill");
    VCY_REQUIRE(row_start && capacity >= 0, "loom_tile_fill: null pointer (row_start) or negative capacity");
    if (capacity == 0) return VCY_OK;
    VCY_REQUIRE(indices && data, "loom_tile_fill: null pointer");
    const LoomWs ws = lt_views(const_cast<void *>(workspace), G, B);
    return lt_launch<LT_FILL>(elem_type, dim3((unsigned)lt_stripes(B), (unsigned)ws.nslab), as_stream(stream), tile, ws, row_start, indices,
                              (uint16_t *)data, capacity, nullptr, 0, 0, 0, (int)G, B, ldt);
}

extern "C" int vcy_loom_tile_dense(const void *tile, void *out, int64_t *sums, int64_t *result, void *workspace, int64_t G, int64_t B,
                                   int64_t ldt, int elem_type, int64_t s, int64_t C, int64_t ld, vcy_stream stream)
{
    VCY_LT_SHAPE("loom_tile_dense");
    VCY_REQUIRE(out && sums && result, "loom_tile_dense: null pointer");
    VCY_REQUIRE(s >= 0 && s + B <= C && ld >= G && ld % 2 == 0 && ld < (1LL << 31) - 2 * LT_SLAB, "loom_tile_dense: bad output shape (0 <= s, s + B <= C, G <= ld even)");
    VCY_REQUIRE((uintptr_t)out % 4 == 0, "loom_tile_dense: out must be 4-byte aligned");
    const LoomWs ws = lt_views(workspace, ld, B);                                       // the slabs cover the padding columns: workspace for (ld, B)
    hipStream_t st = as_stream(stream);
    const int rc = lt_launch<LT_DENSE>(elem_type, dim3((unsigned)lt_stripes(B), (unsigned)ws.nslab), st, tile, ws, nullptr, nullptr, nullptr, 0,
                                       (uint16_t *)out, s, C, ld, (int)G, B, ldt);
    return rc != VCY_OK ? rc : lt_fold(ws, nullptr, sums, result, B, st);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host: one block of cells from the file's chunks
namespace vcy {

// the HDF5 calls a block needs, handed in by the caller (this library does not link HDF5)
typedef int (*h5_chunk_size_fn)(int64_t dset, const uint64_t *offset, uint64_t *nbytes);                       // H5Dget_chunk_storage_size
typedef int (*h5_read_chunk_fn)(int64_t dset, int64_t dxpl, const uint64_t *offset, uint32_t *mask, void *buf); // H5Dread_chunk
typedef int (*h5_quiet_fn)(int64_t estack, void *func, void *client_data);                                     // H5Eset_auto2
typedef int (*h5_clear_fn)(int64_t estack);                                                                    // H5Eclear2

struct ChunkJob {
    h5_chunk_size_fn chunk_size;
    h5_read_chunk_fn read_chunk;
    h5_quiet_fn quiet;
    h5_clear_fn clear;
    int64_t dset;
    int64_t G, C, ch_r, ch_c, c0, c1, ldt, nchunks, ncc, cc0;
    int esz, filters;
    uint8_t *tile;
    std::atomic<int64_t> next{0};
    std::atomic<int64_t> bad{-1};
    std::atomic<int> status{0};
    void stop(int code, int64_t k) { int z = 0; if (status.compare_exchange_strong(z, code)) bad.store(k); }
};

static void chunk_worker(ChunkJob *J)
{
    // a chunk that was never written makes H5Dget_chunk_storage_size fail, which is an answer here, not a diagnostic: this thread's
    // error stack (the thread-safe library keeps one per thread, and this thread ends with the call) stops printing
    if (J->quiet) J->quiet(0, nullptr, nullptr);
    const size_t raw = (size_t)J->ch_r * (size_t)J->ch_c * (size_t)J->esz;
    std::vector<uint8_t> stored(2 * raw + 4096), plain(raw), tmp(J->filters == 2 ? raw : 0);
    for (;;) {
        const int64_t k = J->next.fetch_add(1);
        if (k >= J->nchunks || J->status.load() != 0) return;
        const int64_t cr = k / J->ncc, cc = J->cc0 + k % J->ncc;                       // chunk row / column in the dataset's chunk grid
        const int64_t g_lo = cr * J->ch_r, g_hi = std::min(J->G, g_lo + J->ch_r);
        const int64_t x_lo = std::max(J->c0, cc * J->ch_c), x_hi = std::min(std::min(J->c1, J->C), (cc + 1) * J->ch_c);
        if (g_lo >= g_hi || x_lo >= x_hi) continue;
        const size_t w = (size_t)(x_hi - x_lo) * J->esz;
        const uint64_t at[2] = {(uint64_t)g_lo, (uint64_t)(cc * J->ch_c)};
        uint64_t nb64 = 0;
        if (J->chunk_size(J->dset, at, &nb64) < 0 || nb64 == 0) {                      // never written: the fill value, which the caller checked is zero
            if (J->clear) J->clear(0);                                                 // the failed call's records must not outlive this thread
            for (int64_t g = g_lo; g < g_hi; ++g) memset(J->tile + ((size_t)g * J->ldt + (x_lo - J->c0)) * J->esz, 0, w);
            continue;
        }
        const size_t nb = (size_t)nb64;
        if (nb > stored.size()) { J->stop(-4, k); return; }                            // deflate never grows a chunk by more than a few bytes
        uint32_t m = 0;
        if (J->read_chunk(J->dset, 0, at, &m, stored.data()) < 0) { J->stop(-5, k); return; }     // the library serialises its calls itself
        const bool deflated = J->filters >= 1 && !(m & (J->filters == 2 ? 2u : 1u)), shuffled = J->filters == 2 && !(m & 1u);
        const uint8_t *src = stored.data();
        if (deflated) {
            uLongf n = (uLongf)raw;
            if (uncompress(plain.data(), &n, stored.data(), (uLong)nb) != Z_OK || (size_t)n != raw) { J->stop(-4, k); return; }
            src = plain.data();
        } else if (nb != raw) { J->stop(-4, k); return; }
        if (shuffled && J->esz > 1) {                                                  // byte b of element i was stored at b * n + i
            const size_t n = raw / J->esz;
            for (int b = 0; b < J->esz; ++b)
                for (size_t i = 0; i < n; ++i) tmp[i * J->esz + b] = src[(size_t)b * n + i];
            src = tmp.data();
        }
        for (int64_t g = g_lo; g < g_hi; ++g)
            memcpy(J->tile + ((size_t)g * J->ldt + (x_lo - J->c0)) * J->esz,
                   src + ((size_t)(g - g_lo) * J->ch_c + (x_lo - cc * J->ch_c)) * J->esz, w);
    }
}

}  // namespace vcy

extern "C" int vcy_loom_block_host(void *const *hdf5_calls, int64_t dset, int64_t G, int64_t C, int64_t chunk_rows, int64_t chunk_cols,
                                   int elem_size, int filters, int64_t c0, int64_t c1, void *tile, int64_t ldt, int threads, int64_t *bad_chunk)
{
    VCY_REQUIRE(G > 0 && C > 0 && chunk_rows > 0 && chunk_cols > 0 && 0 <= c0 && c0 < c1 && c1 <= C && ldt >= c1 - c0, "loom_block_host: bad shape");
    VCY_REQUIRE(elem_size == 1 || elem_size == 2 || elem_size == 4 || elem_size == 8, "loom_block_host: elem_size must be 1, 2, 4 or 8");
    VCY_REQUIRE(filters >= 0 && filters <= 2, "loom_block_host: filters must be 0 (none), 1 (deflate) or 2 (shuffle + deflate)");
    VCY_REQUIRE(hdf5_calls && hdf5_calls[0] && hdf5_calls[1] && tile, "loom_block_host: null pointer");
    VCY_REQUIRE(threads >= 1 && threads <= 16, "loom_block_host: threads must be 1 .. 16");
    ChunkJob J;
    J.chunk_size = (h5_chunk_size_fn)hdf5_calls[0]; J.read_chunk = (h5_read_chunk_fn)hdf5_calls[1]; J.quiet = (h5_quiet_fn)hdf5_calls[2]; J.clear = (h5_clear_fn)hdf5_calls[3];
    J.dset = dset;
    J.G = G; J.C = C; J.ch_r = chunk_rows; J.ch_c = chunk_cols; J.c0 = c0; J.c1 = c1; J.ldt = ldt;
    J.cc0 = c0 / chunk_cols;
    J.ncc = (c1 - 1) / chunk_cols - J.cc0 + 1;
    J.nchunks = ((G + chunk_rows - 1) / chunk_rows) * J.ncc;
    J.esz = elem_size; J.filters = filters; J.tile = (uint8_t *)tile;
    const int nt = (int)std::min<int64_t>(threads, J.nchunks);
    std::vector<std::thread> pool;                                                     // the caller's thread only waits: its HDF5 error stack stays as it is
    for (int t = 0; t < nt; ++t) pool.emplace_back(chunk_worker, &J);
    for (auto &t : pool) t.join();
    if (bad_chunk) *bad_chunk = J.bad.load();
    if (J.status.load() == -4) return fail(-4, "loom_block_host: chunk %s%lld of the block does not inflate to the chunk size", "", (long long)J.bad.load());
    if (J.status.load() == -5) return fail(-5, "loom_block_host: chunk %s%lld of the block could not be read", "", (long long)J.bad.load());
    return VCY_OK;
}
