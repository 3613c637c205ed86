// slices.hip -- the transposing pack / unpack of the gene-slice exchange (distributed.GeneSlices).
//
// A cell-sharded run keeps a rank's block of CELLS; the per-gene order statistics of fit_gammas (np.percentile over all cells,
// analysis.py:1197-1206) and the per-gene shuffle of the randomised control (analysis.py:1540-1541, 2407-2420) need all cells of a
// gene in one place.  The exchange moves a cells-sharded matrix to GENE slices (rank r: genes [g0_r, g1_r) of every cell) with one
// all-to-all, and back with another.  Both directions move blocks that are gene-major on the wire:
//
//   the N "virtual" cells of a buffer are split into nseg segments seg[j] .. seg[j+1] (seg[0] = 0, seg[nseg] = N), and
//   element (cell c, gene g) of segment j sits at  seg[j] * G + g * (seg[j+1] - seg[j]) + (c - seg[j]).
//
// With one segment this is the plain gene-major (G, N) transpose, whose consecutive gene ranges are the per-destination blocks of
// the forward direction; with the shard bounds as segments it is the concatenation of per-destination (G, n_j) blocks of the
// backward direction.  `row_map` (optional) names the row of the cells-major matrix that holds virtual cell c - the relabelling
// between a rank's cell order and the user's is applied inside the same pass.  One 64 x 64 LDS tile per workgroup: the cells-major
// side is read / written along genes, the wire side along cells, both coalesced.
#include "common.h"

namespace vcy {

__device__ __forceinline__ int64_t slice_pos(const int64_t *__restrict__ seg, int nseg, int64_t c, int64_t g, int64_t G)
{
    int j = 0;
    while (j + 1 < nseg && c >= seg[j + 1]) ++j;
    const int64_t a = seg[j], n = seg[j + 1] - a;
    return a * G + g * n + (c - a);
}

template <typename T>
__global__ __launch_bounds__(256) void k_slices_pack(const T *__restrict__ src, const int64_t *__restrict__ row_map,
                                                      const int64_t *__restrict__ seg, int nseg, T *__restrict__ buf, int64_t N,
                                                      int64_t G, int64_t ld)
{
    __shared__ T tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.y * 64, g0 = (int64_t)blockIdx.x * 64;
    for (int j = ty; j < 64; j += 4) {                       // lanes along genes: one row segment of the cells-major matrix
        const int64_t c = c0 + j, g = g0 + tx;
        T v = T(0);
        if (c < N && g < G) v = src[(row_map ? row_map[c] : c) * ld + g];
        tile[j][tx] = v;
    }
    __syncthreads();
    for (int j = ty; j < 64; j += 4) {                       // lanes along cells: one run of a gene row on the wire
        const int64_t g = g0 + j, c = c0 + tx;
        if (c < N && g < G) buf[slice_pos(seg, nseg, c, g, G)] = tile[tx][j];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_slices_unpack(const T *__restrict__ buf, const int64_t *__restrict__ row_map,
                                                        const int64_t *__restrict__ seg, int nseg, T *__restrict__ dst, int64_t N,
                                                        int64_t G, int64_t ld)
{
    __shared__ T tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.y * 64, g0 = (int64_t)blockIdx.x * 64;
    for (int j = ty; j < 64; j += 4) {
        const int64_t g = g0 + j, c = c0 + tx;
        T v = T(0);
        if (c < N && g < G) v = buf[slice_pos(seg, nseg, c, g, G)];
        tile[tx][j] = v;
    }
    __syncthreads();
    for (int j = ty; j < 64; j += 4) {
        const int64_t c = c0 + j, g = g0 + tx;
        if (c < N && g < G) dst[(row_map ? row_map[c] : c) * ld + g] = tile[j][tx];
    }
}

template <bool PACK>
static int slices_launch(const void *a, const int64_t *row_map, const int64_t *seg, int nseg, void *b, int64_t N, int64_t G, int64_t ld,
                         int dtype, vcy_stream stream, const char *what)
{
    VCY_REQUIRE(a && b && seg && a != b && nseg > 0 && nseg <= 4096, what);
    VCY_REQUIRE(N > 0 && G > 0 && ld >= G && G < (1ll << 31) && (N + 63) / 64 <= 65535, what);
    VCY_REQUIRE(dtype == VCY_F32 || dtype == VCY_F64, what);
    const dim3 grid((unsigned)((G + 63) / 64), (unsigned)((N + 63) / 64));
    hipStream_t st = as_stream(stream);
    if (PACK) {
        if (dtype == VCY_F32) hipLaunchKernelGGL(k_slices_pack<float>, grid, dim3(256), 0, st, (const float *)a, row_map, seg, nseg, (float *)b, N, G, ld);
        else hipLaunchKernelGGL(k_slices_pack<double>, grid, dim3(256), 0, st, (const double *)a, row_map, seg, nseg, (double *)b, N, G, ld);
    } else {
        if (dtype == VCY_F32) hipLaunchKernelGGL(k_slices_unpack<float>, grid, dim3(256), 0, st, (const float *)a, row_map, seg, nseg, (float *)b, N, G, ld);
        else hipLaunchKernelGGL(k_slices_unpack<double>, grid, dim3(256), 0, st, (const double *)a, row_map, seg, nseg, (double *)b, N, G, ld);
    }
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

}  // namespace vcy

using namespace vcy;

extern "C" int vcy_gene_slices_pack(const void *src, const int64_t *row_map, const int64_t *seg, int nseg, void *buf, int64_t N, int64_t G,
                                    int64_t ld, int dtype, vcy_stream stream)
{
    return slices_launch<true>(src, row_map, seg, nseg, buf, N, G, ld, dtype, stream, "gene_slices_pack: bad arguments");
}

extern "C" int vcy_gene_slices_unpack(const void *buf, const int64_t *row_map, const int64_t *seg, int nseg, void *dst, int64_t N, int64_t G,
                                      int64_t ld, int dtype, vcy_stream stream)
{
    return slices_launch<false>(buf, row_map, seg, nseg, dst, N, G, ld, dtype, stream, "gene_slices_unpack: bad arguments");
}
