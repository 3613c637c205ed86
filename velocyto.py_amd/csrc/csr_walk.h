// csr_walk.h -- the element walk of the kernels that visit a (cell tile) x (gene slab) of a cells-major CSR count layer through the
// per-row slab table of vcy_csr_slab_ptr: k_csr_gene_stats, k_csr_gene_stats_parts (csr_select.hip) and k_csr_hist (csr_quantiles.hip).
#pragma once
#include "common.h"

namespace vcy {

// Calls add(gene number inside the slab, stored count) once for every stored element of the rows [c0, c1) with cell_mask != 0 whose gene
// lies in slab `slab`; g0 = the slab's first gene.  The gene number is NOT range-checked here (a malformed table can hand out anything):
// `add` refuses what it cannot hold.
// A wave takes 64 rows at a time, lane = row: the rows' facts (mask byte, start and length of the slab's segment) are ONE round
// trip for 64 rows, and masked-out or empty rows cost nothing after it.  The rows with something in the slab are then walked
// ROWS at a time: the first NZ x 64 elements of each are requested together - the request phase is nothing but loads, so
// ROWS x NZ x 2 of them are in flight per lane before the first atomic waits - and applied; longer segments finish in a loop.
template <typename CT, int WAVES, int ROWS, int NZ, typename F>
__device__ __forceinline__ void csr_slab_walk(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const CT *__restrict__ data,
                                              const int32_t *__restrict__ slabptr, const uint8_t *__restrict__ cell_mask, int64_t c0, int64_t c1,
                                              int64_t nnz, int slab, int nslab, int g0, F add)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t r0 = c0 + (int64_t)wave * 64; r0 < c1; r0 += 64 * WAVES) {
        const int64_t r = r0 + lane;
        int64_t a_l = 0;
        int n_l = 0;
        if (r < c1 && (!cell_mask || cell_mask[r])) {
            const int32_t *sp = slabptr + r * (nslab + 1) + slab;
            a_l = indptr[r] + sp[0];
            n_l = sp[1] - sp[0];
            if (a_l < 0 || a_l >= nnz || n_l < 0) n_l = 0;    // every position stays inside [0, nnz)
            n_l = (int)min((int64_t)n_l, nnz - a_l);
        }
        unsigned long long todo = __ballot(n_l > 0);
        while (todo) {
            int64_t a[ROWS];
            int n[ROWS];
            int gi[ROWS][NZ];
            unsigned xv[ROWS][NZ];
#pragma unroll
            for (int q = 0; q < ROWS; ++q) {
                const int u = todo ? __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1) : 0;
                n[q] = todo ? __builtin_amdgcn_readlane(n_l, u) : 0;
                a[q] = ((int64_t)__builtin_amdgcn_readlane((int)(a_l >> 32), u) << 32) | (unsigned)__builtin_amdgcn_readlane((int)a_l, u);
                todo &= todo - 1;
#pragma unroll
                for (int k = 0; k < NZ; ++k) {
                    const int t = k * 64 + lane;
                    gi[q][k] = -1;
                    xv[q][k] = 0u;
                    if (t < n[q]) {
                        gi[q][k] = indices[a[q] + t] - g0;
                        xv[q][k] = (unsigned)data[a[q] + t];
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < ROWS; ++q) {
#pragma unroll
                for (int k = 0; k < NZ; ++k) add((unsigned)gi[q][k], xv[q][k]);
                for (int t = NZ * 64 + lane; t < n[q]; t += 64) add((unsigned)(indices[a[q] + t] - g0), (unsigned)data[a[q] + t]);
            }
        }
    }
}

}  // namespace vcy
