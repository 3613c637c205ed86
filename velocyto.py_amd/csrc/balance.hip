// balance.hip -- the balanced kNN selection (neighbors.py:11-183) as a fixed-point iteration on the device.
//
// The reference's greedy loop visits the cells in the order lsi (descending in-degree of the sight graph, ties by descending cell
// number) and lets cell el take node m while fewer than maxl cells visited earlier have taken m.  With rank[lsi[i]] = i and
//
//     s[m] = the maxl-th smallest rank among the cells that take m   (n when fewer than maxl cells take it)
//
// node m is open to el exactly when rank[el] <= s[m].  One ROUND lets every cell walk its sight list against the thresholds of the
// previous round (k_balance_select) and then recomputes the thresholds from who took what (k_balance_thresholds).  The selection of
// the cell of rank r depends on the selections of smaller ranks only, so after round t the cells of rank < t hold the loop's
// selection for good: the iteration ends after at most n rounds, at the loop's result; real inputs take a handful.
// Everything is integer and every output is a function of a SET of integers: no launch order, no atomic fill order can change a bit.
//
// The round loop lives with the caller (the entry points never synchronise): it reads the 4-byte change flag once per round.
//   vcy_balance_select      one wave per cell walks the sight list, writes the picks' positions, one sort key per slot, the flag
//   (caller)                sorts the n * k keys (any sort: the keys of real picks are distinct)
//   vcy_balance_thresholds  s[m] and the in-degree l[m] from the sorted keys
//   vcy_balance_finish      the arrays of vcy_balance_knn_host32 from the final selection
#include "common.h"

namespace vcy {

// A key is (m << 32) | rank[el]: sorted, the takers of a node are one run, in rank order.  The key of an empty slot is the largest
// SIGNED 64-bit value, so that it also sorts last where only a signed 64-bit sort is at hand (a real key is below 2^62).
#define VCY_BALANCE_EMPTY_KEY 0x7fffffffffffffffLL

// One wave per cell (4 cells per workgroup).  Lanes read 64 consecutive list entries; the ballot of "open to me" and the count of
// set bits below a lane give every pick its slot in list order.  The walk stops with the chunk that holds the k-th pick: at
// whole-dataset sight a row is n entries long and the answer sits in its first chunk.
// s == nullptr: every node is open (the first round).  prev == nullptr: every slot counts as changed.
// flag: bit 0 = a position differs from prev, bit 1 = a list entry is outside 0 .. n-1 (such an entry is skipped, never used as an index).
__global__ __launch_bounds__(256) void k_balance_select(const int32_t *__restrict__ dsi, int64_t ldk, const int32_t *__restrict__ rank,
                                                         const int32_t *__restrict__ s, const int64_t *__restrict__ groups,
                                                         const int32_t *__restrict__ prev, int32_t *__restrict__ sel,
                                                         int64_t *__restrict__ keys, int32_t *__restrict__ flag, int n, int K, int k)
{
    const int lane = threadIdx.x & 63;
    const int64_t el = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (el >= n) return;                                        // wave-uniform
    const int32_t *row = dsi + el * ldk;
    const int32_t *prow = prev ? prev + el * k : nullptr;
    int32_t *srow = sel + el * k;
    int64_t *krow = keys + el * k;
    const int my_rank = rank[el];
    const int64_t my_group = groups ? groups[el] : 0;
    int taken = 0, bits = 0;
    for (int64_t c0 = 0; c0 < K && taken < k; c0 += 64) {
        const int64_t j = c0 + lane;                            // (64-bit: c0 + 64 may pass 2^31 on the last chunk)
        const int m = j < K ? row[j] : (int)el;
        const bool inside = (unsigned)m < (unsigned)n;
        bool open = inside && m != (int)el;
        if (j < K && !inside) bits |= 2;
        if (open && groups) open = groups[m] == my_group;
        if (open && s) open = my_rank <= s[m];
        const unsigned long long mask = __ballot(open);
        const int slot = taken + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        if (open && slot < k) {
            if (!prow || prow[slot] != (int)j) bits |= 1;
            srow[slot] = (int)j;
            krow[slot] = ((int64_t)m << 32) | (int64_t)my_rank;
        }
        taken += __popcll(mask);
    }
    for (int slot = taken + lane; slot < k; slot += 64) {       // the sight ran out: empty slots
        if (!prow || prow[slot] != -1) bits |= 1;
        srow[slot] = -1;
        krow[slot] = VCY_BALANCE_EMPTY_KEY;
    }
    if (bits) atomicOr(flag, bits);
}

__global__ __launch_bounds__(256) void k_balance_fill(int32_t *__restrict__ s, int32_t *__restrict__ l, int n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { s[i] = n; l[i] = 0; }
}

// A lane per sorted key.  The lane at the start of a node's run finds the run's end by bisection (the run is at most n keys long,
// only one lane per node searches), writes the run length l[m] and, when the run holds maxl keys, the rank in the maxl-th.
__global__ __launch_bounds__(256) void k_balance_thresholds(const int64_t *__restrict__ keys, int32_t *__restrict__ s,
                                                             int32_t *__restrict__ l, int64_t nk, int64_t maxl, int n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nk) return;
    const int64_t key = keys[i];
    if (key == VCY_BALANCE_EMPTY_KEY) return;
    const int64_t m = key >> 32;
    if (m < 0 || m >= n) return;                                // not a key k_balance_select wrote
    if (i > 0 && (keys[i - 1] >> 32) == m) return;
    const int64_t bound = (m + 1) << 32;                        // first key of any later node; the empty key is larger still
    int64_t lo = i + 1, hi = nk;                                // first position in (i, nk] whose key is >= bound
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < bound) lo = mid + 1; else hi = mid;
    }
    const int64_t len = lo - i;
    l[m] = (int32_t)len;
    if (len >= maxl) s[m] = (int32_t)(keys[i + maxl - 1] & 0xffffffffLL);
}

// The loop's output rows from the final selection, one wave per cell: column 0 is el only if the loop's walk meets the cell itself
// before it stops (it stops right after its k-th pick; with fewer than k picks it reads the whole list), the picks follow, slots
// the sight could not fill are padded with el at position -1 (neighbors.py:47-69).
__global__ __launch_bounds__(256) void k_balance_finish(const int32_t *__restrict__ dsi, int64_t ldk, const int32_t *__restrict__ sel,
                                                         const int32_t *__restrict__ l, int64_t *__restrict__ dsi_new,
                                                         int32_t *__restrict__ pos_new, int64_t *__restrict__ l_out, int n, int K, int k)
{
    const int lane = threadIdx.x & 63;
    const int64_t el = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (el >= n) return;
    const int32_t *row = dsi + el * ldk;
    const int32_t *srow = sel + el * k;
    int64_t *drow = dsi_new + el * (k + 1);
    int32_t *prow = pos_new + el * (k + 1);
    const int last = srow[k - 1];
    const int reach = last >= 0 && last < K ? last : K;                     // the loop reads the entries before this one
    bool met = false;
    for (int64_t c0 = 0; c0 < reach && !met; c0 += 64) {
        const int64_t j = c0 + lane;
        met = __ballot(j < reach && row[j] == (int)el) != 0ull;
    }
    if (lane == 0) {
        drow[0] = met ? el : -1;
        prow[0] = -1;
        l_out[el] = l[el];
    }
    for (int slot = lane; slot < k; slot += 64) {
        const int p = srow[slot];
        const bool pick = p >= 0 && p < K;
        drow[1 + slot] = pick ? (int64_t)row[p] : el;
        prow[1 + slot] = pick ? p : -1;
    }
}

static int balance_shape(const char *what, int64_t n, int64_t K, int64_t k, int64_t ldk)
{
    if (!(n > 0 && n < (1LL << 31) && K > 0 && K < (1LL << 31))) return fail(VCY_ERR_INVALID, "%s: n and K must be positive and below 2^31", what);
    if (!(k > 0 && K >= k)) return fail(VCY_ERR_INVALID, "%s: sight needs to be bigger than k", what);
    if (ldk < K) return fail(VCY_ERR_INVALID, "%s: row pitch below K", what);
    return VCY_OK;
}

}  // namespace vcy

using namespace vcy;

extern "C" int vcy_balance_select(const int32_t *dsi, int64_t ldk, const int32_t *rank, const int32_t *s, const int64_t *groups,
                                  const int32_t *prev, int32_t *sel, int64_t *keys, int32_t *flag, int64_t n, int64_t K, int64_t k,
                                  vcy_stream stream)
{
    VCY_REQUIRE(dsi && rank && sel && keys && flag, "balance_select: null pointer");
    { const int rc = balance_shape("balance_select", n, K, k, ldk); if (rc) return rc; }
    VCY_REQUIRE(sel != prev, "balance_select: sel and prev are the same buffer");
    VCY_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), as_stream(stream)));
    hipLaunchKernelGGL(k_balance_select, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), dsi, ldk, rank, s, groups, prev, sel,
                       keys, flag, (int)n, (int)K, (int)k);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_balance_thresholds(const int64_t *sorted_keys, int32_t *s, int32_t *l, int64_t n, int64_t k, int64_t maxl,
                                      vcy_stream stream)
{
    VCY_REQUIRE(sorted_keys && s && l, "balance_thresholds: null pointer");
    VCY_REQUIRE(n > 0 && n < (1LL << 31) && k > 0 && k < (1LL << 31) && maxl > 0, "balance_thresholds: n, k below 2^31 and maxl must be positive");
    const int64_t nk = n * k, blocks = (nk + 255) / 256;
    VCY_REQUIRE(blocks < (1LL << 31), "balance_thresholds: n * k too large for one launch");
    hipLaunchKernelGGL(k_balance_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), s, l, (int)n);
    VCY_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_balance_thresholds, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), sorted_keys, s, l, nk, maxl, (int)n);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}

extern "C" int vcy_balance_finish(const int32_t *dsi, int64_t ldk, const int32_t *sel, const int32_t *l, int64_t *dsi_new, int32_t *pos_new,
                                  int64_t *l_out, int64_t n, int64_t K, int64_t k, vcy_stream stream)
{
    VCY_REQUIRE(dsi && sel && l && dsi_new && pos_new && l_out, "balance_finish: null pointer");
    { const int rc = balance_shape("balance_finish", n, K, k, ldk); if (rc) return rc; }
    hipLaunchKernelGGL(k_balance_finish, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), dsi, ldk, sel, l, dsi_new, pos_new,
                       l_out, (int)n, (int)K, (int)k);
    VCY_LAUNCH_CHECK();
    return VCY_OK;
}
