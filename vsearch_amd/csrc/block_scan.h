// block_scan.h -- the two-level exclusive scan over the rows of an index that vs_index_compact (mutable.hip), vs_index_select_rows (select.hip)
// and the pointers-from-counts pair of vs_index_prune and vs_index_combine (new_index.hip) share: a pair of uint32 counts a row, blocks of
// kScanRows rows.  Level one is the caller's -- a workgroup sums its block's rows with
// block_excl_scan --, level two is scan_block_sums_kernel over the block sums, and the caller's map kernel scans inside a block again from the
// block's base.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vs {

constexpr int kScanItems = 16;                       // rows per thread of a scan block: 256 x 16 = 4096 rows a block
constexpr int kScanRows = 256 * kScanItems;

__device__ __forceinline__ uint2 add2(uint2 a, uint2 b) { return make_uint2(a.x + b.x, a.y + b.y); }

// exclusive scan over the NW waves of a workgroup; *total = the workgroup's sum.  sh: [NW] uint2 of LDS
template <int NW>
__device__ __forceinline__ uint2 block_excl_scan(uint2 v, uint2* sh, uint2* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint2 inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t a = __shfl_up(inc.x, o, 64), b = __shfl_up(inc.y, o, 64);
        if (lane >= o) { inc.x += a; inc.y += b; }
    }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    uint2 base = make_uint2(0u, 0u), tot = make_uint2(0u, 0u);
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        if (i < w) base = add2(base, sh[i]);
        tot = add2(tot, sh[i]);
    }
    __syncthreads();                                  // (sh is written again by the caller's next round)
    *total = tot;
    return make_uint2(base.x + inc.x - v.x, base.y + inc.y - v.y);
}

// level two: exclusive scan of the block sums in place (one workgroup walks them 1024 at a time); total[0] = the sum over the index
// (a template only so that every unit that includes the header may define it)
template <int UNUSED>
__global__ __launch_bounds__(1024) void scan_block_sums_kernel(uint2* sums, int64_t n_blocks, uint2* total) {
    __shared__ uint2 sh[16];
    uint2 carry = make_uint2(0u, 0u);
    for (int64_t b0 = 0; b0 < n_blocks; b0 += 1024) {
        const int64_t b = b0 + threadIdx.x;
        const uint2 v = b < n_blocks ? sums[b] : make_uint2(0u, 0u);
        uint2 tot;
        const uint2 ex = block_excl_scan<16>(v, sh, &tot);
        if (b < n_blocks) sums[b] = add2(carry, ex);
        carry = add2(carry, tot);
    }
    if (threadIdx.x == 0) total[0] = carry;
}

}  // namespace vs
