// term_cells.h -- how a wave adds the cells of a range of CSR packets to a column tile of 64-bit fixed-point bins: the inner loop the term sums
// (term_sum.hip) and the per-label term sums (label_terms.hip) share, one copy.
#pragma once
#include "packets.h"
#include "term_sum_check.h"

namespace vs {

// the fixed-point image of a stored value: the bits of an int64, added in two's complement (term_fx: term_sum_check.h, shared with the host check)
__device__ __forceinline__ unsigned long long fx(float v) {
#pragma clang fp contract(off)
    return term_fx(v);
}

// bit t set: column id t of the packet lies in the tile [tile0, tile0 + lim)
__device__ __forceinline__ uint32_t tile_hits(const uint4& c, uint32_t tile0, uint32_t lim) {
    uint32_t hit = 0u;
#pragma unroll
    for (int t = 0; t < 8; ++t) hit |= ((packet_col(c, t) - tile0) < lim ? 1u : 0u) << t;
    return hit;
}

// the cells of a packet named by `hit` add their fx to the tile's bins (bin index < lim by the compare that made `hit`)
template <int SD>
__device__ __forceinline__ void add_cells(const float (&v)[8], const uint4& c, uint32_t hit, uint32_t tile0, unsigned long long* bins) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if ((hit >> t) & 1u) {
            unsigned long long a;
            if constexpr (SD == VS_NONE) a = 1ull << VS_TERM_FX_SHIFT;        // a binary index stores 1
            else a = fx(v[t]);
            if (a) atomicAdd(bins + (packet_col(c, t) - tile0), a);           // (a stored +-0, a NaN, a value below 2^-25: nothing to add)
        }
    }
}

// one wave: every cell of packets [p0, p1) whose column lies in the tile adds its fx to the column's bin; a lane takes a packet, two are in flight
template <int SD>
__device__ __forceinline__ void sum_packets(const TermSetArgs& a, uint32_t p0, uint32_t p1, int lane, uint32_t tile0, uint32_t lim,
                                            unsigned long long* bins) {
    // The values are read only after the ids said so: two dependent loads a step.  The ids of the next step are therefore requested before the
    // values of this one, so that a step waits for one round trip, not two (a workgroup with a full tile has 4 waves a SIMD to hide it with).
    const uint4 none = make_uint4(0u, 0u, 0u, 0u);
    uint4 ca = none, cc = none;
    if ((uint64_t)p0 + lane < p1) ca = a.cols[(uint64_t)p0 + lane];
    if ((uint64_t)p0 + 64 + lane < p1) cc = a.cols[(uint64_t)p0 + 64 + lane];
    for (uint64_t pb = p0; pb < p1; pb += 128) {                  // (64-bit: no wrap next to 2^32 packets)
        const uint64_t pa = pb + lane, pc = pb + 64 + lane;
        const uint32_t ha = pa < p1 ? tile_hits(ca, tile0, lim) : 0u, hc = pc < p1 ? tile_hits(cc, tile0, lim) : 0u;
        uint4 na = none, nc = none;
        if (pa + 128 < p1) na = a.cols[pa + 128];
        if (pc + 128 < p1) nc = a.cols[pc + 128];
        float va[8] = {}, vc[8] = {};
        if (ha) load_vals<SD>(a.vals, pa, va);                    // no id in the tile: the values are not read
        if (hc) load_vals<SD>(a.vals, pc, vc);
        add_cells<SD>(va, ca, ha, tile0, bins);
        add_cells<SD>(vc, cc, hc, tile0, bins);
        ca = na;
        cc = nc;
    }
}

}  // namespace vs
