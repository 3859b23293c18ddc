// packets.h -- the CSR packets of an index as the aggregations read them (term counts, term sums, clustering): a packet is a uint4 of 8 uint16
// column ids (the padding id is n_cols) and 8 values of the store dtype (fp32: two uint4, fp16: one, a binary index: none) -- and the walk of a
// workgroup over the packets of a set's rows, bitmap or id list (set_walk.h).
#pragma once
#include <hip/hip_fp16.h>

#include "set_walk.h"

namespace vs {

// column id t (0..7) of packet c
__device__ __forceinline__ uint32_t packet_col(const uint4& c, int t) {
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
    return (t & 1) ? (w[t >> 1] >> 16) : (w[t >> 1] & 0xFFFFu);
}

// the 8 values of packet p, widened to fp32 (nothing for a binary index)
template <int SD>
__device__ __forceinline__ void load_vals(const void* vals, uint64_t p, float (&v)[8]) {
    if constexpr (SD == VS_F32) {
        const float4 x = reinterpret_cast<const float4*>(vals)[2 * p], y = reinterpret_cast<const float4*>(vals)[2 * p + 1];
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w, v[4] = y.x, v[5] = y.y, v[6] = y.z, v[7] = y.w;
    } else if constexpr (SD == VS_F16) {
        const uint4 x = reinterpret_cast<const uint4*>(vals)[p];
        const uint32_t h[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __half2float(__ushort_as_half((unsigned short)(h[j] & 0xFFFFu)));
            v[2 * j + 1] = __half2float(__ushort_as_half((unsigned short)(h[j] >> 16)));
        }
    }
}

// bit t set: cell t of packet p holds a non-zero value (+0.0 and -0.0 are zero; a binary index stores 1 everywhere)
template <int SD>
__device__ __forceinline__ uint32_t nonzero_cells(const void* vals, uint64_t p) {
    if constexpr (SD == VS_F32) {
        const uint4 x = reinterpret_cast<const uint4*>(vals)[2 * p], y = reinterpret_cast<const uint4*>(vals)[2 * p + 1];
        const uint32_t v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        uint32_t nz = 0u;
#pragma unroll
        for (int t = 0; t < 8; ++t) nz |= ((v[t] & 0x7FFFFFFFu) != 0u ? 1u : 0u) << t;
        return nz;
    } else if constexpr (SD == VS_F16) {
        const uint4 x = reinterpret_cast<const uint4*>(vals)[p];
        const uint32_t v[4] = {x.x, x.y, x.z, x.w};
        uint32_t nz = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            nz |= ((v[j] & 0x00007FFFu) != 0u ? 1u : 0u) << (2 * j);
            nz |= ((v[j] & 0x7FFF0000u) != 0u ? 1u : 0u) << (2 * j + 1);
        }
        return nz;
    } else {
        return 0xFFu;
    }
}

// an index's packets and a set of its rows: the kernel arguments the term aggregations share (filled by term_set_args of agg_call.h)
struct TermSetArgs {
    const uint32_t* pk_ptr;           // [n_rows + 1]
    const uint4* cols;                // packets of 8 uint16 column ids
    const void* vals;                 // 8 values a packet (fp32 | fp16), absent for a binary index
    int32_t n_cols;
    RowSet set;                       // bitmap driven; and_words: the handle's live bitmap at bit 0, or null; rows_per_chunk: rows or entries
    const int64_t* ids;               // id-list driven: [B, ld_ids]
    int64_t ld_ids, m, id_offset;
};

// a workgroup of WAVES waves: on_packets(p0, p1) for the packet ranges of the set rows of query b in chunk `chunk` -> the set rows seen.
// IDS = 0: the set is a bitmap over the index's rows; IDS = 1: an id list.
template <int WAVES, int IDS, class F>
__device__ __forceinline__ uint32_t walk_term_set(const TermSetArgs& a, size_t b, int64_t chunk, int w, int lane, F on_packets) {
    const int64_t c0 = chunk * a.set.rows_per_chunk;
    if constexpr (IDS) {
        return walk_ids<WAVES>(a.ids + b * (size_t)a.ld_ids, c0, min(a.m, c0 + a.set.rows_per_chunk), a.id_offset, a.set.n_rows, a.set.and_words,
                               a.pk_ptr, w, lane, on_packets);
    } else {
        return walk_row_packets<WAVES>(a.set, b, c0, min(a.set.n_rows, c0 + a.set.rows_per_chunk), a.pk_ptr, w, lane, on_packets);
    }
}

}  // namespace vs
