// combine.hip -- the combined index: a NEW index whose row r holds wa * (row r of a) + wb * (row r of b), cell by cell over the union of the two
// rows' stored columns (vs_index_combine; the semantics are pinned in vsearch_hip.h).  No reference counterpart: the reference adds its tensors
// and rebuilds.  Three steps on the sources' GPU: count (a wave a row: the union's size, repeated columns), scan (row pointers from the union
// counts: the shared pair of new_index.h), fill (a wave a row, or a 1024-thread workgroup a long row: the row is staged in LDS and leaves as
// 16-byte stores).  The scaffold of the call is new_index.h, the host-only part combine_check.h.  Nothing here touches a walk or scan kernel.
#include "block_scan.h"
#include "common.h"
#include "new_index.h"
#include "packets.h"
#include "combine_check.h"

#include <algorithm>
#include <vector>

using namespace vs;

namespace {

CombineShape shape_of(const vs_index* a) {
    CombineShape s;
    s.kind = a->kind;
    s.store_dtype = a->store_dtype;
    s.device = a->device;
    s.n_rows = a->n_rows;
    s.n_packets = a->n_packets;
    s.n_cols = a->n_cols;
    return s;
}

// what the host reads after the scan (kCombineTotalsBytes)
struct CombineTotals {
    unsigned long long nnz;           // union cells over the index
    uint32_t repeat_a, repeat_b;      // the lowest row that stores a column twice (kCombineNoRow: none)
    uint32_t too_wide;                // the lowest row whose union exceeds the workgroup route's slots
    uint32_t n_long;                  // rows on the list of the workgroup route
    uint32_t pad[10];
};
static_assert(sizeof(CombineTotals) == kCombineTotalsBytes, "the plan counts these bytes");

constexpr uint32_t kLongBit = 0x80000000u;            // of a row's union count: cells_a + cells_b exceed the wave route's slots (bit 31: the scan of new_index.h skips it)

// the writes of a team to LDS precede its reads behind this point.  A team is a wave (LDS executes a wave's operations in order; the fence
// keeps the compiler's order and waits for the counter) or the whole workgroup
template <int TEAM>
__device__ __forceinline__ void team_sync() {
    if constexpr (TEAM == 64) {
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t a = __shfl_up(v, o, 64);
        if (lane >= o) v += a;
    }
    return v;
}

// a source as the kernels read it
struct CombineSrc {
    const uint32_t* pk;               // [n_rows + 1]
    const uint4* cols;                // packets of 8 uint16 column ids, padded with n_cols
    const void* vals;                 // 8 values a packet (fp32 | fp16), absent for a binary index
};

// A thread's packets of a row: f(j, q) for q = tid, tid + TEAM, ...  REG: the row has at most kCombineRegPackets packets a thread, the loop
// unrolls whole (what a thread holds of the row is indexed statically) and f is also called for a q past the row's end, where the held ids
// are padding
template <int TEAM, bool REG, class F>
__device__ __forceinline__ void for_packets(uint32_t np, int tid, F f) {
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < kCombineRegPackets; ++j) f(j, (uint32_t)(j * TEAM + tid));
    } else {
        for (uint32_t q = (uint32_t)tid; q < np; q += TEAM) f(0, q);
    }
}

// the column ids of a thread's packets of one source row.  REG: read once and held in registers for every pass (a packet past the row's end
// holds the id 0xFFFF eight times: never below n_cols); otherwise every pass reads them again
template <bool REG>
struct RowIds {
    const uint4* cols;                // the row's first packet
    uint4 held[REG ? kCombineRegPackets : 1];
    template <int TEAM>
    __device__ __forceinline__ void load(const CombineSrc& s, uint32_t p0, uint32_t np, int tid) {
        cols = s.cols + (size_t)p0;
        if constexpr (REG) {
#pragma unroll
            for (int j = 0; j < kCombineRegPackets; ++j) {
                const uint32_t q = (uint32_t)(j * TEAM + tid);
                held[j] = q < np ? cols[q] : make_uint4(~0u, ~0u, ~0u, ~0u);
            }
        }
    }
    __device__ __forceinline__ uint4 get(int j, uint32_t q) const {
        if constexpr (REG) return held[j];
        else return cols[q];
    }
};

// sets the columns of a row's packets in `bits`; -> (this thread's real cells, whether one of them was set already: a repeated column)
template <int TEAM, bool REG>
__device__ __forceinline__ uint2 set_bits(const RowIds<REG>& ids, uint32_t np, int32_t n_cols, uint32_t* bits, int tid) {
    uint32_t cells = 0u, repeat = 0u;
    for_packets<TEAM, REG>(np, tid, [&](int j, uint32_t q) {
        const uint4 c = ids.get(j, q);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t col = packet_col(c, t);
            if (col < (uint32_t)n_cols) {
                const uint32_t bit = 1u << (col & 31u);
                const uint32_t old = atomicOr(&bits[col >> 5], bit);
                repeat |= (old & bit) ? 1u : 0u;
                ++cells;
            }
        }
    });
    return make_uint2(cells, repeat);
}

// clears the words set_bits set, by walking the packets again
template <int TEAM, bool REG>
__device__ __forceinline__ void clear_bits(const RowIds<REG>& ids, uint32_t np, int32_t n_cols, uint32_t* bits, int tid) {
    for_packets<TEAM, REG>(np, tid, [&](int j, uint32_t q) {
        const uint4 c = ids.get(j, q);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t col = packet_col(c, t);
            if (col < (uint32_t)n_cols) bits[col >> 5] = 0u;
        }
    });
}

// ---- step (a): count ----------------------------------------------------------------------------------------------------------------------------
struct CountArgs {
    CombineSrc a, b;
    int64_t n_rows;
    int32_t n_cols;
    uint32_t* ucnt;                   // out: [n_rows] union cells, kLongBit: the row is the workgroup route's
    uint32_t* long_rows;              // out: the rows with kLongBit, in any order
    uint32_t long_cap;
    CombineTotals* tot;
};

// One row by one wave.  A column that atomicOr finds set already is a repeated one (popc(bits) != cells); the union is a's cells plus b's
// cells whose bit a's bitmap lacks.  Both bitmaps are clear on entry and on return.
template <bool REG>
__device__ __forceinline__ void count_row(const CountArgs& k, int64_t r, uint32_t a0, uint32_t na, uint32_t b0, uint32_t nb, uint32_t* bits_a,
                                          uint32_t* bits_b, int lane) {
    RowIds<REG> ia, ib;
    ia.template load<64>(k.a, a0, na, lane);
    ib.template load<64>(k.b, b0, nb, lane);
    const uint2 sa = set_bits<64, REG>(ia, na, k.n_cols, bits_a, lane);
    const uint2 sb = set_bits<64, REG>(ib, nb, k.n_cols, bits_b, lane);
    team_sync<64>();
    uint32_t fresh = 0u;                                        // b's cells that a lacks
    for_packets<64, REG>(nb, lane, [&](int j, uint32_t q) {
        const uint4 c = ib.get(j, q);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t col = packet_col(c, t);
            if (col < (uint32_t)k.n_cols) fresh += ((bits_a[col >> 5] >> (col & 31u)) & 1u) ^ 1u;
        }
    });
    const uint32_t cells_a = wave_sum(sa.x), cells_b = wave_sum(sb.x), rep_a = wave_sum(sa.y), rep_b = wave_sum(sb.y);
    const uint32_t uni = cells_a + wave_sum(fresh);             // (exact when no column repeats; with a repeat the call ends before it is used)
    if (lane == 0) {
        if (rep_a) atomicMin(&k.tot->repeat_a, (uint32_t)r);
        if (rep_b) atomicMin(&k.tot->repeat_b, (uint32_t)r);
        if (!rep_a && !rep_b && uni > (uint32_t)kCombineGroupCells) atomicMin(&k.tot->too_wide, (uint32_t)r);
        const bool is_long = cells_a + cells_b > (uint32_t)kCombineWaveCells;
        k.ucnt[r] = uni | (is_long ? kLongBit : 0u);
        if (is_long) {
            const uint32_t at = atomicAdd(&k.tot->n_long, 1u);
            if (at < k.long_cap) k.long_rows[at] = (uint32_t)r;        // (the cap is an upper bound of the long rows: combine_long_rows_cap)
        }
    }
    team_sync<64>();
    clear_bits<64, REG>(ia, na, k.n_cols, bits_a, lane);
    clear_bits<64, REG>(ib, nb, k.n_cols, bits_b, lane);
    team_sync<64>();
}

// persistent workgroups of 4 waves stride over the rows, a wave a row.  LDS: two bitmaps of n_cols bits a wave.  Rows of up to
// kCombineRegCells cells a side are read once and held in registers; longer rows are read again by every pass
__global__ __launch_bounds__(kCombineThreads) void combine_count_kernel(CountArgs k) {
    extern __shared__ __attribute__((aligned(16))) uint32_t combine_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int words = (k.n_cols + 31) >> 5;
    uint32_t* bits_a = combine_lds + (size_t)w * 2 * words;
    uint32_t* bits_b = bits_a + words;
    for (int i = lane; i < 2 * words; i += 64) bits_a[i] = 0u;
    team_sync<64>();
    for (int64_t r = (int64_t)blockIdx.x * kCombineWaves + w; r < k.n_rows; r += (int64_t)gridDim.x * kCombineWaves) {
        const uint32_t a0 = k.a.pk[r], na = k.a.pk[r + 1] - a0, b0 = k.b.pk[r], nb = k.b.pk[r + 1] - b0;
        if (na <= 64u * kCombineRegPackets && nb <= 64u * kCombineRegPackets) count_row<true>(k, r, a0, na, b0, nb, bits_a, bits_b, lane);
        else count_row<false>(k, r, a0, na, b0, nb, bits_a, bits_b, lane);
    }
}

// ---- step (c): fill -----------------------------------------------------------------------------------------------------------------------------
struct FillArgs {
    CombineSrc a, b;
    int64_t n_rows;
    int32_t n_cols;
    float wa, wb;
    const uint32_t* ucnt;             // [n_rows] of the count step
    const uint32_t* long_rows;        // the workgroup route's rows
    uint32_t n_long;
    const uint32_t* new_pk;           // [n_rows + 1]
    uint4* dcols;                     // the new index
    uint4* dvals;
};

// the stored value t of a packet's raw words, widened to fp32 (1 for a binary index)
template <int SD>
__device__ __forceinline__ float cell_value(const uint4& v0, const uint4& v1, int t) {
    if constexpr (SD == VS_F32) {
        const uint32_t b[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        return __uint_as_float(b[t]);
    } else if constexpr (SD == VS_F16) {
        const uint32_t h[4] = {v0.x, v0.y, v0.z, v0.w};
        return __half2float(__ushort_as_half((unsigned short)((t & 1) ? (h[t >> 1] >> 16) : (h[t >> 1] & 0xFFFFu))));
    } else {
        return 1.f;
    }
}

template <int SD>
__device__ __forceinline__ void load_raw(const void* vals, size_t p, uint4& v0, uint4& v1) {
    v0 = v1 = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (SD == VS_F16) v0 = reinterpret_cast<const uint4*>(vals)[p];
    if constexpr (SD == VS_F32) {
        v0 = reinterpret_cast<const uint4*>(vals)[2 * p];
        v1 = reinterpret_cast<const uint4*>(vals)[2 * p + 1];
    }
}

// the stored bits of x: fl32(x), or fl16(fl32(x)) in the low half
template <int OD>
__device__ __forceinline__ uint32_t final_bits(double x) {
    float f = (float)x;
    if constexpr (OD == VS_F32) return __float_as_uint(f);
    // two roundings: the fp32 value has to exist.  Left to itself the compiler may fold the conversions into one that rounds the fp64 value
    // once (rescale.hip met the fold as v_fma_mixlo_f16) -- the empty statement makes the float opaque to it
    asm volatile("" : "+v"(f));
    return (uint32_t)__half_as_ushort(__float2half_rn(f));
}

// the raw values of a thread's packets of one source row: REG: read once, with the ids, before the first pass; otherwise read by the pass
template <int SD, bool REG>
struct RowVals {
    const void* vals;
    size_t p0;
    uint4 v0[REG ? kCombineRegPackets : 1], v1[REG && SD == VS_F32 ? kCombineRegPackets : 1];
    template <int TEAM>
    __device__ __forceinline__ void load(const CombineSrc& s, uint32_t first, uint32_t np, int tid) {
        vals = s.vals;
        p0 = first;
        if constexpr (REG && SD != VS_NONE) {
#pragma unroll
            for (int j = 0; j < kCombineRegPackets; ++j) {
                const uint32_t q = (uint32_t)(j * TEAM + tid);
                uint4 x = make_uint4(0u, 0u, 0u, 0u), y = x;
                if (q < np) load_raw<SD>(vals, p0 + q, x, y);
                v0[j] = x;
                if constexpr (SD == VS_F32) v1[j] = y;
            }
        }
    }
    __device__ __forceinline__ void get(int j, uint32_t q, uint4& x, uint4& y) const {
        if constexpr (SD == VS_NONE) {
            x = y = make_uint4(0u, 0u, 0u, 0u);
        } else if constexpr (REG) {
            x = v0[j];
            y = SD == VS_F32 ? v1[SD == VS_F32 ? j : 0] : make_uint4(0u, 0u, 0u, 0u);
        } else {
            load_raw<SD>(vals, p0 + q, x, y);
        }
    }
};

// One row by one team (a wave, or a workgroup of 1024).  bits_a, bits_b, prefix: [words]; slot: one word a union cell.  Both bitmaps are
// clear on entry and on return.  REG (a wave, rows of up to kCombineRegCells cells a side): ids and values are read once, all loads issued
// before the first pass, and held in registers.
template <int SA, int SB, int OD, int TEAM, bool REG>
__device__ __forceinline__ void fill_row(const FillArgs& k, int64_t r, uint32_t uni, uint32_t a0, uint32_t na, uint32_t b0, uint32_t nb, uint32_t* bits_a,
                                         uint32_t* bits_b, uint32_t* prefix, uint32_t* slot, uint2* scan_sh, int tid) {
    const int words = (k.n_cols + 31) >> 5;
    RowIds<REG> ia, ib;
    RowVals<SA, REG> va;
    RowVals<SB, REG> vb;
    ia.template load<TEAM>(k.a, a0, na, tid);
    ib.template load<TEAM>(k.b, b0, nb, tid);
    va.template load<TEAM>(k.a, a0, na, tid);
    vb.template load<TEAM>(k.b, b0, nb, tid);
    (void)set_bits<TEAM, REG>(ia, na, k.n_cols, bits_a, tid);
    (void)set_bits<TEAM, REG>(ib, nb, k.n_cols, bits_b, tid);
    team_sync<TEAM>();
    // the exclusive popcount prefix of the union, word by word.  A wave: a lane sums a run of consecutive words, one wave scan over the 64 run
    // sums, then the lane writes its run's prefixes.  A workgroup: a word a thread, 1024 at a time through block_excl_scan
    if constexpr (TEAM == 64) {
        const int run = (words + 63) >> 6, w0 = tid * run, w1 = min(words, w0 + run);
        uint32_t mine = 0u;
        for (int w = w0; w < w1; ++w) mine += (uint32_t)__popc(bits_a[w] | bits_b[w]);
        uint32_t at = wave_incl_scan(mine, tid) - mine;
        for (int w = w0; w < w1; ++w) {
            prefix[w] = at;
            at += (uint32_t)__popc(bits_a[w] | bits_b[w]);
        }
    } else {
        uint32_t carry = 0u;
        for (int w0 = 0; w0 < words; w0 += TEAM) {
            const int w = w0 + tid;
            const uint32_t c = w < words ? (uint32_t)__popc(bits_a[w] | bits_b[w]) : 0u;
            uint2 tot;
            const uint32_t ex = block_excl_scan<TEAM / 64>(make_uint2(c, 0u), scan_sh, &tot).x;
            if (w < words) prefix[w] = carry + ex;
            carry += tot.x;
        }
    }
    team_sync<TEAM>();
    const double wa = (double)k.wa, wb = (double)k.wb;
    // a's cells: the final bits where b lacks the column, the raw value where b has it
    for_packets<TEAM, REG>(na, tid, [&](int j, uint32_t q) {
        const uint4 c = ia.get(j, q);
        uint4 v0, v1;
        va.get(j, q, v0, v1);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t col = packet_col(c, t);
            if (col < (uint32_t)k.n_cols) {
                const uint32_t w = col >> 5, below = (1u << (col & 31u)) - 1u, ub = bits_b[w];
                const uint32_t rank = prefix[w] + __popc((bits_a[w] | ub) & below);
                const float av = cell_value<SA>(v0, v1, t);
                slot[rank] = ((ub >> (col & 31u)) & 1u) ? __float_as_uint(av) : final_bits<OD>(wa * (double)av);
            }
        }
    });
    team_sync<TEAM>();
    // b's cells: the sum where a has the column (its raw value waits in the slot), the one product where it has not
    for_packets<TEAM, REG>(nb, tid, [&](int j, uint32_t q) {
        const uint4 c = ib.get(j, q);
        uint4 v0, v1;
        vb.get(j, q, v0, v1);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t col = packet_col(c, t);
            if (col < (uint32_t)k.n_cols) {
                const uint32_t w = col >> 5, below = (1u << (col & 31u)) - 1u, ua = bits_a[w];
                const uint32_t rank = prefix[w] + __popc((ua | bits_b[w]) & below);
                const double xb = wb * (double)cell_value<SB>(v0, v1, t);
                const bool both = ((ua >> (col & 31u)) & 1u) != 0u;
                const double x = both ? wa * (double)__uint_as_float(slot[rank]) + xb : xb;
                slot[rank] = final_bits<OD>(x);
            }
        }
    });
    team_sync<TEAM>();
    // the row leaves packet by packet: ids from the union's set bits from rank 8 j on, values from the slots; the tail is padding
    const uint32_t nd = (uni + 7u) >> 3;
    const size_t d0 = k.new_pk[r];
    for (uint32_t j = (uint32_t)tid; j < nd; j += TEAM) {
        const uint32_t rank0 = j * 8u;
        int lo = 0, hi = words - 1;                             // the last word whose prefix is <= rank0: the word that holds rank0 (rank0 < uni)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (prefix[mid] <= rank0) lo = mid;
            else hi = mid - 1;
        }
        int w = lo;
        uint32_t u = bits_a[w] | bits_b[w];
        for (uint32_t s = rank0 - prefix[w]; s > 0u; --s) u &= u - 1u;
        uint32_t ids[8], v[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const bool real = rank0 + (uint32_t)t < uni;
            if (real) {
                while (u == 0u && w + 1 < words) {              // (a real rank has its bit in a word below `words`)
                    ++w;
                    u = bits_a[w] | bits_b[w];
                }
                ids[t] = (uint32_t)w * 32u + (uint32_t)(__ffs((int)u) - 1);
                u &= u - 1u;
                v[t] = slot[rank0 + (uint32_t)t];
            } else {
                ids[t] = (uint32_t)k.n_cols;
                v[t] = 0u;
            }
        }
        k.dcols[d0 + j] = make_uint4(ids[0] | (ids[1] << 16), ids[2] | (ids[3] << 16), ids[4] | (ids[5] << 16), ids[6] | (ids[7] << 16));
        if constexpr (OD == VS_F32) {
            k.dvals[(d0 + j) * 2] = make_uint4(v[0], v[1], v[2], v[3]);
            k.dvals[(d0 + j) * 2 + 1] = make_uint4(v[4], v[5], v[6], v[7]);
        } else {
            k.dvals[d0 + j] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
        }
    }
    team_sync<TEAM>();
    clear_bits<TEAM, REG>(ia, na, k.n_cols, bits_a, tid);
    clear_bits<TEAM, REG>(ib, nb, k.n_cols, bits_b, tid);
    team_sync<TEAM>();
}

// wave route: persistent workgroups of 4 waves stride over the rows, a wave a row; a long row is the other kernel's.  LDS a wave: two
// bitmaps, the prefix, kCombineWaveCells slots
template <int SA, int SB, int OD>
__global__ __launch_bounds__(kCombineThreads) void combine_fill_wave_kernel(FillArgs k) {
    extern __shared__ __attribute__((aligned(16))) uint32_t combine_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int words = (k.n_cols + 31) >> 5;
    uint32_t* base = combine_lds + (size_t)w * (3 * words + kCombineWaveCells);
    for (int i = lane; i < 2 * words; i += 64) base[i] = 0u;
    team_sync<64>();
    for (int64_t r = (int64_t)blockIdx.x * kCombineWaves + w; r < k.n_rows; r += (int64_t)gridDim.x * kCombineWaves) {
        const uint32_t u = k.ucnt[r];
        if (u == 0u || (u & kLongBit)) continue;
        const uint32_t a0 = k.a.pk[r], na = k.a.pk[r + 1] - a0, b0 = k.b.pk[r], nb = k.b.pk[r + 1] - b0;
        if (na <= 64u * kCombineRegPackets && nb <= 64u * kCombineRegPackets)
            fill_row<SA, SB, OD, 64, true>(k, r, u, a0, na, b0, nb, base, base + words, base + 2 * words, base + 3 * words, nullptr, lane);
        else
            fill_row<SA, SB, OD, 64, false>(k, r, u, a0, na, b0, nb, base, base + words, base + 2 * words, base + 3 * words, nullptr, lane);
    }
}

// workgroup route: a workgroup of 1024 a long row.  LDS: two bitmaps, the prefix, k.slots slots, the scan's wave sums
template <int SA, int SB, int OD>
__global__ __launch_bounds__(kCombineGroupThreads) void combine_fill_group_kernel(FillArgs k) {
    extern __shared__ __attribute__((aligned(16))) uint32_t combine_lds[];
    const int words = (k.n_cols + 31) >> 5;
    uint2* scan_sh = reinterpret_cast<uint2*>(combine_lds);     // the scan's 16 wave sums come first: 8-byte aligned whatever the width
    uint32_t* bits = combine_lds + kCombineScanScratch / 4;
    for (int i = threadIdx.x; i < 2 * words; i += kCombineGroupThreads) bits[i] = 0u;
    __syncthreads();
    for (uint32_t i = blockIdx.x; i < k.n_long; i += gridDim.x) {
        const int64_t r = k.long_rows[i];
        const uint32_t u = k.ucnt[r] & ~kLongBit;
        if (u == 0u) continue;                                  // (uniform over the workgroup)
        const uint32_t a0 = k.a.pk[r], na = k.a.pk[r + 1] - a0, b0 = k.b.pk[r], nb = k.b.pk[r + 1] - b0;
        fill_row<SA, SB, OD, kCombineGroupThreads, false>(k, r, u, a0, na, b0, nb, bits, bits + words, bits + 2 * words, bits + 3 * words, scan_sh,
                                                          (int)threadIdx.x);
    }
}

template <int SA, int SB, int OD>
int launch_fill(const CombinePlan& plan, int cu_count, const FillArgs& k) {
    {
        const auto kern = combine_fill_wave_kernel<SA, SB, OD>;
        if (plan.wave_lds_bytes > 32 * 1024) VS_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, plan.wave_lds_bytes));
        hipLaunchKernelGGL(kern, dim3((unsigned)combine_wave_grid(k.n_rows, cu_count)), dim3(kCombineThreads), (size_t)plan.wave_lds_bytes, 0, k);
        VS_HIP(hipGetLastError());
    }
    if (k.n_long > 0u) {
        const auto kern = combine_fill_group_kernel<SA, SB, OD>;
        if (plan.group_lds_bytes > 32 * 1024) VS_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, plan.group_lds_bytes));
        hipLaunchKernelGGL(kern, dim3((unsigned)combine_group_grid(k.n_long, cu_count)), dim3(kCombineGroupThreads), (size_t)plan.group_lds_bytes, 0, k);
        VS_HIP(hipGetLastError());
    }
    return VS_OK;
}
template <int SA, int SB>
int launch_fill_od(int od, const CombinePlan& plan, int cu_count, const FillArgs& k) {
    return od == VS_F32 ? launch_fill<SA, SB, VS_F32>(plan, cu_count, k) : launch_fill<SA, SB, VS_F16>(plan, cu_count, k);
}
template <int SA>
int launch_fill_sb(int sb, int od, const CombinePlan& plan, int cu_count, const FillArgs& k) {
    if (sb == VS_F32) return launch_fill_od<SA, VS_F32>(od, plan, cu_count, k);
    if (sb == VS_F16) return launch_fill_od<SA, VS_F16>(od, plan, cu_count, k);
    return launch_fill_od<SA, VS_NONE>(od, plan, cu_count, k);
}

CombineSrc src_of(const vs_index* x) { return CombineSrc{x->pk_ptr.as<uint32_t>(), x->cols.as<uint4>(), x->vals.p}; }

}  // namespace

extern "C" int vs_combine_plan(int64_t n_rows, int64_t packets_a, int64_t packets_b, int32_t n_cols, int dtype_a, int dtype_b, int out_dtype,
                               int32_t* out_wave_cells, int32_t* out_group_cells, int32_t* out_wave_lds_bytes, int32_t* out_group_lds_bytes,
                               int64_t* out_scratch_bytes) {
    char msg[512] = {0};
    CombinePlan p;
    const int rc = combine_plan(n_rows, packets_a, packets_b, n_cols, dtype_a, dtype_b, out_dtype, &p, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    if (out_wave_cells) *out_wave_cells = p.wave_cells;
    if (out_group_cells) *out_group_cells = p.group_cells;
    if (out_wave_lds_bytes) *out_wave_lds_bytes = p.wave_lds_bytes;
    if (out_group_lds_bytes) *out_group_lds_bytes = p.group_lds_bytes;
    if (out_scratch_bytes) *out_scratch_bytes = p.scratch_bytes;
    return VS_OK;
}

extern "C" int vs_index_combine(const vs_index* a, const vs_index* b, float wa, float wb, int out_dtype, int64_t rows_extra, int64_t packets_extra,
                                int device, vs_index** out) {
    char msg[512] = {0};
    if (out) *out = nullptr;
    int rc = combine_check_args(a != nullptr, b != nullptr, out != nullptr, out_dtype, rows_extra, packets_extra, msg, sizeof msg);
    if (rc == VS_OK) rc = combine_check_sources(shape_of(a), shape_of(b), msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    VS_TRY(device_in_range(device));
    const int64_t n = a->n_rows;
    CombinePlan plan;
    rc = combine_plan(n, a->n_packets, b->n_packets, a->n_cols, a->store_dtype, b->store_dtype, out_dtype, &plan, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);

    VS_TRY(open_sources(a->device));
    // scratch: union counts, the list of long rows, block sums, the totals
    DevBuf ucnt, long_rows, sums, tot;
    if (ucnt.alloc(std::max<size_t>((size_t)n * 4, 4)) != VS_OK || long_rows.alloc(std::max<size_t>((size_t)plan.long_rows_cap * 4, 4)) != VS_OK)
        return fail(VS_ENOMEM, "combining needs %lld bytes of HBM for the union counts of the rows", (long long)plan.scratch_bytes);
    VS_TRY(sums.alloc((size_t)(plan.scan_blocks + 1) * 8));
    VS_TRY(tot.alloc(sizeof(CombineTotals)));
    CombineTotals h_tot = {};
    h_tot.repeat_a = h_tot.repeat_b = h_tot.too_wide = kCombineNoRow;
    VS_HIP(hipMemcpy(tot.p, &h_tot, sizeof h_tot, hipMemcpyHostToDevice));
    // (a) count
    if (n > 0) {
        CountArgs k;
        k.a = src_of(a);
        k.b = src_of(b);
        k.n_rows = n;
        k.n_cols = a->n_cols;
        k.ucnt = ucnt.as<uint32_t>();
        k.long_rows = long_rows.as<uint32_t>();
        k.long_cap = (uint32_t)plan.long_rows_cap;
        k.tot = tot.as<CombineTotals>();
        const auto kern = combine_count_kernel;
        if (plan.count_lds_bytes > 32 * 1024) VS_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, plan.count_lds_bytes));
        hipLaunchKernelGGL(kern, dim3((unsigned)combine_count_grid(n, a->cu_count)), dim3(kCombineThreads), (size_t)plan.count_lds_bytes, 0, k);
        VS_HIP(hipGetLastError());
    }
    // (b) scan
    uint2* d_sums = sums.as<uint2>();
    int64_t p_new = 0;
    VS_TRY(cells_scan(ucnt.as<int32_t>(), n, plan.scan_blocks, d_sums, &tot.as<CombineTotals>()->nnz, &p_new));
    VS_HIP(hipMemcpy(&h_tot, tot.p, sizeof h_tot, hipMemcpyDeviceToHost));
    rc = combine_check_flags(h_tot.repeat_a, h_tot.repeat_b, h_tot.too_wide, msg, sizeof msg);
    if (rc == VS_OK) rc = new_index_check_capacity("combined", n, p_new, rows_extra, packets_extra, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    if ((int64_t)h_tot.n_long > plan.long_rows_cap) return fail(VS_EHIP, "the count step listed %u long rows, the bound is %lld", h_tot.n_long, (long long)plan.long_rows_cap);
    IndexGuard guard{nullptr};
    VS_TRY(new_csr_index("combining", "sources' (drop the postings copy of a source)", n, p_new, rows_extra, packets_extra, a->n_cols, out_dtype, a->device, &guard));
    vs_index* idx = guard.p;
    VS_TRY(cells_row_pointers(ucnt.as<int32_t>(), n, plan.scan_blocks, d_sums, p_new, idx->pk_ptr.as<uint32_t>()));
    // (c) fill
    if (p_new > 0) {
        FillArgs k;
        k.a = src_of(a);
        k.b = src_of(b);
        k.n_rows = n;
        k.n_cols = a->n_cols;
        k.wa = wa;
        k.wb = wb;
        k.ucnt = ucnt.as<uint32_t>();
        k.long_rows = long_rows.as<uint32_t>();
        k.n_long = h_tot.n_long;
        k.new_pk = idx->pk_ptr.as<uint32_t>();
        k.dcols = idx->cols.as<uint4>();
        k.dvals = idx->vals.as<uint4>();
        const int sa = a->store_dtype, sb = b->store_dtype;
        if (sa == VS_F32) VS_TRY(launch_fill_sb<VS_F32>(sb, out_dtype, plan, a->cu_count, k));
        else if (sa == VS_F16) VS_TRY(launch_fill_sb<VS_F16>(sb, out_dtype, plan, a->cu_count, k));
        else VS_TRY(launch_fill_sb<VS_NONE>(sb, out_dtype, plan, a->cu_count, k));
    }
    set_csr_shape(idx, n, p_new, (int64_t)h_tot.nnz, a->logical_dense && b->logical_dense);
    // the deleted rows are a's or b's: the live words are ANDed on the host (a bit a row: 125 KB a million rows); restore() brings a deleted
    // row back combined
    std::vector<uint32_t> live_a, live_b;
    const bool tomb = (a->has_tomb || b->has_tomb) && n > 0;
    if (tomb) {
        VS_TRY(tomb_to_host(a, live_a));
        VS_TRY(tomb_to_host(b, live_b));
        for (size_t i = 0; i < live_a.size(); ++i) live_a[i] &= live_b[i];
    }
    return hand_over(guard, a->device, device, TombFrom::host_words(tomb ? live_a.data() : nullptr), out);
}
