// term_sum.hip -- term sums (vs_term_sum_plan, vs_index_term_sums, vs_index_term_sums_ids, vs_term_sum_topn): for a set of rows, how much weight
// the set puts on each vocabulary column -- its centroid in vocabulary space, times the rows -- and which columns carry the largest mean weight.
// No reference counterpart.  Nothing here touches a search kernel: the set arrives exactly as for the term counts of term_agg.hip (a packed bitmap
// at a bit0, or an id list), the rows are the CSR packets with their uint16 column ids and their values.
//
// The sums are FIXED POINT so that they do not depend on the order of the additions: a stored cell of value v adds
//   fx(v) = llrint(double(clamp(v, -2^20, +2^20)) * 2^24)      (to nearest even; NaN adds 0; +-inf clamp)
// to a 64-bit integer.  Every fp16 value is a multiple of 2^-24, so fp16 and binary stores are summed exactly; a cell is at most 2^44 in
// magnitude, so 2^19 saturated rows fit before the int64 wraps (it wraps modulo 2^64, as numpy's does).
//
// (a) Sums: a workgroup of 16 waves owns a chunk of rows, one query and one COLUMN TILE (work item i of the 1-D grid: tile i % tiles of query
//     (i / tiles) % B of chunk i / (tiles * B) -- the workgroups resident at one time sweep the same packets through L2).  A 64-bit image of the
//     vocabulary does not fit the LDS (29 523 columns: 236 KB of 160 KiB), a tile of at most VS_TERM_SUM_TILE_COLS columns does.  The workgroup
//     walks the bitmap as term_counts_kernel does (bitmap_span.h: 2048-row spans, 64-row steps dealt to the waves, all-zero spans and steps left
//     at once) and streams the runs' packets, one a lane, two in flight.  For a cell of column c: t = c - tile0, and if (unsigned)t < the tile's
//     columns, one 64-bit LDS atomicAdd of fx(v) on bin t -- the one compare drops the padding id n_cols and the other tiles' columns and bounds
//     the bin index.  A row's columns ascend, so most packets lie wholly inside or outside the tile: a lane whose 8 ids all miss reads no value.
//     At the end of the chunk every non-zero bin is one 64-bit vector atomicAdd into sums; tile 0's workgroups add the rows to total.
// (b) The id-list variant: a wave takes 64 entries, each lane resolves its id, the wave streams the surviving rows one after the other.
// (c) Top-n: one workgroup per query scores the columns with a positive sum by their mean weight in fp64 (one rounding to fp32), streams
//     make_key(score, column) through a 4096-key LDS buffer pruned by wg_sort_desc, as vs_term_topn does.
#include "common.h"
#include "bitmap_span.h"
#include "staging.h"
#include "term_sum_check.h"
#include "topk_keys.h"

#include <algorithm>

using namespace vs;

namespace {

constexpr int kSumThreads = 1024;                     // 16 waves: a workgroup with a full tile has the CU to itself
constexpr int kSumWaves = kSumThreads / 64;
constexpr int kTopnThreads = 256;
constexpr int kTopnCap = 4096;                        // keys of the top-n candidate buffer
constexpr int kTopnKeep = 2048;                       // pruned when more are in
static_assert((size_t)VS_TERM_SUM_TILE_COLS * 8 + 1024 <= 160 * 1024, "a tile of 64-bit bins and the counters fit a CU's LDS");

struct SumArgs {
    const uint32_t* pk_ptr;           // [n_rows + 1]
    const uint4* cols;                // packets of 8 uint16 column ids
    const void* vals;                 // 8 values a packet (fp32 | fp16), absent for a binary index
    int32_t n_cols;
    int64_t n_rows;
    const uint32_t* live;             // the handle's live bitmap at bit 0, or null
    // bitmap driven
    const uint32_t* words;            // [B, ld_words] or null (every row set)
    int64_t bit0, ld_words;
    // id-list driven
    const int64_t* ids;               // [B, ld_ids]
    int64_t ld_ids, m, id_offset;
    int64_t rows_per_chunk;           // rows (entries) of a workgroup
    int32_t B, tiles, tile_cols;      // work item i of the grid: tile i % tiles, query (i / tiles) % B, chunk i / (tiles * B)
    unsigned long long* sums;         // [B, ld_sums], zeroed by the caller
    int64_t ld_sums;
    unsigned long long* total;        // [B], zeroed by the caller
};

// the fixed-point image of a stored value: the bits of an int64, added in two's complement (term_fx: term_sum_check.h, shared with the host check)
__device__ __forceinline__ unsigned long long fx(float v) {
#pragma clang fp contract(off)
    return term_fx(v);
}

// bit t set: column id t of the packet lies in the tile [tile0, tile0 + lim)
__device__ __forceinline__ uint32_t tile_hits(const uint4& c, uint32_t tile0, uint32_t lim) {
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
    uint32_t hit = 0u;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uint32_t col = (t & 1) ? (w[t >> 1] >> 16) : (w[t >> 1] & 0xFFFFu);
        hit |= ((col - tile0) < lim ? 1u : 0u) << t;
    }
    return hit;
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

// the cells of a packet named by `hit` add their fx to the tile's bins (bin index < lim by the compare that made `hit`)
template <int SD>
__device__ __forceinline__ void add_cells(const float (&v)[8], const uint4& c, uint32_t hit, uint32_t tile0, unsigned long long* bins) {
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if ((hit >> t) & 1u) {
            const uint32_t col = (t & 1) ? (w[t >> 1] >> 16) : (w[t >> 1] & 0xFFFFu);
            unsigned long long a;
            if constexpr (SD == VS_NONE) a = 1ull << VS_TERM_FX_SHIFT;        // a binary index stores 1
            else a = fx(v[t]);
            if (a) atomicAdd(bins + (col - tile0), a);            // (a stored +-0, a NaN, a value below 2^-25: nothing to add)
        }
    }
}

// one wave: every cell of packets [p0, p1) whose column lies in the tile adds its fx to the column's bin; a lane takes a packet, two are in flight
template <int SD>
__device__ __forceinline__ void sum_packets(const SumArgs& a, uint32_t p0, uint32_t p1, int lane, uint32_t tile0, uint32_t lim,
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

// IDS = 0: the set is a bitmap over the index's rows; IDS = 1: an id list
template <int SD, int IDS>
__global__ __launch_bounds__(kSumThreads) void term_sums_kernel(SumArgs a) {
    extern __shared__ uint4 term_bins4[];                        // [ceil(tile_cols / 2)]: the tile's 64-bit bins
    __shared__ uint32_t s_tot;
    unsigned long long* bins = reinterpret_cast<unsigned long long*>(term_bins4);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t tile = blockIdx.x % (uint32_t)a.tiles;        // tile and query run fastest: resident workgroups sweep the same packets
    const uint32_t rest = blockIdx.x / (uint32_t)a.tiles;
    const size_t b = rest % (uint32_t)a.B;
    const int64_t chunk = rest / (uint32_t)a.B;
    const uint32_t tile0 = tile * (uint32_t)a.tile_cols;         // < n_cols: no tile of the plan is empty
    const uint32_t lim = min((uint32_t)a.tile_cols, (uint32_t)a.n_cols - tile0);     // the padding id n_cols is never inside
    for (int i = tid; i < (a.tile_cols + 1) / 2; i += kSumThreads) term_bins4[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) s_tot = 0u;
    __syncthreads();
    uint32_t tot = 0u;                                           // wave-uniform: a chunk holds fewer than 2^32 rows
    if constexpr (IDS) {
        const int64_t e0 = chunk * a.rows_per_chunk, e1 = min(a.m, e0 + a.rows_per_chunk);
        const int64_t* list = a.ids + b * (size_t)a.ld_ids;
        for (int64_t eb = e0 + (int64_t)w * 64; eb < e1; eb += (int64_t)kSumWaves * 64) {
            const int64_t e = eb + lane;
            bool ok = false;
            uint32_t plo = 0u, phi = 0u;
            if (e < e1) {
                const int64_t id = list[e];
                const uint64_t row = (uint64_t)id - (uint64_t)a.id_offset;
                ok = id != -1 && id >= a.id_offset && row < (uint64_t)a.n_rows;          // anything else is not this index's: skipped
                if (ok && a.live) ok = ((a.live[row >> 5] >> (row & 31u)) & 1u) != 0u;  // a deleted row is skipped
                if (ok) {
                    plo = a.pk_ptr[row];
                    phi = a.pk_ptr[row + 1];
                }
            }
            unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
            tot += (uint32_t)__popcll(m);                                                // an id listed twice counts twice
            while (m) {
                const int l = __builtin_ctzll(m);
                m &= m - 1ull;
                const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)plo, l), p1 = (uint32_t)__builtin_amdgcn_readlane((int)phi, l);
                sum_packets<SD>(a, p0, p1, lane, tile0, lim, bins);
            }
        }
    } else {
        const int64_t r0 = chunk * a.rows_per_chunk, r1 = min(a.n_rows, r0 + a.rows_per_chunk);
        const int64_t n_w = (a.bit0 + a.n_rows + 31) >> 5, n_lw = (a.n_rows + 31) >> 5;
        const uint32_t* wq = a.words ? a.words + b * (size_t)a.ld_words : nullptr;
        for (int64_t rb = r0; rb < r1; rb += kTermSpanRows) {                            // every wave holds the span, its steps are dealt out
            const int nsub = (int)((min(r1, rb + kTermSpanRows) - rb + 63) >> 6);
            Span lv{~0u, ~0u}, sp{~0u, ~0u};
            int shl = 0, sh = 0;
            if (a.live) {
                lv = load_span(a.live, rb >> 5, n_lw, lane);
                shl = (int)(rb & 31);
                if (__builtin_amdgcn_ballot_w64((lv.lo | lv.hi) != 0u) == 0ull) continue;
            }
            if (wq) {
                const int64_t p = a.bit0 + rb;
                sp = load_span(wq, p >> 5, n_w, lane);
                sh = (int)(p & 31);
                if (__builtin_amdgcn_ballot_w64((sp.lo | sp.hi) != 0u) == 0ull) continue;
            }
            for (int s = w; s < nsub; s += kSumWaves) {
                const int64_t row0 = rb + (int64_t)s * 64;
                const int64_t nvalid = r1 - row0;                                        // >= 1
                const uint64_t vm = nvalid >= 64 ? ~0ull : ((1ull << nvalid) - 1ull);    // bits at or past the last row are ignored
                uint64_t m = window64(lv, s, shl) & window64(sp, s, sh) & vm;
                if (m == 0ull) continue;                                                 // (uniform) no row is touched
                tot += (uint32_t)__popcll(m);
                uint32_t plo = 0u, phi = 0u;
                if (lane < nvalid) {
                    plo = a.pk_ptr[row0 + lane];
                    phi = a.pk_ptr[row0 + lane + 1];
                }
                while (m) {                                                              // runs of consecutive set rows: one packet range each
                    const int first = __builtin_ctzll(m);
                    const uint64_t up = ~(m >> first);                                   // (bit `len` is the first clear one behind the run)
                    const int len = up ? __builtin_ctzll(up) : 64;
                    const int last = first + len - 1;                                    // <= 63
                    const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)plo, first);
                    const uint32_t p1 = (uint32_t)__builtin_amdgcn_readlane((int)phi, last);
                    sum_packets<SD>(a, p0, p1, lane, tile0, lim, bins);
                    m = last >= 63 ? 0ull : (m & (~0ull << (last + 1)));
                }
            }
        }
    }
    if (tile == 0u && lane == 0 && tot) atomicAdd(&s_tot, tot);   // every tile walks the same rows: one of them reports them
    __syncthreads();
    unsigned long long* dst = a.sums + b * (size_t)a.ld_sums + tile0;
    for (uint32_t i = tid; i < lim; i += kSumThreads) {
        const unsigned long long v = bins[i];
        if (v) atomicAdd(dst + i, v);
    }
    if (tid == 0 && s_tot) atomicAdd(&a.total[b], (unsigned long long)s_tot);
}

int plan_or_fail(int rc, const char* msg) { return rc == VS_OK ? VS_OK : fail(rc, "%s", msg); }

template <int SD, int IDS>
int sums_launch(const SumArgs& a, dim3 grid, hipStream_t s) {
    const size_t lds = (size_t)((a.tile_cols + 1) / 2) * 16;
    VS_HIP(hipFuncSetAttribute((const void*)term_sums_kernel<SD, IDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((term_sums_kernel<SD, IDS>), grid, dim3(kSumThreads), lds, s, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int index_ok(const vs_index* idx) {
    if (idx->kind != VS_KIND_CSR) return fail(VS_EUNSUPPORTED, "term sums read the CSR packets: a dense index on the matrix cores has none");
    if (idx->n_cols > kTermMaxCols) return fail(VS_EUNSUPPORTED, "n_cols = %d is too wide", idx->n_cols);
    return VS_OK;
}

// One call on the index's device: the set is (words, bit0, ld_words) when ids == nullptr, else the id lists.
int sums_call(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, const int64_t* ids, int64_t m, int64_t ld_ids, int64_t id_offset,
              int strict, int32_t B, const TermSumPlan& plan, int64_t* sums, int64_t ld_sums, int64_t* total, void* stream) {
    const int32_t V = idx->n_cols;
    const void* ptrs[4] = {words, ids, sums, total};
    const char* names[4] = {"words", "ids", "sums", "total"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 4, idx->device, &dev));
    if (ids && !dev && strict) {
        char msg[256];
        VS_TRY(plan_or_fail(term_check_ids_host(ids, B, m, ld_ids, id_offset, idx->n_rows, msg, sizeof msg), msg));
    }
    VS_HIP(hipSetDevice(idx->device));
    hipStream_t s = (hipStream_t)stream;
    Staged st_w, st_i;
    DevBuf out;
    SumArgs a{};
    uint32_t* d_w = nullptr;
    int64_t* d_i = nullptr;
    if (ids) {
        VS_TRY(st_i.in(ids, (size_t)(B - 1) * (size_t)ld_ids + (size_t)m, dev, true, s, &d_i));
    } else {
        const int64_t span = (bit0 + idx->n_rows + 31) >> 5;
        VS_TRY(st_w.in(words, (size_t)((B - 1) * ld_words + span), dev, true, s, &d_w));
    }
    a.pk_ptr = idx->pk_ptr.as<uint32_t>();
    a.cols = idx->cols.as<uint4>();
    a.vals = idx->vals.p;
    a.n_cols = V;
    a.n_rows = idx->n_rows;
    a.live = idx->has_tomb ? idx->live.as<uint32_t>() : nullptr;     // tombstones are ANDed in at bit 0 whatever bit0 is
    a.words = d_w;
    a.bit0 = bit0;
    a.ld_words = words ? ld_words : 0;
    a.ids = d_i;
    a.ld_ids = ld_ids;
    a.m = m;
    a.id_offset = id_offset;
    a.rows_per_chunk = plan.rows_per_chunk;
    a.B = B;
    a.tiles = plan.tiles;
    a.tile_cols = plan.tile_cols;
    const size_t n_sum = (size_t)B * (size_t)V;
    if (dev) {
        a.sums = reinterpret_cast<unsigned long long*>(sums);
        a.ld_sums = ld_sums;
        a.total = reinterpret_cast<unsigned long long*>(total);
        if (ld_sums == V || B == 1) VS_HIP(hipMemsetAsync(a.sums, 0, n_sum * 8, s));
        else VS_HIP(hipMemset2DAsync(a.sums, (size_t)ld_sums * 8, 0, (size_t)V * 8, (size_t)B, s));
        VS_HIP(hipMemsetAsync(a.total, 0, (size_t)B * 8, s));
    } else {
        VS_TRY(out.alloc((n_sum + (size_t)B) * 8));
        a.sums = out.as<unsigned long long>();
        a.ld_sums = V;
        a.total = a.sums + n_sum;
        VS_HIP(hipMemsetAsync(out.p, 0, out.bytes, s));
    }
    if (idx->n_rows > 0) {
        ProfScope prof("term_sums", s);
        const dim3 grid((unsigned)(plan.chunks * B * plan.tiles));
        const int sd = idx->store_dtype;
        const int rc = ids ? (sd == VS_F32 ? sums_launch<VS_F32, 1>(a, grid, s)
                              : sd == VS_F16 ? sums_launch<VS_F16, 1>(a, grid, s)
                                             : sums_launch<VS_NONE, 1>(a, grid, s))
                           : (sd == VS_F32 ? sums_launch<VS_F32, 0>(a, grid, s)
                              : sd == VS_F16 ? sums_launch<VS_F16, 0>(a, grid, s)
                                             : sums_launch<VS_NONE, 0>(a, grid, s));
        if (rc != VS_OK) {
            (void)hipStreamSynchronize(s);                          // staging buffers die here
            return rc;
        }
    }
    VS_STAGE("term_sums", s);
    if (!dev) {
        VS_HIP(hipMemcpy2DAsync(sums, (size_t)ld_sums * 8, a.sums, (size_t)V * 8, (size_t)V * 8, (size_t)B, hipMemcpyDeviceToHost, s));
        VS_HIP(hipMemcpyAsync(total, a.total, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    }
    if (!stream || !dev) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}

// ---- top-n ---------------------------------------------------------------------------------------------------------------------------
struct SumTopnArgs {
    const int64_t* sums;              // [B, ld_sums]
    int64_t ld_sums;
    const int64_t* total;             // [B]
    const int64_t* counts;            // [B, ld_counts] or null
    int64_t ld_counts, min_count;
    int32_t n_cols, n;
    int32_t* out_cols;                // [B, n]
    float* out_score;                 // [B, n]
    int64_t* out_sums;                // [B, n]
};

// the mean weight of a column (sum >= 1, total >= 1): conversions, x and / in fp64, one rounding to fp32
__device__ __forceinline__ float mean_weight(int64_t sum, int64_t total) {
#pragma clang fp contract(off)
    const double s = ((double)sum * 5.9604644775390625e-08) / (double)total;       // 2^-VS_TERM_FX_SHIFT
    return (float)s;
}

__global__ __launch_bounds__(kTopnThreads) void term_sum_topn_kernel(SumTopnArgs a) {
    __shared__ uint64_t cand[kTopnCap];
    __shared__ int cnt_sh;
    const int tid = threadIdx.x, lane = tid & 63;
    constexpr int SB = (kTopnCap - kTopnKeep) / kTopnThreads;    // steps between prune checks
    static_assert(SB >= 1, "a step adds up to kTopnThreads candidates");
    const int K = a.n;
    const size_t b = blockIdx.x;
    const int64_t* src = a.sums + b * (size_t)a.ld_sums;
    const int64_t* cnt_row = a.counts ? a.counts + b * (size_t)a.ld_counts : nullptr;
    const int64_t total = a.total[b];
    if (tid == 0) cnt_sh = 0;
    __syncthreads();
    uint64_t tau = 0;
    const int iters = (a.n_cols + kTopnThreads - 1) / kTopnThreads;
    for (int it0 = 0; it0 < iters; it0 += SB) {
        const int it1 = min(iters, it0 + SB);
        for (int it = it0; it < it1; ++it) {
            const int c = it * kTopnThreads + tid;
            uint64_t key = 0ull;
            if (total > 0 && c < a.n_cols) {
                const int64_t sum = src[c];
                if (sum > 0 && (!cnt_row || cnt_row[c] >= a.min_count)) key = make_key(mean_weight(sum, total), (uint32_t)c);
            }
            const bool pass = key > tau;                          // (key 0: no candidate -- a score is not negative, its key has the top bit set)
            const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
            if (m) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&cnt_sh, __popcll(m));
                base = __shfl(base, 0, 64);
                if (pass) cand[base + __popcll(m & ((1ull << lane) - 1ull))] = key;
            }
        }
        __syncthreads();
        const int cnt = cnt_sh;
        const bool last = it1 >= iters;
        if (last || cnt > kTopnKeep) {                           // uniform: cnt read after the barrier
            for (int i = cnt + tid; i < kTopnCap; i += kTopnThreads) cand[i] = 0ull;
            wg_sort_desc<kTopnThreads>(cand, kTopnCap, tid);
            if (!last && cnt > K) {
                tau = cand[K - 1];
                __syncthreads();
                if (tid == 0) cnt_sh = K;
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < K; i += kTopnThreads) {                 // every slot is written: -1 / -inf / 0 behind the last
        const uint64_t key = cand[i];
        const size_t o = b * (size_t)K + i;
        const uint32_t c = key_row(key);
        a.out_cols[o] = key ? (int32_t)c : -1;
        a.out_score[o] = key ? key_score(key) : -INFINITY;
        a.out_sums[o] = key ? src[c] : 0;
    }
}

}  // namespace

extern "C" int vs_term_sum_plan(int64_t n_rows, int32_t B, int32_t n_cols, int per_query, int64_t rows_per_chunk, int32_t tile_cols,
                                int32_t* out_tiles, int32_t* out_tile_cols, int64_t* out_chunks, int64_t* out_rows_per_chunk) {
    if (!out_tiles || !out_tile_cols || !out_chunks || !out_rows_per_chunk) return fail(VS_EINVAL, "NULL argument");
    TermSumPlan p;
    char msg[256];
    VS_TRY(plan_or_fail(term_sum_plan(n_rows, B, n_cols, per_query != 0, rows_per_chunk, tile_cols, &p, msg, sizeof msg), msg));
    *out_tiles = p.tiles;
    *out_tile_cols = p.tile_cols;
    *out_chunks = p.chunks;
    *out_rows_per_chunk = p.rows_per_chunk;
    return VS_OK;
}

extern "C" int vs_index_term_sums(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, int64_t rows_per_chunk,
                                  int32_t tile_cols, int64_t* sums, int64_t ld_sums, int64_t* total, void* stream) {
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    VS_TRY(index_ok(idx));
    TermSumPlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(term_sum_check_sums(words != nullptr, bit0, ld_words, B, std::max<int64_t>(idx->n_rows, 1), idx->n_cols, rows_per_chunk,
                                            tile_cols, sums && total, ld_sums, &plan, msg, sizeof msg), msg));
    return sums_call(idx, words, bit0, ld_words, nullptr, 0, 0, 0, 0, B, plan, sums, ld_sums, total, stream);
}

extern "C" int vs_index_term_sums_ids(vs_index* idx, const int64_t* ids, int32_t B, int64_t m, int64_t ld, int64_t id_offset, int strict,
                                      int32_t tile_cols, int64_t* sums, int64_t ld_sums, int64_t* total, void* stream) {
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    VS_TRY(index_ok(idx));
    TermSumPlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(term_sum_check_ids(ids != nullptr, B, m, ld, idx->n_cols, tile_cols, sums && total, ld_sums, &plan, msg, sizeof msg), msg));
    return sums_call(idx, nullptr, 0, 0, ids, m, ld, id_offset, strict, B, plan, sums, ld_sums, total, stream);
}

extern "C" int vs_term_sum_topn(const int64_t* sums, int64_t ld_sums, const int64_t* total, const int64_t* counts, int64_t ld_counts, int32_t B,
                                int32_t n_cols, int32_t n, int64_t min_count, int32_t* out_cols, float* out_score, int64_t* out_sums, int device,
                                void* stream) {
    char msg[256];
    VS_TRY(plan_or_fail(term_sum_check_topn(sums && total && out_cols && out_score && out_sums, counts != nullptr, B, n_cols, ld_sums, ld_counts, n,
                                            msg, sizeof msg), msg));
    VS_TRY(need_device());
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range", device);
    const void* ptrs[6] = {sums, total, counts, out_cols, out_score, out_sums};
    const char* names[6] = {"sums", "total", "counts", "out_cols", "out_score", "out_sums"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 6, device, &dev));
    VS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    Staged st[6];
    SumTopnArgs a{};
    int64_t *d_sums, *d_total, *d_counts;
    VS_TRY(st[0].in(sums, (size_t)(B - 1) * (size_t)ld_sums + (size_t)n_cols, dev, true, s, &d_sums));
    VS_TRY(st[1].in(total, (size_t)B, dev, true, s, &d_total));
    VS_TRY(st[2].in(counts, counts ? (size_t)(B - 1) * (size_t)ld_counts + (size_t)n_cols : 0, dev, true, s, &d_counts));    // (NULL stays NULL)
    VS_TRY(st[3].in(out_cols, (size_t)B * n, dev, false, s, &a.out_cols));
    VS_TRY(st[4].in(out_score, (size_t)B * n, dev, false, s, &a.out_score));
    VS_TRY(st[5].in(out_sums, (size_t)B * n, dev, false, s, &a.out_sums));
    a.sums = d_sums;
    a.ld_sums = ld_sums;
    a.total = d_total;
    a.counts = d_counts;
    a.ld_counts = ld_counts;
    a.min_count = min_count;
    a.n_cols = n_cols;
    a.n = n;
    {
        ProfScope prof("term_sum_topn", s);
        hipLaunchKernelGGL(term_sum_topn_kernel, dim3((unsigned)B), dim3(kTopnThreads), 0, s, a);
        VS_HIP(hipGetLastError());
    }
    VS_STAGE("term_sum_topn", s);
    if (!dev)
        for (int i = 3; i < 6; ++i) VS_TRY(st[i].back(s));
    if (!stream || !dev) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}
