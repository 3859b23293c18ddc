// values.hip -- numeric fields (vs_value_range_bitmaps, vs_value_plan, vs_value_stats, vs_value_histogram, vs_value_topk and their vs_index_*
// variants): range filters, stats, histograms and sort by value over one 32-bit quantity per row.  No reference counterpart
// (the reference only has topk, index.py:92).  Nothing here touches a search kernel: a set arrives as a packed bitmap in the layout of
// vs_index_search_filtered, the values as fp32 or int32 [n_rows].  Everything is decided on the uint32 order keys of value_check.h (0 = the
// row has no value), so every result is exact and independent of the launch.
//
// (a) Range bitmaps: a wave owns 64 bits of every bitmap.  It loads its rows' keys once and, per range, forms the two words with one ballot;
//     lane b of a batch of 64 ranges keeps the ballot of range b and stores it: plain stores, every word written exactly once.
// (b) Stats / histogram: a workgroup owns a chunk of rows and a tile of QT queries and walks the bitmaps with walk_tile (set_walk.h: 2048-row
//     spans, all-zero spans left at once); a row's value is loaded once for the tile.
//       histogram: the edge keys in LDS, bin = value_bin (branch-free, 11 steps), one uint32 histogram of n_edges + 2 slots per query in LDS
//                  (slot 0 below, 1 .. n_edges - 1 the bins, n_edges above, n_edges + 1 missing), flushed with 64-bit atomicAdd.
//       stats:     min key, max key and sum per lane and query; wave reduction by shuffles, workgroup reduction by LDS atomics, one global
//                  atomic per (workgroup, query) and output.  The min / max outputs hold KEYS until value_finish_kernel turns them into values.
// (c) Top-k: a workgroup owns a chunk and one query.  All four waves walk the same span (walk_rows), each a quarter of its 64-row steps, and
//     push (key or ~key) << 32 | ~row above the threshold into the buffer of topn_stream.h; after a span with more than 2048 keys in, the
//     buffer is sorted, cut to k, and the k-th key becomes the threshold.  Per-chunk lists go to scratch; value_topk_merge_kernel, one
//     workgroup per query, streams them through the same buffer (stream_topn) and writes ids and the rows' stored values.
#include "agg_call.h"
#include "term_sum_check.h"
#include "topn_stream.h"
#include "value_check.h"

using namespace vs;

namespace {

static_assert(kTopCap - kTopKeep >= kSpanRows, "a span adds up to kSpanRows candidates");

// ---- (a) range bitmaps -----------------------------------------------------------------------------------------------------------------------
struct RangeArgs {
    const uint32_t* values;           // [n_rows] raw
    int dtype;
    int64_t n_rows;
    const uint32_t *lo, *hi;          // [B] raw
    int32_t B;
    int64_t bit0, n_words;            // n_words = (bit0 + n_rows + 31) / 32 words of a row are written
    uint32_t* out;                    // [B, ld]
    int64_t ld;
};

__global__ __launch_bounds__(kValThreads) void value_range_kernel(RangeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kValWaves + (threadIdx.x >> 6);          // this wave owns words 2 g and 2 g + 1 of every row
    const int64_t w0 = 2 * g;
    if (w0 >= a.n_words) return;                                                     // (wave-uniform)
    const int64_t r = 64 * g + lane - a.bit0;                                         // the row behind bit 64 g + lane
    const bool valid = r >= 0 && r < a.n_rows;
    const uint32_t key = valid ? value_key(a.values[r], a.dtype) : 0u;                // 0: no value, in no range
    const bool two = w0 + 1 < a.n_words;
    for (int32_t b0 = 0; b0 < a.B; b0 += 64) {
        const int n = min(64, a.B - b0);
        uint32_t klo = 1u, khi = 0u;                                                  // (empty)
        if (lane < n) {
            klo = value_key(a.lo[b0 + lane], a.dtype);
            khi = value_key(a.hi[b0 + lane], a.dtype);
            if (klo == 0u || khi == 0u) {                                             // a missing bound matches nothing
                klo = 1u;
                khi = 0u;
            }
        }
        uint64_t bits = 0ull;
        for (int k = 0; k < n; ++k) {
            const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)klo, k);
            const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)khi, k);
            const uint64_t m = __builtin_amdgcn_ballot_w64(key != 0u && l <= key && key <= h);
            if (lane == k) bits = m;
        }
        if (lane < n) {                                                               // range b0 + lane: its two words
            uint32_t* dst = a.out + (size_t)(b0 + lane) * (size_t)a.ld + w0;
            dst[0] = (uint32_t)bits;
            if (two) dst[1] = (uint32_t)(bits >> 32);
        }
    }
}

// ---- (b) stats and histogram -------------------------------------------------------------------------------------------------------------------
struct StatsArgs {
    SetArgs s;
    unsigned long long *count, *missing, *sum;     // [B], zeroed by the caller
    uint32_t *min_key, *max_key;                   // [B], 0xFFFFFFFF / 0 set by the caller
};

struct HistArgs {
    SetArgs s;
    const uint32_t* edges;            // [n_edges] raw
    int32_t n_edges;
    unsigned long long* counts;       // [B, ld_counts], columns [0, n_edges - 1) zeroed by the caller
    int64_t ld_counts;
    unsigned long long *below, *above, *missing;   // [B], zeroed by the caller
};

template <int QT>
__global__ __launch_bounds__(kValThreads) void value_stats_kernel(StatsArgs a) {
    __shared__ uint32_t s_cnt[QT], s_mis[QT], s_min[QT], s_max[QT];
    __shared__ unsigned long long s_sum[QT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q0 = (int)blockIdx.y * QT;
    const int nq = min(QT, a.s.set.B - q0);
    const int64_t r0 = (int64_t)blockIdx.x * a.s.set.rows_per_chunk;
    const int64_t r1 = min(a.s.set.n_rows, r0 + a.s.set.rows_per_chunk);
    if (tid < QT) {
        s_cnt[tid] = s_mis[tid] = 0u;
        s_min[tid] = 0xFFFFFFFFu;
        s_max[tid] = 0u;
        s_sum[tid] = 0ull;
    }
    __syncthreads();
    uint32_t cnt[QT], mis[QT];                                   // wave-uniform: a chunk holds fewer than 2^32 rows
    uint32_t kmin[QT], kmax[QT];                                 // per lane
    uint64_t sum[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        cnt[q] = mis[q] = 0u;
        kmin[q] = 0xFFFFFFFFu;
        kmax[q] = 0u;
        sum[q] = 0ull;
    }
    const bool f32 = a.s.dtype == VS_VAL_F32;
    walk_tile<QT, kValWaves>(a.s.set, q0, nq, r0, r1, w, lane, [&](int64_t row0, uint64_t many, const Span* sp, int s, int sh, uint64_t live) {
        const uint32_t raw = (many >> lane) & 1ull ? a.s.values[row0 + lane] : 0u;   // once for the tile
        const uint32_t key = (many >> lane) & 1ull ? value_key(raw, a.s.dtype) : 0u;
        // what the row adds to a sum: fx(v) of the term sums for fp32, the integer itself for int32; nothing without a value
        uint64_t add = 0ull;
        if (key != 0u) add = f32 ? term_fx(__uint_as_float(raw)) : (uint64_t)(int64_t)(int32_t)raw;
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            if (q >= nq) continue;
            const uint64_t m = window64(sp[q], s, sh) & live;
            if (m == 0ull) continue;
            const bool in = (m >> lane) & 1ull;
            const bool has = in && key != 0u;
            const uint32_t c = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(has));
            cnt[q] += c;
            mis[q] += (uint32_t)__popcll(m) - c;
            if (has) {
                kmin[q] = min(kmin[q], key);
                kmax[q] = max(kmax[q], key);
                sum[q] += add;
            }
        }
    });
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        if (q >= nq) continue;
        uint32_t lo = kmin[q], hi = kmax[q];
        uint64_t sm = sum[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
            hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, 64));
            sm += (uint64_t)__shfl_xor((unsigned long long)sm, o, 64);
        }
        if (lane == 0 && (cnt[q] | mis[q])) {
            atomicAdd(&s_cnt[q], cnt[q]);
            atomicAdd(&s_mis[q], mis[q]);
            atomicMin(&s_min[q], lo);
            atomicMax(&s_max[q], hi);
            atomicAdd(&s_sum[q], (unsigned long long)sm);
        }
    }
    __syncthreads();
    if (tid < nq) {
        const int b = q0 + tid;
        if (s_cnt[tid]) {
            atomicAdd(&a.count[b], (unsigned long long)s_cnt[tid]);
            atomicMin(&a.min_key[b], s_min[tid]);
            atomicMax(&a.max_key[b], s_max[tid]);
            if (s_sum[tid]) atomicAdd(&a.sum[b], s_sum[tid]);
        }
        if (s_mis[tid]) atomicAdd(&a.missing[b], (unsigned long long)s_mis[tid]);
    }
}

// keys -> raw values, in place; no row with a value: the missing sentinel
__global__ void value_finish_kernel(uint32_t* min_key, uint32_t* max_key, const unsigned long long* count, int32_t B, int dtype) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const bool any = count[b] != 0ull;
    min_key[b] = value_unkey(any ? min_key[b] : 0u, dtype);
    max_key[b] = value_unkey(any ? max_key[b] : 0u, dtype);
}

template <int QT>
__global__ __launch_bounds__(kValThreads) void value_hist_kernel(HistArgs a) {
    extern __shared__ uint32_t val_lds[];                        // edge keys [n_edges], then the histograms [nq][n_edges + 2]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q0 = (int)blockIdx.y * QT;
    const int nq = min(QT, a.s.set.B - q0);
    const int64_t r0 = (int64_t)blockIdx.x * a.s.set.rows_per_chunk;
    const int64_t r1 = min(a.s.set.n_rows, r0 + a.s.set.rows_per_chunk);
    const int E = a.n_edges;
    const uint32_t S = (uint32_t)E + 2u;                         // slots of a query
    uint32_t* ekeys = val_lds;
    uint32_t* hist = val_lds + E;
    for (int i = tid; i < E; i += kValThreads) ekeys[i] = value_key(a.edges[i], a.s.dtype);
    for (uint32_t i = tid; i < (uint32_t)nq * S; i += kValThreads) hist[i] = 0u;
    __syncthreads();
    walk_tile<QT, kValWaves>(a.s.set, q0, nq, r0, r1, w, lane, [&](int64_t row0, uint64_t many, const Span* sp, int s, int sh, uint64_t live) {
        const uint32_t key = (many >> lane) & 1ull ? value_key(a.s.values[row0 + lane], a.s.dtype) : 0u;
        const uint32_t slot = key == 0u ? (uint32_t)E + 1u : (uint32_t)value_bin(ekeys, E, key);      // once for the tile
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            if (q >= nq) continue;
            const uint64_t m = window64(sp[q], s, sh) & live;
            if (m == 0ull) continue;
            const bool in = (m >> lane) & 1ull;
            const int first = __builtin_ctzll(m);
            const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)slot, first);
            const bool one = __builtin_amdgcn_ballot_w64(in && slot == s0) == m;      // every row of the step in one slot: add once
            uint32_t* dst = hist + (size_t)q * S;
            if (one) {
                if (lane == first) atomicAdd(dst + s0, (uint32_t)__popcll(m));
            } else if (in) {
                atomicAdd(dst + slot, 1u);
            }
        }
    });
    __syncthreads();
    for (int q = 0; q < nq; ++q) {
        const size_t b = (size_t)(q0 + q);
        unsigned long long* dst = a.counts + b * (size_t)a.ld_counts;
        for (uint32_t i = tid; i < S; i += kValThreads) {
            const uint32_t v = hist[(size_t)q * S + i];
            if (!v) continue;
            unsigned long long* p = i == 0u ? a.below + b : i == (uint32_t)E ? a.above + b : i == (uint32_t)E + 1u ? a.missing + b : dst + (i - 1u);
            atomicAdd(p, (unsigned long long)v);
        }
    }
}

// ---- (c) top-k ------------------------------------------------------------------------------------------------------------------------------------
struct TopArgs {
    SetArgs s;
    int32_t k;
    uint32_t flip;                    // 0: descending (key as it is), 0xFFFFFFFF: ascending (~key)
    int64_t chunks;
    uint64_t* scratch;                // [B, chunks, k]
    int64_t id_offset;
    int64_t* out_ids;                 // [B, k]
    uint32_t* out_values;             // [B, k] raw
};

__global__ __launch_bounds__(kValThreads) void value_topk_chunk_kernel(TopArgs a) {
    __shared__ uint64_t cand[kTopCap];
    __shared__ int cnt_sh;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t c = blockIdx.x;
    const size_t b = blockIdx.y;
    const int K = a.k;
    const int64_t r0 = c * a.s.set.rows_per_chunk;
    const int64_t r1 = min(a.s.set.n_rows, r0 + a.s.set.rows_per_chunk);
    if (tid == 0) cnt_sh = 0;
    __syncthreads();
    uint64_t tau = 0ull;
    walk_rows<kValWaves>(a.s.set, b, r0, r1, w, lane, [&](int64_t row0, uint64_t m, int64_t) {
        uint64_t key = 0ull;
        if ((m >> lane) & 1ull) {
            const uint32_t k32 = value_key(a.s.values[row0 + lane], a.s.dtype);
            if (k32 != 0u) key = ((uint64_t)(k32 ^ a.flip) << 32) | (uint32_t)~(uint32_t)(row0 + lane);      // never 0: row < 2^32 - 1
        }
        top_push(cand, &cnt_sh, key > tau, key, lane);
    }, [&] {                                                     // (the walk leaves a span for the whole workgroup or not at all)
        __syncthreads();
        tau = top_cut<kValThreads>(cand, &cnt_sh, K, false, tau, tid);
    });
    __syncthreads();
    (void)top_cut<kValThreads>(cand, &cnt_sh, K, true, tau, tid);
    uint64_t* dst = a.scratch + (b * (size_t)a.chunks + (size_t)c) * (size_t)K;
    for (int i = tid; i < K; i += kValThreads) dst[i] = cand[i];                     // sorted, zeros behind the last
}

__global__ __launch_bounds__(kValThreads) void value_topk_merge_kernel(TopArgs a) {
    __shared__ uint64_t cand[kTopCap];
    __shared__ int cnt_sh;
    const int tid = threadIdx.x;
    const int K = a.k;
    const size_t b = blockIdx.x;
    const uint64_t* src = a.scratch + b * (size_t)a.chunks * (size_t)K;
    stream_topn<kValThreads>(a.chunks * K, K, [&](int64_t i) { return src[i]; }, cand, &cnt_sh);
    const uint32_t miss = a.s.dtype == VS_VAL_F32 ? kValueNanF32 : kValueMissI32;
    for (int i = tid; i < K; i += kValThreads) {                  // every slot is written: id -1 / the missing sentinel behind the last
        const uint64_t key = cand[i];
        const uint32_t row = ~(uint32_t)key;
        a.out_ids[b * (size_t)K + i] = key ? (int64_t)row + a.id_offset : -1;
        a.out_values[b * (size_t)K + i] = key ? a.s.values[row] : miss;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
// host arrays are looked at before the device is (a pointer the runtime does not know, or no runtime at all: a host pointer)
int check_edges(const void* edges, int32_t n_edges, int dtype) {
    if (is_device_ptr(edges)) return VS_OK;
    char msg[256];
    return plan_or_fail(value_check_edges_host(static_cast<const uint32_t*>(edges), n_edges, dtype, msg, sizeof msg), msg);
}

// the set of a call -> its plan (n_bins: the LDS slots of a query, 0 = none; max_qt: the widest tile of the kernel)
int check_set(const SetSrc& src, bool have_ptrs, int dtype, int32_t n_bins, int64_t rows_per_chunk, int32_t max_qt, ValuePlan* plan) {
    char msg[256];
    return plan_or_fail(value_check_set(have_ptrs, src.words != nullptr, src.bit0, src.ld_words, src.B, dtype, src.n_rows, n_bins, rows_per_chunk, max_qt,
                                        plan, msg, sizeof msg), msg);
}

// vs_value_stats and vs_index_value_stats: one call on the set's device
int value_stats(const SetSrc& src, const void* values, int dtype, int64_t rows_per_chunk, int64_t* count, int64_t* missing, void* out_min,
                void* out_max, int64_t* sum, void* stream) {
    ValuePlan plan;
    VS_TRY(check_set(src, values && count && missing && out_min && out_max && sum, dtype, 0, rows_per_chunk, 8, &plan));
    VS_TRY(src.device_ok());
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"values", values}, {"count", count}, {"missing", missing},
                                       {"out_min", out_min}, {"out_max", out_max}, {"sum", sum}}));
    const int32_t B = src.B;
    SetStage st;
    StatsArgs a{};
    DevBuf out;                                                   // host outputs: count, missing, sum [B] x 8 bytes, then min, max [B] x 4
    return c.run("value_stats", Finish::kStream, [&] {
        VS_TRY(st.in(src, values, dtype, plan.rows_per_chunk, c.dev, c.s, &a.s));
        if (c.dev) {
            a.count = reinterpret_cast<unsigned long long*>(count);
            a.missing = reinterpret_cast<unsigned long long*>(missing);
            a.sum = reinterpret_cast<unsigned long long*>(sum);
            a.min_key = static_cast<uint32_t*>(out_min);
            a.max_key = static_cast<uint32_t*>(out_max);
        } else {
            VS_TRY(out.alloc((size_t)B * 32));
            a.count = out.as<unsigned long long>();
            a.missing = a.count + B;
            a.sum = a.missing + B;
            a.min_key = reinterpret_cast<uint32_t*>(a.sum + B);
            a.max_key = a.min_key + B;
        }
        VS_HIP(hipMemsetAsync(a.count, 0, (size_t)B * 8, c.s));
        VS_HIP(hipMemsetAsync(a.missing, 0, (size_t)B * 8, c.s));
        VS_HIP(hipMemsetAsync(a.sum, 0, (size_t)B * 8, c.s));
        VS_HIP(hipMemsetAsync(a.min_key, 0xFF, (size_t)B * 4, c.s));
        VS_HIP(hipMemsetAsync(a.max_key, 0, (size_t)B * 4, c.s));
        ProfScope prof("value_stats", c.s);
        const dim3 grid((unsigned)plan.chunks, (unsigned)ceil_div64(B, plan.qt));
        if (plan.qt == 8) hipLaunchKernelGGL(value_stats_kernel<8>, grid, dim3(kValThreads), 0, c.s, a);
        else hipLaunchKernelGGL(value_stats_kernel<1>, grid, dim3(kValThreads), 0, c.s, a);
        hipLaunchKernelGGL(value_finish_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, c.s, a.min_key, a.max_key, a.count, B, dtype);
        return VS_OK;
    }, [&] {
        VS_HIP(hipMemcpyAsync(count, a.count, (size_t)B * 8, hipMemcpyDeviceToHost, c.s));
        VS_HIP(hipMemcpyAsync(missing, a.missing, (size_t)B * 8, hipMemcpyDeviceToHost, c.s));
        VS_HIP(hipMemcpyAsync(sum, a.sum, (size_t)B * 8, hipMemcpyDeviceToHost, c.s));
        VS_HIP(hipMemcpyAsync(out_min, a.min_key, (size_t)B * 4, hipMemcpyDeviceToHost, c.s));
        VS_HIP(hipMemcpyAsync(out_max, a.max_key, (size_t)B * 4, hipMemcpyDeviceToHost, c.s));
        return VS_OK;
    });
}

// vs_value_histogram and vs_index_value_histogram
int value_histogram(const SetSrc& src, const void* values, int dtype, const void* edges, int32_t n_edges, int64_t rows_per_chunk, int64_t* counts,
                    int64_t ld_counts, int64_t* below, int64_t* above, int64_t* missing, void* stream) {
    ValuePlan plan;
    char msg[256];
    if (!values || !edges || !counts || !below || !above || !missing) return fail(VS_EINVAL, "NULL argument");
    VS_TRY(plan_or_fail(value_check_hist(n_edges, ld_counts, msg, sizeof msg), msg));
    VS_TRY(check_set(src, true, dtype, n_edges + 2, rows_per_chunk, 8, &plan));
    VS_TRY(check_edges(edges, n_edges, dtype));
    VS_TRY(src.device_ok());
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"values", values}, {"edges", edges}, {"counts", counts},
                                       {"below", below}, {"above", above}, {"missing", missing}}));
    SetStage st;
    Staged st_e;
    CountsOut out;
    return c.run("value_histogram", Finish::kStream, [&] {
        HistArgs a{};
        VS_TRY(st.in(src, values, dtype, plan.rows_per_chunk, c.dev, c.s, &a.s));
        uint32_t* d_e;
        VS_TRY(st_e.in(static_cast<const uint32_t*>(edges), (size_t)n_edges, c.dev, true, c.s, &d_e));
        a.edges = d_e;
        a.n_edges = n_edges;
        VS_TRY(out.bind(c.dev, counts, ld_counts, n_edges - 1, src.B, {below, above, missing}, c.s));
        a.counts = out.mat;
        a.ld_counts = out.ld;
        a.below = out.vec[0];
        a.above = out.vec[1];
        a.missing = out.vec[2];
        ProfScope prof("value_histogram", c.s);
        const dim3 grid((unsigned)plan.chunks, (unsigned)ceil_div64(src.B, plan.qt));
        const size_t lds = ((size_t)n_edges + (size_t)plan.qt * ((size_t)n_edges + 2)) * 4;      // at most 37 KB
        if (plan.qt == 8) hipLaunchKernelGGL(value_hist_kernel<8>, grid, dim3(kValThreads), lds, c.s, a);
        else hipLaunchKernelGGL(value_hist_kernel<1>, grid, dim3(kValThreads), lds, c.s, a);
        return VS_OK;
    }, [&] { return out.back(c.s); });
}

// vs_value_topk and vs_index_value_topk
int value_topk(const SetSrc& src, const void* values, int dtype, int32_t k, int descending, int64_t id_offset, int64_t rows_per_chunk,
               int64_t* out_ids, void* out_values, void* stream) {
    ValuePlan plan;
    char msg[256];
    VS_TRY(check_set(src, values && out_ids && out_values, dtype, 0, rows_per_chunk, 1, &plan));
    VS_TRY(plan_or_fail(value_check_topk(k, src.B, plan, msg, sizeof msg), msg));
    VS_TRY(src.device_ok());
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"values", values}, {"out_ids", out_ids},
                                       {"out_values", out_values}}));
    SetStage st;
    Staged st_i, st_v;
    DevBuf scratch;
    return c.run("value_topk", Finish::kSync, [&] {
        TopArgs a{};
        VS_TRY(st.in(src, values, dtype, plan.rows_per_chunk, c.dev, c.s, &a.s));
        VS_TRY(st_i.in(out_ids, (size_t)src.B * k, c.dev, false, c.s, &a.out_ids));
        VS_TRY(st_v.in(static_cast<uint32_t*>(out_values), (size_t)src.B * k, c.dev, false, c.s, &a.out_values));
        VS_TRY(scratch.alloc((size_t)src.B * (size_t)plan.chunks * (size_t)k * 8));
        a.k = k;
        a.flip = descending ? 0u : 0xFFFFFFFFu;
        a.chunks = plan.chunks;
        a.scratch = scratch.as<uint64_t>();
        a.id_offset = id_offset;
        ProfScope prof("value_topk", c.s);
        hipLaunchKernelGGL(value_topk_chunk_kernel, dim3((unsigned)plan.chunks, (unsigned)src.B), dim3(kValThreads), 0, c.s, a);
        hipLaunchKernelGGL(value_topk_merge_kernel, dim3((unsigned)src.B), dim3(kValThreads), 0, c.s, a);
        return VS_OK;
    }, [&] {
        VS_TRY(st_i.back(c.s));
        return st_v.back(c.s);
    });
}

}  // namespace

extern "C" int vs_value_plan(int64_t n_rows, int32_t B, int32_t n_bins, int per_query, int64_t rows_per_chunk, int32_t* out_qt, int64_t* out_chunks,
                             int64_t* out_rows_per_chunk) {
    if (!out_qt || !out_chunks || !out_rows_per_chunk) return fail(VS_EINVAL, "NULL argument");
    ValuePlan p;
    char msg[256];
    VS_TRY(plan_or_fail(value_plan(n_rows, B, n_bins, per_query != 0, rows_per_chunk, 8, &p, msg, sizeof msg), msg));
    *out_qt = p.qt;
    *out_chunks = p.chunks;
    *out_rows_per_chunk = p.rows_per_chunk;
    return VS_OK;
}

extern "C" int vs_value_range_bitmaps(const void* values, int dtype, int64_t n_rows, const void* lo, const void* hi, int32_t B, int64_t bit0,
                                      uint32_t* out_words, int64_t ld_words, int device, void* stream) {
    char msg[256];
    VS_TRY(plan_or_fail(value_check_ranges(values && lo && hi && out_words, dtype, n_rows, B, bit0, ld_words, msg, sizeof msg), msg));
    if (!is_device_ptr(lo) && !is_device_ptr(hi))
        VS_TRY(plan_or_fail(value_check_bounds_host(static_cast<const uint32_t*>(lo), static_cast<const uint32_t*>(hi), B, dtype, msg, sizeof msg), msg));
    VS_TRY(device_in_range(device));
    Call c;
    VS_TRY(c.open(device, stream, {{"values", values}, {"lo", lo}, {"hi", hi}, {"out_words", out_words}}));
    Staged st_v, st_l, st_h, st_o;
    return c.run("value_range_bitmaps", Finish::kStream, [&] {
        RangeArgs a{};
        a.dtype = dtype;
        a.n_rows = n_rows;
        a.B = B;
        a.bit0 = bit0;
        a.n_words = (bit0 + n_rows + 31) >> 5;
        uint32_t *d_v, *d_l, *d_h;
        VS_TRY(st_v.in(static_cast<const uint32_t*>(values), (size_t)n_rows, c.dev, true, c.s, &d_v));
        VS_TRY(st_l.in(static_cast<const uint32_t*>(lo), (size_t)B, c.dev, true, c.s, &d_l));
        VS_TRY(st_h.in(static_cast<const uint32_t*>(hi), (size_t)B, c.dev, true, c.s, &d_h));
        // (a host buffer's gaps between the rows come back as they went in: the staged copy starts from the caller's words)
        VS_TRY(st_o.in(out_words, (size_t)(B - 1) * (size_t)ld_words + (size_t)a.n_words, c.dev, true, c.s, &a.out));
        a.values = d_v;
        a.lo = d_l;
        a.hi = d_h;
        a.ld = ld_words;
        ProfScope prof("value_range_bitmaps", c.s);
        const int64_t waves = (a.n_words + 1) / 2;
        hipLaunchKernelGGL(value_range_kernel, dim3((unsigned)((waves + kValWaves - 1) / kValWaves)), dim3(kValThreads), 0, c.s, a);
        return VS_OK;
    }, [&] { return st_o.back(c.s); });
}

extern "C" int vs_value_stats(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const void* values,
                              int dtype, int64_t n_rows, int64_t rows_per_chunk, int64_t* count, int64_t* missing, void* out_min, void* out_max,
                              int64_t* sum, int device, void* stream) {
    return value_stats(free_set(words, bit0, ld_words, and_words, B, n_rows, device), values, dtype, rows_per_chunk, count, missing, out_min, out_max,
                       sum, stream);
}

extern "C" int vs_index_value_stats(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const void* values, int dtype,
                                    int64_t rows_per_chunk, int64_t* count, int64_t* missing, void* out_min, void* out_max, int64_t* sum,
                                    void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return value_stats(src, values, dtype, rows_per_chunk, count, missing, out_min, out_max, sum, stream);
}

extern "C" int vs_value_histogram(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const void* values,
                                  int dtype, int64_t n_rows, const void* edges, int32_t n_edges, int64_t rows_per_chunk, int64_t* counts,
                                  int64_t ld_counts, int64_t* below, int64_t* above, int64_t* missing, int device, void* stream) {
    return value_histogram(free_set(words, bit0, ld_words, and_words, B, n_rows, device), values, dtype, edges, n_edges, rows_per_chunk, counts,
                           ld_counts, below, above, missing, stream);
}

extern "C" int vs_index_value_histogram(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const void* values,
                                        int dtype, const void* edges, int32_t n_edges, int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts,
                                        int64_t* below, int64_t* above, int64_t* missing, void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return value_histogram(src, values, dtype, edges, n_edges, rows_per_chunk, counts, ld_counts, below, above, missing, stream);
}

extern "C" int vs_value_topk(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const void* values,
                             int dtype, int64_t n_rows, int32_t k, int descending, int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids,
                             void* out_values, int device, void* stream) {
    return value_topk(free_set(words, bit0, ld_words, and_words, B, n_rows, device), values, dtype, k, descending, id_offset, rows_per_chunk, out_ids,
                      out_values, stream);
}

extern "C" int vs_index_value_topk(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const void* values, int dtype,
                                   int32_t k, int descending, int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids, void* out_values,
                                   void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return value_topk(src, values, dtype, k, descending, id_offset, rows_per_chunk, out_ids, out_values, stream);
}
