// facets.hip -- facet counts (vs_facet_counts, vs_index_facet_counts, vs_facet_topn): how a document set spreads over per-row integer labels.
// No reference counterpart (the reference only has topk, index.py:92).  Nothing here touches a search kernel: the set arrives as a packed
// bitmap in the layout of vs_index_search_filtered (a match_filter result, a DocFilter), the labels as int32 [n_rows].
//
// (a) Counts: a workgroup owns a chunk of rows and a tile of QT queries and walks the bitmaps with walk_tile (set_walk.h): a wave per 2048-row
//     span, all-zero spans and steps left at once, and only lanes whose row is in SOME query's set load their label: once for the whole tile.
//       LDS regime    (QT x n_labels <= VS_FACET_LDS_BINS): one uint32 histogram per query of the tile in LDS, filled with LDS atomics and
//                     flushed at the end of the chunk -- one 64-bit vector atomicAdd per non-zero bin into counts (zeroed on the stream first).
//       global regime (n_labels > VS_FACET_LDS_BINS): 64-bit vector atomicAdd straight into counts.
//     A wave whose rows of a step all carry one label adds once (the popcount): the one-label worst case costs an add a step, not 64
//     serialised ones.  total / other are summed per wave in scalar registers, per workgroup in LDS, and added to global memory once.
// (b) Top-n: one workgroup per query streams the counts as keys (count << 32) | (0xFFFFFFFF - label) -- larger key = larger count, then
//     smaller label -- through stream_topn (topn_stream.h).
#include "agg_call.h"
#include "topn_stream.h"

#include <algorithm>

using namespace vs;

namespace {

constexpr int kFacetThreads = 256;
constexpr int kFacetWaves = kFacetThreads / 64;

struct FacetArgs {
    RowSet set;
    const int32_t* labels;            // [n_rows]
    int32_t n_labels;
    unsigned long long* counts;       // [B, ld_counts], zeroed by the caller
    int64_t ld_counts;
    unsigned long long* total;        // [B], zeroed by the caller
    unsigned long long* other;        // [B], zeroed by the caller
};

template <int QT, int GLOBAL>
__global__ __launch_bounds__(kFacetThreads) void facet_counts_kernel(FacetArgs a) {
    extern __shared__ uint32_t facet_hist[];                     // [nq][n_labels] (LDS regime)
    __shared__ uint32_t s_tot[QT], s_oth[QT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q0 = (int)blockIdx.y * QT;
    const int nq = min(QT, a.set.B - q0);
    const int64_t r0 = (int64_t)blockIdx.x * a.set.rows_per_chunk;
    const int64_t r1 = min(a.set.n_rows, r0 + a.set.rows_per_chunk);
    const uint32_t L = (uint32_t)a.n_labels;
    if constexpr (!GLOBAL)
        for (uint32_t i = tid; i < (uint32_t)nq * L; i += kFacetThreads) facet_hist[i] = 0u;
    if (tid < QT) {
        s_tot[tid] = 0u;
        s_oth[tid] = 0u;
    }
    __syncthreads();
    uint32_t tot[QT], oth[QT];                                   // wave-uniform: a chunk holds fewer than 2^32 rows
#pragma unroll
    for (int q = 0; q < QT; ++q) tot[q] = oth[q] = 0u;
    walk_tile<QT, kFacetWaves>(a.set, q0, nq, r0, r1, w, lane, [&](int64_t row0, uint64_t many, const Span* sp, int s, int sh, uint64_t live) {
        int32_t label = -1;
        if ((many >> lane) & 1ull) label = a.labels[row0 + lane];                    // once for the tile
        const bool in_range = (uint32_t)label < L;                                   // -1 and anything too large: `other`
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            if (q >= nq) continue;
            const uint64_t m = window64(sp[q], s, sh) & live;
            if (m == 0ull) continue;
            const bool ok = ((m >> lane) & 1ull) && in_range;
            const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
            tot[q] += (uint32_t)__popcll(m);
            oth[q] += (uint32_t)(__popcll(m) - __popcll(okm));
            if (okm == 0ull) continue;
            const int first = __builtin_ctzll(okm);
            const int32_t l0 = __builtin_amdgcn_readlane(label, first);
            const bool one = __builtin_amdgcn_ballot_w64(ok && label == l0) == okm;     // every row of the step on one label: add once
            if constexpr (GLOBAL) {
                unsigned long long* dst = a.counts + (size_t)(q0 + q) * (size_t)a.ld_counts;
                if (one) {
                    if (lane == first) atomicAdd(dst + l0, (unsigned long long)__popcll(okm));
                } else if (ok) {
                    atomicAdd(dst + label, 1ull);
                }
            } else {
                uint32_t* dst = facet_hist + (size_t)q * L;
                if (one) {
                    if (lane == first) atomicAdd(dst + l0, (uint32_t)__popcll(okm));
                } else if (ok) {
                    atomicAdd(dst + label, 1u);
                }
            }
        }
    });
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            if (tot[q]) atomicAdd(&s_tot[q], tot[q]);
            if (oth[q]) atomicAdd(&s_oth[q], oth[q]);
        }
    }
    __syncthreads();
    if constexpr (!GLOBAL) {
        for (int q = 0; q < nq; ++q) {
            unsigned long long* dst = a.counts + (size_t)(q0 + q) * (size_t)a.ld_counts;
            for (uint32_t i = tid; i < L; i += kFacetThreads) {
                const uint32_t v = facet_hist[(size_t)q * L + i];
                if (v) atomicAdd(dst + i, (unsigned long long)v);
            }
        }
    }
    if (tid < nq) {
        if (s_tot[tid]) atomicAdd(&a.total[q0 + tid], (unsigned long long)s_tot[tid]);
        if (s_oth[tid]) atomicAdd(&a.other[q0 + tid], (unsigned long long)s_oth[tid]);
    }
}

struct FacetPlan {
    int32_t regime = 0, qt = 1;       // regime: 0 = LDS histograms, 1 = global atomics
    int64_t chunks = 1, rows_per_chunk = 64;
};

// the plan rule: pure host arithmetic
int facet_plan(int64_t n_rows, int32_t B, int32_t n_labels, bool per_query, int64_t rows_per_chunk, FacetPlan* out) {
    char msg[256];
    VS_TRY(plan_or_fail(check_n_rows(n_rows, msg, sizeof msg), msg));
    if (B < 1) return fail(VS_EINVAL, "B must be positive");
    if (n_labels < 1) return fail(VS_EINVAL, "n_labels must be at least 1 (got %d)", n_labels);
    VS_TRY(plan_or_fail(check_chunking(per_query, B, rows_per_chunk, "bitmap", msg, sizeof msg), msg));
    FacetPlan p;
    p.regime = n_labels > VS_FACET_LDS_BINS ? 1 : 0;
    p.qt = 1;
    if (per_query) {
        p.qt = 8;                                                 // (global regime: the tile only shares the label loads)
        if (!p.regime)
            while (p.qt > 1 && (int64_t)p.qt * n_labels > VS_FACET_LDS_BINS) p.qt >>= 1;
    }
    // enough workgroups to fill the chip, chunks long enough that zeroing and flushing a histogram stays a sixteenth of the bit tests
    if (rows_per_chunk == 0)
        rows_per_chunk = auto_chunk(n_rows, ceil_div64(B, p.qt), p.regime ? kMinChunk : std::max<int64_t>(kMinChunk, (int64_t)16 * n_labels));
    p.rows_per_chunk = rows_per_chunk;
    p.chunks = ceil_div64(n_rows, rows_per_chunk);
    *out = p;
    return VS_OK;
}

template <int QT>
int facet_launch_qt(const FacetPlan& p, const FacetArgs& a, dim3 grid, hipStream_t s) {
    if (p.regime) {
        hipLaunchKernelGGL((facet_counts_kernel<QT, 1>), grid, dim3(kFacetThreads), 0, s, a);
    } else {
        const size_t lds = (size_t)QT * (size_t)a.n_labels * 4;
        VS_HIP(hipFuncSetAttribute((const void*)facet_counts_kernel<QT, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((facet_counts_kernel<QT, 0>), grid, dim3(kFacetThreads), lds, s, a);
    }
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// the argument checks that need no device
int facet_check(const SetSrc& src, const int32_t* labels, int32_t n_labels, int64_t rows_per_chunk, const int64_t* counts, int64_t ld_counts,
                const int64_t* total, const int64_t* other, FacetPlan* plan) {
    if (!labels || !counts || !total || !other) return fail(VS_EINVAL, "NULL argument");
    if (src.bit0 < 0) return fail(VS_EINVAL, "bit0 must be >= 0");
    VS_TRY(facet_plan(src.n_rows, src.B, n_labels, src.per_query(), rows_per_chunk, plan));
    char msg[256];
    VS_TRY(plan_or_fail(check_ld_words(src.words != nullptr, src.bit0, src.ld_words, src.n_rows, msg, sizeof msg), msg));
    if (ld_counts < n_labels) return fail(VS_EINVAL, "ld_counts = %lld is shorter than n_labels = %d", (long long)ld_counts, n_labels);
    if (plan->chunks > 0x7FFFFFFF || ceil_div64(src.B, plan->qt) > 65535)
        return fail(VS_EINVAL, "%lld chunks x %d queries are too many for one call", (long long)plan->chunks, src.B);
    return VS_OK;
}

// vs_facet_counts and vs_index_facet_counts: one call on the set's device
int facet_counts(const SetSrc& src, const int32_t* labels, int32_t n_labels, int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts,
                 int64_t* total, int64_t* other, void* stream) {
    FacetPlan plan;
    VS_TRY(facet_check(src, labels, n_labels, rows_per_chunk, counts, ld_counts, total, other, &plan));
    VS_TRY(src.device_ok());
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"labels", labels}, {"counts", counts}, {"total", total},
                                       {"other", other}}));
    BitmapStage st;
    Staged st_l;
    CountsOut out;
    return c.run("facet_counts", Finish::kStream, [&] {
        FacetArgs a{};
        int32_t* d_l;
        VS_TRY(st.in(src, plan.rows_per_chunk, c.dev, c.s, &a.set));
        VS_TRY(st_l.in(labels, (size_t)src.n_rows, c.dev, true, c.s, &d_l));
        a.labels = d_l;
        a.n_labels = n_labels;
        VS_TRY(out.bind(c.dev, counts, ld_counts, n_labels, src.B, {total, other}, c.s));
        a.counts = out.mat;
        a.ld_counts = out.ld;
        a.total = out.vec[0];
        a.other = out.vec[1];
        ProfScope prof("facet_counts", c.s);
        const dim3 grid((unsigned)plan.chunks, (unsigned)ceil_div64(src.B, plan.qt));
        return launch_by_qt(plan.qt, [&](auto qt) { return facet_launch_qt<decltype(qt)::value>(plan, a, grid, c.s); });
    }, [&] { return out.back(c.s); });
}

// ---- top-n ---------------------------------------------------------------------------------------------------------------------------
struct TopnArgs {
    const int64_t* counts;
    int64_t ld_counts;
    int32_t n_labels, n;
    int64_t min_count;                // >= 1
    int32_t* out_labels;              // [B, n]
    int64_t* out_counts;              // [B, n]
};

__global__ __launch_bounds__(kFacetThreads) void facet_topn_kernel(TopnArgs a) {
    __shared__ uint64_t cand[kTopCap];
    __shared__ int cnt_sh;
    const int K = a.n;
    const size_t b = blockIdx.x;
    const int64_t* src = a.counts + b * (size_t)a.ld_counts;
    stream_topn<kFacetThreads>(a.n_labels, K, [&](int64_t l) -> uint64_t {
        const int64_t c = src[l];
        if (c < a.min_count) return 0ull;
        return ((uint64_t)(c < 0xFFFFFFFFll ? c : 0xFFFFFFFFll) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)l);
    }, cand, &cnt_sh);
    for (int i = threadIdx.x; i < K; i += kFacetThreads) {        // every slot is written: label -1 / count 0 behind the last
        const uint64_t key = cand[i];
        a.out_labels[b * (size_t)K + i] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
        a.out_counts[b * (size_t)K + i] = (int64_t)(key >> 32);
    }
}

}  // namespace

extern "C" int vs_facet_plan(int64_t n_rows, int32_t B, int32_t n_labels, int per_query, int64_t rows_per_chunk, int32_t* out_regime,
                             int32_t* out_qt, int64_t* out_chunks, int64_t* out_rows_per_chunk) {
    if (!out_regime || !out_qt || !out_chunks || !out_rows_per_chunk) return fail(VS_EINVAL, "NULL argument");
    FacetPlan p;
    VS_TRY(facet_plan(n_rows, B, n_labels, per_query != 0, rows_per_chunk, &p));
    *out_regime = p.regime;
    *out_qt = p.qt;
    *out_chunks = p.chunks;
    *out_rows_per_chunk = p.rows_per_chunk;
    return VS_OK;
}

extern "C" int vs_facet_counts(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const int32_t* labels,
                               int64_t n_rows, int32_t n_labels, int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts, int64_t* total,
                               int64_t* other, int device, void* stream) {
    return facet_counts(free_set(words, bit0, ld_words, and_words, B, n_rows, device), labels, n_labels, rows_per_chunk, counts, ld_counts, total,
                        other, stream);
}

extern "C" int vs_index_facet_counts(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const int32_t* labels,
                                     int32_t n_labels, int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts, int64_t* total, int64_t* other,
                                     void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return facet_counts(src, labels, n_labels, rows_per_chunk, counts, ld_counts, total, other, stream);
}

extern "C" int vs_facet_topn(const int64_t* counts, int64_t ld_counts, int32_t B, int32_t n_labels, int32_t n, int64_t min_count,
                             int32_t* out_labels, int64_t* out_counts, int device, void* stream) {
    if (!counts || !out_labels || !out_counts) return fail(VS_EINVAL, "NULL argument");
    if (B < 1) return fail(VS_EINVAL, "B must be positive");
    if (n_labels < 1) return fail(VS_EINVAL, "n_labels must be at least 1 (got %d)", n_labels);
    if (n < 1 || n > VS_FACET_MAX_TOPN) return fail(VS_EINVAL, "n must be in 1..%d (got %d)", VS_FACET_MAX_TOPN, n);
    if (ld_counts < n_labels) return fail(VS_EINVAL, "ld_counts = %lld is shorter than n_labels = %d", (long long)ld_counts, n_labels);
    VS_TRY(device_in_range(device));
    Call c;
    VS_TRY(c.open(device, stream, {{"counts", counts}, {"out_labels", out_labels}, {"out_counts", out_counts}}));
    Staged st[3];
    return c.run("facet_topn", Finish::kStream, [&] {
        TopnArgs a{};
        int64_t* d_counts;
        VS_TRY(st[0].in(counts, (size_t)(B - 1) * (size_t)ld_counts + (size_t)n_labels, c.dev, true, c.s, &d_counts));
        VS_TRY(st[1].in(out_labels, (size_t)B * n, c.dev, false, c.s, &a.out_labels));
        VS_TRY(st[2].in(out_counts, (size_t)B * n, c.dev, false, c.s, &a.out_counts));
        a.counts = d_counts;
        a.ld_counts = ld_counts;
        a.n_labels = n_labels;
        a.n = n;
        a.min_count = std::max<int64_t>(min_count, 1);
        ProfScope prof("facet_topn", c.s);
        hipLaunchKernelGGL(facet_topn_kernel, dim3((unsigned)B), dim3(kFacetThreads), 0, c.s, a);
        VS_HIP(hipGetLastError());
        return VS_OK;
    }, [&] {
        VS_TRY(st[1].back(c.s));
        return st[2].back(c.s);
    });
}
