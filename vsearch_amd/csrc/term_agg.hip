// term_agg.hip -- term aggregations (vs_term_plan, vs_index_term_counts, vs_index_term_counts_ids, vs_term_topn): for a set of rows, how many
// of them have each vocabulary column, and which columns are over-represented in the set against a background.  No reference counterpart (the
// reference only has topk).  Nothing here touches a search kernel: the set arrives as a packed bitmap in the layout of vs_index_search_filtered
// (a match_filter result, a DocFilter) or as an id list (a hit list), the rows are the CSR packets with their uint16 column ids.
//
// (a) Counts: a workgroup of 16 waves owns a chunk of rows and one query (work item i of the 1-D grid: chunk i / B of query i % B, so the
//     workgroups resident at one time sweep the same rows for different queries and share the packets through L2 / Infinity Cache).  It
//     walks the set with walk_term_set (packets.h, set_walk.h): the packets of a run of set rows are one contiguous range, which a wave
//     streams, one 16-byte packet of 8 column ids a lane (two in flight); it reads the values only where the store has them, and adds 1 to
//     the bin of every cell whose value is not zero; the padding id n_cols is compared away.
//       LDS regime    (n_cols <= VS_TERM_LDS_COLS): one uint32 histogram of all columns in LDS (29 523 columns: 118 KB of the CU's 160 KiB),
//                     zeroed at the start and flushed at the end of the chunk -- one 64-bit vector atomicAdd per non-zero bin into counts.
//       global regime (wider): 64-bit vector atomicAdd straight into counts.
//     total: popcounts of the steps' masks, summed per wave in scalar registers, per workgroup in LDS, added to global memory once.
// (b) The id-list variant: a workgroup owns a slice of one query's list (walk_ids) and streams the surviving rows' packets through the same code.
// (c) Top-n: one workgroup per query scores every candidate column in fp64 (conversions, + - x / and one rounding to fp32: bit-reproducible)
//     and streams make_key(score, column) through stream_topn (topn_stream.h).
#include "agg_call.h"
#include "topn_stream.h"

#include <algorithm>

using namespace vs;

namespace {

constexpr int kTermThreads = 1024;                    // 16 waves: an LDS-regime workgroup has the CU to itself
constexpr int kTermWaves = kTermThreads / 64;
constexpr int kTopnThreads = 256;

struct TermArgs {
    TermSetArgs t;
    unsigned long long* counts;       // [B, ld_counts], zeroed by the caller
    int64_t ld_counts;
    unsigned long long* total;        // [B], zeroed by the caller
};

template <int GLOBAL>
__device__ __forceinline__ void add_cells(const uint4& c, uint32_t nz, uint32_t n_cols, uint32_t* hist, unsigned long long* dst) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uint32_t col = packet_col(c, t);
        if (((nz >> t) & 1u) && col < n_cols) {                   // (the padding id is n_cols: never a bin)
            if constexpr (GLOBAL) atomicAdd(dst + col, 1ull);
            else atomicAdd(hist + col, 1u);
        }
    }
}

// one wave: every cell of packets [p0, p1) that has its term adds 1 to the term's bin; a lane takes a packet, two are in flight
template <int SD, int GLOBAL>
__device__ __forceinline__ void count_packets(const TermSetArgs& a, uint32_t p0, uint32_t p1, int lane, uint32_t* hist, unsigned long long* dst) {
    for (uint64_t pb = p0; pb < p1; pb += 128) {                  // (64-bit: no wrap next to 2^32 packets)
        const uint64_t pa = pb + lane, pc = pb + 64 + lane;
        const bool oa = pa < p1, oc = pc < p1;
        uint4 ca = make_uint4(0u, 0u, 0u, 0u), cc = ca;
        uint32_t na = 0u, nc = 0u;
        if (oa) ca = a.cols[pa];
        if (oc) cc = a.cols[pc];
        if (oa) na = nonzero_cells<SD>(a.vals, pa);
        if (oc) nc = nonzero_cells<SD>(a.vals, pc);
        add_cells<GLOBAL>(ca, na, (uint32_t)a.n_cols, hist, dst);
        add_cells<GLOBAL>(cc, nc, (uint32_t)a.n_cols, hist, dst);
    }
}

// IDS = 0: the set is a bitmap over the index's rows; IDS = 1: an id list
template <int SD, int GLOBAL, int IDS>
__global__ __launch_bounds__(kTermThreads) void term_counts_kernel(TermArgs a) {
    extern __shared__ uint4 term_hist4[];                        // [ceil(n_cols / 4)] (LDS regime)
    __shared__ uint32_t s_tot;
    uint32_t* hist = reinterpret_cast<uint32_t*>(term_hist4);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t b = blockIdx.x % (uint32_t)a.t.set.B;            // the query runs fastest: resident workgroups sweep the same rows
    const int64_t chunk = blockIdx.x / (uint32_t)a.t.set.B;
    const int n_cols = a.t.n_cols;
    if constexpr (!GLOBAL)
        for (int i = tid; i < (n_cols + 3) / 4; i += kTermThreads) term_hist4[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) s_tot = 0u;
    __syncthreads();
    unsigned long long* dst = a.counts + b * (size_t)a.ld_counts;
    const uint32_t tot = walk_term_set<kTermWaves, IDS>(a.t, b, chunk, w, lane, [&](uint32_t p0, uint32_t p1) {
        count_packets<SD, GLOBAL>(a.t, p0, p1, lane, hist, dst);
    });
    if (lane == 0 && tot) atomicAdd(&s_tot, tot);
    __syncthreads();
    if constexpr (!GLOBAL) {
        for (int i = tid; i < n_cols; i += kTermThreads) {
            const uint32_t v = hist[i];
            if (v) atomicAdd(dst + i, (unsigned long long)v);
        }
    }
    if (tid == 0 && s_tot) atomicAdd(&a.total[b], (unsigned long long)s_tot);
}

template <int SD, int IDS>
int term_launch(const TermPlan& p, const TermArgs& a, dim3 grid, hipStream_t s) {
    if (p.regime) {
        hipLaunchKernelGGL((term_counts_kernel<SD, 1, IDS>), grid, dim3(kTermThreads), 0, s, a);
    } else {
        const size_t lds = (size_t)((a.t.n_cols + 3) / 4) * 16;
        VS_HIP(hipFuncSetAttribute((const void*)term_counts_kernel<SD, 0, IDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((term_counts_kernel<SD, 0, IDS>), grid, dim3(kTermThreads), lds, s, a);
    }
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// One call on the index's device: the set is (words, bit0, ld_words) when ids == nullptr, else the id lists.
int term_call(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, const int64_t* ids, int64_t m, int64_t ld_ids, int64_t id_offset,
              int strict, int32_t B, const TermPlan& plan, int64_t* counts, int64_t ld_counts, int64_t* total, void* stream) {
    return term_agg_call(idx, words, bit0, ld_words, ids, m, ld_ids, id_offset, strict, B, plan.rows_per_chunk, "counts", "term_counts", counts,
                         ld_counts, total, stream, [&](auto sd, auto is_ids, const TermSetArgs& t, const CountsOut& o) {
                             const TermArgs a{t, o.mat, o.ld, o.vec[0]};
                             return term_launch<decltype(sd)::value, decltype(is_ids)::value>(plan, a, dim3((unsigned)(plan.chunks * B)), (hipStream_t)stream);
                         });
}

// ---- top-n ---------------------------------------------------------------------------------------------------------------------------
struct TermTopnArgs {
    const int64_t* counts;            // [B, ld_counts]
    int64_t ld_counts;
    const int64_t* total;             // [B]
    const int64_t* bg;                // [n_cols]
    int64_t bg_total, min_count;      // min_count >= 1
    int32_t n_cols, n, method;
    int32_t* out_cols;                // [B, n]
    float* out_score;                 // [B, n]
    int64_t* out_fg;                  // [B, n]
    int64_t* out_bg;                  // [B, n]
};

// the score of a candidate (fg >= 1, bg >= 1, total >= 1, bg_total >= 1): conversions, + - x / in fp64 and one rounding to fp32
__device__ __forceinline__ bool term_score(int64_t fg, int64_t total, int64_t bg, int64_t bg_total, int method, float* out) {
#pragma clang fp contract(off)
    const double fgp = (double)fg / (double)total;
    const double bgp = (double)bg / (double)bg_total;
    double s;
    if (method == VS_TERM_JLH) {
        if (!(fgp > bgp)) return false;
        s = (fgp - bgp) * (fgp / bgp);
    } else {
        s = fgp / bgp;
    }
    *out = (float)s;
    return true;
}

__global__ __launch_bounds__(kTopnThreads) void term_topn_kernel(TermTopnArgs a) {
    __shared__ uint64_t cand[kTopCap];
    __shared__ int cnt_sh;
    const int tid = threadIdx.x;
    const int K = a.n;
    const size_t b = blockIdx.x;
    const int64_t* src = a.counts + b * (size_t)a.ld_counts;
    const int64_t total = a.total[b];
    const bool any = total > 0 && a.bg_total > 0;
    stream_topn<kTopnThreads>(a.n_cols, K, [&](int64_t c) -> uint64_t {          // (a score is positive: its key has the top bit set, never 0)
        if (!any) return 0ull;
        const int64_t fg = src[c], bg = a.bg[c];
        float sc;
        if (fg >= a.min_count && bg > 0 && term_score(fg, total, bg, a.bg_total, a.method, &sc)) return make_key(sc, (uint32_t)c);
        return 0ull;
    }, cand, &cnt_sh);
    for (int i = tid; i < K; i += kTopnThreads) {                 // every slot is written: -1 / -inf / 0 / 0 behind the last
        const uint64_t key = cand[i];
        const size_t o = b * (size_t)K + i;
        const uint32_t c = key_row(key);
        a.out_cols[o] = key ? (int32_t)c : -1;
        a.out_score[o] = key ? key_score(key) : -INFINITY;
        a.out_fg[o] = key ? src[c] : 0;
        a.out_bg[o] = key ? a.bg[c] : 0;
    }
}

}  // namespace

extern "C" int vs_term_plan(int64_t n_rows, int32_t B, int32_t n_cols, int per_query, int64_t rows_per_chunk, int32_t* out_regime,
                            int64_t* out_chunks, int64_t* out_rows_per_chunk) {
    if (!out_regime || !out_chunks || !out_rows_per_chunk) return fail(VS_EINVAL, "NULL argument");
    TermPlan p;
    char msg[256];
    VS_TRY(plan_or_fail(term_plan(n_rows, B, n_cols, per_query != 0, rows_per_chunk, &p, msg, sizeof msg), msg));
    *out_regime = p.regime;
    *out_chunks = p.chunks;
    *out_rows_per_chunk = p.rows_per_chunk;
    return VS_OK;
}

extern "C" int vs_index_term_counts(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, int64_t rows_per_chunk,
                                    int64_t* counts, int64_t ld_counts, int64_t* total, void* stream) {
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    VS_TRY(csr_index_ok(idx, "term counts"));
    TermPlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(term_check_counts(words != nullptr, bit0, ld_words, B, std::max<int64_t>(idx->n_rows, 1), idx->n_cols, rows_per_chunk,
                                          counts && total, ld_counts, &plan, msg, sizeof msg), msg));
    return term_call(idx, words, bit0, ld_words, nullptr, 0, 0, 0, 0, B, plan, counts, ld_counts, total, stream);
}

extern "C" int vs_index_term_counts_ids(vs_index* idx, const int64_t* ids, int32_t B, int64_t m, int64_t ld, int64_t id_offset, int strict,
                                        int64_t* counts, int64_t ld_counts, int64_t* total, void* stream) {
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    VS_TRY(csr_index_ok(idx, "term counts"));
    TermPlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(term_check_ids(ids != nullptr, B, m, ld, idx->n_cols, counts && total, ld_counts, &plan, msg, sizeof msg), msg));
    return term_call(idx, nullptr, 0, 0, ids, m, ld, id_offset, strict, B, plan, counts, ld_counts, total, stream);
}

extern "C" int vs_term_topn(const int64_t* counts, int64_t ld_counts, const int64_t* total, int32_t B, int32_t n_cols, const int64_t* bg,
                            int64_t bg_total, int method, int32_t n, int64_t min_count, int32_t* out_cols, float* out_score, int64_t* out_fg,
                            int64_t* out_bg, int device, void* stream) {
    char msg[256];
    VS_TRY(plan_or_fail(term_check_topn(counts && total && bg && out_cols && out_score && out_fg && out_bg, B, n_cols, ld_counts, n, method, msg,
                                        sizeof msg), msg));
    VS_TRY(device_in_range(device));
    const void* ptrs[7] = {counts, total, bg, out_cols, out_score, out_fg, out_bg};
    const char* names[7] = {"counts", "total", "bg", "out_cols", "out_score", "out_fg", "out_bg"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 7, device, &dev));
    VS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    Staged st[7];
    TermTopnArgs a{};
    int64_t *d_counts, *d_total, *d_bg;
    VS_TRY(st[0].in(counts, (size_t)(B - 1) * (size_t)ld_counts + (size_t)n_cols, dev, true, s, &d_counts));
    VS_TRY(st[1].in(total, (size_t)B, dev, true, s, &d_total));
    VS_TRY(st[2].in(bg, (size_t)n_cols, dev, true, s, &d_bg));
    VS_TRY(st[3].in(out_cols, (size_t)B * n, dev, false, s, &a.out_cols));
    VS_TRY(st[4].in(out_score, (size_t)B * n, dev, false, s, &a.out_score));
    VS_TRY(st[5].in(out_fg, (size_t)B * n, dev, false, s, &a.out_fg));
    VS_TRY(st[6].in(out_bg, (size_t)B * n, dev, false, s, &a.out_bg));
    a.counts = d_counts;
    a.ld_counts = ld_counts;
    a.total = d_total;
    a.bg = d_bg;
    a.bg_total = bg_total;
    a.min_count = std::max<int64_t>(min_count, 1);
    a.n_cols = n_cols;
    a.n = n;
    a.method = method;
    {
        ProfScope prof("term_topn", s);
        hipLaunchKernelGGL(term_topn_kernel, dim3((unsigned)B), dim3(kTopnThreads), 0, s, a);
        VS_HIP(hipGetLastError());
    }
    return close_call("term_topn", dev, stream, s, Finish::kStream, [&] {
        for (int i = 3; i < 7; ++i) VS_TRY(st[i].back(s));
        return VS_OK;
    });
}
