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
//     walks the set as term_counts_kernel does (walk_term_set: packets.h, set_walk.h) and streams the runs' packets, one a lane, two in flight.  For a cell of column c: t = c - tile0, and if (unsigned)t < the tile's
//     columns, one 64-bit LDS atomicAdd of fx(v) on bin t -- the one compare drops the padding id n_cols and the other tiles' columns and bounds
//     the bin index.  A row's columns ascend, so most packets lie wholly inside or outside the tile: a lane whose 8 ids all miss reads no value.
//     At the end of the chunk every non-zero bin is one 64-bit vector atomicAdd into sums; tile 0's workgroups add the rows to total.
// (b) The id-list variant: the same through walk_ids.
// (c) Top-n: one workgroup per query scores the columns with a positive sum by their mean weight in fp64 (one rounding to fp32) and streams
//     make_key(score, column) through stream_topn (topn_stream.h), as vs_term_topn does.
#include "agg_call.h"
#include "term_cells.h"
#include "term_sum_check.h"
#include "topn_stream.h"

#include <algorithm>

using namespace vs;

namespace {

constexpr int kSumThreads = 1024;                     // 16 waves: a workgroup with a full tile has the CU to itself
constexpr int kSumWaves = kSumThreads / 64;
constexpr int kTopnThreads = 256;
static_assert((size_t)VS_TERM_SUM_TILE_COLS * 8 + 1024 <= 160 * 1024, "a tile of 64-bit bins and the counters fit a CU's LDS");

struct SumArgs {
    TermSetArgs t;
    int32_t tiles, tile_cols;         // work item i of the grid: tile i % tiles, query (i / tiles) % B, chunk i / (tiles * B)
    unsigned long long* sums;         // [B, ld_sums], zeroed by the caller
    int64_t ld_sums;
    unsigned long long* total;        // [B], zeroed by the caller
};

// (fx, tile_hits, add_cells and sum_packets -- a wave's packets into the tile's bins -- are term_cells.h's, shared with label_terms.hip)

// IDS = 0: the set is a bitmap over the index's rows; IDS = 1: an id list
template <int SD, int IDS>
__global__ __launch_bounds__(kSumThreads) void term_sums_kernel(SumArgs a) {
    extern __shared__ uint4 term_bins4[];                        // [ceil(tile_cols / 2)]: the tile's 64-bit bins
    __shared__ uint32_t s_tot;
    unsigned long long* bins = reinterpret_cast<unsigned long long*>(term_bins4);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t tile = blockIdx.x % (uint32_t)a.tiles;        // tile and query run fastest: resident workgroups sweep the same packets
    const uint32_t rest = blockIdx.x / (uint32_t)a.tiles;
    const size_t b = rest % (uint32_t)a.t.set.B;
    const int64_t chunk = rest / (uint32_t)a.t.set.B;
    const uint32_t tile0 = tile * (uint32_t)a.tile_cols;         // < n_cols: no tile of the plan is empty
    const uint32_t lim = min((uint32_t)a.tile_cols, (uint32_t)a.t.n_cols - tile0);   // the padding id n_cols is never inside
    for (int i = tid; i < (a.tile_cols + 1) / 2; i += kSumThreads) term_bins4[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) s_tot = 0u;
    __syncthreads();
    const uint32_t tot = walk_term_set<kSumWaves, IDS>(a.t, b, chunk, w, lane, [&](uint32_t p0, uint32_t p1) {
        sum_packets<SD>(a.t, p0, p1, lane, tile0, lim, bins);
    });
    if (tile == 0u && lane == 0 && tot) atomicAdd(&s_tot, tot);   // every tile walks the same rows: one of them reports them
    __syncthreads();
    unsigned long long* dst = a.sums + b * (size_t)a.ld_sums + tile0;
    for (uint32_t i = tid; i < lim; i += kSumThreads) {
        const unsigned long long v = bins[i];
        if (v) atomicAdd(dst + i, v);
    }
    if (tid == 0 && s_tot) atomicAdd(&a.total[b], (unsigned long long)s_tot);
}

template <int SD, int IDS>
int sums_launch(const SumArgs& a, dim3 grid, hipStream_t s) {
    const size_t lds = (size_t)((a.tile_cols + 1) / 2) * 16;
    VS_HIP(hipFuncSetAttribute((const void*)term_sums_kernel<SD, IDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((term_sums_kernel<SD, IDS>), grid, dim3(kSumThreads), lds, s, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// One call on the index's device: the set is (words, bit0, ld_words) when ids == nullptr, else the id lists.
int sums_call(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, const int64_t* ids, int64_t m, int64_t ld_ids, int64_t id_offset,
              int strict, int32_t B, const TermSumPlan& plan, int64_t* sums, int64_t ld_sums, int64_t* total, void* stream) {
    return term_agg_call(idx, words, bit0, ld_words, ids, m, ld_ids, id_offset, strict, B, plan.rows_per_chunk, "sums", "term_sums", sums, ld_sums,
                         total, stream, [&](auto sd, auto is_ids, const TermSetArgs& t, const CountsOut& o) {
                             const SumArgs a{t, plan.tiles, plan.tile_cols, o.mat, o.ld, o.vec[0]};
                             return sums_launch<decltype(sd)::value, decltype(is_ids)::value>(a, dim3((unsigned)(plan.chunks * B * plan.tiles)),
                                                                                              (hipStream_t)stream);
                         });
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
    __shared__ uint64_t cand[kTopCap];
    __shared__ int cnt_sh;
    const int tid = threadIdx.x;
    const int K = a.n;
    const size_t b = blockIdx.x;
    const int64_t* src = a.sums + b * (size_t)a.ld_sums;
    const int64_t* cnt_row = a.counts ? a.counts + b * (size_t)a.ld_counts : nullptr;
    const int64_t total = a.total[b];
    stream_topn<kTopnThreads>(a.n_cols, K, [&](int64_t c) -> uint64_t {          // (a score is not negative: its key has the top bit set, never 0)
        if (total <= 0) return 0ull;
        const int64_t sum = src[c];
        if (sum > 0 && (!cnt_row || cnt_row[c] >= a.min_count)) return make_key(mean_weight(sum, total), (uint32_t)c);
        return 0ull;
    }, cand, &cnt_sh);
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
    VS_TRY(csr_index_ok(idx, "term sums"));
    TermSumPlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(term_sum_check_sums(words != nullptr, bit0, ld_words, B, std::max<int64_t>(idx->n_rows, 1), idx->n_cols, rows_per_chunk,
                                            tile_cols, sums && total, ld_sums, &plan, msg, sizeof msg), msg));
    return sums_call(idx, words, bit0, ld_words, nullptr, 0, 0, 0, 0, B, plan, sums, ld_sums, total, stream);
}

extern "C" int vs_index_term_sums_ids(vs_index* idx, const int64_t* ids, int32_t B, int64_t m, int64_t ld, int64_t id_offset, int strict,
                                      int32_t tile_cols, int64_t* sums, int64_t ld_sums, int64_t* total, void* stream) {
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    VS_TRY(csr_index_ok(idx, "term sums"));
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
    VS_TRY(device_in_range(device));
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
    return close_call("term_sum_topn", dev, stream, s, Finish::kStream, [&] {
        for (int i = 3; i < 6; ++i) VS_TRY(st[i].back(s));
        return VS_OK;
    });
}
