// set_scores.hip -- the scores of a document set as a value array (vs_set_score_plan, vs_index_set_scores): the library's exact
// score -- fp32 products summed in fp64, what vs_index_search_range decides by and vs_index_explain reports -- of every live row of a set, the
// missing sentinel everywhere else.  The result is a float32 field like any other: the value kernels (values.hip, quantiles.hip,
// facet_values.hip) take it unchanged, so stats, histograms, percentiles and breakdowns of scores need no kernel of their own.  No reference
// counterpart.
//
// One wave per row is the only shape row_sum_f64 has, and a sparse set must not cost a scan of idle waves: the set rows of a 2048-row span are
// compacted through LDS into a list, and the waves deal the list out.  The sentinel is a 32-bit memset of the output on the stream ahead of the
// kernel (as range.hip zeroes its bitmap): 4 bytes a row against the kilobytes a row's packets take, and the kernel keeps plain stores for the
// set rows only.
#include "agg_call.h"
#include "csr_scan.h"
#include "set_score_check.h"
#include "set_walk.h"
#include "value_check.h"

using namespace vs;

namespace vs {
namespace {

// (scan_image_fits spelled out: it is no constant expression)
constexpr size_t image_and_keys(int32_t n_cols) { return ((((size_t)n_cols + 1) * 4 + 15) & ~(size_t)15) + (size_t)kWgCap * 8 + 16; }
static_assert(image_and_keys(kSetScoreMaxCols) <= kScanLdsMax && image_and_keys(kSetScoreMaxCols + 1) > kScanLdsMax,
              "kSetScoreMaxCols is the widest index with an LDS image");

constexpr int kSpanSteps = kSpanRows / 64;            // 64-row steps of a span
constexpr int kXcds = 8;                              // accelerator dies of an MI355X, 32 CUs and one L2 each
static_assert(kSpanSteps == 2 * kScanWaves && kSpanSteps <= 64, "a wave owns two steps of a span; a lane holds one step's count in the prefix");

// LDS behind the image: the span's list of set rows, and per step its rows' mask and its first row
constexpr size_t kSetScoreListBytes = (size_t)kSpanRows * 4 + (size_t)kSpanSteps * (8 + 4);
__host__ __device__ inline size_t set_score_lds_bytes(int32_t n_cols) { return scan_img_bytes(n_cols) + kSetScoreListBytes; }
static_assert(kSetScoreListBytes <= (size_t)kWgCap * 8 + 16, "the call fits wherever the scans' image + candidate buffer does (scan_image_fits)");

struct SetScoreArgs {
    ScanArgs scan;                    // pk_ptr, cols, vals, q [B, n_cols] (rounded to the index dtype), n_rows, n_cols, B, nchunk, rows_per_chunk
    RowSet set;                       // the caller's bitmaps; and_words: the index's live rows (or null)
    float* out;                       // [B, ld_out], preset to the sentinel
    int64_t ld_out;
};

// Work item = (query, row chunk), grid-strided.  The query's image is loaded when a workgroup's query changes (one query: once).  A span:
//   1. a wave's lane 0 writes the mask and the first row of each of its steps with a set row (walk_rows hands out steps w and w + 16);
//   2. barrier; every wave takes the prefix of the 32 popcounts (a lane a step) and scatters its own steps' rows into the list;
//   3. barrier; the waves take list entries w, w + 16, ...: row_sum_f64, lane 0 stores (float)sum;
//   4. barrier (the list and the masks are free); a wave clears the masks of its steps -- it is also the one that writes them next.
// The three barriers sit in after_span, which walk_rows calls on every wave of the workgroup or on none (its span test is on words every wave
// loaded alike).
template <int VM>
__global__ __launch_bounds__(kScanThreads) void set_scores_kernel(SetScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* img = reinterpret_cast<float*>(smem);
    uint32_t* list = reinterpret_cast<uint32_t*>(smem + scan_img_bytes(a.scan.n_cols));
    uint64_t* step_mask = reinterpret_cast<uint64_t*>(list + kSpanRows);
    uint32_t* step_row = reinterpret_cast<uint32_t*>(step_mask + kSpanSteps);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < kSpanSteps) step_mask[tid] = 0ull;
    int cur_q = -1;
    const int64_t items = (int64_t)a.scan.B * a.scan.nchunk;
    // The order of the work items: the B queries of a chunk are neighbours, and a workgroup's place in the order keeps the workgroups of one
    // XCD together (workgroups go to the XCDs round robin, blockIdx % 8, as bp_choose_chunks relies on) -- so the queries of a chunk stream the
    // same packets through ONE XCD's L2 at the same time, and all but the first hit it.
    const int grid = (int)gridDim.x;
    const int place = grid % kXcds == 0 ? (int)(blockIdx.x % kXcds) * (grid / kXcds) + (int)(blockIdx.x / kXcds) : (int)blockIdx.x;
    for (int64_t item = place; item < items; item += grid) {
        const int qi = (int)(item % a.scan.B), c = (int)(item / a.scan.B);
        const int64_t r0 = (int64_t)c * a.scan.rows_per_chunk;
        const int64_t r1 = min(a.scan.n_rows, r0 + a.scan.rows_per_chunk);
        if (qi != cur_q) {                                        // (uniform)
            __syncthreads();                                      // nobody reads the previous image any more
            load_image(a.scan, img, qi, tid);
            __syncthreads();
            cur_q = qi;
        }
        float* out = a.out + (size_t)qi * (size_t)a.ld_out;
        walk_rows<kScanWaves>(a.set, (size_t)qi, r0, r1, w, lane,
            [&](int64_t row0, uint64_t m, int64_t) {
                const int s = (int)(((row0 - r0) >> 6) & (kSpanSteps - 1));          // spans start at r0
                if (lane == 0) {
                    step_mask[s] = m;
                    step_row[s] = (uint32_t)row0;
                }
            },
            [&] {
                __syncthreads();
                const int cnt = lane < kSpanSteps ? __popcll(step_mask[lane]) : 0;
                int incl = cnt;
#pragma unroll
                for (int o = 1; o < kSpanSteps; o <<= 1) {
                    const int t = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += t;
                }
                const int total = __shfl(incl, kSpanSteps - 1, 64);                  // <= kSpanRows
                const int excl = incl - cnt;
#pragma unroll
                for (int s = w; s < kSpanSteps; s += kScanWaves) {
                    const uint64_t m = step_mask[s];
                    const int at = __shfl(excl, s, 64);
                    if ((m >> lane) & 1ull) list[at + __popcll(m & ((1ull << lane) - 1ull))] = step_row[s] + (uint32_t)lane;
                }
                __syncthreads();
                for (int i = w; i < total; i += kScanWaves) {
                    const uint32_t row = list[i];
                    const double sum = row_sum_f64<VM>(a.scan.pk_ptr, a.scan.cols, a.scan.vals, row, lane, [&](uint32_t col) { return img[col]; });
                    if (lane == 0) out[row] = (float)sum;
                }
                __syncthreads();
                if (lane == 0) {
#pragma unroll
                    for (int s = w; s < kSpanSteps; s += kScanWaves) step_mask[s] = 0ull;
                }
            });
    }
}

template <int VM>
int launch_set_scores(const SetScoreArgs& a, int grid, size_t lds, hipStream_t s) {
    VS_HIP(hipFuncSetAttribute((const void*)set_scores_kernel<VM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((set_scores_kernel<VM>), dim3(grid), dim3(kScanThreads), lds, s, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// q (fp32 | fp16, leading dim ldq) -> contiguous fp32 [B, n_cols], rounded through fp16 for an fp16 index: the search's prep
template <class T>
__global__ void set_score_prep_kernel(const T* q, int64_t ldq, int32_t B, int32_t n_cols, int round_f16, float* out) {
    const int64_t n = (int64_t)B * n_cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / n_cols, c = i % n_cols;
        float v;
        if constexpr (std::is_same<T, float>::value) v = q[b * ldq + c];
        else v = __half2float(q[b * ldq + c]);
        if (round_f16) v = __half2float(__float2half_rn(v));
        out[i] = v;
    }
}

int prep_queries(vs_index* idx, const void* q_dev, int q_dtype, int64_t ldq, int32_t B, hipStream_t s, const float** out) {
    const int round_f16 = idx->store_dtype == VS_F16;
    if (q_dtype == VS_F32 && !round_f16 && ldq == idx->n_cols) {
        *out = static_cast<const float*>(q_dev);
        return VS_OK;
    }
    VS_TRY(idx->ws_q.reserve((size_t)B * idx->n_cols * 4));
    const int64_t n = (int64_t)B * idx->n_cols;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div64(n, 256), 4096);
    if (q_dtype == VS_F32)
        hipLaunchKernelGGL((set_score_prep_kernel<float>), dim3(grid), dim3(256), 0, s, (const float*)q_dev, ldq, B, idx->n_cols, round_f16, idx->ws_q.as<float>());
    else
        hipLaunchKernelGGL((set_score_prep_kernel<__half>), dim3(grid), dim3(256), 0, s, (const __half*)q_dev, ldq, B, idx->n_cols, round_f16, idx->ws_q.as<float>());
    VS_HIP(hipGetLastError());
    *out = idx->ws_q.as<float>();
    return VS_OK;
}

// the sentinel in [b, 0 .. n_rows) of every query; columns behind the rows are not touched
int fill_missing(float* out, int64_t ld, int64_t n_rows, int32_t B, hipStream_t s) {
    if (ld == n_rows || B == 1) {
        VS_HIP(hipMemsetD32Async((hipDeviceptr_t)out, (int)kValueNanF32, (size_t)(B - 1) * (size_t)ld + (size_t)n_rows, s));
        return VS_OK;
    }
    for (int32_t b = 0; b < B; ++b) VS_HIP(hipMemsetD32Async((hipDeviceptr_t)(out + (size_t)b * (size_t)ld), (int)kValueNanF32, (size_t)n_rows, s));
    return VS_OK;
}

}  // namespace
}  // namespace vs

extern "C" int vs_set_score_plan(int64_t n_rows, int32_t B, int32_t n_cols, int per_query, int64_t rows_per_chunk, int64_t* out_chunks,
                                 int64_t* out_rows_per_chunk) {
    if (!out_chunks || !out_rows_per_chunk) return fail(VS_EINVAL, "NULL argument");
    SetScorePlan p;
    char msg[256];
    VS_TRY(plan_or_fail(set_score_plan(n_rows, B, n_cols, per_query != 0, rows_per_chunk, &p, msg, sizeof msg), msg));
    *out_chunks = p.chunks;
    *out_rows_per_chunk = p.rows_per_chunk;
    return VS_OK;
}

extern "C" int vs_index_set_scores(vs_index* idx, const void* q, int q_dtype, int64_t ldq, int32_t B, const uint32_t* words, int64_t bit0,
                                   int64_t ld_words, int64_t rows_per_chunk, float* out_scores, int64_t ld_scores, void* stream) {
    char msg[256];
    VS_TRY(plan_or_fail(set_score_check_call(q && out_scores, q_dtype == VS_F32 || q_dtype == VS_F16, B, bit0, ld_words, rows_per_chunk, msg, sizeof msg),
                        msg));
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    if (idx->kind != VS_KIND_CSR) return fail(VS_EUNSUPPORTED, "the scores of a set read the CSR packets: a dense index on the matrix cores has none");
    if (!scan_image_fits(idx->n_cols))
        return fail(VS_EUNSUPPORTED, "the scores of a set need the LDS query image: n_cols = %d is too wide (at most %d columns)", idx->n_cols, kSetScoreMaxCols);
    SetScorePlan plan;
    VS_TRY(plan_or_fail(set_score_check_shape(std::max<int64_t>(idx->n_rows, 1), idx->n_cols, ldq, words != nullptr, bit0, ld_words, B, rows_per_chunk,
                                              idx->n_rows > 0 ? ld_scores : std::max<int64_t>(ld_scores, 1), &plan, msg, sizeof msg), msg));
    const void* ptrs[3] = {q, words, out_scores};
    const char* names[3] = {"q", "words", "out_scores"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 3, idx->device, &dev));
    if (idx->n_rows == 0) return VS_OK;                             // no row: nothing to write
    VS_HIP(hipSetDevice(idx->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = idx->n_rows;
    BitmapStage st;
    Staged st_q;
    DevBuf st_out;
    SetScoreArgs a{};
    VS_TRY(st.in(index_set(*idx, words, bit0, ld_words, B), plan.rows_per_chunk, dev, s, &a.set));
    const size_t q_elems = (size_t)(B - 1) * (size_t)ldq + (size_t)idx->n_cols;
    const void* d_q = q;
    if (!dev) {
        char* d = nullptr;
        VS_TRY(st_q.in(static_cast<const char*>(q), q_elems * dtype_size(q_dtype), false, true, s, &d));
        d_q = d;
        VS_TRY(st_out.alloc((size_t)B * (size_t)n * 4));            // (host outputs: one dense block, copied out row by row of the caller's stride)
    }
    a.out = dev ? out_scores : st_out.as<float>();
    a.ld_out = dev ? ld_scores : n;
    VS_TRY(prep_queries(idx, d_q, q_dtype, ldq, B, s, &a.scan.q));
    a.scan.pk_ptr = idx->pk_ptr.as<uint32_t>();
    a.scan.cols = idx->cols.as<uint4>();
    a.scan.vals = idx->vals.p;
    a.scan.n_rows = n;
    a.scan.n_cols = idx->n_cols;
    a.scan.B = B;
    a.scan.nchunk = (int32_t)plan.chunks;
    a.scan.rows_per_chunk = plan.rows_per_chunk;
    VS_TRY(launch_rc(fill_missing(a.out, a.ld_out, n, B, s), s));
    {
        ProfScope prof("set_scores", s);
        const int grid = (int)std::min<int64_t>((int64_t)B * plan.chunks, idx->cu_count);
        const size_t lds = set_score_lds_bytes(idx->n_cols);
        const int rcode = idx->store_dtype == VS_F32 ? launch_set_scores<VM_F32>(a, grid, lds, s)
                        : idx->store_dtype == VS_F16 ? launch_set_scores<VM_F16>(a, grid, lds, s)
                                                     : launch_set_scores<VM_BIN>(a, grid, lds, s);
        VS_TRY(launch_rc(rcode, s));
    }
    return close_call("set_scores", dev, stream, s, Finish::kStream, [&] {
        VS_HIP(hipMemcpy2DAsync(out_scores, (size_t)ld_scores * 4, a.out, (size_t)n * 4, (size_t)n * 4, (size_t)B, hipMemcpyDeviceToHost, s));
        return VS_OK;
    });
}
