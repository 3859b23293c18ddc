// range.hip -- range search (vs_index_search_range): every live, allowed row scoring at least a per-query threshold -- counted, set in a
// match bitmap, and its best max_hits listed in the canonical order.  No reference counterpart (the reference only has topk, index.py:92).
//
// A threshold needs ONE numerics for every row, so only the exact scans take part: fp32 products summed in fp64 (row_sum_f64 /
// csr_scan_topk_mq), never the fmaf chains of the dense-image top-k scan nor the fixed-point postings walks (their filter proves a
// top-k, not a threshold).  The threshold enters the scans as a FLOOR KEY (range_floor_key, csr_scan.h): the mirror image of the
// exclusive `upper` key of the "search after" passes.  Every row at or above the floor that the filter allows is counted and its bit
// set BEFORE the usual `key > tau` admission, so the prune cycles (K = max_hits) lose no count.
//   CSR packets:   the 8-queries-a-pass tile scan (RG = 1 instantiation of csr_scan_topk_mq) when the batch qualifies for tiles and
//                  max_hits <= kMaxKMq, else range_scan_kernel: one query per pass, one wave per row.  Identical bits either way.
//   matrix cores:  vs_dense_scores into scratch, then range_select_dense_kernel over the [Bt, N] tile (the dense search's own fp32 score).
//
// Boosted search (vs_index_search_boosted) is the same call with boost_apply(S, weights, the row's values) (boost_check.h) in the place of
// fl32(S): the BO = 1 instantiations of the three kernels, one or a few 32-bit loads a row at the point where the fp64 sum is still whole.
// Floor, count, bitmap, candidate buffers, prune cycles, merge, tombstones, filter and routing are the range search's own.
#include "csr_internal.h"

#include <limits>
#include <vector>

using namespace vs;

int vs_dense_scores(vs_index*, const void*, int, int64_t, int32_t, float*, hipStream_t);

namespace vs {
namespace {

static_assert(VS_RANGE_MAX_HITS == kMaxKShared, "max_hits is bounded by the shared candidate buffer's K");

// ---- one query per pass ---------------------------------------------------------------------------------------------------------
struct RangeArgs : ScanArgs {
    const float* thr;                 // [B]
    unsigned long long* count;        // [B], zeroed by the caller
    uint32_t* words;                  // optional [B, ld_words], zeroed by the caller
    int64_t ld_words;
};

// Boosted search: the BO = 1 instantiations take the boost arguments behind their range arguments (WithBoost, csr_scan_mq.h), the BO = 0 ones
// the structs they took.  The score of a row becomes boost_apply(sum, ...) (boost_check.h) at the point where the fp64 sum is still whole.
template <class A, int BO>
using BArg = typename std::conditional<BO != 0, WithBoost<A>, A>::type;
template <int BO, class A>
inline BArg<A, BO> with_boost(const A& a, const BoostArgs& b) {
    if constexpr (BO != 0) return WithBoost<A>{a, b};
    else return a;
}
// the F values of a row (a missing field's slot stays 0: boost_apply reads none past F)
__device__ __forceinline__ void boost_load(const BoostArgs& b, int64_t row, uint32_t* raw) {
#pragma unroll
    for (int j = 0; j < VS_BOOST_MAX_FIELDS; ++j) raw[j] = j < b.F ? b.field[j][row] : 0u;
}

// Sibling of exact_scan_topk_kernel (csr_scan.h): the LDS query image, one wave per row, row_sum_f64, the shared 4096-key buffer pruned
// to K = a.k.  Work item = (query, row chunk).  K = 0: count / bitmap only, no candidate is kept and no barrier taken inside the scan.
template <int VM, int FL, int BO = 0>
__global__ __launch_bounds__(kScanThreads) void range_scan_kernel(KArg<BArg<RangeArgs, BO>, FL> a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* img = reinterpret_cast<float*>(smem);
    uint64_t* cand = reinterpret_cast<uint64_t*>(smem + scan_img_bytes(a.n_cols));
    int* cnt_sh = reinterpret_cast<int*>(cand + kWgCap);
    unsigned int* mcnt_sh = reinterpret_cast<unsigned int*>(cnt_sh + 1);      // matches of the work item
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int SB = (kWgCap - kMaxKShared) / kScanWaves;      // iterations between prune checks
    const int K = a.k;
    const int64_t items = (int64_t)a.B * a.nchunk;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int qi = (int)(item / a.nchunk), c = (int)(item % a.nchunk);
        const int64_t r0 = (int64_t)c * a.rows_per_chunk;
        const int64_t r1 = min(a.n_rows, r0 + a.rows_per_chunk);
        __syncthreads();
        load_image(a, img, qi, tid);
        if (tid == 0) { *cnt_sh = 0; *mcnt_sh = 0u; }
        __syncthreads();
        const uint64_t floor = range_floor_key(a.thr[qi]);
        float bw[VS_BOOST_MAX_FIELDS] = {0.f, 0.f, 0.f, 0.f};       // the query's weights, for the work item
        if constexpr (BO != 0) {
#pragma unroll
            for (int j = 0; j < VS_BOOST_MAX_FIELDS; ++j)
                if (j < a.boost.F) bw[j] = a.boost.w[(size_t)qi * (size_t)a.boost.F + j];
        }
        uint64_t tau = 0;
        const int64_t iters = r1 > r0 ? (r1 - r0 + kScanWaves - 1) / kScanWaves : 0;
        for (int64_t it0 = 0; it0 < iters; it0 += SB) {
            const int64_t it1 = min(iters, it0 + SB);
            for (int64_t it = it0; it < it1; ++it) {
                const int64_t row = r0 + it * kScanWaves + w;
                bool live = row < r1 && floor != kRangeNoMatch;
                if constexpr (FL != 0) live = live && filter_ok(a, qi, row);      // (one wave a row: a disallowed row is not summed)
                if (live) {
                    // boosted: lane 0 will hold the sum, so it loads the row's values -- ahead of the packets, their latency passes under the sum
                    uint32_t raw[VS_BOOST_MAX_FIELDS] = {0u, 0u, 0u, 0u};
                    if constexpr (BO != 0) { if (lane == 0) boost_load(a.boost, row, raw); }
                    const double sum = row_sum_f64<VM>(a.pk_ptr, a.cols, a.vals, (uint32_t)row, lane, [&](uint32_t col) { return img[col]; });
                    uint64_t key = 0ull;
                    bool ok = true;
                    if constexpr (BO != 0) {
                        ok = false;
                        if (lane == 0) {
                            float x;
                            ok = boost_apply(sum, bw, raw, a.boost.dtype, a.boost.F, a.boost.mode, &x);
                            if (ok) key = make_key(x, (uint32_t)row);
                        }
                    } else {
                        key = make_key((float)sum, (uint32_t)row);
                    }
                    if (lane == 0 && ok && key >= floor) {
                        atomicAdd(mcnt_sh, 1u);
                        if (a.words) atomicOr(&a.words[(size_t)qi * (size_t)a.ld_words + (size_t)(row >> 5)], 1u << (row & 31));
                        if (K > 0 && key > tau) cand[atomicAdd(cnt_sh, 1)] = key;
                    }
                }
            }
            if (K > 0) {                                        // uniform
                __syncthreads();
                const int cnt = *cnt_sh;
                const bool last = it1 >= iters;
                if (last || cnt > kMaxKShared) {                // uniform: cnt read after the barrier
                    for (int i = cnt + tid; i < kWgCap; i += kScanThreads) cand[i] = 0ull;
                    wg_sort_desc<kScanThreads>(cand, kWgCap, tid);
                    if (!last && cnt > K) {
                        tau = cand[K - 1];
                        __syncthreads();
                        if (tid == 0) *cnt_sh = K;
                    }
                }
                __syncthreads();
            }
        }
        if (K > 0) {
            if (iters == 0) {                                   // empty chunk: emit sentinels
                for (int i = tid; i < kWgCap; i += kScanThreads) cand[i] = 0ull;
                __syncthreads();
            }
            uint64_t* out = a.cand + ((size_t)qi * a.nchunk + c) * (size_t)K;
            for (int i = tid; i < K; i += kScanThreads) out[i] = cand[i];
        }
        __syncthreads();                                        // every wave's matches are in
        if (tid == 0 && *mcnt_sh) atomicAdd(&a.count[qi], (unsigned long long)*mcnt_sh);
    }
}

template <int VM, int BO>
int launch_range_scan_bo(const RangeArgs& a, const BoostArgs& bo, const FilterArgs& f, int grid, size_t lds, hipStream_t s) {
    if (f.words) {
        VS_HIP(hipFuncSetAttribute((const void*)range_scan_kernel<VM, 1, BO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((range_scan_kernel<VM, 1, BO>), dim3(grid), dim3(kScanThreads), lds, s, with_filter<1>(with_boost<BO>(a, bo), f));
    } else {
        VS_HIP(hipFuncSetAttribute((const void*)range_scan_kernel<VM, 0, BO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((range_scan_kernel<VM, 0, BO>), dim3(grid), dim3(kScanThreads), lds, s, with_boost<BO>(a, bo));
    }
    VS_HIP(hipGetLastError());
    return VS_OK;
}
// bo: the boost of the launch's queries, or null (the plain range search)
template <int VM>
int launch_range_scan_vm(const RangeArgs& a, const BoostArgs* bo, const FilterArgs& f, int grid, size_t lds, hipStream_t s) {
    return bo ? launch_range_scan_bo<VM, 1>(a, *bo, f, grid, lds, s) : launch_range_scan_bo<VM, 0>(a, BoostArgs{}, f, grid, lds, s);
}

// ---- 8 queries per pass: the RG = 1 instantiations of csr_scan_topk_mq (plain variant, DN = 0) -----------------------------------------
template <int G, int VM, int U, int BO>
int launch_range_mq_bo(const MqRangeArgs& a, const BoostArgs& bo, const FilterArgs& f, int grid, size_t lds, hipStream_t s) {
    if (f.words) {
        VS_HIP(hipFuncSetAttribute((const void*)csr_scan_topk_mq<G, VM, kQT, U, 0, 1, 1, BO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((csr_scan_topk_mq<G, VM, kQT, U, 0, 1, 1, BO>), dim3(grid), dim3(kScanThreads), lds, s, with_filter<1>(with_boost<BO>(a, bo), f));
    } else {
        VS_HIP(hipFuncSetAttribute((const void*)csr_scan_topk_mq<G, VM, kQT, U, 0, 0, 1, BO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((csr_scan_topk_mq<G, VM, kQT, U, 0, 0, 1, BO>), dim3(grid), dim3(kScanThreads), lds, s, with_boost<BO>(a, bo));
    }
    VS_HIP(hipGetLastError());
    return VS_OK;
}
template <int G, int VM, int U>
int launch_range_mq_gu(const MqRangeArgs& a, const BoostArgs* bo, const FilterArgs& f, int grid, size_t lds, hipStream_t s) {
    return bo ? launch_range_mq_bo<G, VM, U, 1>(a, *bo, f, grid, lds, s) : launch_range_mq_bo<G, VM, U, 0>(a, BoostArgs{}, f, grid, lds, s);
}
template <int G, int VM>
int launch_range_mq_g(int u, const MqRangeArgs& a, const BoostArgs* bo, const FilterArgs& f, int grid, size_t lds, hipStream_t s) {
    if (u <= 1) return launch_range_mq_gu<G, VM, 1>(a, bo, f, grid, lds, s);
    if (u == 2) return launch_range_mq_gu<G, VM, 2>(a, bo, f, grid, lds, s);
    return launch_range_mq_gu<G, VM, 3>(a, bo, f, grid, lds, s);
}
template <int VM>
int launch_range_mq_vm(int g, int u, const MqRangeArgs& a, const BoostArgs* bo, const FilterArgs& f, int grid, size_t lds, hipStream_t s) {
    switch (g) {
        case 8: return launch_range_mq_g<8, VM>(u, a, bo, f, grid, lds, s);
        case 16: return launch_range_mq_g<16, VM>(u, a, bo, f, grid, lds, s);
        case 32: return launch_range_mq_g<32, VM>(u, a, bo, f, grid, lds, s);
        default: return launch_range_mq_g<64, VM>(u, a, bo, f, grid, lds, s);
    }
}

// ---- matrix-core index: select over a [B, N] tile of its fp32 scores ------------------------------------------------------------------
struct RangeSelArgs {
    const float* scores;              // [B, N]
    int64_t N;
    int32_t B;
    int32_t k;
    const float* thr;                 // [B]
    unsigned long long* count;        // [B]
    uint32_t* words;                  // optional [B, ld_words]
    int64_t ld_words;
    uint64_t* cand;                   // [B, k] keys, sorted descending
};

// One workgroup per query, a thread per row and step: a wave's 64 rows are two whole bitmap words (ballot), so the bitmap takes plain
// stores here.  Candidates as in csr_scan_topk_shared: the 4096-key LDS buffer, pruned to K when more than 2048 are in.
template <int FL, int BO = 0>
__global__ __launch_bounds__(kScanThreads) void range_select_dense_kernel(KArg<BArg<RangeSelArgs, BO>, FL> a) {
    __shared__ uint64_t cand[kWgCap];
    __shared__ int cnt_sh;
    __shared__ unsigned int mcnt_sh;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int SB = (kWgCap - kMaxKShared) / kScanThreads;    // steps between prune checks
    static_assert(SB >= 1, "a step adds up to kScanThreads candidates");
    const int K = a.k;
    const int64_t n_words = (a.N + 31) >> 5;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        __syncthreads();
        if (tid == 0) { cnt_sh = 0; mcnt_sh = 0u; }
        __syncthreads();
        const uint64_t floor = range_floor_key(a.thr[b]);
        float bw[VS_BOOST_MAX_FIELDS] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BO != 0) {
#pragma unroll
            for (int j = 0; j < VS_BOOST_MAX_FIELDS; ++j)
                if (j < a.boost.F) bw[j] = a.boost.w[(size_t)b * (size_t)a.boost.F + j];
        }
        const float* src = a.scores + (size_t)b * (size_t)a.N;
        uint64_t tau = 0;
        unsigned int mine = 0;
        const int64_t iters = (a.N + kScanThreads - 1) / kScanThreads;
        for (int64_t it0 = 0; it0 < iters; it0 += SB) {
            const int64_t it1 = min(iters, it0 + SB);
            for (int64_t it = it0; it < it1; ++it) {
                const int64_t n = it * kScanThreads + tid;
                bool match = n < a.N && floor != kRangeNoMatch;
                uint64_t key = 0ull;
                if constexpr (BO != 0) {
                    // the filter first: a disallowed row loads no value.  S = fp64(the dense search's fp32 score)
                    if constexpr (FL != 0) { if (match) match = filter_ok(a, b, n); }
                    if (match) {
                        uint32_t raw[VS_BOOST_MAX_FIELDS];
                        boost_load(a.boost, n, raw);
                        float x;
                        match = boost_apply((double)src[n], bw, raw, a.boost.dtype, a.boost.F, a.boost.mode, &x);
                        if (match) {
                            key = make_key(x, (uint32_t)n);
                            match = key >= floor;
                        }
                    }
                } else {
                    if (match) {
                        key = make_key(canon_zero(src[n]), (uint32_t)n);
                        match = key >= floor;
                    }
                    if constexpr (FL != 0) { if (match) match = filter_ok(a, b, n); }
                }
                const unsigned long long mm = __builtin_amdgcn_ballot_w64(match);
                if (a.words && lane < 2) {
                    const int64_t wi = ((it * kScanThreads + (int64_t)w * 64) >> 5) + lane;
                    if (wi < n_words) a.words[(size_t)b * (size_t)a.ld_words + (size_t)wi] = (uint32_t)(mm >> (32 * lane));
                }
                if (lane == 0) mine += (unsigned int)__popcll(mm);
                const bool pass = match && K > 0 && key > tau;
                const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
                if (m) {
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&cnt_sh, __popcll(m));
                    base = __shfl(base, 0, 64);
                    if (pass) cand[base + __popcll(m & ((1ull << lane) - 1ull))] = key;
                }
            }
            if (K > 0) {                                        // uniform
                __syncthreads();
                const int cnt = cnt_sh;
                const bool last = it1 >= iters;
                if (last || cnt > kMaxKShared) {
                    for (int i = cnt + tid; i < kWgCap; i += kScanThreads) cand[i] = 0ull;
                    wg_sort_desc<kScanThreads>(cand, kWgCap, tid);
                    if (!last && cnt > K) {
                        tau = cand[K - 1];
                        __syncthreads();
                        if (tid == 0) cnt_sh = K;
                    }
                }
                __syncthreads();
            }
        }
        if (lane == 0 && mine) atomicAdd(&mcnt_sh, mine);
        if (K > 0) {
            if (iters == 0) {
                for (int i = tid; i < kWgCap; i += kScanThreads) cand[i] = 0ull;
                __syncthreads();
            }
            uint64_t* out = a.cand + (size_t)b * (size_t)K;
            for (int i = tid; i < K; i += kScanThreads) out[i] = cand[i];
        }
        __syncthreads();
        if (tid == 0) a.count[b] = (unsigned long long)mcnt_sh;
    }
}

// q (fp32 | fp16, leading dim ldq) -> contiguous fp32 [B, n_cols], rounded through fp16 for an fp16 index (what the search kernels read)
template <class T>
__global__ void range_prep_kernel(const T* q, int64_t ldq, int32_t B, int32_t n_cols, int round_f16, float* out) {
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

// what one call carries through its sub-batches (device pointers)
struct RangeCall {
    const float* thr;
    int32_t K;
    int64_t id_offset;
    int64_t* ids;                     // [B, K] (K > 0)
    float* scores;
    unsigned long long* count;        // [B]
    uint32_t* words;                  // [B, ld_words] or null
    int64_t ld_words;
    const BoostArgs* boost;           // null: the plain range search; else the boost, w at the call's first query
};

// the boost of queries [b0, ...) of the call
inline BoostArgs boost_from(const BoostArgs& b, int64_t b0) {
    BoostArgs r = b;
    r.w += (size_t)b0 * (size_t)b.F;
    return r;
}

int range_merge(vs_index* idx, const uint64_t* cand, int64_t n_cand, int b0, int bs, const RangeCall& rc, hipStream_t s) {
    if (rc.K == 0) return VS_OK;
    MergeArgs m{};
    m.cand = cand;
    m.n_cand = n_cand;
    m.B = bs;
    m.k = rc.K;
    m.id_offset = rc.id_offset;
    m.out_ids = rc.ids + (size_t)b0 * rc.K;
    m.out_scores = rc.scores + (size_t)b0 * rc.K;
    m.out_ld = rc.K;
    m.col0 = 0;
    m.run_len = rc.K;                                  // every chunk's list is sorted
    ProfScope prof("merge_topk", s);
    // (PAD = 1: fewer matches than max_hits come out as id -1, score -inf)
    hipLaunchKernelGGL(merge_topk_kernel<1>, dim3(std::min(bs, idx->cu_count * 2)), dim3(kScanThreads), 0, s, m);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// Queries [b0, b0 + bs) on the tile scan.  *done = false (and nothing launched that writes an output) when the batch does not qualify
// for tiles: the test mq_search makes -- a query denser than the LDS weight capacity.
int range_tiles(vs_index* idx, const float* dq, int b0, int bs, const RangeCall& rc, const FilterArgs& filt, int plan_nchunk, hipStream_t s, bool* done) {
    *done = false;
    const int vals_cap = mq_vals_cap(idx);
    if (vals_cap <= 0 || rc.K > kMaxKMq) return VS_OK;
    const int B = bs, K = rc.K;
    // 1. the batch's sparse form and tile plan: mq_search's own (mq_sparsify), so "qualifies for tiles" is one test in one place
    MqBatch mb{};
    bool fits = false;
    VS_TRY(mq_sparsify(idx, dq, B, kQT, vals_cap, false, s, &mb, &fits));
    if (!fits) return VS_OK;                                     // some query is too dense for the tile tables
    // 2. scan.  Work items = (tile, row chunk)
    const int n_tiles = mb.n_tiles;
    const int nchunk = choose_chunks(idx, n_tiles, plan_nchunk);
    const int64_t items = (int64_t)n_tiles * nchunk;
    const int grid = (int)std::min<int64_t>(items, idx->cu_count);
    VS_TRY(idx->ws_mq_cand.reserve((size_t)grid * kQT * kMqCap * 8));
    VS_TRY(idx->ws_cand.reserve(std::max<size_t>((size_t)B * nchunk * K * 8, 16)));
    MqRangeArgs a{};
    mq_fill_args(idx, mb, K, nchunk, vals_cap, &a);
    a.thr = rc.thr + b0;
    a.count = rc.count + b0;
    a.words = rc.words ? rc.words + (size_t)b0 * (size_t)rc.ld_words : nullptr;
    a.ld_words = rc.ld_words;
    idx->last_scan_bytes += (int64_t)n_tiles * csr_bytes_per_pass(idx);
    idx->last_chunks = nchunk;
    {
        ProfScope prof("range_scan", s);
        const int u = mq_packets_per_trip(idx);
        const size_t lds = mq_lds_bytes(idx, vals_cap);
        const FilterArgs f = filter_from(filt, b0);
        const BoostArgs bo_sub = rc.boost ? boost_from(*rc.boost, b0) : BoostArgs{};
        const BoostArgs* bo = rc.boost ? &bo_sub : nullptr;
        const int rcode = idx->store_dtype == VS_F32 ? launch_range_mq_vm<VM_F32>(mq_lanes(idx), u, a, bo, f, grid, lds, s)
                        : idx->store_dtype == VS_F16 ? launch_range_mq_vm<VM_F16>(mq_lanes(idx), u, a, bo, f, grid, lds, s)
                                                     : launch_range_mq_vm<VM_BIN>(mq_lanes(idx), u, a, bo, f, grid, lds, s);
        VS_TRY(rcode);
    }
    VS_STAGE("range tile scan", s);
    VS_TRY(range_merge(idx, a.cand, (int64_t)nchunk * K, b0, bs, rc, s));
    *done = true;
    return VS_OK;
}

// Queries [b0, b0 + bs) on the one-query scan
int range_one(vs_index* idx, const float* dq, int b0, int bs, const RangeCall& rc, const FilterArgs& filt, int plan_nchunk, hipStream_t s) {
    const int K = rc.K;
    const int nchunk = choose_chunks(idx, bs, plan_nchunk);
    VS_TRY(idx->ws_cand.reserve(std::max<size_t>((size_t)bs * nchunk * K * 8, 16)));
    RangeArgs a{};
    a.pk_ptr = idx->pk_ptr.as<uint32_t>();
    a.cols = idx->cols.as<uint4>();
    a.vals = idx->vals.p;
    a.q = dq;
    a.n_rows = idx->n_rows;
    a.n_cols = idx->n_cols;
    a.B = bs;
    a.k = K;
    a.nchunk = nchunk;
    a.rows_per_chunk = ceil_div64(idx->n_rows, nchunk);
    a.cand = idx->ws_cand.as<uint64_t>();
    a.thr = rc.thr + b0;
    a.count = rc.count + b0;
    a.words = rc.words ? rc.words + (size_t)b0 * (size_t)rc.ld_words : nullptr;
    a.ld_words = rc.ld_words;
    const int grid = (int)std::min<int64_t>((int64_t)bs * nchunk, idx->cu_count);
    const size_t lds = scan_lds_bytes(idx->n_cols);
    idx->last_scan_bytes += (int64_t)bs * csr_bytes_per_pass(idx);
    idx->last_chunks = nchunk;
    {
        ProfScope prof("range_scan", s);
        const FilterArgs f = filter_from(filt, b0);
        const BoostArgs bo_sub = rc.boost ? boost_from(*rc.boost, b0) : BoostArgs{};
        const BoostArgs* bo = rc.boost ? &bo_sub : nullptr;
        const int rcode = idx->store_dtype == VS_F32 ? launch_range_scan_vm<VM_F32>(a, bo, f, grid, lds, s)
                        : idx->store_dtype == VS_F16 ? launch_range_scan_vm<VM_F16>(a, bo, f, grid, lds, s)
                                                     : launch_range_scan_vm<VM_BIN>(a, bo, f, grid, lds, s);
        VS_TRY(rcode);
    }
    VS_STAGE("range one-query scan", s);
    return range_merge(idx, a.cand, (int64_t)nchunk * K, b0, bs, rc, s);
}

int range_csr(vs_index* idx, const void* q_dev, int q_dtype, int64_t ldq, int32_t B, const RangeCall& rc, const FilterArgs& filt, hipStream_t s) {
    // queries: contiguous fp32 rows rounded to the index dtype (the search's prep)
    const float* dq = nullptr;
    const int round_f16 = idx->store_dtype == VS_F16;
    if (q_dtype == VS_F32 && !round_f16 && ldq == idx->n_cols) {
        dq = (const float*)q_dev;
    } else {
        VS_TRY(idx->ws_q.reserve((size_t)B * idx->n_cols * 4));
        const int64_t n = (int64_t)B * idx->n_cols;
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div64(n, 256), 4096);
        if (q_dtype == VS_F32)
            hipLaunchKernelGGL((range_prep_kernel<float>), dim3(grid), dim3(256), 0, s, (const float*)q_dev, ldq, B, idx->n_cols, round_f16, idx->ws_q.as<float>());
        else
            hipLaunchKernelGGL((range_prep_kernel<__half>), dim3(grid), dim3(256), 0, s, (const __half*)q_dev, ldq, B, idx->n_cols, round_f16, idx->ws_q.as<float>());
        VS_HIP(hipGetLastError());
        dq = idx->ws_q.as<float>();
    }
    // the row chunks of a scan at most (plan_scan of the search): one per CU, 512 rows at least
    const int64_t rpc = std::max<int64_t>(512, ceil_div64(idx->n_rows, idx->cu_count));
    const int plan_nchunk = (int)std::max<int64_t>(1, ceil_div64(idx->n_rows, rpc));
    // bound the candidate scratch: sub-batches of whole tiles
    const size_t per_q = (size_t)plan_nchunk * std::max(rc.K, 1) * 8;
    int bs_max = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)512 << 20) / per_q));
    if (bs_max < B && bs_max >= kQT) bs_max -= bs_max % kQT;   // (a batch that fits runs whole: ceil(B / 8) tiles in one launch)
    idx->last_qt = kQT;
    idx->last_path = 1;
    for (int b0 = 0; b0 < B; b0 += bs_max) {
        const int bs = std::min(bs_max, B - b0);
        bool done = false;
        if (idx->qt_pref != 1) VS_TRY(range_tiles(idx, dq + (size_t)b0 * idx->n_cols, b0, bs, rc, filt, plan_nchunk, s, &done));
        if (!done) {
            VS_TRY(range_one(idx, dq + (size_t)b0 * idx->n_cols, b0, bs, rc, filt, plan_nchunk, s));
            idx->last_qt = 1;
            idx->last_path = 0;
        }
    }
    return VS_OK;
}

int range_dense(vs_index* idx, const void* q_dev, int q_dtype, int64_t ldq, int32_t B, const RangeCall& rc, const FilterArgs& filt, hipStream_t s) {
    const int64_t N = idx->n_rows;
    const int bs_max = (int)std::max<int64_t>(1, std::min<int64_t>(B, ((int64_t)1 << 30) / (N * 4)));
    VS_TRY(idx->ws_cand.reserve((size_t)bs_max * N * 4));
    VS_TRY(idx->ws_mq_cand.reserve(std::max<size_t>((size_t)bs_max * rc.K * 8, 16)));
    idx->last_qt = 1;
    idx->last_path = 0;
    idx->last_chunks = 1;
    for (int b0 = 0; b0 < B; b0 += bs_max) {
        const int bs = std::min(bs_max, B - b0);
        {
            ProfScope prof("dense_scores", s);
            VS_TRY(vs_dense_scores(idx, (const char*)q_dev + (size_t)b0 * (size_t)ldq * dtype_size(q_dtype), q_dtype, ldq, bs, idx->ws_cand.as<float>(), s));
        }
        RangeSelArgs a{};
        a.scores = idx->ws_cand.as<float>();
        a.N = N;
        a.B = bs;
        a.k = rc.K;
        a.thr = rc.thr + b0;
        a.count = rc.count + b0;
        a.words = rc.words ? rc.words + (size_t)b0 * (size_t)rc.ld_words : nullptr;
        a.ld_words = rc.ld_words;
        a.cand = idx->ws_mq_cand.as<uint64_t>();
        const int grid = std::min(bs, idx->cu_count * 2);
        {
            ProfScope prof("range_scan", s);
            const FilterArgs f = filter_from(filt, b0);
            if (rc.boost) {
                const BoostArgs bo = boost_from(*rc.boost, b0);
                if (f.words) hipLaunchKernelGGL((range_select_dense_kernel<1, 1>), dim3(grid), dim3(kScanThreads), 0, s, with_filter<1>(with_boost<1>(a, bo), f));
                else hipLaunchKernelGGL((range_select_dense_kernel<0, 1>), dim3(grid), dim3(kScanThreads), 0, s, with_boost<1>(a, bo));
            } else if (f.words) hipLaunchKernelGGL(range_select_dense_kernel<1>, dim3(grid), dim3(kScanThreads), 0, s, with_filter<1>(a, f));
            else hipLaunchKernelGGL(range_select_dense_kernel<0>, dim3(grid), dim3(kScanThreads), 0, s, a);
            VS_HIP(hipGetLastError());
        }
        VS_STAGE("range dense select", s);
        VS_TRY(range_merge(idx, a.cand, rc.K, b0, bs, rc, s));
    }
    return VS_OK;
}

// what vs_index_search_boosted adds to a range search, as the caller gave it (null: the plain range search)
struct BoostIn {
    const void* const* fields;
    const int32_t* dtypes;
    int32_t F;
    const float* weights;
    int mode;
};

// vs_index_search_range and vs_index_search_boosted: one entry, so that checks, staging, tombstones and the stream rules are one code
int range_entry(vs_index* idx, const void* q, int q_dtype, int64_t ldq, int32_t B, const float* thr, int32_t max_hits, const uint32_t* filter,
                int64_t filter_bit0, int64_t filter_ld, int64_t id_offset, int64_t* out_ids, float* out_scores, int64_t* out_count,
                uint32_t* out_words, int64_t ld_words, const BoostIn* bi, void* stream) {
    if (!idx || !q || (!thr && !bi)) return fail(VS_EINVAL, "NULL argument");
    if (bi) {
        char msg[256] = {0};
        const int rc = boost_check_fields(bi->fields, bi->dtypes, bi->F, bi->mode, bi->weights, msg, sizeof msg);
        if (rc != VS_OK) return fail(rc, "%s", msg);
    }
    if (B <= 0) return fail(VS_EINVAL, "B must be positive");
    if (q_dtype != VS_F32 && q_dtype != VS_F16) return fail(VS_EINVAL, "q_dtype must be VS_F32 or VS_F16");
    if (ldq < idx->n_cols) return fail(VS_EINVAL, "query has %lld columns, index has %d", (long long)ldq, idx->n_cols);
    if (max_hits < 0 || max_hits > VS_RANGE_MAX_HITS) return fail(VS_EINVAL, "max_hits must be in 0..%d (got %d)", VS_RANGE_MAX_HITS, max_hits);
    if (max_hits > 0 && (!out_ids || !out_scores)) return fail(VS_EINVAL, "out_ids / out_scores are NULL with max_hits = %d", max_hits);
    if (max_hits == 0 && !out_count && !out_words) return fail(VS_EINVAL, "max_hits = 0 with neither out_count nor out_words: nothing to compute");
    const int64_t n_words = (idx->n_rows + 31) >> 5;
    if (out_words && ld_words < n_words) return fail(VS_EINVAL, "ld_words = %lld is shorter than the %lld words a query's bitmap spans", (long long)ld_words, (long long)n_words);
    if (filter) {
        if (filter_bit0 < 0) return fail(VS_EINVAL, "filter_bit0 must be >= 0");
        const int64_t span = (filter_bit0 + idx->n_rows + 31) >> 5;
        if (filter_ld < 0 || (filter_ld > 0 && filter_ld < span))
            return fail(VS_EINVAL, "filter_ld = %lld words is shorter than the %lld a query's bitmap spans", (long long)filter_ld, (long long)span);
    }
    if (idx->kind == VS_KIND_CSR && !scan_image_fits(idx->n_cols))
        return fail(VS_EUNSUPPORTED, "range search needs the LDS query image: n_cols = %d is too wide (at most 32763 columns)", idx->n_cols);
    // all host, or all device on the index's device
    const bool dev = is_device_ptr(q);
    const void* ptrs[6 + 1 + VS_BOOST_MAX_FIELDS] = {thr, filter, max_hits > 0 ? out_ids : nullptr, max_hits > 0 ? out_scores : nullptr, out_count, out_words};
    if (bi) {
        ptrs[6] = bi->weights;
        for (int j = 0; j < bi->F; ++j) ptrs[7 + j] = bi->fields[j];
    }
    for (const void* p : ptrs)
        if (p && is_device_ptr(p) != dev) return fail(VS_EINVAL, "the buffers of a range search must all be host or all device pointers");
    if (dev) {
        const void* all[7 + 1 + VS_BOOST_MAX_FIELDS] = {q, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], ptrs[7], ptrs[8], ptrs[9], ptrs[10]};
        for (const void* p : all) {
            if (!p) continue;
            hipPointerAttribute_t attr;
            VS_HIP(hipPointerGetAttributes(&attr, p));
            if (attr.device != idx->device) return fail(VS_EINVAL, "a buffer lives on device %d, the index on device %d", attr.device, idx->device);
        }
    } else {
        for (int b = 0; thr && b < B; ++b)
            if (thr[b] != thr[b]) return fail(VS_EINVAL, "thr[%d] is NaN", b);
        if (bi) {
            char msg[256] = {0};
            const int rc = boost_check_weights_host(bi->weights, B, bi->F, msg, sizeof msg);
            if (rc != VS_OK) return fail(rc, "%s", msg);
        }
    }
    VS_HIP(hipSetDevice(idx->device));
    hipStream_t s = (hipStream_t)stream;
    const int K = max_hits;
    // staging of host buffers; a count the caller did not ask for still has a home (the kernels always count)
    DevBuf st_in, st_out, st_boost;
    // thr == NULL (a boosted search): a floor of -inf for every query
    const std::vector<float> no_floor(thr ? 0 : (size_t)B, -std::numeric_limits<float>::infinity());
    if (!thr) thr = no_floor.data();
    const bool thr_dev = dev && no_floor.empty();
    const void* d_q = q;
    const uint32_t* d_filter = filter;
    RangeCall rc{};
    rc.K = K;
    rc.id_offset = id_offset;
    rc.ld_words = ld_words;
    const size_t sz_ids = (size_t)B * K * 8, sz_sc = (size_t)B * K * 4, sz_cnt = (size_t)B * 8;
    const size_t sz_words = out_words ? ((size_t)(B - 1) * (size_t)ld_words + (size_t)n_words) * 4 : 0;
    if (dev) {
        if (thr_dev) rc.thr = thr;
        else {
            VS_TRY(st_in.alloc((size_t)B * 4));
            VS_HIP(hipMemcpyAsync(st_in.p, thr, (size_t)B * 4, hipMemcpyHostToDevice, s));
            rc.thr = st_in.as<float>();
        }
        rc.ids = out_ids;
        rc.scores = out_scores;
        rc.words = out_words;
        if (out_count) rc.count = reinterpret_cast<unsigned long long*>(out_count);
        else {
            VS_TRY(st_out.alloc(sz_cnt));
            rc.count = st_out.as<unsigned long long>();
        }
    } else {
        const size_t q_bytes = ((size_t)(B - 1) * ldq + idx->n_cols) * dtype_size(q_dtype);
        VS_TRY(idx->ws_misc.reserve(q_bytes));
        VS_HIP(hipMemcpyAsync(idx->ws_misc.p, q, q_bytes, hipMemcpyHostToDevice, s));
        d_q = idx->ws_misc.p;
        VS_TRY(st_in.alloc((size_t)B * 4));
        VS_HIP(hipMemcpyAsync(st_in.p, thr, (size_t)B * 4, hipMemcpyHostToDevice, s));
        rc.thr = st_in.as<float>();
        if (filter) {
            const size_t bytes = (size_t)((filter_ld > 0 ? (int64_t)(B - 1) * filter_ld : 0) + ((filter_bit0 + idx->n_rows + 31) >> 5)) * 4;
            VS_TRY(idx->ws_filt.reserve(bytes));
            VS_HIP(hipMemcpyAsync(idx->ws_filt.p, filter, bytes, hipMemcpyHostToDevice, s));
            d_filter = idx->ws_filt.as<uint32_t>();
        }
        const size_t a8 = (sz_ids + 15) & ~(size_t)15, a4 = (sz_sc + 15) & ~(size_t)15, ac = (sz_cnt + 15) & ~(size_t)15;
        VS_TRY(st_out.alloc(a8 + a4 + ac + sz_words + 16));
        char* p = st_out.as<char>();
        rc.ids = reinterpret_cast<int64_t*>(p);
        rc.scores = reinterpret_cast<float*>(p + a8);
        rc.count = reinterpret_cast<unsigned long long*>(p + a8 + a4);
        rc.words = out_words ? reinterpret_cast<uint32_t*>(p + a8 + a4 + ac) : nullptr;
    }
    // the boost: the value arrays and the weights as they are (device), or staged
    BoostArgs bo{};
    if (bi) {
        bo.F = bi->F;
        bo.mode = bi->mode;
        for (int j = 0; j < bi->F; ++j) bo.dtype[j] = bi->dtypes[j];
        if (dev) {
            bo.w = bi->weights;
            for (int j = 0; j < bi->F; ++j) bo.field[j] = static_cast<const uint32_t*>(bi->fields[j]);
        } else {
            const size_t col = (((size_t)idx->n_rows * 4) + 15) & ~(size_t)15, wb = (size_t)B * bi->F * 4;
            VS_TRY(st_boost.alloc(col * bi->F + wb));
            char* p = st_boost.as<char>();
            for (int j = 0; j < bi->F; ++j) {
                VS_HIP(hipMemcpyAsync(p + col * j, bi->fields[j], (size_t)idx->n_rows * 4, hipMemcpyHostToDevice, s));
                bo.field[j] = reinterpret_cast<const uint32_t*>(p + col * j);
            }
            VS_HIP(hipMemcpyAsync(p + col * bi->F, bi->weights, wb, hipMemcpyHostToDevice, s));
            bo.w = reinterpret_cast<const float*>(p + col * bi->F);
        }
        rc.boost = &bo;
    }
    VS_HIP(hipMemsetAsync(rc.count, 0, sz_cnt, s));
    if (rc.words) {
        // words [0, n_words) of every query's row: the scans set bits with atomicOr
        if (ld_words == n_words || B == 1) VS_HIP(hipMemsetAsync(rc.words, 0, ((size_t)(B - 1) * (size_t)ld_words + (size_t)n_words) * 4, s));
        else VS_HIP(hipMemset2DAsync(rc.words, (size_t)ld_words * 4, 0, (size_t)n_words * 4, (size_t)B, s));
    }
    // tombstones are ANDed in, as every search does
    const FilterArgs user = filter ? FilterArgs{d_filter, filter_bit0, filter_ld} : FilterArgs{};
    FilterArgs filt = user;
    if (idx->has_tomb) VS_TRY(tomb_effective_filter(idx, user, B, s, &filt));
    idx->last_scan_bytes = 0;
    idx->last_walk_postings = 0;
    idx->last_flags = nullptr;
    idx->last_flags_n = 0;
    idx->last_plan_dev = nullptr;
    const int rcode = idx->kind == VS_KIND_CSR ? range_csr(idx, d_q, q_dtype, ldq, B, rc, filt, s) : range_dense(idx, d_q, q_dtype, ldq, B, rc, filt, s);
    if (rcode != VS_OK) {
        (void)hipStreamSynchronize(s);                              // staging buffers die here
        return rcode;
    }
    if (!dev) {
        if (K > 0) {
            VS_HIP(hipMemcpyAsync(out_ids, rc.ids, sz_ids, hipMemcpyDeviceToHost, s));
            VS_HIP(hipMemcpyAsync(out_scores, rc.scores, sz_sc, hipMemcpyDeviceToHost, s));
        }
        if (out_count) VS_HIP(hipMemcpyAsync(out_count, rc.count, sz_cnt, hipMemcpyDeviceToHost, s));
        // (only the words a bitmap spans: what lies between them in the caller's rows is not touched)
        if (out_words && n_words > 0)
            VS_HIP(hipMemcpy2DAsync(out_words, (size_t)ld_words * 4, rc.words, (size_t)ld_words * 4, (size_t)n_words * 4, (size_t)B, hipMemcpyDeviceToHost, s));
    }
    // staging buffers die here: a call that used any waits for its work (device pointers + a stream: only enqueued)
    if (!stream || st_in.p || st_out.p || st_boost.p) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}

}  // namespace
}  // namespace vs

extern "C" int vs_index_search_range(vs_index* idx, const void* q, int q_dtype, int64_t ldq, int32_t B, const float* thr, int32_t max_hits,
                                     const uint32_t* filter, int64_t filter_bit0, int64_t filter_ld, int64_t id_offset, int64_t* out_ids,
                                     float* out_scores, int64_t* out_count, uint32_t* out_words, int64_t ld_words, void* stream) {
    return range_entry(idx, q, q_dtype, ldq, B, thr, max_hits, filter, filter_bit0, filter_ld, id_offset, out_ids, out_scores, out_count, out_words,
                       ld_words, nullptr, stream);
}

extern "C" int vs_index_search_boosted(vs_index* idx, const void* q, int q_dtype, int64_t ldq, int32_t B, const float* thr, int32_t max_hits,
                                       const uint32_t* filter, int64_t filter_bit0, int64_t filter_ld, int64_t id_offset, int64_t* out_ids,
                                       float* out_scores, int64_t* out_count, uint32_t* out_words, int64_t ld_words, const void* const* fields,
                                       const int32_t* field_dtypes, int32_t n_fields, const float* weights, int mode, void* stream) {
    const BoostIn bi{fields, field_dtypes, n_fields, weights, mode};
    return range_entry(idx, q, q_dtype, ldq, B, thr, max_hits, filter, filter_bit0, filter_ld, id_offset, out_ids, out_scores, out_count, out_words,
                       ld_words, &bi, stream);
}

extern "C" int vs_index_last_range_plan(const vs_index* idx, int32_t* out_chunks, int64_t* out_rows_per_chunk) {
    if (!idx || !out_chunks || !out_rows_per_chunk) return fail(VS_EINVAL, "NULL argument");
    *out_chunks = idx->last_chunks;
    *out_rows_per_chunk = idx->last_chunks > 0 ? ceil_div64(idx->n_rows, idx->last_chunks) : 0;
    return VS_OK;
}
