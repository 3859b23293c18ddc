// term_agg.hip -- term aggregations (vs_term_plan, vs_index_term_counts, vs_index_term_counts_ids, vs_term_topn): for a set of rows, how many
// of them have each vocabulary column, and which columns are over-represented in the set against a background.  No reference counterpart (the
// reference only has topk).  Nothing here touches a search kernel: the set arrives as a packed bitmap in the layout of vs_index_search_filtered
// (a match_filter result, a DocFilter) or as an id list (a hit list), the rows are the CSR packets with their uint16 column ids.
//
// (a) Counts: a workgroup of 16 waves owns a chunk of rows and one query (work item i of the 1-D grid: chunk i / B of query i % B, so the
//     workgroups resident at one time sweep the same rows for different queries and share the packets through L2 / Infinity Cache).  It
//     walks the bitmap as facets.hip does -- spans of 2048 rows (lane l holds words l and l + 1, so the 64 bits of any 64-row step come out
//     of three lane reads whatever bit0 is), an all-zero span is left at once -- and deals the span's 64-row steps to its waves; a step
//     with no bit set is skipped.  The set rows of a step fall into runs of
//     consecutive rows, and the packets of a run are one contiguous range [pk_ptr[first], pk_ptr[last + 1]): the wave streams it, one 16-byte
//     packet of 8 column ids a lane (two in flight), reads the values only where the store has them, and adds 1 to the bin of every cell whose
//     value is not zero; the padding id n_cols is compared away.
//       LDS regime    (n_cols <= VS_TERM_LDS_COLS): one uint32 histogram of all columns in LDS (29 523 columns: 118 KB of the CU's 160 KiB),
//                     zeroed at the start and flushed at the end of the chunk -- one 64-bit vector atomicAdd per non-zero bin into counts.
//       global regime (wider): 64-bit vector atomicAdd straight into counts.
//     total: popcounts of the steps' masks, summed per wave in scalar registers, per workgroup in LDS, added to global memory once.
// (b) The id-list variant: a workgroup owns a slice of one query's list; a wave takes 64 entries, each lane resolves its id (-1, outside the
//     index, deleted: skipped), and the wave streams the packets of the surviving rows one row after the other through the same row code.
// (c) Top-n: one workgroup per query scores every candidate column in fp64 (conversions, + - x / and one rounding to fp32: bit-reproducible),
//     streams make_key(score, column) through the 4096-key LDS buffer of vs_facet_topn, pruned to n by wg_sort_desc when more than 2048 are in.
#include "common.h"
#include "bitmap_span.h"
#include "staging.h"
#include "term_agg_check.h"
#include "topk_keys.h"

#include <algorithm>

using namespace vs;

namespace {

constexpr int kTermThreads = 1024;                    // 16 waves: an LDS-regime workgroup has the CU to itself
constexpr int kTermWaves = kTermThreads / 64;
constexpr int kTopnThreads = 256;
constexpr int kTopnCap = 4096;                        // keys of the top-n candidate buffer
constexpr int kTopnKeep = 2048;                       // pruned when more are in

struct TermArgs {
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
    int32_t B;                        // work item i of the grid: chunk i / B of query i % B
    unsigned long long* counts;       // [B, ld_counts], zeroed by the caller
    int64_t ld_counts;
    unsigned long long* total;        // [B], zeroed by the caller
};

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

template <int GLOBAL>
__device__ __forceinline__ void add_cells(const uint4& c, uint32_t nz, uint32_t n_cols, uint32_t* hist, unsigned long long* dst) {
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uint32_t col = (t & 1) ? (w[t >> 1] >> 16) : (w[t >> 1] & 0xFFFFu);
        if (((nz >> t) & 1u) && col < n_cols) {                   // (the padding id is n_cols: never a bin)
            if constexpr (GLOBAL) atomicAdd(dst + col, 1ull);
            else atomicAdd(hist + col, 1u);
        }
    }
}

// one wave: every cell of packets [p0, p1) that has its term adds 1 to the term's bin; a lane takes a packet, two are in flight
template <int SD, int GLOBAL>
__device__ __forceinline__ void count_packets(const TermArgs& a, uint32_t p0, uint32_t p1, int lane, uint32_t* hist, unsigned long long* dst) {
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
    const size_t b = blockIdx.x % (uint32_t)a.B;                  // the query runs fastest: resident workgroups sweep the same rows
    const int64_t chunk = blockIdx.x / (uint32_t)a.B;
    if constexpr (!GLOBAL)
        for (int i = tid; i < (a.n_cols + 3) / 4; i += kTermThreads) term_hist4[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) s_tot = 0u;
    __syncthreads();
    unsigned long long* dst = a.counts + b * (size_t)a.ld_counts;
    uint32_t tot = 0u;                                           // wave-uniform: a chunk holds fewer than 2^32 rows
    if constexpr (IDS) {
        const int64_t e0 = chunk * a.rows_per_chunk, e1 = min(a.m, e0 + a.rows_per_chunk);
        const int64_t* list = a.ids + b * (size_t)a.ld_ids;
        for (int64_t eb = e0 + (int64_t)w * 64; eb < e1; eb += (int64_t)kTermWaves * 64) {
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
                count_packets<SD, GLOBAL>(a, p0, p1, lane, hist, dst);
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
            for (int s = w; s < nsub; s += kTermWaves) {
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
                    count_packets<SD, GLOBAL>(a, p0, p1, lane, hist, dst);
                    m = last >= 63 ? 0ull : (m & (~0ull << (last + 1)));
                }
            }
        }
    }
    if (lane == 0 && tot) atomicAdd(&s_tot, tot);
    __syncthreads();
    if constexpr (!GLOBAL) {
        for (int i = tid; i < a.n_cols; i += kTermThreads) {
            const uint32_t v = hist[i];
            if (v) atomicAdd(dst + i, (unsigned long long)v);
        }
    }
    if (tid == 0 && s_tot) atomicAdd(&a.total[b], (unsigned long long)s_tot);
}

int plan_or_fail(int rc, const char* msg) { return rc == VS_OK ? VS_OK : fail(rc, "%s", msg); }

template <int SD, int IDS>
int term_launch(const TermPlan& p, const TermArgs& a, dim3 grid, hipStream_t s) {
    if (p.regime) {
        hipLaunchKernelGGL((term_counts_kernel<SD, 1, IDS>), grid, dim3(kTermThreads), 0, s, a);
    } else {
        const size_t lds = (size_t)((a.n_cols + 3) / 4) * 16;
        VS_HIP(hipFuncSetAttribute((const void*)term_counts_kernel<SD, 0, IDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((term_counts_kernel<SD, 0, IDS>), grid, dim3(kTermThreads), lds, s, a);
    }
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int index_ok(const vs_index* idx) {
    if (idx->kind != VS_KIND_CSR) return fail(VS_EUNSUPPORTED, "term counts read the CSR packets: a dense index on the matrix cores has none");
    if (idx->n_cols > kTermMaxCols) return fail(VS_EUNSUPPORTED, "n_cols = %d is too wide", idx->n_cols);
    return VS_OK;
}

// One call on the index's device: the set is (words, bit0, ld_words) when ids == nullptr, else the id lists.
int term_call(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, const int64_t* ids, int64_t m, int64_t ld_ids, int64_t id_offset,
              int strict, int32_t B, const TermPlan& plan, int64_t* counts, int64_t ld_counts, int64_t* total, void* stream) {
    const int32_t V = idx->n_cols;
    const void* ptrs[4] = {words, ids, counts, total};
    const char* names[4] = {"words", "ids", "counts", "total"};
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
    TermArgs a{};
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
    const size_t n_cnt = (size_t)B * (size_t)V;
    if (dev) {
        a.counts = reinterpret_cast<unsigned long long*>(counts);
        a.ld_counts = ld_counts;
        a.total = reinterpret_cast<unsigned long long*>(total);
        if (ld_counts == V || B == 1) VS_HIP(hipMemsetAsync(a.counts, 0, n_cnt * 8, s));
        else VS_HIP(hipMemset2DAsync(a.counts, (size_t)ld_counts * 8, 0, (size_t)V * 8, (size_t)B, s));
        VS_HIP(hipMemsetAsync(a.total, 0, (size_t)B * 8, s));
    } else {
        VS_TRY(out.alloc((n_cnt + (size_t)B) * 8));
        a.counts = out.as<unsigned long long>();
        a.ld_counts = V;
        a.total = a.counts + n_cnt;
        VS_HIP(hipMemsetAsync(out.p, 0, out.bytes, s));
    }
    if (idx->n_rows > 0) {
        ProfScope prof("term_counts", s);
        const dim3 grid((unsigned)(plan.chunks * B));
        const int sd = idx->store_dtype;
        const int rc = ids ? (sd == VS_F32 ? term_launch<VS_F32, 1>(plan, a, grid, s)
                              : sd == VS_F16 ? term_launch<VS_F16, 1>(plan, a, grid, s)
                                             : term_launch<VS_NONE, 1>(plan, a, grid, s))
                           : (sd == VS_F32 ? term_launch<VS_F32, 0>(plan, a, grid, s)
                              : sd == VS_F16 ? term_launch<VS_F16, 0>(plan, a, grid, s)
                                             : term_launch<VS_NONE, 0>(plan, a, grid, s));
        if (rc != VS_OK) {
            (void)hipStreamSynchronize(s);                          // staging buffers die here
            return rc;
        }
    }
    VS_STAGE("term_counts", s);
    if (!dev) {
        VS_HIP(hipMemcpy2DAsync(counts, (size_t)ld_counts * 8, a.counts, (size_t)V * 8, (size_t)V * 8, (size_t)B, hipMemcpyDeviceToHost, s));
        VS_HIP(hipMemcpyAsync(total, a.total, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    }
    if (!stream || !dev) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
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
    __shared__ uint64_t cand[kTopnCap];
    __shared__ int cnt_sh;
    const int tid = threadIdx.x, lane = tid & 63;
    constexpr int SB = (kTopnCap - kTopnKeep) / kTopnThreads;    // steps between prune checks
    static_assert(SB >= 1, "a step adds up to kTopnThreads candidates");
    const int K = a.n;
    const size_t b = blockIdx.x;
    const int64_t* src = a.counts + b * (size_t)a.ld_counts;
    const int64_t total = a.total[b];
    const bool any = total > 0 && a.bg_total > 0;
    if (tid == 0) cnt_sh = 0;
    __syncthreads();
    uint64_t tau = 0;
    const int iters = (a.n_cols + kTopnThreads - 1) / kTopnThreads;
    for (int it0 = 0; it0 < iters; it0 += SB) {
        const int it1 = min(iters, it0 + SB);
        for (int it = it0; it < it1; ++it) {
            const int c = it * kTopnThreads + tid;
            uint64_t key = 0ull;
            if (any && c < a.n_cols) {
                const int64_t fg = src[c], bg = a.bg[c];
                float sc;
                if (fg >= a.min_count && bg > 0 && term_score(fg, total, bg, a.bg_total, a.method, &sc)) key = make_key(sc, (uint32_t)c);
            }
            const bool pass = key > tau;                          // (key 0: no candidate -- a score is positive, its key has the top bit set)
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
    VS_TRY(index_ok(idx));
    TermPlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(term_check_counts(words != nullptr, bit0, ld_words, B, std::max<int64_t>(idx->n_rows, 1), idx->n_cols, rows_per_chunk,
                                          counts && total, ld_counts, &plan, msg, sizeof msg), msg));
    return term_call(idx, words, bit0, ld_words, nullptr, 0, 0, 0, 0, B, plan, counts, ld_counts, total, stream);
}

extern "C" int vs_index_term_counts_ids(vs_index* idx, const int64_t* ids, int32_t B, int64_t m, int64_t ld, int64_t id_offset, int strict,
                                        int64_t* counts, int64_t ld_counts, int64_t* total, void* stream) {
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    VS_TRY(index_ok(idx));
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
    VS_TRY(need_device());
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range", device);
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
    VS_STAGE("term_topn", s);
    if (!dev)
        for (int i = 3; i < 7; ++i) VS_TRY(st[i].back(s));
    if (!stream || !dev) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}
