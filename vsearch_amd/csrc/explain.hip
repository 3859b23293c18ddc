// explain.hip -- score and explain given (query, document id) pairs against the device index (vs_index_explain): per pair the exact
// score, the number of matched terms (q[c] * v != 0) and the top `topn` vocabulary columns by contribution fl32(q[c] * v).
//
// Shape (after refine_topk_kernel, bp_refine.h): one workgroup per query, its dense fp32 row staged as an LDS image when it fits; one
// wave per hit.  A hit's terms are streamed whole packets per lane (lane l: packets p0 + l, p0 + l + 64, ...) and the matched ones
// become 64-bit keys (make_key(contribution, column): contribution descending, then column ascending) appended to a wave-private LDS
// list of kExplCap keys.  When a row matches more than that, the wave finds the cut by an MSD radix select over re-reads of the row
// (8-bit digits, the histogram aliases the list) and collects only the keys above it; ranks beyond kExplCap come in slices below the
// previous slice's last key.  Every slice is sorted in registers (wave_sort256_desc).
//
// Scores: a CSR-packet index is scored by row_sum_f64 itself (same lane-to-packet mapping, same xor reduction), the function the refine
// step, the exact pass and the exact fallback score rows with: the score is bit-identical to what those paths return for the pair.  The
// MFMA dense kind (`mat`) is scored as the fp64 sum of the products over the query's non-zeros (compacted once per query): equal to the
// matrix-core search's fp32 sum to within rounding, not bit for bit.
#include "common.h"
#include "csr_scan.h"
#include "topk_keys.h"

#include <algorithm>

using namespace vs;

namespace {

constexpr int kExplThreads = 1024;
constexpr int kExplWaves = kExplThreads / 64;
constexpr int kExplCap = 256;                     // keys a wave's list holds (wave_sort256_desc sorts 256)
constexpr int kExplMaxTopn = 1024;

enum : int { SRC_CSR = 0, SRC_CSR_ROW = 1, SRC_DENSE = 2, SRC_DENSE_ROW = 3 };   // *_ROW: disentangle (q == NULL)

struct ExplainArgs {
    const uint32_t* pk_ptr;   // CSR packets
    const uint4* cols;
    const void* vals;
    const float* mat;         // dense [n_rows, ldp] fp32
    int32_t ldp;
    const float* q;           // [B, n_cols] fp32 (rounded to the index dtype); null in disentangle mode
    int32_t* qc_cols;         // dense: per-workgroup scratch [grid][n_cols] of the query's non-zero columns
    float* qc_w;              // ... and their weights
    int32_t n_cols;
    int64_t n_rows;
    int32_t B, k, topn;
    const int64_t* ids;       // [B, ld_ids]
    int64_t ld_ids;
    int64_t id_offset;
    int32_t* out_cols;        // [B, k, topn]
    float* out_contrib;
    float* out_scores;        // [B, k]
    int32_t* out_matched;
};

__host__ __device__ inline size_t explain_lds_bytes(int32_t n_cols, int img) {
    return (img ? scan_img_bytes(n_cols) : 0) + (size_t)kExplWaves * kExplCap * 8 + 16;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Calls f(on, key) for every term of the hit, uniformly across the wave (lanes without a term pass on = false).  on = the term is
// matched (its contribution is non-zero).
template <int SRC, int VM, int IMG>
struct Terms {
    const ExplainArgs& a;
    const float* img;         // SRC_CSR: the query (LDS image or global row); SRC_DENSE: unused
    const int32_t* qc;        // SRC_DENSE: compacted query columns / weights, nq of them
    const float* qw;
    int32_t nq;
    int64_t row;

    template <class F>
    __device__ __forceinline__ void run(int lane, F f) const {
        if constexpr (SRC == SRC_CSR || SRC == SRC_CSR_ROW) {
            const uint32_t p0 = a.pk_ptr[row], p1 = a.pk_ptr[row + 1];
            for (uint32_t pb = p0; pb < p1; pb += 64) {
                const uint32_t p = pb + lane;
                const bool live = p < p1;
                uint32_t cwv[4] = {0u, 0u, 0u, 0u};
                float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (live) {
                    const uint4 cw = a.cols[p];
                    cwv[0] = cw.x; cwv[1] = cw.y; cwv[2] = cw.z; cwv[3] = cw.w;
                    if constexpr (VM == VM_F32) {
                        const float4* vp = reinterpret_cast<const float4*>(a.vals);
                        const float4 v0 = vp[2 * (size_t)p], v1 = vp[2 * (size_t)p + 1];
                        v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
                    } else if constexpr (VM == VM_F16) {
                        const uint4 hv = reinterpret_cast<const uint4*>(a.vals)[p];
                        const __half2* h = reinterpret_cast<const __half2*>(&hv);
#pragma unroll
                        for (int t = 0; t < 4; ++t) { const float2 x = __half22float2(h[t]); v[2 * t] = x.x; v[2 * t + 1] = x.y; }
                    } else {
#pragma unroll
                        for (int t = 0; t < 8; ++t) v[t] = 1.f;
                    }
                }
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const uint32_t c = (t & 1) ? (cwv[t >> 1] >> 16) : (cwv[t >> 1] & 0xFFFFu);
                    const bool real = live && c < (uint32_t)a.n_cols;                  // (pad columns: id n_cols)
                    float prod = 0.f;
                    if constexpr (SRC == SRC_CSR) prod = real ? img[c] * v[t] : 0.f;
                    else prod = real ? v[t] : 0.f;
                    f(prod != 0.f, make_key(prod, c));
                }
            }
        } else {
            const float* r = a.mat + (size_t)row * a.ldp;
            const int32_t n = SRC == SRC_DENSE ? nq : a.n_cols;
            for (int32_t eb = 0; eb < n; eb += 64) {
                const int32_t e = eb + lane;
                float prod = 0.f;
                uint32_t c = 0u;
                if (e < n) {
                    if constexpr (SRC == SRC_DENSE) { c = (uint32_t)qc[e]; prod = qw[e] * r[c]; }
                    else { c = (uint32_t)e; prod = r[c]; }
                }
                f(prod != 0.f, make_key(prod, c));
            }
        }
    }
};

// The wave's keys at ranks [0, want) among the matched keys below `upper`, into list[0, cnt) (cnt >= want, cnt <= kExplCap, any order).
// rem = how many matched keys lie below `upper`.  hist aliases the list.
template <class T>
__device__ __forceinline__ uint32_t select_slice(const T& terms, uint64_t upper, int want, int rem, uint64_t* list, int lane) {
    uint32_t* hist = reinterpret_cast<uint32_t*>(list);
    uint64_t prefix = 0;
    int pbits = 0, need = want, total_above = 0, pop = 0;
    if (rem > kExplCap) {
        for (;;) {
            wave_sync();
#pragma unroll
            for (int j = 0; j < 4; ++j) hist[4 * lane + j] = 0u;
            wave_sync();
            const int sh = 56 - pbits;
            terms.run(lane, [&](bool on, uint64_t key) {
                on = on && key < upper && (pbits == 0 || (key >> (64 - pbits)) == prefix);
                if (on) atomicAdd(&hist[(uint32_t)(key >> sh) & 255u], 1u);
            });
            wave_sync();
            // lane l holds bins 4 l .. 4 l + 3: keys in the bins of higher lanes, then the bin inside the lane where rank `need` falls
            const uint4 c = reinterpret_cast<const uint4*>(hist)[lane];
            const int s = (int)(c.x + c.y + c.z + c.w);
            int incl = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(incl, o, 64); if (lane + o < 64) incl += t; }
            const int above = incl - s;
            int sel_bin = -1, sel_above = 0, sel_pop = 0;
            if (above < need && need <= incl) {
                int a0 = above;
                if (need <= a0 + (int)c.w) { sel_bin = 4 * lane + 3; sel_pop = (int)c.w; }
                else { a0 += (int)c.w; if (need <= a0 + (int)c.z) { sel_bin = 4 * lane + 2; sel_pop = (int)c.z; }
                else { a0 += (int)c.z; if (need <= a0 + (int)c.y) { sel_bin = 4 * lane + 1; sel_pop = (int)c.y; }
                else { a0 += (int)c.y; sel_bin = 4 * lane; sel_pop = (int)c.x; } } }
                sel_above = a0;
            }
            const unsigned long long m = __ballot(sel_bin >= 0);
            const int src = (int)__builtin_ctzll(m);
            sel_bin = __shfl(sel_bin, src, 64);
            sel_above = __shfl(sel_above, src, 64);
            sel_pop = __shfl(sel_pop, src, 64);
            total_above += sel_above;
            need -= sel_above;
            prefix = (prefix << 8) | (uint64_t)sel_bin;
            pbits += 8;
            pop = sel_pop;
            if (total_above + pop <= kExplCap || pbits >= 64) break;
        }
    }
    // collect the keys below `upper` whose decided bits are >= prefix (all of them when rem fits the list)
    wave_sync();
    uint32_t cnt = 0;
    terms.run(lane, [&](bool on, uint64_t key) {
        on = on && key < upper && (pbits == 0 || (key >> (64 - pbits)) >= prefix);
        const unsigned long long m = __ballot(on);
        const uint32_t pos = cnt + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (on && pos < (uint32_t)kExplCap) list[pos] = key;
        cnt += (uint32_t)__popcll(m);
    });
    wave_sync();
    return min(cnt, (uint32_t)kExplCap);
}

template <int SRC, int VM, int IMG>
__global__ __launch_bounds__(kExplThreads) void explain_kernel(ExplainArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_e[];
    float* img = reinterpret_cast<float*>(smem_e);
    uint64_t* lists = reinterpret_cast<uint64_t*>(smem_e + (IMG ? scan_img_bytes(a.n_cols) : 0));
    int* nq_sh = reinterpret_cast<int*>(lists + kExplWaves * kExplCap);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint64_t* list = lists + w * kExplCap;
    int32_t* qc = a.qc_cols ? a.qc_cols + (size_t)blockIdx.x * a.n_cols : nullptr;
    float* qw = a.qc_w ? a.qc_w + (size_t)blockIdx.x * a.n_cols : nullptr;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float* qrow = a.q ? a.q + (size_t)b * a.n_cols : nullptr;
        __syncthreads();                                                  // (the previous query's look-ups are done)
        if constexpr (IMG != 0) {
            for (int i = tid; i <= a.n_cols; i += kExplThreads) img[i] = i < a.n_cols ? qrow[i] : 0.f;
        }
        if constexpr (SRC == SRC_DENSE) {
            // the query's non-zero columns in ascending order, compacted into this workgroup's scratch (ballot + wave offsets)
            int* wcnt = reinterpret_cast<int*>(lists);                   // (the lists are free until the hits start)
            int base = 0;
            for (int c0 = 0; c0 < a.n_cols; c0 += kExplThreads) {
                const int c = c0 + tid;
                const float x = c < a.n_cols ? qrow[c] : 0.f;
                const bool on = x != 0.f;
                const unsigned long long m = __ballot(on);
                if (lane == 0) wcnt[w] = __popcll(m);
                __syncthreads();
                int off = base;
                for (int j = 0; j < w; ++j) off += wcnt[j];
                int tot = base;
                for (int j = 0; j < kExplWaves; ++j) tot += wcnt[j];
                if (on) { const int pos = off + __popcll(m & ((1ull << lane) - 1ull)); qc[pos] = c; qw[pos] = x; }
                __syncthreads();
                base = tot;
            }
            if (tid == 0) *nq_sh = base;
        }
        __syncthreads();
        const int nq = SRC == SRC_DENSE ? *nq_sh : 0;
        const float* look = IMG ? img : qrow;
        for (int j = w; j < a.k; j += kExplWaves) {
            const size_t pair = (size_t)b * a.k + j;
            const int64_t id = a.ids[(size_t)b * a.ld_ids + j];
            int32_t* oc = a.out_cols ? a.out_cols + pair * a.topn : nullptr;
            float* ov = a.out_contrib ? a.out_contrib + pair * a.topn : nullptr;
            if (id == -1) {                                               // a filtered search's padding
                if (lane == 0) { a.out_scores[pair] = -INFINITY; a.out_matched[pair] = 0; }
                for (int r = lane; r < a.topn; r += 64) { oc[r] = -1; ov[r] = 0.f; }
                continue;
            }
            const int64_t row = id - a.id_offset;
            if (row < 0 || row >= a.n_rows) {                             // not this index's row: leave the pair to its owner
                if (lane == 0) a.out_matched[pair] = -1;
                continue;
            }
            const Terms<SRC, VM, IMG> terms{a, look, qc, qw, nq, row};
            // score: a CSR row through row_sum_f64 (the library's exact numerics, bit for bit); a dense row as the fp64 sum of its products
            double sum = 0.0;
            if constexpr (SRC == SRC_CSR) {
                sum = row_sum_f64<VM>(a.pk_ptr, a.cols, a.vals, (uint32_t)row, lane, [&](uint32_t c) {
                    if constexpr (IMG != 0) return look[c];
                    else return c < (uint32_t)a.n_cols ? look[c] : 0.f;
                });
            } else if constexpr (SRC == SRC_CSR_ROW) {
                sum = row_sum_f64<VM>(a.pk_ptr, a.cols, a.vals, (uint32_t)row, lane, [&](uint32_t c) { return c < (uint32_t)a.n_cols ? 1.f : 0.f; });
            } else {
                terms.run(lane, [&](bool, uint64_t key) { sum += (double)key_score(key); });
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            }
            // matched terms: counted, and listed while they fit
            wave_sync();
            int nm = 0;
            terms.run(lane, [&](bool on, uint64_t key) {
                const unsigned long long m = __ballot(on);
                const int pos = nm + __popcll(m & ((1ull << lane) - 1ull));
                if (on && pos < kExplCap) list[pos] = key;
                nm += __popcll(m);
            });
            wave_sync();
            if (lane == 0) { a.out_scores[pair] = (float)sum; a.out_matched[pair] = nm; }
            const int total = min(a.topn, nm);
            int done = 0;
            uint64_t upper = ~0ull;
            while (done < total) {
                const int want = min(kExplCap, total - done);
                const int rem = nm - done;
                uint32_t cnt = (uint32_t)min(rem, kExplCap);
                if (done > 0 || rem > kExplCap) cnt = select_slice(terms, upper, want, rem, list, lane);
                uint64_t k4[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { const uint32_t e = (uint32_t)(r * 64 + lane); k4[r] = e < cnt ? list[e] : 0ull; }
                wave_sort256_desc(k4, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = r * 64 + lane;
                    if (e < want) { oc[done + e] = (int32_t)key_row(k4[r]); ov[done + e] = key_score(k4[r]); }
                }
                const int last = want - 1;
                const uint64_t kl = (last >> 6) == 0 ? k4[0] : (last >> 6) == 1 ? k4[1] : (last >> 6) == 2 ? k4[2] : k4[3];
                upper = __shfl(kl, last & 63, 64);
                done += want;
                wave_sync();
            }
            for (int r = total + lane; r < a.topn; r += 64) { oc[r] = -1; ov[r] = 0.f; }
        }
    }
}

// q (fp32 | fp16, leading dim ldq) -> contiguous fp32 [B, n_cols], rounded through fp16 for an fp16 index (what the search kernels read)
template <class T>
__global__ void explain_prep_kernel(const T* q, int64_t ldq, int32_t B, int32_t n_cols, int round_f16, float* out) {
    const int64_t n = (int64_t)B * n_cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / n_cols, c = i % n_cols;
        float v;
        if constexpr (sizeof(T) == 4) v = q[b * ldq + c];
        else v = __half2float(q[b * ldq + c]);
        if (round_f16) v = __half2float(__float2half_rn(v));
        out[i] = v;
    }
}

template <int SRC, int VM, int IMG>
int launch_explain(const ExplainArgs& a, int grid, size_t lds, hipStream_t s) {
    VS_HIP(hipFuncSetAttribute((const void*)explain_kernel<SRC, VM, IMG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((explain_kernel<SRC, VM, IMG>), dim3(grid), dim3(kExplThreads), lds, s, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

template <int SRC, int IMG>
int launch_explain_vm(int store_dtype, const ExplainArgs& a, int grid, size_t lds, hipStream_t s) {
    if (store_dtype == VS_F32) return launch_explain<SRC, VM_F32, IMG>(a, grid, lds, s);
    if (store_dtype == VS_F16) return launch_explain<SRC, VM_F16, IMG>(a, grid, lds, s);
    return launch_explain<SRC, VM_BIN, IMG>(a, grid, lds, s);
}

int check_device(const void* p, int device, const char* what) {
    if (!is_device_ptr(p)) return VS_OK;
    hipPointerAttribute_t attr;
    VS_HIP(hipPointerGetAttributes(&attr, p));
    if (attr.device != device) return fail(VS_EINVAL, "%s lives on device %d, the index on device %d", what, attr.device, device);
    return VS_OK;
}

}  // namespace

extern "C" int vs_index_explain(vs_index* idx, const void* q, int q_dtype, int64_t ldq, int32_t B, const int64_t* ids, int64_t ld_ids, int32_t k,
                                int64_t id_offset, int32_t topn, int32_t* out_cols, float* out_contrib, float* out_scores, int32_t* out_matched,
                                void* stream) {
    if (!idx || !ids || !out_scores || !out_matched) return fail(VS_EINVAL, "NULL argument");
    if (B <= 0) return fail(VS_EINVAL, "B must be positive");
    if (k < 0) return fail(VS_EINVAL, "k must be >= 0");
    if (ld_ids < k) return fail(VS_EINVAL, "ld_ids = %lld is shorter than k = %d", (long long)ld_ids, k);
    if (topn < 0 || topn > kExplMaxTopn) return fail(VS_EINVAL, "topn must be in 0..%d (got %d)", kExplMaxTopn, topn);
    if (topn > 0 && (!out_cols || !out_contrib)) return fail(VS_EINVAL, "out_cols / out_contrib are NULL with topn = %d", topn);
    if (q) {
        if (q_dtype != VS_F32 && q_dtype != VS_F16) return fail(VS_EINVAL, "q_dtype must be VS_F32 or VS_F16");
        if (ldq < idx->n_cols) return fail(VS_EINVAL, "query has %lld columns, index has %d", (long long)ldq, idx->n_cols);
    }
    const bool dense = idx->kind != VS_KIND_CSR;
    if (!dense && scan_img_bytes(idx->n_cols) > 160 * 1024) return fail(VS_EUNSUPPORTED, "n_cols = %d is too wide", idx->n_cols);
    const void* outs[4] = {out_cols, out_contrib, out_scores, out_matched};
    const bool out_dev = is_device_ptr(out_scores);
    for (const void* p : outs)
        if (p && is_device_ptr(p) != out_dev) return fail(VS_EINVAL, "the outputs must all be host or all device pointers");
    VS_TRY(check_device(q, idx->device, "q"));
    VS_TRY(check_device(ids, idx->device, "ids"));
    for (const void* p : outs) VS_TRY(check_device(p, idx->device, "an output"));
    VS_HIP(hipSetDevice(idx->device));
    hipStream_t s = (hipStream_t)stream;
    if (k == 0) {
        if (!stream) VS_HIP(hipStreamSynchronize(s));
        return VS_OK;
    }
    // staging of host buffers (the handle's scratch, as vs_index_search's host queries / outputs)
    const size_t n_pairs = (size_t)B * k;
    DevBuf st_ids, st_out, st_qc;
    const int64_t* d_ids = ids;
    if (!is_device_ptr(ids)) {
        const size_t bytes = ((size_t)(B - 1) * ld_ids + k) * 8;
        VS_TRY(st_ids.alloc(bytes));
        VS_HIP(hipMemcpyAsync(st_ids.p, ids, bytes, hipMemcpyHostToDevice, s));
        d_ids = st_ids.as<int64_t>();
    }
    int32_t* d_cols = out_cols;
    float* d_contrib = out_contrib;
    float* d_scores = out_scores;
    int32_t* d_matched = out_matched;
    const size_t sz_cols = topn > 0 ? n_pairs * topn * 4 : 0;
    if (!out_dev) {
        VS_TRY(st_out.alloc(2 * sz_cols + n_pairs * 8));
        char* p = st_out.as<char>();
        d_cols = topn > 0 ? reinterpret_cast<int32_t*>(p) : nullptr;
        d_contrib = topn > 0 ? reinterpret_cast<float*>(p + sz_cols) : nullptr;
        d_scores = reinterpret_cast<float*>(p + 2 * sz_cols);
        d_matched = reinterpret_cast<int32_t*>(p + 2 * sz_cols + n_pairs * 4);
    }
    if (topn == 0) { d_cols = nullptr; d_contrib = nullptr; }
    // queries: contiguous fp32 rows rounded to the index dtype (the search's prep; a dense index reads them at ld n_cols here)
    const float* dq = nullptr;
    if (q) {
        const void* src = q;
        if (!is_device_ptr(q)) {
            const size_t bytes = ((size_t)(B - 1) * ldq + idx->n_cols) * dtype_size(q_dtype);
            VS_TRY(idx->ws_misc.reserve(bytes));
            VS_HIP(hipMemcpyAsync(idx->ws_misc.p, q, bytes, hipMemcpyHostToDevice, s));
            src = idx->ws_misc.p;
        }
        const int round_f16 = idx->store_dtype == VS_F16;
        if (q_dtype == VS_F32 && !round_f16 && ldq == idx->n_cols) {
            dq = (const float*)src;
        } else {
            VS_TRY(idx->ws_q.reserve((size_t)B * idx->n_cols * 4));
            const int64_t n = (int64_t)B * idx->n_cols;
            const unsigned grid = (unsigned)std::min<int64_t>(ceil_div64(n, 256), 4096);
            if (q_dtype == VS_F32)
                hipLaunchKernelGGL((explain_prep_kernel<float>), dim3(grid), dim3(256), 0, s, (const float*)src, ldq, B, idx->n_cols, round_f16, idx->ws_q.as<float>());
            else
                hipLaunchKernelGGL((explain_prep_kernel<__half>), dim3(grid), dim3(256), 0, s, (const __half*)src, ldq, B, idx->n_cols, round_f16, idx->ws_q.as<float>());
            VS_HIP(hipGetLastError());
            dq = idx->ws_q.as<float>();
        }
    }
    ExplainArgs a{};
    a.pk_ptr = idx->pk_ptr.as<uint32_t>();
    a.cols = idx->cols.as<uint4>();
    a.vals = idx->vals.p;
    a.mat = idx->mat.as<float>();
    a.ldp = (idx->n_cols + 31) / 32 * 32;                                    // (dense.hip's row pitch)
    a.q = dq;
    a.n_cols = idx->n_cols;
    a.n_rows = idx->n_rows;
    a.B = B;
    a.k = k;
    a.topn = topn;
    a.ids = d_ids;
    a.ld_ids = ld_ids;
    a.id_offset = id_offset;
    a.out_cols = d_cols;
    a.out_contrib = d_contrib;
    a.out_scores = d_scores;
    a.out_matched = d_matched;
    {
        ProfScope prof("explain", s);
        if (dense) {
            const int grid = std::min(B, idx->cu_count * 2);
            const size_t lds = explain_lds_bytes(idx->n_cols, 0);
            if (q) {
                VS_TRY(st_qc.alloc((size_t)grid * idx->n_cols * 8));
                a.qc_cols = st_qc.as<int32_t>();
                a.qc_w = reinterpret_cast<float*>(st_qc.as<int32_t>() + (size_t)grid * idx->n_cols);
                VS_TRY((launch_explain<SRC_DENSE, VM_F32, 0>(a, grid, lds, s)));
            } else {
                VS_TRY((launch_explain<SRC_DENSE_ROW, VM_F32, 0>(a, grid, lds, s)));
            }
        } else if (!q) {
            VS_TRY((launch_explain_vm<SRC_CSR_ROW, 0>(idx->store_dtype, a, std::min(B, idx->cu_count * 2), explain_lds_bytes(idx->n_cols, 0), s)));
        } else {
            const bool img = explain_lds_bytes(idx->n_cols, 1) <= 160 * 1024;
            const int grid = std::min(B, idx->cu_count * (img ? 1 : 2));
            if (img) VS_TRY((launch_explain_vm<SRC_CSR, 1>(idx->store_dtype, a, grid, explain_lds_bytes(idx->n_cols, 1), s)));
            else VS_TRY((launch_explain_vm<SRC_CSR, 0>(idx->store_dtype, a, grid, explain_lds_bytes(idx->n_cols, 0), s)));
        }
    }
    VS_STAGE("explain", s);
    if (!out_dev) {
        if (topn > 0) {
            VS_HIP(hipMemcpyAsync(out_cols, d_cols, sz_cols, hipMemcpyDeviceToHost, s));
            VS_HIP(hipMemcpyAsync(out_contrib, d_contrib, sz_cols, hipMemcpyDeviceToHost, s));
        }
        VS_HIP(hipMemcpyAsync(out_scores, d_scores, n_pairs * 4, hipMemcpyDeviceToHost, s));
        VS_HIP(hipMemcpyAsync(out_matched, d_matched, n_pairs * 4, hipMemcpyDeviceToHost, s));
    }
    // staging buffers die here: a call that used any waits for its work (device pointers + a stream: only enqueued)
    if (!stream || st_ids.p || st_out.p || st_qc.p) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}

// ---- shard group: pairs whose explaining shard is `src` (its n_matched >= 0) and that no earlier shard took (dst n_matched < 0) ----
__global__ __launch_bounds__(256) void explain_combine_kernel(const int32_t* s_cols, const float* s_contrib, const float* s_scores, const int32_t* s_matched,
                                                              int64_t n_pairs, int32_t topn, int32_t* d_cols, float* d_contrib, float* d_scores,
                                                              int32_t* d_matched) {
    const int lane = threadIdx.x & 63;
    for (int64_t pr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); pr < n_pairs; pr += (int64_t)gridDim.x * 4) {
        if (s_matched[pr] < 0 || d_matched[pr] >= 0) continue;         // (uniform per wave)
        for (int r = lane; r < topn; r += 64) {
            d_cols[(size_t)pr * topn + r] = s_cols[(size_t)pr * topn + r];
            d_contrib[(size_t)pr * topn + r] = s_contrib[(size_t)pr * topn + r];
        }
        if (lane == 0) { d_scores[pr] = s_scores[pr]; d_matched[pr] = s_matched[pr]; }
    }
}

int vs_shard_group_explain_impl(const std::vector<vs_index*>& shards, const std::vector<int64_t>& row0, const std::vector<hipStream_t>& streams,
                                const void* q, int q_dtype, int64_t ldq, int32_t B, const int64_t* ids, int64_t ld_ids, int32_t k, int32_t topn,
                                int32_t* out_cols, float* out_contrib, float* out_scores, int32_t* out_matched) {
    if (!ids || !out_scores || !out_matched) return fail(VS_EINVAL, "NULL argument");
    if (B <= 0) return fail(VS_EINVAL, "B must be positive");
    if (k < 0) return fail(VS_EINVAL, "k must be >= 0");
    if (ld_ids < k) return fail(VS_EINVAL, "ld_ids = %lld is shorter than k = %d", (long long)ld_ids, k);
    if (topn < 0 || topn > kExplMaxTopn) return fail(VS_EINVAL, "topn must be in 0..%d (got %d)", kExplMaxTopn, topn);
    if (topn > 0 && (!out_cols || !out_contrib)) return fail(VS_EINVAL, "out_cols / out_contrib are NULL with topn = %d", topn);
    if (q && q_dtype != VS_F32 && q_dtype != VS_F16) return fail(VS_EINVAL, "q_dtype must be VS_F32 or VS_F16");
    const int n = (int)shards.size();
    const int V = shards[0]->n_cols;
    if (q && ldq < V) return fail(VS_EINVAL, "query has %lld columns, index has %d", (long long)ldq, V);
    const int dev0 = shards[0]->device;
    const void* outs[4] = {out_cols, out_contrib, out_scores, out_matched};
    const bool out_dev = is_device_ptr(out_scores);
    for (const void* p : outs) {
        if (p && is_device_ptr(p) != out_dev) return fail(VS_EINVAL, "the outputs must all be host or all device pointers");
        VS_TRY(check_device(p, dev0, "an output"));
    }
    if (k == 0) return VS_OK;
    const size_t n_pairs = (size_t)B * k;
    const size_t sz_cols = topn > 0 ? n_pairs * topn * 4 : 0;
    const size_t esz = q ? dtype_size(q_dtype) : 0;
    const size_t q_bytes = q ? ((size_t)(B - 1) * ldq + V) * esz : 0;
    const size_t id_bytes = ((size_t)(B - 1) * ld_ids + k) * 8;
    auto device_of = [](const void* p, int* d) -> int {
        hipPointerAttribute_t attr;
        VS_HIP(hipPointerGetAttributes(&attr, p));
        *d = attr.device;
        return VS_OK;
    };
    const bool q_dev = is_device_ptr(q), i_dev = is_device_ptr(ids);
    int q_device = 0, i_device = 0;
    if (q_dev) { VS_TRY(device_of(q, &q_device)); VS_HIP(hipSetDevice(q_device)); VS_HIP(hipDeviceSynchronize()); }
    if (i_dev) { VS_TRY(device_of(ids, &i_device)); VS_HIP(hipSetDevice(i_device)); VS_HIP(hipDeviceSynchronize()); }
    if (out_dev) { VS_HIP(hipSetDevice(dev0)); VS_HIP(hipDeviceSynchronize()); }
    // per shard: its inputs on its device, its results in buffers there; shard 0 writes the group's result buffers directly
    std::vector<DevBuf> bq((size_t)n), bi((size_t)n), bo((size_t)n);
    std::vector<hipEvent_t> ev((size_t)n, nullptr);
    struct EvGuard { std::vector<hipEvent_t>& e; ~EvGuard() { for (auto x : e) if (x) (void)hipEventDestroy(x); } } evg{ev};
    DevBuf out0, stage;
    char* o0 = nullptr;
    VS_HIP(hipSetDevice(dev0));
    if (!out_dev) {
        VS_TRY(out0.alloc(2 * sz_cols + n_pairs * 8));
        o0 = out0.as<char>();
    }
    int32_t* g_cols = out_dev ? out_cols : reinterpret_cast<int32_t*>(o0);
    float* g_contrib = out_dev ? out_contrib : reinterpret_cast<float*>(o0 + sz_cols);
    float* g_scores = out_dev ? out_scores : reinterpret_cast<float*>(o0 + 2 * sz_cols);
    int32_t* g_matched = out_dev ? out_matched : reinterpret_cast<int32_t*>(o0 + 2 * sz_cols + n_pairs * 4);
    if (topn == 0) { g_cols = nullptr; g_contrib = nullptr; }
    for (int i = 0; i < n; ++i) {
        vs_index* sh = shards[i];
        VS_HIP(hipSetDevice(sh->device));
        const void* dq = q;
        if (q && (!q_dev || q_device != sh->device)) {
            VS_TRY(bq[i].alloc(q_bytes));
            if (q_dev) VS_HIP(hipMemcpyPeerAsync(bq[i].p, sh->device, q, q_device, q_bytes, streams[i]));
            else VS_HIP(hipMemcpyAsync(bq[i].p, q, q_bytes, hipMemcpyHostToDevice, streams[i]));
            dq = bq[i].p;
        }
        const int64_t* di = ids;
        if (!i_dev || i_device != sh->device) {
            VS_TRY(bi[i].alloc(id_bytes));
            if (i_dev) VS_HIP(hipMemcpyPeerAsync(bi[i].p, sh->device, ids, i_device, id_bytes, streams[i]));
            else VS_HIP(hipMemcpyAsync(bi[i].p, ids, id_bytes, hipMemcpyHostToDevice, streams[i]));
            di = bi[i].as<int64_t>();
        }
        int32_t* c = g_cols; float* v = g_contrib; float* sc = g_scores; int32_t* m = g_matched;
        if (i > 0) {
            VS_TRY(bo[i].alloc(2 * sz_cols + n_pairs * 8));
            char* p = bo[i].as<char>();
            c = topn > 0 ? reinterpret_cast<int32_t*>(p) : nullptr;
            v = topn > 0 ? reinterpret_cast<float*>(p + sz_cols) : nullptr;
            sc = reinterpret_cast<float*>(p + 2 * sz_cols);
            m = reinterpret_cast<int32_t*>(p + 2 * sz_cols + n_pairs * 4);
        }
        VS_TRY(vs_index_explain(sh, dq, q_dtype, ldq, B, di, ld_ids, k, row0[i], topn, c, v, sc, m, (void*)streams[i]));
        VS_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        VS_HIP(hipEventRecord(ev[i], streams[i]));
    }
    // gather on the first shard's device: every later shard fills the pairs it owns
    VS_HIP(hipSetDevice(dev0));
    hipStream_t st0 = streams[0];
    for (int i = 1; i < n; ++i) {
        VS_HIP(hipStreamWaitEvent(st0, ev[i], 0));
        const char* src = bo[i].as<char>();
        if (shards[i]->device != dev0) {
            VS_TRY(stage.reserve(2 * sz_cols + n_pairs * 8));
            VS_HIP(hipMemcpyAsync(stage.p, src, 2 * sz_cols + n_pairs * 8, hipMemcpyDefault, st0));
            src = stage.as<char>();
        }
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div64((int64_t)n_pairs, 4), 65536);
        hipLaunchKernelGGL(explain_combine_kernel, dim3(grid), dim3(256), 0, st0, reinterpret_cast<const int32_t*>(src),
                           reinterpret_cast<const float*>(src + sz_cols), reinterpret_cast<const float*>(src + 2 * sz_cols),
                           reinterpret_cast<const int32_t*>(src + 2 * sz_cols + n_pairs * 4), (int64_t)n_pairs, topn, g_cols, g_contrib, g_scores, g_matched);
        VS_HIP(hipGetLastError());
    }
    if (!out_dev) {
        if (topn > 0) {
            VS_HIP(hipMemcpyAsync(out_cols, g_cols, sz_cols, hipMemcpyDeviceToHost, st0));
            VS_HIP(hipMemcpyAsync(out_contrib, g_contrib, sz_cols, hipMemcpyDeviceToHost, st0));
        }
        VS_HIP(hipMemcpyAsync(out_scores, g_scores, n_pairs * 4, hipMemcpyDeviceToHost, st0));
        VS_HIP(hipMemcpyAsync(out_matched, g_matched, n_pairs * 4, hipMemcpyDeviceToHost, st0));
    }
    for (int i = 0; i < n; ++i) { VS_HIP(hipSetDevice(shards[i]->device)); VS_HIP(hipStreamSynchronize(streams[i])); }
    VS_HIP(hipSetDevice(dev0));
    return VS_OK;
}
