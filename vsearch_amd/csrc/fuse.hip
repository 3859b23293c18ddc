// fuse.hip -- fused search: rank and score fusion of hit lists (vs_fuse_topk).  No reference counterpart.  It runs behind the searches, on
// their merged results; no search kernel is touched.
//
// One workgroup of 8 waves per query.  LDS holds two arrays of N 64-bit keys, N = L * kk rounded up to a power of two (64 KiB at the limit
// L * kk = 4096), and 25 words: the lists' lengths, their smallest / largest score as ordered bits, the number of documents.
//   lengths: a list ends at its first id outside [0, 2^32 - 1) (atomicMin of the position)  | barrier |
//   entry keys: bit 63 | ~(id : list : position) in 45 bits, 0 for an entry behind its list's end and for the slots up to N: one descending
//     sort puts the entries in (id, list, position) ascending order with every filler behind them.  A document's entries are adjacent, and
//     its first entry of a list is its lowest position: the union and the duplicates come out of the same sort.  Meanwhile the score modes
//     reduce each list's smallest / largest score per wave (integer atomics on ordered bits into LDS)  | sort |
//   one thread per run head (an entry whose predecessor carries another id) folds its run into the fused value, list by list, and files
//     the rank key (topk_keys.h: fused in the high word, ~position of the head in the low word: heads are in id order, so the lower id wins
//     a tie and keys never tie); every other slot files 0.  The heads are counted by ballots  | sort |
//   thread t < min(k, documents) folds the run of rank key t once more, now writing its [L] ranks and scores; the rest write unused slots.
// No float atomics: every output bit is deterministic.  The arithmetic is pinned operation by operation to tests/_fuse_ref.py.
#include "common.h"
#include "fuse_check.h"
#include "staging.h"
#include "topk_keys.h"

using namespace vs;

namespace {

constexpr int kThreads = 512;
constexpr int kMiscWords = 32;                               // behind the keys: len [8], mn [8], mx [8], [24] documents
constexpr uint64_t kLive = 1ull << 63;
constexpr uint64_t kEntryMask = (1ull << 45) - 1ull;         // id 32 bits : list 3 bits : position 10 bits

struct FuseArgs {
    const int64_t* ids;      // list l of query b: [l * stride + b * ld, + kk)
    const float* sc;
    int64_t ld, stride;
    const float* w;          // NULL: all 1
    int64_t ldw;             // 0: one [L] for the batch
    const float* fill;       // NULL: 0 (VS_FUSE_RAW only)
    int64_t ldf;
    int32_t L, kk, k, mode, N;
    float c;
    int64_t* oi;             // [B, k]
    float* of;               // [B, k]
    int32_t* orank;          // [B, k, L]
    float* osc;              // [B, k, L]
    int32_t* on;             // [B]
};

size_t lds_bytes(int32_t N) { return 2 * (size_t)N * sizeof(uint64_t) + kMiscWords * 4; }

__device__ __forceinline__ uint64_t entry_key(uint32_t id, int l, int pos) {
    const uint64_t asc = ((uint64_t)id << 13) | ((uint64_t)l << 10) | (uint64_t)pos;
    return kLive | (~asc & kEntryMask);
}
__device__ __forceinline__ uint32_t entry_id(uint64_t key) { return (uint32_t)((~key & kEntryMask) >> 13); }
__device__ __forceinline__ int entry_list(uint64_t key) { return (int)((~key >> 10) & 7ull); }
__device__ __forceinline__ int entry_pos(uint64_t key) { return (int)(~key & 1023ull); }

// fl32(x / y) (an fp64 quotient of two fp32 values rounded to fp32 IS the correctly rounded fp32 quotient: 53 >= 2 * 24 + 2)
__device__ __forceinline__ float div_rn(float x, float y) { return (float)((double)x / (double)y); }

// The run of document entry_id(keys[i]) -- entries [i, ...) of the sorted keys, M of them live -- folded in list order -> fused.  EMIT: the
// [L] ranks and scores of the document are written to orank / osc.
template <bool EMIT>
__device__ __forceinline__ float fold_run(const FuseArgs& a, const uint64_t* keys, int i, int M, const float* sc, const float* w, const float* fill,
                                          const uint32_t* mn, const uint32_t* mx, int32_t* orank, float* osc) {
    const uint32_t id = entry_id(keys[i]);
    int j = i, m = 0;
    float fused = 0.f;
    for (int l = 0; l < a.L; ++l) {
        const float wl = w ? w[l] : 1.f;
        int pos = -1;
        float s = -INFINITY;
        if (j < M && entry_id(keys[j]) == id && entry_list(keys[j]) == l) {
            pos = entry_pos(keys[j]);
            do ++j;                                                           // the id's later entries in this list are ignored
            while (j < M && entry_id(keys[j]) == id && entry_list(keys[j]) == l);
            ++m;
            if (EMIT || a.mode != VS_FUSE_RRF) s = sc[(size_t)l * (size_t)a.stride + (size_t)pos];
        }
        float c = 0.f;
        if (a.mode == VS_FUSE_RRF) {
            if (pos >= 0) c = div_rn(wl, __fadd_rn(a.c, (float)(pos + 1)));
        } else if (a.mode == VS_FUSE_RAW) {
            c = __fmul_rn(wl, pos >= 0 ? s : (fill ? fill[l] : 0.f));
        } else if (pos >= 0) {
            const float lo = unflip_f32(mn[l]), hi = unflip_f32(mx[l]);
            c = __fmul_rn(wl, hi == lo ? 1.f : div_rn(__fsub_rn(s, lo), __fsub_rn(hi, lo)));
        }
        fused = l == 0 ? c : __fadd_rn(fused, c);
        if (EMIT) {
            orank[l] = pos;
            osc[l] = s;
        }
    }
    if (a.mode == VS_FUSE_MNZ) fused = __fmul_rn(fused, (float)m);
    return fused;
}

__global__ __launch_bounds__(kThreads) void fuse_topk_kernel(FuseArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t fuse_sh[];
    uint64_t* k1 = fuse_sh;                                                   // [N] entry keys
    uint64_t* k2 = k1 + a.N;                                                  // [N] rank keys
    int32_t* len = reinterpret_cast<int32_t*>(k2 + a.N);                      // [8]
    uint32_t* mn = reinterpret_cast<uint32_t*>(len + 8);                      // [8] flip_f32 of the list's smallest score
    uint32_t* mx = mn + 8;                                                    // [8] ... largest
    int32_t* docs = reinterpret_cast<int32_t*>(mx + 8);                       // [1]
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t b = blockIdx.x;
    const int L = a.L, kk = a.kk, N = a.N, E = L * kk;
    const int64_t* ids = a.ids + b * (size_t)a.ld;
    const float* sc = a.sc + b * (size_t)a.ld;
    const float* w = a.w ? a.w + b * (size_t)a.ldw : nullptr;
    const float* fill = a.fill ? a.fill + b * (size_t)a.ldf : nullptr;

    if (tid < 8) {
        len[tid] = kk;
        mn[tid] = 0xFFFFFFFFu;
        mx[tid] = 0u;
    }
    if (tid == 0) docs[0] = 0;
    __syncthreads();
    for (int e = tid; e < E; e += kThreads) {
        const int l = e / kk, pos = e - l * kk;
        const int64_t id = ids[(size_t)l * (size_t)a.stride + (size_t)pos];
        if (id < 0 || id >= kFuseIdEnd) atomicMin(&len[l], pos);              // the list ends at its first id -1 (or outside the keys' range)
    }
    __syncthreads();
    for (int e = tid; e < N; e += kThreads) {
        uint64_t key = 0ull;
        if (e < E) {
            const int l = e / kk, pos = e - l * kk;
            if (pos < len[l]) key = entry_key((uint32_t)ids[(size_t)l * (size_t)a.stride + (size_t)pos], l, pos);
        }
        k1[e] = key;
    }
    int M = 0;
    for (int l = 0; l < L; ++l) M += len[l];
    if (a.mode == VS_FUSE_SUM || a.mode == VS_FUSE_MNZ)
        for (int l = 0; l < L; ++l) {
            uint32_t lo = 0xFFFFFFFFu, hi = 0u;
            for (int pos = tid; pos < len[l]; pos += kThreads) {
                const uint32_t u = flip_f32(sc[(size_t)l * (size_t)a.stride + (size_t)pos]);
                lo = min(lo, u);
                hi = max(hi, u);
            }
            for (int o = 32; o > 0; o >>= 1) {
                lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
                hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, 64));
            }
            if (lane == 0 && lo <= hi) {
                atomicMin(&mn[l], lo);
                atomicMax(&mx[l], hi);
            }
        }
    wg_sort_desc<kThreads>(k1, N, tid);

    for (int base = 0; base < N; base += kThreads) {
        const int i = base + tid;
        const bool head = i < M && (i == 0 || entry_id(k1[i - 1]) != entry_id(k1[i]));
        uint64_t key = 0ull;
        if (head) key = make_key(canon_zero(fold_run<false>(a, k1, i, M, sc, w, fill, mn, mx, nullptr, nullptr)), (uint32_t)i);
        if (i < N) k2[i] = key;
        const unsigned long long heads = __ballot(head);
        if (lane == 0 && heads) atomicAdd(&docs[0], (int)__popcll(heads));
    }
    wg_sort_desc<kThreads>(k2, N, tid);

    const int U = docs[0];
    const int n_res = min(a.k, U);
    for (int t = tid; t < a.k; t += kThreads) {
        const size_t slot = b * (size_t)a.k + (size_t)t;
        int32_t* orank = a.orank + slot * (size_t)L;
        float* osc = a.osc + slot * (size_t)L;
        if (t < n_res) {
            const int i = (int)key_row(k2[t]);
            a.oi[slot] = (int64_t)entry_id(k1[i]);
            a.of[slot] = fold_run<true>(a, k1, i, M, sc, w, fill, mn, mx, orank, osc);
        } else {
            a.oi[slot] = -1;
            a.of[slot] = -INFINITY;
            for (int l = 0; l < L; ++l) {
                orank[l] = -1;
                osc[l] = -INFINITY;
            }
        }
    }
    if (tid == 0) a.on[b] = U;
}

}  // namespace

extern "C" int vs_fuse_topk(const int64_t* ids, const float* scores, int32_t L, int32_t B, int32_t kk, int64_t ld, int64_t list_stride,
                            const float* weights, int64_t ldw, const float* fill, int64_t ldf, int mode, float rrf_c, int32_t k, int64_t* out_ids,
                            float* out_fused, int32_t* out_ranks, float* out_scores, int32_t* out_n, int device, void* stream) {
    VS_TRY(need_device());
    if (!ids || !scores || !out_ids || !out_fused || !out_ranks || !out_scores || !out_n) return fail(VS_EINVAL, "NULL argument");
    VS_TRY(fuse_check_sizes(L, B, kk, ld, list_stride, weights != nullptr, ldw, fill != nullptr, ldf, mode, rrf_c, k, err_buf(), 512));
    if (mode != VS_FUSE_RAW) fill = nullptr;                                  // (read in that mode only)
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range", device);
    const void* ptrs[9] = {ids, scores, weights, fill, out_ids, out_fused, out_ranks, out_scores, out_n};
    const char* names[9] = {"ids", "scores", "weights", "fill", "out_ids", "out_fused", "out_ranks", "out_scores", "out_n"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 9, device, &dev));
    if (!dev)                                                                 // host arrays are checked here; device arrays are not read on the host
        VS_TRY(fuse_check_host(ids, L, B, kk, ld, list_stride, weights, ldw, fill, ldf, err_buf(), 512));
    VS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    Staged st[9];
    FuseArgs a{};
    int64_t* d_ids;
    float *d_sc, *d_w, *d_fill;
    const size_t n_in = (size_t)(L - 1) * (size_t)list_stride + (size_t)(B - 1) * (size_t)ld + (size_t)kk;
    const size_t n_out = (size_t)B * (size_t)k;
    VS_TRY(st[0].in(ids, n_in, dev, true, s, &d_ids));
    VS_TRY(st[1].in(scores, n_in, dev, true, s, &d_sc));
    VS_TRY(st[2].in(weights, ldw ? (size_t)(B - 1) * (size_t)ldw + (size_t)L : (size_t)L, dev, true, s, &d_w));
    VS_TRY(st[3].in(fill, (size_t)(B - 1) * (size_t)ldf + (size_t)L, dev, true, s, &d_fill));
    VS_TRY(st[4].in(out_ids, n_out, dev, false, s, &a.oi));
    VS_TRY(st[5].in(out_fused, n_out, dev, false, s, &a.of));
    VS_TRY(st[6].in(out_ranks, n_out * (size_t)L, dev, false, s, &a.orank));
    VS_TRY(st[7].in(out_scores, n_out * (size_t)L, dev, false, s, &a.osc));
    VS_TRY(st[8].in(out_n, (size_t)B, dev, false, s, &a.on));
    a.ids = d_ids; a.sc = d_sc; a.ld = ld; a.stride = list_stride; a.w = d_w; a.ldw = ldw; a.fill = d_fill; a.ldf = ldf;
    a.L = L; a.kk = kk; a.k = k; a.mode = mode; a.c = rrf_c;
    a.N = 1;
    while (a.N < L * kk) a.N <<= 1;                                           // the sort's width: at most 4096 keys
    const size_t lds = lds_bytes(a.N);
    VS_HIP(hipFuncSetAttribute((const void*)fuse_topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    {
        ProfScope prof("fuse_topk", s);
        hipLaunchKernelGGL(fuse_topk_kernel, dim3((unsigned)B), dim3(kThreads), lds, s, a);
        VS_HIP(hipGetLastError());
    }
    VS_STAGE("fuse_topk", s);
    if (!dev)
        for (int i = 4; i < 9; ++i) VS_TRY(st[i].back(s));
    if (!stream || !dev) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}
