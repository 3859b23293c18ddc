// term_filter.hip -- must / must-not / should document filters built from the index's own columns: one bitmap of rows per term
// (vs_index_term_bitmaps, vs_shard_group_term_bitmaps) and their combination into allowed-row bitmaps (vs_term_filter_combine), in the
// layout vs_index_search_filtered reads.  No reference counterpart: the reference has no filtered search.
//
// The scan (term_scan_kernel) is one pass over the packets' column ids for up to kSlots distinct terms.  A workgroup owns runs of kRunRows
// rows -- 32 bitmap words, one 128-byte line per term -- and keeps in LDS a column -> slot table of one byte per column (0xFF: no term; the
// pad id maps there), the run's row pointers and a tile [slots][32] of bitmap words.  Lanes stream the run's packets with 16-byte loads,
// look their eight ids up in the table, and only a packet with a hit finds its row (binary search of the run's row pointers), reads the
// values of the hit entries (valued stores: the non-zero / threshold test) and ORs the bit into the tile with an LDS atomic.  The tile
// leaves as whole lines.  The terms of a pass travel in the kernel's arguments, so a call with device outputs only enqueues work.
#include "common.h"
#include "new_index.h"

#include <algorithm>
#include <cmath>

using namespace vs;

namespace {

constexpr int kSlots = VS_TERM_FILTER_SLOTS;
constexpr int kRunRows = 1024;
constexpr int kRunWords = kRunRows / 32;
constexpr int kScanThreads = 512;
constexpr int kScanUnroll = 4;          // packets a lane has in flight
constexpr int kPkLds = kRunRows + 4;    // row pointers of a run (kRunRows + 1), kept 16-byte sized

int check_device(const void* p, int device, const char* what) {
    if (!is_device_ptr(p)) return VS_OK;
    hipPointerAttribute_t attr;
    VS_HIP(hipPointerGetAttributes(&attr, p));
    if (attr.device != device) return fail(VS_EINVAL, "%s lives on device %d, expected device %d", what, attr.device, device);
    return VS_OK;
}

// the distinct terms of one pass: column, threshold (NaN: none) and the first term of the call that asked for the pair
struct PassTerms {
    int32_t n;
    uint16_t col[kSlots];
    uint16_t term[kSlots];
    float thr[kSlots];
};

struct ScanArgs {
    const uint32_t* pk_ptr;
    const uint4* cols;
    const void* vals;
    const float* mat;       // dense matrix kind: [n_rows, ldp] fp32
    int32_t ldp;
    int64_t n_rows;
    int32_t n_cols;
    uint32_t* out;          // [T, ld]
    int64_t ld;
    int vec;                // out rows take 16-byte stores
    PassTerms pt;
};

__host__ __device__ inline size_t scan_lds_bytes(int32_t n_cols, int n_slots) {
    return (size_t)((n_cols + 1 + 15) & ~15) + (size_t)kPkLds * 4 + (size_t)n_slots * kRunWords * 4 + (size_t)n_slots * 4;
}

__device__ __forceinline__ bool term_test(float v, float thr) { return thr != thr ? v != 0.f : v >= thr; }

template <int SD>
__global__ __launch_bounds__(kScanThreads) void term_scan_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_t[];
    const int tb = (a.n_cols + 1 + 15) & ~15;
    uint8_t* table = reinterpret_cast<uint8_t*>(smem_t);
    uint32_t* pkl = reinterpret_cast<uint32_t*>(smem_t + tb);
    uint32_t* tile = pkl + kPkLds;
    const int tid = threadIdx.x, ns = a.pt.n;
    float* thr = reinterpret_cast<float*>(tile + ns * kRunWords);
    for (int s = tid; s < ns; s += kScanThreads) thr[s] = a.pt.thr[s];
    for (int i = tid; i < tb / 16; i += kScanThreads) reinterpret_cast<uint4*>(table)[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
    __syncthreads();
    for (int s = tid; s < ns; s += kScanThreads) table[a.pt.col[s]] = (uint8_t)s;
    const uint32_t pad = (uint32_t)a.n_cols | ((uint32_t)a.n_cols << 16);
    const int64_t n_runs = (a.n_rows + kRunRows - 1) / kRunRows;
    for (int64_t run = blockIdx.x; run < n_runs; run += gridDim.x) {
        const int64_t r0 = run * kRunRows;
        const int nr = (int)min((int64_t)kRunRows, a.n_rows - r0);
        __syncthreads();                                          // (the table is built; the previous run's tile has left)
        for (int i = tid; i <= nr; i += kScanThreads) pkl[i] = a.pk_ptr[r0 + i];
        for (int i = tid; i < ns * kRunWords; i += kScanThreads) tile[i] = 0u;
        __syncthreads();
        const uint32_t p_begin = pkl[0], p_end = pkl[nr];
        for (uint64_t pb = p_begin; pb < p_end; pb += kScanThreads * kScanUnroll) {      // (64-bit: no wrap next to 2^32 packets)
            uint4 cw[kScanUnroll];
#pragma unroll
            for (int u = 0; u < kScanUnroll; ++u) {
                const uint64_t p = pb + u * kScanThreads + tid;
                cw[u] = p < p_end ? a.cols[p] : make_uint4(pad, pad, pad, pad);
            }
#pragma unroll
            for (int u = 0; u < kScanUnroll; ++u) {
                const uint64_t p = pb + u * kScanThreads + tid;
                const uint32_t w[4] = {cw[u].x, cw[u].y, cw[u].z, cw[u].w};
                uint32_t sl[8], all = 0xFFu;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    sl[t] = table[(t & 1) ? (w[t >> 1] >> 16) : (w[t >> 1] & 0xFFFFu)];
                    all &= sl[t];
                }
                if (all == 0xFFu) continue;                       // (no id of the packet is a term: the common case)
                int lo = 0, hi = nr;                              // the row of packet p: the last one whose first packet is <= p
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (pkl[mid] <= p) lo = mid; else hi = mid;
                }
                const uint32_t bit = 1u << (lo & 31);
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    if (sl[t] == 0xFFu) continue;
                    float v = 1.f;
                    if constexpr (SD == VS_F32) v = reinterpret_cast<const float*>(a.vals)[(size_t)p * 8 + t];
                    else if constexpr (SD == VS_F16) v = __half2float(reinterpret_cast<const __half*>(a.vals)[(size_t)p * 8 + t]);
                    if (term_test(v, thr[sl[t]])) atomicOr(&tile[sl[t] * kRunWords + (lo >> 5)], bit);
                }
            }
        }
        __syncthreads();
        // the tile leaves: eight lanes a slot, 16 bytes a lane (one 128-byte line a slot); the last run of the index may end inside a line
        const int nw = (nr + 31) >> 5;
        for (int i = tid; i < ns * 8; i += kScanThreads) {
            const int s = i >> 3, q = i & 7;
            if (4 * q >= nw) continue;
            const uint32_t* src = tile + s * kRunWords + 4 * q;
            uint32_t* dst = a.out + (size_t)a.pt.term[s] * (size_t)a.ld + (size_t)run * kRunWords + 4 * q;
            if (a.vec && 4 * q + 4 <= nw) {
                *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
            } else {
                for (int j = 0; j < 4 && 4 * q + j < nw; ++j) dst[j] = src[j];
            }
        }
    }
}

// dense matrix kind: one thread a row reads the row's element of every term of the pass and votes its bit (a wave: two words).  A zero
// element is not stored (as vs_index_get_rows reports the row), so it never has the term, whatever the threshold
__global__ __launch_bounds__(256) void term_dense_kernel(ScanArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t n64 = (a.n_rows + 63) >> 6;
    for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g < n64; g += (int64_t)gridDim.x * 4) {
        const int64_t row = g * 64 + lane;
        const float* r = a.mat + (size_t)min(row, a.n_rows - 1) * (size_t)a.ldp;
        const bool two = g * 64 + 32 < a.n_rows;                  // (the second word of the pair exists)
        for (int s = 0; s < a.pt.n; ++s) {
            const float v = r[a.pt.col[s]];
            const bool on = row < a.n_rows && v != 0.f && term_test(v, a.pt.thr[s]);
            const unsigned long long m = __ballot(on);
            uint32_t* dst = a.out + (size_t)a.pt.term[s] * (size_t)a.ld + (size_t)g * 2;
            if (lane == 0) dst[0] = (uint32_t)m;
            if (lane == 32 && two) dst[1] = (uint32_t)(m >> 32);
        }
    }
}

// set bits of rows [0, n_rows) of bitmap blockIdx.y (AND live, when given): count_bits_kernel (mutable.hip) over T bitmaps
__global__ __launch_bounds__(256) void term_df_kernel(const uint32_t* words, int64_t ld, int64_t n_rows, const uint32_t* live, unsigned long long* df) {
    const int64_t nw = (n_rows + 31) >> 5;
    const uint32_t* wds = words + (size_t)blockIdx.y * (size_t)ld;
    unsigned long long c = 0;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < nw; w += (int64_t)gridDim.x * 256) {
        uint32_t v = wds[w];
        if (live) v &= live[w];
        if (w == nw - 1 && (n_rows & 31)) v &= (1u << (n_rows & 31)) - 1u;
        c += __popc(v);
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&df[blockIdx.y], c);
}

// ---- combine ------------------------------------------------------------------------------------------------------------------------
struct CombineArgs {
    const uint32_t* terms;
    int64_t ld, n_rows;
    int32_t T;
    const int32_t *must, *must_not, *should, *min_should;
    int32_t n_must, n_must_not, n_should;
    uint32_t* out;
    int64_t out_ld;
    int vec_in, vec_out;
};

__device__ __forceinline__ uint4 load_quad(const CombineArgs& a, int32_t t, int64_t q, int64_t nw) {
    const uint32_t* p = a.terms + (size_t)t * (size_t)a.ld + (size_t)q * 4;
    if (a.vec_in) return *reinterpret_cast<const uint4*>(p);
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (4 * q + 0 < nw) r.x = p[0];
    if (4 * q + 1 < nw) r.y = p[1];
    if (4 * q + 2 < nw) r.z = p[2];
    if (4 * q + 3 < nw) r.w = p[3];
    return r;
}
__device__ __forceinline__ uint4 and4(uint4 a, uint4 b) { return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w); }
__device__ __forceinline__ uint4 or4(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }
__device__ __forceinline__ uint4 xor4(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
__device__ __forceinline__ uint4 not4(uint4 a) { return make_uint4(~a.x, ~a.y, ~a.z, ~a.w); }

// A lane takes four output words of query blockIdx.y.  should: the up-to-64 words are added into a bit-sliced counter of 7 planes (a
// ripple of half adders per word) and the count is compared with min_should plane by plane; min_should == 1 is the OR.
__global__ __launch_bounds__(256) void term_combine_kernel(CombineArgs a) {
    const int64_t nw = (a.n_rows + 31) >> 5, nq = (nw + 3) >> 2;
    const int b = blockIdx.y;
    const int32_t* must = a.must + (size_t)b * a.n_must;
    const int32_t* must_not = a.must_not + (size_t)b * a.n_must_not;
    const int32_t* should = a.should + (size_t)b * a.n_should;
    const int32_t ms = a.min_should ? a.min_should[b] : 0;
    const uint4 ones = make_uint4(~0u, ~0u, ~0u, ~0u), zero = make_uint4(0u, 0u, 0u, 0u);
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        uint4 acc = ones;
        for (int j = 0; j < a.n_must; ++j) {
            const int32_t t = must[j];
            if (t >= 0 && t < a.T) acc = and4(acc, load_quad(a, t, q, nw));
        }
        uint4 deny = zero;
        for (int j = 0; j < a.n_must_not; ++j) {
            const int32_t t = must_not[j];
            if (t >= 0 && t < a.T) deny = or4(deny, load_quad(a, t, q, nw));
        }
        acc = and4(acc, not4(deny));
        if (ms == 1) {
            uint4 any = zero;
            for (int j = 0; j < a.n_should; ++j) {
                const int32_t t = should[j];
                if (t >= 0 && t < a.T) any = or4(any, load_quad(a, t, q, nw));
            }
            acc = and4(acc, any);
        } else if (ms > VS_TERM_FILTER_LIST) {
            acc = zero;
        } else if (ms > 1) {
            uint4 pl[7] = {zero, zero, zero, zero, zero, zero, zero};
            for (int j = 0; j < a.n_should; ++j) {
                const int32_t t = should[j];
                if (t < 0 || t >= a.T) continue;
                uint4 carry = load_quad(a, t, q, nw);
#pragma unroll
                for (int p = 0; p < 7; ++p) {
                    const uint4 c2 = and4(pl[p], carry);
                    pl[p] = xor4(pl[p], carry);
                    carry = c2;
                }
            }
            uint4 gt = zero, eq = ones;                           // count > ms / count == ms on the planes seen so far, from the top
#pragma unroll
            for (int p = 6; p >= 0; --p) {
                const uint4 mb = ((ms >> p) & 1) ? ones : zero;
                gt = or4(gt, and4(eq, and4(pl[p], not4(mb))));
                eq = and4(eq, not4(xor4(pl[p], mb)));
            }
            acc = and4(acc, or4(gt, eq));
        }
        uint32_t r[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t w = 4 * q + j;
            if (w >= nw) r[j] = 0u;
            else if (w == nw - 1 && (a.n_rows & 31)) r[j] &= (1u << (a.n_rows & 31)) - 1u;
        }
        uint32_t* dst = a.out + (size_t)b * (size_t)a.out_ld + (size_t)q * 4;
        if (a.vec_out) {
            *reinterpret_cast<uint4*>(dst) = make_uint4(r[0], r[1], r[2], r[3]);
        } else {
            for (int j = 0; j < 4 && 4 * q + j < nw; ++j) dst[j] = r[j];
        }
    }
}

// ---- shard groups: dst word w0 + j |= the shard's words shifted up by `sh` bits (one writer a word inside a launch; launches of the
// shards follow each other on one stream, so the seam words -- the bits of two shards -- are read-modify-written in turn) -----------
__global__ __launch_bounds__(256) void term_rebase_or_kernel(const uint32_t* src, int64_t src_ld, int64_t src_nw, uint32_t* dst, int64_t dst_ld, int64_t w0,
                                                             uint32_t sh) {
    const uint32_t* s = src + (size_t)blockIdx.y * (size_t)src_ld;
    uint32_t* d = dst + (size_t)blockIdx.y * (size_t)dst_ld + (size_t)w0;
    const int64_t n = src_nw + (sh ? 1 : 0);
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        const uint32_t lo = j > 0 ? s[j - 1] : 0u, hi = j < src_nw ? s[j] : 0u;
        const uint32_t v = __funnelshift_l(lo, hi, sh);            // (hi << sh) | (lo >> (32 - sh)); sh == 0: hi
        if (v) d[j] |= v;
    }
}

template <int SD>
int launch_scan(const ScanArgs& a, int grid, size_t lds, hipStream_t s) {
    VS_HIP(hipFuncSetAttribute((const void*)term_scan_kernel<SD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((term_scan_kernel<SD>), dim3(grid), dim3(kScanThreads), lds, s, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// cols / thr as host arrays (device arrays are read back: control data)
int host_terms(const int32_t* cols, const float* thr, int32_t T, hipStream_t s, std::vector<int32_t>& hc, std::vector<float>& ht) {
    hc.resize((size_t)T);
    ht.assign((size_t)T, NAN);
    if (is_device_ptr(cols)) {
        VS_HIP(hipMemcpyAsync(hc.data(), cols, (size_t)T * 4, hipMemcpyDeviceToHost, s));
        VS_HIP(hipStreamSynchronize(s));
    } else {
        std::copy(cols, cols + T, hc.begin());
    }
    if (thr) {
        if (is_device_ptr(thr)) {
            VS_HIP(hipMemcpyAsync(ht.data(), thr, (size_t)T * 4, hipMemcpyDeviceToHost, s));
            VS_HIP(hipStreamSynchronize(s));
        } else {
            std::copy(thr, thr + T, ht.begin());
        }
    }
    return VS_OK;
}

// The distinct (column, threshold) pairs of a call dealt to passes: a pass holds at most kSlots pairs and a column once (its table maps a
// column to one slot).  dup[t] = the earlier term whose bitmap term t repeats, or -1.
void plan_passes(const std::vector<int32_t>& cols, const std::vector<float>& thr, std::vector<PassTerms>& passes, std::vector<int32_t>& dup) {
    const int T = (int)cols.size();
    dup.assign((size_t)T, -1);
    std::map<std::pair<int32_t, uint32_t>, int> first;
    std::vector<std::map<int32_t, bool>> used;
    for (int t = 0; t < T; ++t) {
        uint32_t bits = 0x7FC00000u;                              // one NaN for "no threshold"
        if (thr[t] == thr[t]) memcpy(&bits, &thr[t], 4);
        const auto key = std::make_pair(cols[t], bits);
        const auto it = first.find(key);
        if (it != first.end()) { dup[t] = it->second; continue; }
        first[key] = t;
        size_t p = 0;
        while (p < passes.size() && (passes[p].n >= kSlots || used[p].count(cols[t]))) ++p;
        if (p == passes.size()) { passes.emplace_back(PassTerms{}); used.emplace_back(); }
        PassTerms& pt = passes[p];
        pt.col[pt.n] = (uint16_t)cols[t];
        pt.term[pt.n] = (uint16_t)t;
        memcpy(&pt.thr[pt.n], &bits, 4);
        pt.n += 1;
        used[p][cols[t]] = true;
    }
}

}  // namespace

extern "C" int vs_index_term_bitmaps(vs_index* idx, const int32_t* cols, const float* thr, int32_t T, uint32_t* out_words, int64_t ld_words,
                                     int64_t* out_df, int live_only, void* stream) {
    VS_TRY(need_device());
    if (!idx || !cols || !out_words) return fail(VS_EINVAL, "NULL argument");
    if (T < 1 || T > VS_TERM_FILTER_TERMS) return fail(VS_EINVAL, "T must be in 1..%d (got %d)", VS_TERM_FILTER_TERMS, T);
    const int64_t W = bit_words(idx->n_rows);
    if (ld_words < W) return fail(VS_EINVAL, "ld_words = %lld is shorter than the %lld words of %lld rows", (long long)ld_words, (long long)W, (long long)idx->n_rows);
    const bool dense = idx->kind != VS_KIND_CSR;
    if (!dense && idx->n_cols > 65535) return fail(VS_EUNSUPPORTED, "n_cols = %d is too wide", idx->n_cols);
    const bool out_dev = is_device_ptr(out_words);
    if (out_df && is_device_ptr(out_df) != out_dev) return fail(VS_EINVAL, "out_words and out_df must both be host or both device pointers");
    VS_TRY(check_device(out_words, idx->device, "out_words"));
    VS_TRY(check_device(out_df, idx->device, "out_df"));
    VS_HIP(hipSetDevice(idx->device));
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> hc;
    std::vector<float> ht;
    VS_TRY(host_terms(cols, thr, T, s, hc, ht));
    for (int t = 0; t < T; ++t)
        if (hc[t] < 0 || hc[t] >= idx->n_cols) return fail(VS_EINVAL, "term %d: column %d is outside [0, %d)", t, hc[t], idx->n_cols);
    if (idx->n_rows == 0) {
        if (out_df) {
            if (out_dev) VS_HIP(hipMemsetAsync(out_df, 0, (size_t)T * 8, s));
            else memset(out_df, 0, (size_t)T * 8);
        }
        if (!stream) VS_HIP(hipStreamSynchronize(s));
        return VS_OK;
    }
    std::vector<PassTerms> passes;
    std::vector<int32_t> dup;
    plan_passes(hc, ht, passes, dup);
    // host outputs: bitmaps [T, W] and counts in a buffer of the call
    DevBuf tmp;
    uint32_t* d_out = out_words;
    int64_t ld = ld_words;
    unsigned long long* d_df = reinterpret_cast<unsigned long long*>(out_df);
    if (!out_dev) {
        ld = (W + 3) / 4 * 4;
        VS_TRY(tmp.alloc((size_t)T * (size_t)ld * 4 + (size_t)T * 8));
        d_df = tmp.as<unsigned long long>();
        d_out = reinterpret_cast<uint32_t*>(tmp.as<char>() + (size_t)T * 8);
    }
    ScanArgs a{};
    a.pk_ptr = idx->pk_ptr.as<uint32_t>();
    a.cols = idx->cols.as<uint4>();
    a.vals = idx->vals.p;
    a.mat = idx->mat.as<float>();
    a.ldp = (idx->n_cols + 31) / 32 * 32;                                  // (dense.hip's row pitch)
    a.n_rows = idx->n_rows;
    a.n_cols = idx->n_cols;
    a.out = d_out;
    a.ld = ld;
    a.vec = (reinterpret_cast<uintptr_t>(d_out) % 16 == 0 && ld % 4 == 0) ? 1 : 0;
    {
        ProfScope prof("term_scan", s);
        for (const PassTerms& pt : passes) {
            a.pt = pt;
            if (dense) {
                hipLaunchKernelGGL(term_dense_kernel, dim3(grid_for((idx->n_rows + 63) / 64, 4, (int64_t)idx->cu_count * 8)), dim3(256), 0, s, a);
                VS_HIP(hipGetLastError());
                continue;
            }
            const size_t lds = scan_lds_bytes(idx->n_cols, pt.n);
            const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / lds));
            const int64_t n_runs = (idx->n_rows + kRunRows - 1) / kRunRows;
            const int grid = (int)std::min<int64_t>(n_runs, (int64_t)idx->cu_count * per_cu);
            if (idx->store_dtype == VS_F32) VS_TRY(launch_scan<VS_F32>(a, grid, lds, s));
            else if (idx->store_dtype == VS_F16) VS_TRY(launch_scan<VS_F16>(a, grid, lds, s));
            else VS_TRY(launch_scan<VS_NONE>(a, grid, lds, s));
        }
    }
    VS_STAGE("term_scan", s);
    for (int t = 0; t < T; ++t)                                            // a repeated term: a copy of its first bitmap
        if (dup[t] >= 0)
            VS_HIP(hipMemcpyAsync(d_out + (size_t)t * (size_t)ld, d_out + (size_t)dup[t] * (size_t)ld, (size_t)W * 4, hipMemcpyDeviceToDevice, s));
    if (out_df) {
        VS_HIP(hipMemsetAsync(d_df, 0, (size_t)T * 8, s));
        const uint32_t* live = (live_only && idx->has_tomb) ? idx->live.as<uint32_t>() : nullptr;
        hipLaunchKernelGGL(term_df_kernel, dim3(grid_for(W, 256, 256), (unsigned)T), dim3(256), 0, s, d_out, ld, idx->n_rows, live, d_df);
        VS_HIP(hipGetLastError());
    }
    if (!out_dev) {
        VS_HIP(hipMemcpy2DAsync(out_words, (size_t)ld_words * 4, d_out, (size_t)ld * 4, (size_t)W * 4, (size_t)T, hipMemcpyDeviceToHost, s));
        if (out_df) VS_HIP(hipMemcpyAsync(out_df, d_df, (size_t)T * 8, hipMemcpyDeviceToHost, s));
    }
    if (!stream || tmp.p) VS_HIP(hipStreamSynchronize(s));                 // blocking call / the call's buffer dies here
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}

extern "C" int vs_term_filter_combine(const uint32_t* term_words, int64_t ld_words, int64_t n_rows, int32_t T, const int32_t* must, int32_t n_must,
                                      const int32_t* must_not, int32_t n_must_not, const int32_t* should, int32_t n_should,
                                      const int32_t* min_should, int32_t B, uint32_t* out_words, int64_t out_ld, int device, void* stream) {
    VS_TRY(need_device());
    if (!out_words) return fail(VS_EINVAL, "NULL argument");
    if (B < 1 || B > 65535) return fail(VS_EINVAL, "B must be in 1..65535 (got %d)", B);
    if (n_rows < 1) return fail(VS_EINVAL, "n_rows must be positive");
    if (T < 0 || T > VS_TERM_FILTER_TERMS) return fail(VS_EINVAL, "T must be in 0..%d (got %d)", VS_TERM_FILTER_TERMS, T);
    const int32_t ns[3] = {n_must, n_must_not, n_should};
    const int32_t* lists[3] = {must, must_not, should};
    const char* names[3] = {"must", "must_not", "should"};
    for (int i = 0; i < 3; ++i) {
        if (ns[i] < 0 || ns[i] > VS_TERM_FILTER_LIST) return fail(VS_EINVAL, "%s: at most %d entries a query (got %d)", names[i], VS_TERM_FILTER_LIST, ns[i]);
        if (ns[i] > 0 && !lists[i]) return fail(VS_EINVAL, "%s is NULL with %d entries a query", names[i], ns[i]);
    }
    if (T > 0 && !term_words) return fail(VS_EINVAL, "term_words is NULL");
    const int64_t W = bit_words(n_rows);
    if (T > 0 && ld_words < W) return fail(VS_EINVAL, "ld_words = %lld is shorter than the %lld words of %lld rows", (long long)ld_words, (long long)W, (long long)n_rows);
    if (out_ld < W) return fail(VS_EINVAL, "out_ld = %lld is shorter than the %lld words of %lld rows", (long long)out_ld, (long long)W, (long long)n_rows);
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range (have %d)", device, ndev);
    const bool dev = is_device_ptr(out_words);
    const void* ptrs[6] = {term_words, must, must_not, should, min_should, out_words};
    for (const void* p : ptrs) {
        if (p && is_device_ptr(p) != dev) return fail(VS_EINVAL, "the pointers must all be host or all device pointers");
        VS_TRY(check_device(p, device, "a pointer"));
    }
    if (!dev)
        for (int i = 0; i < 3; ++i)
            for (int64_t j = 0; j < (int64_t)B * ns[i]; ++j)
                if (lists[i][j] < -1 || lists[i][j] >= T) return fail(VS_EINVAL, "%s: index %d is outside [-1, %d)", names[i], lists[i][j], T);
    VS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    CombineArgs a{};
    a.ld = ld_words;
    a.n_rows = n_rows;
    a.T = T;
    a.n_must = n_must;
    a.n_must_not = n_must_not;
    a.n_should = n_should;
    a.out_ld = out_ld;
    DevBuf tmp;
    if (dev) {
        a.terms = term_words;
        a.must = must;
        a.must_not = must_not;
        a.should = should;
        a.min_should = min_should;
        a.out = out_words;
    } else {
        const size_t ld4 = (size_t)(W + 3) / 4 * 4;
        const size_t sz_terms = (size_t)T * ld4 * 4, sz_out = (size_t)B * ld4 * 4;
        size_t sz_l[3], off = sz_terms + sz_out;
        for (int i = 0; i < 3; ++i) sz_l[i] = ((size_t)B * ns[i] * 4 + 15) / 16 * 16;
        VS_TRY(tmp.alloc(off + sz_l[0] + sz_l[1] + sz_l[2] + (size_t)B * 4 + 16));
        char* p = tmp.as<char>();
        if (T > 0) VS_HIP(hipMemcpy2DAsync(p, ld4 * 4, term_words, (size_t)ld_words * 4, (size_t)W * 4, (size_t)T, hipMemcpyHostToDevice, s));
        a.terms = reinterpret_cast<const uint32_t*>(p);
        a.ld = (int64_t)ld4;
        a.out = reinterpret_cast<uint32_t*>(p + sz_terms);
        a.out_ld = (int64_t)ld4;
        const int32_t** dst[3] = {&a.must, &a.must_not, &a.should};
        for (int i = 0; i < 3; ++i) {
            if (ns[i] > 0) VS_HIP(hipMemcpyAsync(p + off, lists[i], (size_t)B * ns[i] * 4, hipMemcpyHostToDevice, s));
            *dst[i] = reinterpret_cast<const int32_t*>(p + off);
            off += sz_l[i];
        }
        if (min_should) {
            VS_HIP(hipMemcpyAsync(p + off, min_should, (size_t)B * 4, hipMemcpyHostToDevice, s));
            a.min_should = reinterpret_cast<const int32_t*>(p + off);
        }
    }
    a.vec_in = (T > 0 && reinterpret_cast<uintptr_t>(a.terms) % 16 == 0 && a.ld % 4 == 0) ? 1 : 0;
    a.vec_out = (reinterpret_cast<uintptr_t>(a.out) % 16 == 0 && a.out_ld % 4 == 0) ? 1 : 0;
    {
        ProfScope prof("term_combine", s);
        hipLaunchKernelGGL(term_combine_kernel, dim3(grid_for((W + 3) / 4, 256, 2048), (unsigned)B), dim3(256), 0, s, a);
        VS_HIP(hipGetLastError());
    }
    VS_STAGE("term_combine", s);
    if (!dev) VS_HIP(hipMemcpy2DAsync(out_words, (size_t)out_ld * 4, a.out, (size_t)a.out_ld * 4, (size_t)W * 4, (size_t)B, hipMemcpyDeviceToHost, s));
    if (!stream || tmp.p) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}

// ---- shard groups (api.hip binds it to vs_shard_group) ---------------------------------------------------------------------------------
int vs_shard_group_term_bitmaps_impl(const std::vector<vs_index*>& shards, const std::vector<int64_t>& row0, const std::vector<hipStream_t>& streams,
                                     const int32_t* cols, const float* thr, int32_t T, uint32_t* out_words, int64_t ld_words, int64_t* out_df,
                                     int live_only) {
    VS_TRY(need_device());
    if (!cols || !out_words) return fail(VS_EINVAL, "NULL argument");
    if (T < 1 || T > VS_TERM_FILTER_TERMS) return fail(VS_EINVAL, "T must be in 1..%d (got %d)", VS_TERM_FILTER_TERMS, T);
    const int n = (int)shards.size();
    const int64_t n_total = row0[n - 1] + shards[n - 1]->n_rows;
    const int64_t W = bit_words(n_total);
    if (ld_words < W) return fail(VS_EINVAL, "ld_words = %lld is shorter than the %lld words of %lld rows", (long long)ld_words, (long long)W, (long long)n_total);
    const int dev0 = shards[0]->device;
    const bool out_dev = is_device_ptr(out_words);
    if (out_df && is_device_ptr(out_df) != out_dev) return fail(VS_EINVAL, "out_words and out_df must both be host or both device pointers");
    VS_TRY(check_device(out_words, dev0, "out_words"));
    VS_TRY(check_device(out_df, dev0, "out_df"));
    VS_HIP(hipSetDevice(dev0));
    if (out_dev) VS_HIP(hipDeviceSynchronize());                           // (work the caller queued on the output buffers: the group runs on its own streams)
    std::vector<int32_t> hc;
    std::vector<float> ht;
    VS_TRY(host_terms(cols, thr, T, streams[0], hc, ht));
    for (int t = 0; t < T; ++t)
        if (hc[t] < 0 || hc[t] >= shards[0]->n_cols) return fail(VS_EINVAL, "term %d: column %d is outside [0, %d)", t, hc[t], shards[0]->n_cols);
    // 1. every shard scans its rows on its own device and stream
    std::vector<DevBuf> bw((size_t)n);
    std::vector<int64_t> ldi((size_t)n, 0);
    std::vector<hipEvent_t> ev((size_t)n, nullptr);
    struct EvGuard { std::vector<hipEvent_t>& e; ~EvGuard() { for (auto x : e) if (x) (void)hipEventDestroy(x); } } evg{ev};
    for (int i = 0; i < n; ++i) {
        vs_index* sh = shards[i];
        if (sh->n_rows == 0) continue;
        VS_HIP(hipSetDevice(sh->device));
        ldi[i] = (bit_words(sh->n_rows) + 3) / 4 * 4;
        VS_TRY(bw[i].alloc((size_t)T * (size_t)ldi[i] * 4 + (out_df ? (size_t)T * 8 : 0)));
        int64_t* dfi = out_df ? reinterpret_cast<int64_t*>(bw[i].as<char>() + (size_t)T * (size_t)ldi[i] * 4) : nullptr;
        VS_TRY(vs_index_term_bitmaps(sh, hc.data(), thr ? ht.data() : nullptr, T, bw[i].as<uint32_t>(), ldi[i], dfi, live_only, (void*)streams[i]));
        VS_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        VS_HIP(hipEventRecord(ev[i], streams[i]));
    }
    // 2. the first shard's device ORs every shard's words in at the shard's first global row
    VS_HIP(hipSetDevice(dev0));
    hipStream_t st0 = streams[0];
    DevBuf g, stage;
    uint32_t* d_out = out_words;
    int64_t ld = ld_words;
    if (!out_dev) {
        ld = (W + 3) / 4 * 4;
        VS_TRY(g.alloc((size_t)T * (size_t)ld * 4));
        d_out = g.as<uint32_t>();
    }
    VS_HIP(hipMemset2DAsync(d_out, (size_t)ld * 4, 0, (size_t)W * 4, (size_t)T, st0));
    std::vector<int64_t> df((size_t)T, 0), dfh((size_t)T);
    for (int i = 0; i < n; ++i) {
        if (shards[i]->n_rows == 0) continue;
        VS_HIP(hipStreamWaitEvent(st0, ev[i], 0));
        const uint32_t* src = bw[i].as<uint32_t>();
        if (shards[i]->device != dev0) {
            VS_TRY(stage.reserve((size_t)T * (size_t)ldi[i] * 4));
            VS_HIP(hipMemcpyAsync(stage.p, src, (size_t)T * (size_t)ldi[i] * 4, hipMemcpyDefault, st0));
            src = stage.as<uint32_t>();
        }
        const int64_t nw = bit_words(shards[i]->n_rows);
        hipLaunchKernelGGL(term_rebase_or_kernel, dim3(grid_for(nw + 1, 256, 1024), (unsigned)T), dim3(256), 0, st0, src, ldi[i], nw, d_out, ld, row0[i] >> 5,
                           (uint32_t)(row0[i] & 31));
        VS_HIP(hipGetLastError());
        if (out_df) {
            VS_HIP(hipMemcpyAsync(dfh.data(), bw[i].as<char>() + (size_t)T * (size_t)ldi[i] * 4, (size_t)T * 8, hipMemcpyDefault, st0));
            VS_HIP(hipStreamSynchronize(st0));
            for (int t = 0; t < T; ++t) df[(size_t)t] += dfh[(size_t)t];
        }
    }
    if (!out_dev) VS_HIP(hipMemcpy2DAsync(out_words, (size_t)ld_words * 4, d_out, (size_t)ld * 4, (size_t)W * 4, (size_t)T, hipMemcpyDeviceToHost, st0));
    if (out_df) {
        if (out_dev) VS_HIP(hipMemcpyAsync(out_df, df.data(), (size_t)T * 8, hipMemcpyHostToDevice, st0));
        else std::copy(df.begin(), df.end(), out_df);
    }
    for (int i = 0; i < n; ++i) { VS_HIP(hipSetDevice(shards[i]->device)); VS_HIP(hipStreamSynchronize(streams[i])); }
    VS_HIP(hipSetDevice(dev0));
    return VS_OK;
}
