// by_example.hip -- query by example: stored index rows as queries (vs_index_get_rows, vs_index_queries_from_rows, vs_topk_exclude and
// their shard-group versions).
//
// (a) Row extract: the stored rows of a list of ids as a compact CSR (int32 columns ascending, fp32 values; fp16 widens exactly, a binary
//     index gives 1).  A length pass (one wave per id: packets x 8 minus the padding cells of the row's last packet -- padding, column
//     n_cols, only sits at the end of a row -- or the non-zeros of a `mat` row) and a one-workgroup exclusive scan give the rowptr; the copy
//     is one wave per id with a lane per packet, cell t of packet p landing at 8 (p - first packet) + t.
// (b) Accumulate: out[b, c] = fl32(alpha * q[b, c]), then for j = 0 .. m-1 (skipping id -1) acc[c] = fl32(acc[c] + fl32(w[b, j] * v[j, c]))
//     over the stored columns of row ids[b, j].  One workgroup per query holds an fp32 LDS image of a column tile; the threads take distinct
//     cells of row j (the columns of a row are distinct: no conflicts) and a barrier separates the rows, so every column sees the rows in
//     j order.  No atomics, no contraction to fma: the numbers are those of a numpy loop in float32.  The rows come from the index itself
//     (CSR packets or `mat`) or from staged compact rows of (a) (shard groups); both do the same fl32 operations in the same order.
// (c) Exclude: drop each query's example ids from its top kk (one wave per query: ballot + mbcnt compaction), keep the first k, pad with
//     id -1 / score -inf.  Under the canonical order the top k of "all rows minus E" lies inside the top k + |E|: exact.
#include "common.h"
#include "csr_scan.h"
#include "new_index.h"

#include <algorithm>

using namespace vs;

namespace {

constexpr int kRowWaves = 4;              // get_rows: waves (ids) per workgroup
constexpr int kAccThreads = 1024;
constexpr int kAccTileCols = 32768;       // columns of the LDS image (128 KiB of the CU's 160 KiB)
constexpr int kExclMaxM = 16384;          // example ids a query may exclude (their LDS copy: 128 KiB)

enum : int { SRC_PK = 0, SRC_MAT = 1, SRC_STAGED = 2 };

// where an index keeps its rows
struct RowSrc {
    const uint32_t* pk_ptr;   // CSR packets
    const uint16_t* cols;
    const void* vals;
    int store_dtype;
    const float* mat;         // MFMA dense kind: fp32 [n_rows, ldp]
    int32_t ldp;
    int32_t n_cols;
    int64_t n_rows;
    int dense;
};

RowSrc row_src(const vs_index* idx) {
    RowSrc s{};
    s.pk_ptr = idx->pk_ptr.as<uint32_t>();
    s.cols = idx->cols.as<uint16_t>();
    s.vals = idx->vals.p;
    s.store_dtype = idx->store_dtype;
    s.mat = idx->mat.as<float>();
    s.ldp = (idx->n_cols + 31) / 32 * 32;                                    // (dense.hip's row pitch)
    s.n_cols = idx->n_cols;
    s.n_rows = idx->n_rows;
    s.dense = idx->kind != VS_KIND_CSR;
    return s;
}

// ---- (a) row extract ----------------------------------------------------------------------------------------------------------------
// len[i] = stored entries of row ids[i] - id_offset; 0 for id -1 and for ids outside the index (strict: those also set *bad)
__global__ __launch_bounds__(kRowWaves * 64) void rows_len_kernel(RowSrc s, const int64_t* ids, int64_t n, int64_t id_offset, int strict,
                                                                  int64_t* len, int* bad) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kRowWaves + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t id = ids[i];
    const int64_t row = id - id_offset;
    int64_t cnt = 0;
    if (id != -1 && row >= 0 && row < s.n_rows) {
        if (!s.dense) {
            const uint32_t p0 = s.pk_ptr[row], p1 = s.pk_ptr[row + 1];
            if (p1 > p0) {
                const bool pad = lane < 8 && s.cols[(size_t)(p1 - 1) * 8 + lane] == (uint16_t)s.n_cols;
                cnt = (int64_t)(p1 - p0) * 8 - __popcll(__ballot(pad));
            }
        } else {
            const float* r = s.mat + (size_t)row * s.ldp;
            int c = 0;
            for (int j = lane; j < s.n_cols; j += 64) c += r[j] != 0.f;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            cnt = c;
        }
    } else if (id != -1 && strict && lane == 0) {
        *bad = 1;
    }
    if (lane == 0) len[i] = cnt;
}

// rp[0] = 0, rp[i + 1] = len[0] + ... + len[i]  (one workgroup)
__global__ __launch_bounds__(1024) void scan_len_kernel(const int64_t* len, int64_t n, int64_t* rp) {
    __shared__ int64_t wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) rp[0] = 0;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        const int64_t x = i < n ? len[i] : 0;
        int64_t incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        int64_t off = carry, tot = carry;
        for (int j = 0; j < 16; ++j) {
            if (j < w) off += wsum[j];
            tot += wsum[j];
        }
        if (i < n) rp[i + 1] = off + incl;
        __syncthreads();
        carry = tot;
    }
}

// the rows of ids into rp's positions (rows that are not this index's stay empty)
__global__ __launch_bounds__(kRowWaves * 64) void rows_copy_kernel(RowSrc s, const int64_t* ids, int64_t n, int64_t id_offset, const int64_t* rp,
                                                                   int32_t* out_cols, float* out_vals) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kRowWaves + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t id = ids[i];
    const int64_t row = id - id_offset;
    if (id == -1 || row < 0 || row >= s.n_rows) return;
    const int64_t o0 = rp[i], len = rp[i + 1] - o0;
    if (!s.dense) {
        const uint32_t p0 = s.pk_ptr[row], p1 = s.pk_ptr[row + 1];
        const uint4* cw4 = reinterpret_cast<const uint4*>(s.cols);
        for (uint32_t p = p0 + lane; p < p1; p += 64) {
            const uint4 cw = cw4[p];
            const uint32_t cwv[4] = {cw.x, cw.y, cw.z, cw.w};
            float v[8];
            if (s.store_dtype == VS_F32) {
                const float4* vp = reinterpret_cast<const float4*>(s.vals);
                const float4 v0 = vp[2 * (size_t)p], v1 = vp[2 * (size_t)p + 1];
                v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
            } else if (s.store_dtype == VS_F16) {
                const uint4 hv = reinterpret_cast<const uint4*>(s.vals)[p];
                const __half2* h = reinterpret_cast<const __half2*>(&hv);
#pragma unroll
                for (int t = 0; t < 4; ++t) { const float2 x = __half22float2(h[t]); v[2 * t] = x.x; v[2 * t + 1] = x.y; }
            } else {
#pragma unroll
                for (int t = 0; t < 8; ++t) v[t] = 1.f;
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const uint32_t c = (t & 1) ? (cwv[t >> 1] >> 16) : (cwv[t >> 1] & 0xFFFFu);
                const int64_t pos = (int64_t)(p - p0) * 8 + t;
                if (c < (uint32_t)s.n_cols && pos < len) {
                    out_cols[o0 + pos] = (int32_t)c;
                    out_vals[o0 + pos] = v[t];
                }
            }
        }
    } else {
        const float* r = s.mat + (size_t)row * s.ldp;
        int64_t base = 0;
        for (int j0 = 0; j0 < s.n_cols; j0 += 64) {
            const int j = j0 + lane;
            const float x = j < s.n_cols ? r[j] : 0.f;
            const bool on = x != 0.f;
            const unsigned long long m = __ballot(on);
            const int64_t pos = base + __popcll(m & ((1ull << lane) - 1ull));
            if (on && pos < len) {
                out_cols[o0 + pos] = j;
                out_vals[o0 + pos] = x;
            }
            base += __popcll(m);
        }
    }
}

// shard groups: len[i] += the length of row i in one shard's rowptr
__global__ void add_len_kernel(const int64_t* rp, int64_t n, int64_t* len) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) len[i] += rp[i + 1] - rp[i];
}

// shard groups: the rows one shard extracted (its rowptr rp, empty where it owns no row) into the group's positions g_rp
__global__ __launch_bounds__(256) void stitch_rows_kernel(const int64_t* rp, const int32_t* cols, const float* vals, int64_t n, const int64_t* g_rp,
                                                          int32_t* out_cols, float* out_vals) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4) {
        const int64_t s0 = rp[i], len = rp[i + 1] - s0, d0 = g_rp[i];
        for (int64_t e = lane; e < len; e += 64) {
            out_cols[d0 + e] = cols[s0 + e];
            out_vals[d0 + e] = vals[s0 + e];
        }
    }
}

// ---- (b) accumulate ----------------------------------------------------------------------------------------------------------------
struct AccArgs {
    RowSrc s;                 // SRC_PK / SRC_MAT
    const int64_t* st_rp;     // SRC_STAGED: the rows of ids [B, m] (row b * m + j), from (a)
    const int32_t* st_cols;
    const float* st_vals;
    const int64_t* ids;       // [B, ld_ids]
    int64_t ld_ids;
    int32_t B, m;
    const float* w;           // [B, ldw] or null (1)
    int64_t ldw;
    const void* q;            // [B, ldq] fp32 | fp16, or null (0)
    int q_f16;
    int64_t ldq;
    float alpha;
    float* out;               // [B, ldo]
    int64_t ldo;
    int32_t n_cols;
    int32_t tile;             // columns of the LDS image
};

template <int VM>
__device__ __forceinline__ float pk_value(const void* vals, size_t e) {
    if constexpr (VM == VM_F32) return reinterpret_cast<const float*>(vals)[e];
    else if constexpr (VM == VM_F16) return __half2float(reinterpret_cast<const __half*>(vals)[e]);
    else return 1.f;
}

template <int SRC, int VM>
__global__ __launch_bounds__(kAccThreads) void acc_rows_kernel(AccArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float img_a[];
    const int tid = threadIdx.x;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        for (int c0 = 0; c0 < a.n_cols; c0 += a.tile) {
            const int c1 = min(a.n_cols, c0 + a.tile);
            __syncthreads();                                              // (the previous tile's stores are done)
            for (int c = c0 + tid; c < c1; c += kAccThreads) {
                float x = 0.f;
                if (a.q) {
                    const size_t e = (size_t)b * a.ldq + c;
                    const float qv = a.q_f16 ? __half2float(reinterpret_cast<const __half*>(a.q)[e]) : reinterpret_cast<const float*>(a.q)[e];
                    x = a.alpha * qv;
                }
                img_a[c - c0] = x;
            }
            __syncthreads();
            for (int j = 0; j < a.m; ++j) {
                const int64_t id = a.ids[(size_t)b * a.ld_ids + j];
                if (id == -1) continue;                                   // (uniform across the workgroup)
                const float wj = a.w ? a.w[(size_t)b * a.ldw + j] : 1.f;
                if constexpr (SRC == SRC_PK) {
                    if (id < 0 || id >= a.s.n_rows) continue;
                    const size_t e0 = (size_t)a.s.pk_ptr[id] * 8, e1 = (size_t)a.s.pk_ptr[id + 1] * 8;
                    for (size_t e = e0 + tid; e < e1; e += kAccThreads) {
                        const int c = a.s.cols[e];                         // (padding: column n_cols, outside every tile)
                        if (c >= c0 && c < c1) img_a[c - c0] = img_a[c - c0] + wj * pk_value<VM>(a.s.vals, e);
                    }
                } else if constexpr (SRC == SRC_MAT) {
                    if (id < 0 || id >= a.s.n_rows) continue;
                    const float* r = a.s.mat + (size_t)id * a.s.ldp;
                    for (int c = c0 + tid; c < c1; c += kAccThreads) {
                        const float v = r[c];
                        if (v != 0.f) img_a[c - c0] = img_a[c - c0] + wj * v;
                    }
                } else {
                    const size_t r = (size_t)b * a.m + j;
                    const int64_t e0 = a.st_rp[r], e1 = a.st_rp[r + 1];
                    for (int64_t e = e0 + tid; e < e1; e += kAccThreads) {
                        const int c = a.st_cols[e];
                        if (c >= c0 && c < c1) img_a[c - c0] = img_a[c - c0] + wj * a.st_vals[e];
                    }
                }
                __syncthreads();                                          // (row j is in before row j + 1 touches a column)
            }
            float* o = a.out + (size_t)b * a.ldo;
            for (int c = c0 + tid; c < c1; c += kAccThreads) o[c] = img_a[c - c0];
        }
    }
}

template <int SRC, int VM>
int launch_acc(const AccArgs& a, int grid, hipStream_t s) {
    const size_t lds = (size_t)a.tile * 4;
    VS_HIP(hipFuncSetAttribute((const void*)acc_rows_kernel<SRC, VM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((acc_rows_kernel<SRC, VM>), dim3(grid), dim3(kAccThreads), lds, s, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// ---- (c) exclude -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void topk_exclude_kernel(const int64_t* ids, const float* sc, int32_t kk, int64_t ld, const int64_t* excl, int32_t m,
                                                          int64_t ld_excl, int32_t k, int64_t* out_ids, float* out_sc) {
    extern __shared__ int64_t ex_sh[];
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    for (int j = lane; j < m; j += 64) ex_sh[j] = excl[b * ld_excl + j];
    __syncthreads();
    int cnt = 0;
    for (int i0 = 0; i0 < kk && cnt < k; i0 += 64) {
        const int i = i0 + lane;
        int64_t id = -1;
        float s = -INFINITY;
        bool keep = false;
        if (i < kk) {
            id = ids[b * ld + i];
            s = sc[b * ld + i];
            keep = true;
            if (id != -1)                                                 // (padding stays; an excluded -1 is no id)
                for (int j = 0; j < m; ++j)
                    if (ex_sh[j] == id) { keep = false; break; }
        }
        const unsigned long long mk = __ballot(keep);
        const int pos = cnt + __popcll(mk & ((1ull << lane) - 1ull));
        if (keep && pos < k) { out_ids[b * k + pos] = id; out_sc[b * k + pos] = s; }
        cnt += __popcll(mk);
    }
    for (int p = cnt + lane; p < k; p += 64) { out_ids[b * k + p] = -1; out_sc[b * k + p] = -INFINITY; }
}

// ---- host helpers ------------------------------------------------------------------------------------------------------------------
int device_of(const void* p, int* d) {
    hipPointerAttribute_t attr;
    VS_HIP(hipPointerGetAttributes(&attr, p));
    *d = attr.device;
    return VS_OK;
}

int check_on(const void* p, int device, const char* what) {
    if (!is_device_ptr(p)) return VS_OK;
    int d = 0;
    VS_TRY(device_of(p, &d));
    if (d != device) return fail(VS_EINVAL, "%s lives on device %d, the index on device %d", what, d, device);
    return VS_OK;
}

// the outputs must be all host or all device pointers; -> *dev
int outputs_kind(const void* const* outs, int n, bool* dev) {
    const void* first = nullptr;
    for (int i = 0; i < n && !first; ++i) first = outs[i];
    *dev = is_device_ptr(first);
    for (int i = 0; i < n; ++i)
        if (outs[i] && is_device_ptr(outs[i]) != *dev) return fail(VS_EINVAL, "the outputs must all be host or all device pointers");
    return VS_OK;
}

// lengths + scan of the rows of d_ids (device, on idx's device and stream) into d_rp [n + 1]; *nnz = d_rp[n].  Blocking (reads nnz back).
int rows_rowptr(const vs_index* idx, const int64_t* d_ids, int64_t n, int64_t id_offset, int strict, hipStream_t s, DevBuf& d_rp, int64_t* nnz) {
    DevBuf d_len, d_bad;
    VS_TRY(d_rp.alloc((size_t)(n + 1) * 8));
    VS_TRY(d_len.alloc(std::max<size_t>((size_t)n * 8, 8)));
    VS_TRY(d_bad.alloc(4));
    VS_HIP(hipMemsetAsync(d_bad.p, 0, 4, s));
    if (n > 0) {
        hipLaunchKernelGGL(rows_len_kernel, dim3((unsigned)ceil_div64(n, kRowWaves)), dim3(kRowWaves * 64), 0, s, row_src(idx), d_ids, n, id_offset, strict,
                           d_len.as<int64_t>(), d_bad.as<int>());
        VS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(scan_len_kernel, dim3(1), dim3(1024), 0, s, (const int64_t*)d_len.as<int64_t>(), n, d_rp.as<int64_t>());
    VS_HIP(hipGetLastError());
    int bad = 0;
    VS_HIP(hipMemcpyAsync(nnz, d_rp.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, s));
    VS_HIP(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));
    if (bad) return fail(VS_EINVAL, "a document id is outside [-1, %lld)", (long long)(id_offset + idx->n_rows));
    return VS_OK;
}

int rows_copy(const vs_index* idx, const int64_t* d_ids, int64_t n, int64_t id_offset, const int64_t* d_rp, int32_t* d_cols, float* d_vals, hipStream_t s) {
    if (n <= 0) return VS_OK;
    hipLaunchKernelGGL(rows_copy_kernel, dim3((unsigned)ceil_div64(n, kRowWaves)), dim3(kRowWaves * 64), 0, s, row_src(idx), d_ids, n, id_offset, d_rp, d_cols, d_vals);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// host or device ids -> a device pointer on `device` (a copy in `stage` unless they already live there)
int ids_on(const int64_t* ids, size_t bytes, int device, DevBuf& stage, hipStream_t s, const int64_t** out) {
    if (is_device_ptr(ids)) {
        int d = 0;
        VS_TRY(device_of(ids, &d));
        if (d == device) { *out = ids; return VS_OK; }
        VS_TRY(stage.alloc(bytes));
        VS_HIP(hipMemcpyPeerAsync(stage.p, device, ids, d, bytes, s));
    } else {
        VS_TRY(stage.alloc(bytes));
        VS_HIP(hipMemcpyAsync(stage.p, ids, bytes, hipMemcpyHostToDevice, s));
    }
    *out = stage.as<int64_t>();
    return VS_OK;
}

// the group's rows of host ids [n] on the first shard's device: g_rp [n + 1], and with `copy` g_cols / g_vals [nnz]
int group_rows(const std::vector<vs_index*>& shards, const std::vector<int64_t>& row0, const std::vector<hipStream_t>& streams, const int64_t* h_ids,
               int64_t n, bool copy, DevBuf& g_rp, DevBuf& g_cols, DevBuf& g_vals, int64_t* nnz) {
    const int ns = (int)shards.size();
    const int dev0 = shards[0]->device;
    std::vector<DevBuf> b_ids((size_t)ns), b_rp((size_t)ns), b_cols((size_t)ns), b_vals((size_t)ns);
    std::vector<int64_t> nnz_i((size_t)ns, 0);
    for (int i = 0; i < ns; ++i) {
        vs_index* sh = shards[i];
        VS_HIP(hipSetDevice(sh->device));
        VS_TRY(b_ids[i].alloc(std::max<size_t>((size_t)n * 8, 8)));
        if (n > 0) VS_HIP(hipMemcpyAsync(b_ids[i].p, h_ids, (size_t)n * 8, hipMemcpyHostToDevice, streams[i]));
        VS_TRY(rows_rowptr(sh, b_ids[i].as<int64_t>(), n, row0[i], 0, streams[i], b_rp[i], &nnz_i[i]));
        if (copy && nnz_i[i] > 0) {
            VS_TRY(b_cols[i].alloc((size_t)nnz_i[i] * 4));
            VS_TRY(b_vals[i].alloc((size_t)nnz_i[i] * 4));
            VS_TRY(rows_copy(sh, b_ids[i].as<int64_t>(), n, row0[i], b_rp[i].as<int64_t>(), b_cols[i].as<int32_t>(), b_vals[i].as<float>(), streams[i]));
        }
    }
    for (int i = 0; i < ns; ++i) { VS_HIP(hipSetDevice(shards[i]->device)); VS_HIP(hipStreamSynchronize(streams[i])); }
    // on the first shard's device: every id's length is its owner's; scan; each shard's rows into their places
    VS_HIP(hipSetDevice(dev0));
    hipStream_t st0 = streams[0];
    DevBuf len, stage_rp, stage_c, stage_v;
    VS_TRY(len.alloc(std::max<size_t>((size_t)n * 8, 8)));
    VS_HIP(hipMemsetAsync(len.p, 0, std::max<size_t>((size_t)n * 8, 8), st0));
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(n, 256), 4096));
    for (int i = 0; i < ns; ++i) {
        const int64_t* rp = b_rp[i].as<int64_t>();
        if (shards[i]->device != dev0) {
            VS_TRY(stage_rp.reserve((size_t)(n + 1) * 8));
            VS_HIP(hipMemcpyAsync(stage_rp.p, rp, (size_t)(n + 1) * 8, hipMemcpyDefault, st0));
            rp = stage_rp.as<int64_t>();
        }
        if (n > 0) hipLaunchKernelGGL(add_len_kernel, dim3(grid), dim3(256), 0, st0, rp, n, len.as<int64_t>());
        VS_HIP(hipGetLastError());
    }
    VS_TRY(g_rp.alloc((size_t)(n + 1) * 8));
    hipLaunchKernelGGL(scan_len_kernel, dim3(1), dim3(1024), 0, st0, (const int64_t*)len.as<int64_t>(), n, g_rp.as<int64_t>());
    VS_HIP(hipGetLastError());
    VS_HIP(hipMemcpyAsync(nnz, g_rp.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, st0));
    VS_HIP(hipStreamSynchronize(st0));
    if (!copy) return VS_OK;
    VS_TRY(g_cols.alloc(std::max<size_t>((size_t)*nnz * 4, 4)));
    VS_TRY(g_vals.alloc(std::max<size_t>((size_t)*nnz * 4, 4)));
    const unsigned grid_w = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(n, 4), 65536));
    for (int i = 0; i < ns; ++i) {
        if (nnz_i[i] == 0) continue;
        const int64_t* rp = b_rp[i].as<int64_t>();
        const int32_t* c = b_cols[i].as<int32_t>();
        const float* v = b_vals[i].as<float>();
        if (shards[i]->device != dev0) {
            VS_TRY(stage_rp.reserve((size_t)(n + 1) * 8));
            VS_TRY(stage_c.reserve((size_t)nnz_i[i] * 4));
            VS_TRY(stage_v.reserve((size_t)nnz_i[i] * 4));
            VS_HIP(hipMemcpyAsync(stage_rp.p, rp, (size_t)(n + 1) * 8, hipMemcpyDefault, st0));
            VS_HIP(hipMemcpyAsync(stage_c.p, c, (size_t)nnz_i[i] * 4, hipMemcpyDefault, st0));
            VS_HIP(hipMemcpyAsync(stage_v.p, v, (size_t)nnz_i[i] * 4, hipMemcpyDefault, st0));
            rp = stage_rp.as<int64_t>(); c = stage_c.as<int32_t>(); v = stage_v.as<float>();
        }
        hipLaunchKernelGGL(stitch_rows_kernel, dim3(grid_w), dim3(256), 0, st0, rp, c, v, n, (const int64_t*)g_rp.as<int64_t>(), g_cols.as<int32_t>(),
                           g_vals.as<float>());
        VS_HIP(hipGetLastError());
        VS_HIP(hipStreamSynchronize(st0));                                // (the stage buffers are reused by the next shard)
    }
    return VS_OK;
}

// the rowptr / rows on the device (d_*) -> the caller's outputs (host or device on the same device)
int rows_out(const DevBuf& d_rp, int64_t n, const int32_t* d_cols, const float* d_vals, int64_t nnz, int64_t* out_rowptr, int32_t* out_cols,
             float* out_vals, hipStream_t s) {
    VS_HIP(hipMemcpyAsync(out_rowptr, d_rp.p, (size_t)(n + 1) * 8, hipMemcpyDefault, s));
    if (out_cols && nnz > 0) {
        if (out_cols != d_cols) VS_HIP(hipMemcpyAsync(out_cols, d_cols, (size_t)nnz * 4, hipMemcpyDefault, s));
        if (out_vals != d_vals) VS_HIP(hipMemcpyAsync(out_vals, d_vals, (size_t)nnz * 4, hipMemcpyDefault, s));
    }
    VS_HIP(hipStreamSynchronize(s));
    return VS_OK;
}

int qfr_checks(int32_t B, int32_t m, int64_t ld_ids, const float* weights, int64_t ldw, const void* q, int q_dtype, int64_t ldq, int32_t V, int64_t ldo) {
    if (B <= 0) return fail(VS_EINVAL, "B must be positive");
    if (m < 1) return fail(VS_EINVAL, "m must be >= 1");
    if (ld_ids < m) return fail(VS_EINVAL, "ld_ids = %lld is shorter than m = %d", (long long)ld_ids, m);
    if (weights && ldw < m) return fail(VS_EINVAL, "ldw = %lld is shorter than m = %d", (long long)ldw, m);
    if (q) {
        if (q_dtype != VS_F32 && q_dtype != VS_F16) return fail(VS_EINVAL, "q_dtype must be VS_F32 or VS_F16");
        if (ldq < V) return fail(VS_EINVAL, "query has %lld columns, index has %d", (long long)ldq, V);
    }
    if (ldo < V) return fail(VS_EINVAL, "ldo = %lld is shorter than the index's %d columns", (long long)ldo, V);
    if (V > 65535) return fail(VS_EUNSUPPORTED, "n_cols = %d is too wide", V);
    return VS_OK;
}

int check_host_ids(const int64_t* ids, int64_t rows, int64_t ld, int64_t cols, int64_t n_rows) {
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t j = 0; j < cols; ++j) {
            const int64_t id = ids[r * ld + j];
            if (id < -1 || id >= n_rows) return fail(VS_EINVAL, "document id %lld is outside [-1, %lld)", (long long)id, (long long)n_rows);
        }
    return VS_OK;
}

int launch_acc_src(int src, int store_dtype, const AccArgs& a, int grid, hipStream_t s) {
    if (src == SRC_STAGED) return launch_acc<SRC_STAGED, VM_F32>(a, grid, s);
    if (src == SRC_MAT) return launch_acc<SRC_MAT, VM_F32>(a, grid, s);
    if (store_dtype == VS_F32) return launch_acc<SRC_PK, VM_F32>(a, grid, s);
    if (store_dtype == VS_F16) return launch_acc<SRC_PK, VM_F16>(a, grid, s);
    return launch_acc<SRC_PK, VM_BIN>(a, grid, s);
}

}  // namespace

extern "C" int vs_index_get_rows(vs_index* idx, const int64_t* ids, int64_t n, int64_t id_offset, int64_t* out_rowptr, int32_t* out_cols, float* out_vals,
                                 void* stream) {
    VS_TRY(need_device());
    if (!idx || !out_rowptr || (n > 0 && !ids)) return fail(VS_EINVAL, "NULL argument");
    if (n < 0) return fail(VS_EINVAL, "n must be >= 0");
    if ((out_cols == nullptr) != (out_vals == nullptr)) return fail(VS_EINVAL, "out_cols and out_vals are both given or both NULL");
    const void* outs[3] = {out_rowptr, out_cols, out_vals};
    bool out_dev = false;
    VS_TRY(outputs_kind(outs, 3, &out_dev));
    VS_TRY(check_on(ids, idx->device, "ids"));
    for (const void* p : outs) VS_TRY(check_on(p, idx->device, "an output"));
    VS_HIP(hipSetDevice(idx->device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf st_ids, d_rp, st_c, st_v;
    const int64_t* d_ids = nullptr;
    if (n > 0) VS_TRY(ids_on(ids, (size_t)n * 8, idx->device, st_ids, s, &d_ids));
    int64_t nnz = 0;
    VS_TRY(rows_rowptr(idx, d_ids, n, id_offset, 1, s, d_rp, &nnz));
    int32_t* d_cols = out_cols;
    float* d_vals = out_vals;
    if (out_cols) {
        if (!out_dev) {
            VS_TRY(st_c.alloc(std::max<size_t>((size_t)nnz * 4, 4)));
            VS_TRY(st_v.alloc(std::max<size_t>((size_t)nnz * 4, 4)));
            d_cols = st_c.as<int32_t>();
            d_vals = st_v.as<float>();
        }
        ProfScope prof("get_rows", s);
        VS_TRY(rows_copy(idx, d_ids, n, id_offset, d_rp.as<int64_t>(), d_cols, d_vals, s));
    }
    VS_STAGE("get_rows", s);
    return rows_out(d_rp, n, d_cols, d_vals, nnz, out_rowptr, out_cols, out_vals, s);
}

extern "C" int vs_index_queries_from_rows(vs_index* idx, const int64_t* ids, int32_t B, int32_t m, int64_t ld_ids, const float* weights, int64_t ldw,
                                          const void* q, int q_dtype, int64_t ldq, float alpha, float* out_q, int64_t ldo, void* stream) {
    VS_TRY(need_device());
    if (!idx || !ids || !out_q) return fail(VS_EINVAL, "NULL argument");
    const int32_t V = idx->n_cols;
    VS_TRY(qfr_checks(B, m, ld_ids, weights, ldw, q, q_dtype, ldq, V, ldo));
    VS_TRY(check_on(ids, idx->device, "ids"));
    VS_TRY(check_on(weights, idx->device, "weights"));
    VS_TRY(check_on(q, idx->device, "q"));
    VS_TRY(check_on(out_q, idx->device, "out_q"));
    if (!is_device_ptr(ids)) VS_TRY(check_host_ids(ids, B, ld_ids, m, idx->n_rows));
    VS_HIP(hipSetDevice(idx->device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf st_ids, st_w, st_q, st_o;
    const size_t id_bytes = ((size_t)(B - 1) * ld_ids + m) * 8;
    const int64_t* d_ids = ids;
    if (!is_device_ptr(ids)) {
        VS_TRY(st_ids.alloc(id_bytes));
        VS_HIP(hipMemcpyAsync(st_ids.p, ids, id_bytes, hipMemcpyHostToDevice, s));
        d_ids = st_ids.as<int64_t>();
    }
    const float* d_w = weights;
    if (weights && !is_device_ptr(weights)) {
        const size_t bytes = ((size_t)(B - 1) * ldw + m) * 4;
        VS_TRY(st_w.alloc(bytes));
        VS_HIP(hipMemcpyAsync(st_w.p, weights, bytes, hipMemcpyHostToDevice, s));
        d_w = st_w.as<float>();
    }
    const void* d_q = q;
    if (q && !is_device_ptr(q)) {
        const size_t bytes = ((size_t)(B - 1) * ldq + V) * dtype_size(q_dtype);
        VS_TRY(st_q.alloc(bytes));
        VS_HIP(hipMemcpyAsync(st_q.p, q, bytes, hipMemcpyHostToDevice, s));
        d_q = st_q.p;
    }
    const bool out_dev = is_device_ptr(out_q);
    float* d_o = out_q;
    int64_t d_ldo = ldo;
    if (!out_dev) {
        VS_TRY(st_o.alloc((size_t)B * V * 4));
        d_o = st_o.as<float>();
        d_ldo = V;
    }
    AccArgs a{};
    a.s = row_src(idx);
    a.ids = d_ids;
    a.ld_ids = ld_ids;
    a.B = B;
    a.m = m;
    a.w = d_w;
    a.ldw = ldw;
    a.q = d_q;
    a.q_f16 = q_dtype == VS_F16;
    a.ldq = ldq;
    a.alpha = alpha;
    a.out = d_o;
    a.ldo = d_ldo;
    a.n_cols = V;
    a.tile = std::min(V, kAccTileCols);
    {
        ProfScope prof("queries_from_rows", s);
        VS_TRY(launch_acc_src(a.s.dense ? SRC_MAT : SRC_PK, idx->store_dtype, a, std::min(B, idx->cu_count), s));
    }
    VS_STAGE("queries_from_rows", s);
    if (!out_dev) VS_HIP(hipMemcpy2DAsync(out_q, (size_t)ldo * 4, d_o, (size_t)V * 4, (size_t)V * 4, (size_t)B, hipMemcpyDeviceToHost, s));
    // staging buffers die here: a call that used any waits for its work (device pointers + a stream: only enqueued)
    if (!stream || st_ids.p || st_w.p || st_q.p || st_o.p) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}

extern "C" int vs_topk_exclude(const int64_t* ids, const float* scores, int32_t B, int32_t kk, int64_t ld, const int64_t* excl, int32_t m, int64_t ld_excl,
                               int32_t k, int64_t* out_ids, float* out_scores, int device, void* stream) {
    VS_TRY(need_device());
    if (!ids || !scores || !excl || !out_ids || !out_scores) return fail(VS_EINVAL, "NULL argument");
    if (B <= 0 || kk <= 0 || k <= 0) return fail(VS_EINVAL, "B, kk and k must be positive");
    if (ld < kk) return fail(VS_EINVAL, "ld = %lld is shorter than kk = %d", (long long)ld, kk);
    if (m < 1 || m > kExclMaxM) return fail(VS_EINVAL, "m must be in 1..%d (got %d)", kExclMaxM, m);
    if (ld_excl < m) return fail(VS_EINVAL, "ld_excl = %lld is shorter than m = %d", (long long)ld_excl, m);
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range", device);
    const void* outs[2] = {out_ids, out_scores};
    bool out_dev = false;
    VS_TRY(outputs_kind(outs, 2, &out_dev));
    const void* all[5] = {ids, scores, excl, out_ids, out_scores};
    for (const void* p : all) VS_TRY(check_on(p, device, "a buffer"));
    VS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    DevBuf st_in, st_ex, st_out;
    const size_t n_in = (size_t)(B - 1) * ld + kk;
    const int64_t* d_ids = ids;
    const float* d_sc = scores;
    if (!is_device_ptr(ids) || !is_device_ptr(scores)) {
        VS_TRY(st_in.alloc(n_in * 12));
        VS_HIP(hipMemcpyAsync(st_in.p, ids, n_in * 8, hipMemcpyDefault, s));
        VS_HIP(hipMemcpyAsync(st_in.as<char>() + n_in * 8, scores, n_in * 4, hipMemcpyDefault, s));
        d_ids = st_in.as<int64_t>();
        d_sc = reinterpret_cast<const float*>(st_in.as<char>() + n_in * 8);
    }
    const int64_t* d_ex = excl;
    if (!is_device_ptr(excl)) {
        const size_t bytes = ((size_t)(B - 1) * ld_excl + m) * 8;
        VS_TRY(st_ex.alloc(bytes));
        VS_HIP(hipMemcpyAsync(st_ex.p, excl, bytes, hipMemcpyHostToDevice, s));
        d_ex = st_ex.as<int64_t>();
    }
    const size_t n_out = (size_t)B * k;
    int64_t* d_oi = out_ids;
    float* d_os = out_scores;
    if (!out_dev) {
        VS_TRY(st_out.alloc(n_out * 12));
        d_oi = st_out.as<int64_t>();
        d_os = reinterpret_cast<float*>(st_out.as<char>() + n_out * 8);
    }
    {
        ProfScope prof("topk_exclude", s);
        VS_HIP(hipFuncSetAttribute((const void*)topk_exclude_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)m * 8)));
        hipLaunchKernelGGL(topk_exclude_kernel, dim3((unsigned)B), dim3(64), (size_t)m * 8, s, d_ids, d_sc, kk, ld, d_ex, m, ld_excl, k, d_oi, d_os);
        VS_HIP(hipGetLastError());
    }
    VS_STAGE("topk_exclude", s);
    if (!out_dev) {
        VS_HIP(hipMemcpyAsync(out_ids, d_oi, n_out * 8, hipMemcpyDeviceToHost, s));
        VS_HIP(hipMemcpyAsync(out_scores, d_os, n_out * 4, hipMemcpyDeviceToHost, s));
    }
    if (!stream || st_in.p || st_ex.p || st_out.p) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}

// ---- shard groups (api.hip binds them to vs_shard_group) -------------------------------------------------------------------------
// ids / inputs: host or device pointers on any GPU; outputs: host or device pointers on the first shard's device.  Blocking.
static int group_ids_to_host(const int64_t* ids, int64_t rows, int64_t ld, int64_t cols, std::vector<int64_t>& h) {
    h.resize((size_t)std::max<int64_t>(rows * cols, 1));
    if (rows * cols == 0) return VS_OK;
    if (is_device_ptr(ids)) {
        int d = 0;
        VS_TRY(device_of(ids, &d));
        VS_HIP(hipSetDevice(d));
        VS_HIP(hipDeviceSynchronize());                                   // (work the caller queued on any stream of that device)
    }
    VS_HIP(hipMemcpy2D(h.data(), (size_t)cols * 8, ids, (size_t)ld * 8, (size_t)cols * 8, (size_t)rows, hipMemcpyDefault));
    return VS_OK;
}

static int64_t group_rows_total(const std::vector<vs_index*>& shards) {
    int64_t t = 0;
    for (auto* s : shards) t += s->n_rows;
    return t;
}

int vs_shard_group_get_rows_impl(const std::vector<vs_index*>& shards, const std::vector<int64_t>& row0, const std::vector<hipStream_t>& streams,
                                 const int64_t* ids, int64_t n, int64_t* out_rowptr, int32_t* out_cols, float* out_vals) {
    VS_TRY(need_device());
    if (!out_rowptr || (n > 0 && !ids)) return fail(VS_EINVAL, "NULL argument");
    if (n < 0) return fail(VS_EINVAL, "n must be >= 0");
    if ((out_cols == nullptr) != (out_vals == nullptr)) return fail(VS_EINVAL, "out_cols and out_vals are both given or both NULL");
    const int dev0 = shards[0]->device;
    const void* outs[3] = {out_rowptr, out_cols, out_vals};
    bool out_dev = false;
    VS_TRY(outputs_kind(outs, 3, &out_dev));
    for (const void* p : outs) VS_TRY(check_on(p, dev0, "an output"));
    std::vector<int64_t> h;
    VS_TRY(group_ids_to_host(ids, 1, n, n, h));
    VS_TRY(check_host_ids(h.data(), 1, n, n, group_rows_total(shards)));
    if (out_dev) { VS_HIP(hipSetDevice(dev0)); VS_HIP(hipDeviceSynchronize()); }
    DevBuf g_rp, g_cols, g_vals;
    int64_t nnz = 0;
    VS_TRY(group_rows(shards, row0, streams, h.data(), n, out_cols != nullptr, g_rp, g_cols, g_vals, &nnz));
    VS_HIP(hipSetDevice(dev0));
    return rows_out(g_rp, n, g_cols.as<int32_t>(), g_vals.as<float>(), nnz, out_rowptr, out_cols, out_vals, streams[0]);
}

int vs_shard_group_queries_from_rows_impl(const std::vector<vs_index*>& shards, const std::vector<int64_t>& row0, const std::vector<hipStream_t>& streams,
                                          const int64_t* ids, int32_t B, int32_t m, int64_t ld_ids, const float* weights, int64_t ldw, const void* q,
                                          int q_dtype, int64_t ldq, float alpha, float* out_q, int64_t ldo) {
    VS_TRY(need_device());
    if (!ids || !out_q) return fail(VS_EINVAL, "NULL argument");
    const int32_t V = shards[0]->n_cols;
    VS_TRY(qfr_checks(B, m, ld_ids, weights, ldw, q, q_dtype, ldq, V, ldo));
    const int dev0 = shards[0]->device;
    VS_TRY(check_on(out_q, dev0, "out_q"));
    // the example ids, compacted to [B * m] on the host: the owners extract their rows, the first device stitches and accumulates
    std::vector<int64_t> h;
    VS_TRY(group_ids_to_host(ids, B, ld_ids, m, h));
    VS_TRY(check_host_ids(h.data(), B, m, m, group_rows_total(shards)));
    const int64_t n = (int64_t)B * m;
    const bool out_dev = is_device_ptr(out_q);
    int w_dev = -1, q_dev = -1;
    if (weights && is_device_ptr(weights)) { VS_TRY(device_of(weights, &w_dev)); VS_HIP(hipSetDevice(w_dev)); VS_HIP(hipDeviceSynchronize()); }
    if (q && is_device_ptr(q)) { VS_TRY(device_of(q, &q_dev)); VS_HIP(hipSetDevice(q_dev)); VS_HIP(hipDeviceSynchronize()); }
    if (out_dev) { VS_HIP(hipSetDevice(dev0)); VS_HIP(hipDeviceSynchronize()); }
    DevBuf g_rp, g_cols, g_vals;
    int64_t nnz = 0;
    VS_TRY(group_rows(shards, row0, streams, h.data(), n, true, g_rp, g_cols, g_vals, &nnz));
    VS_HIP(hipSetDevice(dev0));
    hipStream_t st0 = streams[0];
    DevBuf d_ids, st_w, st_q, st_o;
    VS_TRY(d_ids.alloc((size_t)n * 8));
    VS_HIP(hipMemcpyAsync(d_ids.p, h.data(), (size_t)n * 8, hipMemcpyHostToDevice, st0));
    const float* d_w = weights;
    if (weights && w_dev != dev0) {
        const size_t bytes = ((size_t)(B - 1) * ldw + m) * 4;
        VS_TRY(st_w.alloc(bytes));
        VS_HIP(hipMemcpyAsync(st_w.p, weights, bytes, hipMemcpyDefault, st0));
        d_w = st_w.as<float>();
    }
    const void* d_q = q;
    if (q && q_dev != dev0) {
        const size_t bytes = ((size_t)(B - 1) * ldq + V) * dtype_size(q_dtype);
        VS_TRY(st_q.alloc(bytes));
        VS_HIP(hipMemcpyAsync(st_q.p, q, bytes, hipMemcpyDefault, st0));
        d_q = st_q.p;
    }
    float* d_o = out_q;
    int64_t d_ldo = ldo;
    if (!out_dev) {
        VS_TRY(st_o.alloc((size_t)B * V * 4));
        d_o = st_o.as<float>();
        d_ldo = V;
    }
    AccArgs a{};
    a.st_rp = g_rp.as<int64_t>();
    a.st_cols = g_cols.as<int32_t>();
    a.st_vals = g_vals.as<float>();
    a.ids = d_ids.as<int64_t>();
    a.ld_ids = m;
    a.B = B;
    a.m = m;
    a.w = d_w;
    a.ldw = ldw;
    a.q = d_q;
    a.q_f16 = q_dtype == VS_F16;
    a.ldq = ldq;
    a.alpha = alpha;
    a.out = d_o;
    a.ldo = d_ldo;
    a.n_cols = V;
    a.tile = std::min(V, kAccTileCols);
    VS_TRY(launch_acc_src(SRC_STAGED, VS_F32, a, std::min(B, shards[0]->cu_count), st0));
    if (!out_dev) VS_HIP(hipMemcpy2DAsync(out_q, (size_t)ldo * 4, d_o, (size_t)V * 4, (size_t)V * 4, (size_t)B, hipMemcpyDeviceToHost, st0));
    VS_HIP(hipStreamSynchronize(st0));
    return VS_OK;
}
