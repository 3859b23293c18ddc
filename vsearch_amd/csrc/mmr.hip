// mmr.hip -- diversified search: Maximal Marginal Relevance over a search's hit list (vs_mmr_select_csr).  No reference counterpart.  It
// runs behind a search and vs_index_get_rows; no search kernel is touched.
//
// One workgroup of 16 waves per query.  LDS holds an fp32 image of n_cols cells (128 KiB at the limit), and per candidate its relevance,
// penalty, g(j, j), row offset and a picked flag (20 KiB at kk = 1024).  The image holds ONE row at a time: the last pick's.  A step is
//   zero the cells of the pick before (by its own columns)  | barrier |  scatter the last pick's row (columns of a row are distinct)  | barrier |
//   wave w takes the unpicked candidates j = w (mod 16): lanes stride row j and gather image[col] (fp32 products, fp64 lane sums, a wave
//   reduction), all lanes form sim, lane 0 stores the larger penalty; the wave keeps its best candidate as a 64-bit key (topk_keys.h: val in
//   the high word, ~position in the low word, so the lower position wins a tie and keys never tie)  | barrier |  every wave reads the 16 keys.
// The first step has nothing in the image and only ranks the relevances.  No float atomics: the picks and every output bit are deterministic;
// the only freedom is the order of the fp64 sum inside g.  Arithmetic outside g is pinned operation by operation to tests/_mmr_ref.py.
#include "common.h"
#include "mmr_check.h"
#include "staging.h"
#include "topk_keys.h"

using namespace vs;

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kHeadWords = 2 * kWaves + 4;   // LDS in front of the image: the waves' keys (uint64 each), then [0] n

struct MmrArgs {
    const int64_t* rowptr;   // [B * kk + 1]
    const int32_t* cols;     // NULL: every row is empty
    const float* vals;
    const int64_t* ids;      // [B, ld]
    const float* sc;
    int64_t ld;
    const float* lam;        // [B]
    int32_t kk, k, n_cols, mode;
    int64_t* oi;             // [B, k] each
    float* os;
    int32_t* op;
    float* om;
    float* open;
};

size_t lds_bytes(int32_t n_cols, int32_t kk) { return ((size_t)kHeadWords + (size_t)n_cols + 5 * (size_t)kk + 1) * 4; }

__device__ __forceinline__ double wave_sum(double x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// val = fl32(fl32(lam * rel) - fl32(mu * pen)): two roundings and a subtraction, never an fma
__device__ __forceinline__ float mmr_val(float lam, float mu, float rel, float pen) {
#pragma clang fp contract(off)
    const float x = lam * rel;
    const float y = mu * pen;
    return x - y;
}

__global__ __launch_bounds__(kThreads) void mmr_select_kernel(MmrArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) uint64_t mmr_sh[];
    uint64_t* wkeys = mmr_sh;                                                 // [kWaves]
    int32_t* misc = reinterpret_cast<int32_t*>(mmr_sh + kWaves);              // [4]
    float* img = reinterpret_cast<float*>(misc + 4);                          // [n_cols]
    float* rel = img + a.n_cols;                                              // [kk]
    float* pen = rel + a.kk;                                                  // [kk]
    float* nrm = pen + a.kk;                                                  // [kk] g(j, j)
    uint32_t* off = reinterpret_cast<uint32_t*>(nrm + a.kk);                  // [kk + 1] first cell of row j, from the query's first cell
    int32_t* picked = reinterpret_cast<int32_t*>(off + a.kk + 1);             // [kk]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const int kk = a.kk, k = a.k;
    const uint32_t n_cols = (uint32_t)a.n_cols;
    const int64_t* ids = a.ids + b * (size_t)a.ld;
    const float* sc = a.sc + b * (size_t)a.ld;
    const int64_t* rp = a.rowptr + b * (size_t)kk;
    const bool cells = a.cols != nullptr && a.vals != nullptr;
    const int64_t base = rp[0];
    const int32_t* cols = a.cols + (cells ? base : 0);
    const float* vals = a.vals + (cells ? base : 0);

    if (tid == 0) misc[0] = kk;
    for (uint32_t c = tid; c < n_cols; c += kThreads) img[c] = 0.f;
    __syncthreads();
    for (int j = tid; j < kk; j += kThreads) {
        if (ids[j] == -1) atomicMin(&misc[0], j);                             // the list ends at its first id -1
        off[j] = cells ? (uint32_t)(rp[j] - base) : 0u;
        picked[j] = 0;
        pen[j] = 0.f;
    }
    if (tid == 0) off[kk] = cells ? (uint32_t)(rp[kk] - base) : 0u;
    __syncthreads();
    const int n = misc[0];
    const float lam = a.lam[b];
    const float mu = 1.f - lam;
    const float s0 = n > 0 ? sc[0] : 0.f;
    const bool ratio = a.mode == VS_MMR_COSINE && s0 > 0.f;

    // prologue: g(j, j) and rel_j, waves round-robin over the candidates
    for (int j = wave; j < n; j += kWaves) {
        const uint32_t e1 = off[j + 1];
        double s = 0.0;
        for (uint32_t e = off[j] + lane; e < e1; e += 64) {
            const float v = vals[e];
            if ((uint32_t)cols[e] < n_cols) {
                const float p = v * v;
                s += (double)p;
            }
        }
        s = wave_sum(s);
        if (lane == 0) {
            nrm[j] = (float)s;
            // (an fp64 quotient of two fp32 values rounded to fp32 IS the correctly rounded fp32 quotient: 53 >= 2 * 24 + 2)
            rel[j] = ratio ? (float)((double)sc[j] / (double)s0) : sc[j];
        }
    }
    __syncthreads();

    int n_pick = min(k, n);
    int prev = -1;
    for (int t = 0; t < n_pick; ++t) {
        uint64_t best = 0ull;
        const float nrm_p = prev >= 0 ? nrm[prev] : 0.f;
        for (int j = wave; j < n; j += kWaves) {
            if (picked[j]) continue;
            float pj = pen[j];
            if (prev >= 0) {
                const uint32_t e1 = off[j + 1];
                double s = 0.0;
                for (uint32_t e = off[j] + lane; e < e1; e += 64) {
                    const uint32_t c = (uint32_t)cols[e];
                    if (c < n_cols) {                                         // (never an LDS address otherwise)
                        const float p = img[c] * vals[e];
                        s += (double)p;
                    }
                }
                const float g = (float)wave_sum(s);
                float sim = g;
                if (a.mode == VS_MMR_COSINE) {
                    const float nrm_j = nrm[j];
                    sim = (nrm_p == 0.f || nrm_j == 0.f) ? 0.f : (float)((double)g / sqrt((double)nrm_p * (double)nrm_j));
                }
                if (sim > pj) {
                    pj = sim;
                    if (lane == 0) pen[j] = pj;
                }
            }
            const uint64_t key = make_key(canon_zero(mmr_val(lam, mu, rel[j], pj)), (uint32_t)j);
            best = key > best ? key : best;
        }
        if (lane == 0) wkeys[wave] = best;
        __syncthreads();
        uint64_t kb = 0ull;
        for (int w = 0; w < kWaves; ++w) kb = wkeys[w] > kb ? wkeys[w] : kb;
        if (kb == 0ull) {                                                     // (no key: only a val of all-ones NaN bits gets here; the rest is padding)
            n_pick = t;
            break;
        }
        const int p = (int)key_row(kb);
        if (tid == 0) {
            const size_t o = b * (size_t)k + (size_t)t;
            const float pp = pen[p];
            a.oi[o] = ids[p];
            a.os[o] = sc[p];
            a.op[o] = p;
            a.om[o] = mmr_val(lam, mu, rel[p], pp);
            a.open[o] = pp;
            picked[p] = 1;
        }
        if (t + 1 == n_pick) break;
        if (prev >= 0)                                                        // the image is all zeros again ...
            for (uint32_t e = off[prev] + tid; e < off[prev + 1]; e += kThreads) {
                const uint32_t c = (uint32_t)cols[e];
                if (c < n_cols) img[c] = 0.f;
            }
        __syncthreads();
        for (uint32_t e = off[p] + tid; e < off[p + 1]; e += kThreads) {      // ... and takes the new pick's row
            const uint32_t c = (uint32_t)cols[e];
            if (c < n_cols) img[c] = vals[e];
        }
        __syncthreads();
        prev = p;
    }
    for (int t = n_pick + tid; t < k; t += kThreads) {
        const size_t o = b * (size_t)k + (size_t)t;
        a.oi[o] = -1;
        a.os[o] = -INFINITY;
        a.op[o] = -1;
        a.om[o] = -INFINITY;
        a.open[o] = 0.f;
    }
}

}  // namespace

extern "C" int vs_mmr_select_csr(const int64_t* rowptr, const int32_t* cols, const float* vals, const int64_t* ids, const float* scores, int32_t B,
                                 int32_t kk, int64_t ld, int32_t n_cols, const float* lam, int32_t k, int mode, int64_t* out_ids, float* out_scores,
                                 int32_t* out_pos, float* out_mmr, float* out_pen, int device, void* stream) {
    VS_TRY(need_device());
    if (!rowptr || !ids || !scores || !lam || !out_ids || !out_scores || !out_pos || !out_mmr || !out_pen) return fail(VS_EINVAL, "NULL argument");
    VS_TRY(mmr_check_sizes(B, kk, ld, n_cols, k, mode, err_buf(), 512));
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range", device);
    const void* ptrs[11] = {rowptr, cols, vals, ids, scores, lam, out_ids, out_scores, out_pos, out_mmr, out_pen};
    const char* names[11] = {"rowptr", "cols", "vals", "ids", "scores", "lam", "out_ids", "out_scores", "out_pos", "out_mmr", "out_pen"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 11, device, &dev));
    const size_t rows = (size_t)B * (size_t)kk;
    size_t nnz = 0;
    if (!dev) {                                                              // host arrays are checked here; device arrays are not read on the host
        if (rowptr[rows] > 0 && (!cols || !vals)) return fail(VS_EINVAL, "NULL cols / vals with %lld stored cells", (long long)rowptr[rows]);
        VS_TRY(mmr_check_host(rowptr, cols, lam, B, kk, n_cols, err_buf(), 512));
        nnz = (size_t)rowptr[rows];
    }
    VS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    Staged st[11];
    MmrArgs a{};
    int64_t *d_rp, *d_ids;
    int32_t* d_cols;
    float *d_vals, *d_sc, *d_lam;
    const size_t n_in = (size_t)(B - 1) * (size_t)ld + (size_t)kk, n_out = (size_t)B * (size_t)k;
    VS_TRY(st[0].in(rowptr, rows + 1, dev, true, s, &d_rp));
    VS_TRY(st[1].in(cols, nnz, dev, true, s, &d_cols));
    VS_TRY(st[2].in(vals, nnz, dev, true, s, &d_vals));
    VS_TRY(st[3].in(ids, n_in, dev, true, s, &d_ids));
    VS_TRY(st[4].in(scores, n_in, dev, true, s, &d_sc));
    VS_TRY(st[5].in(lam, (size_t)B, dev, true, s, &d_lam));
    VS_TRY(st[6].in(out_ids, n_out, dev, false, s, &a.oi));
    VS_TRY(st[7].in(out_scores, n_out, dev, false, s, &a.os));
    VS_TRY(st[8].in(out_pos, n_out, dev, false, s, &a.op));
    VS_TRY(st[9].in(out_mmr, n_out, dev, false, s, &a.om));
    VS_TRY(st[10].in(out_pen, n_out, dev, false, s, &a.open));
    a.rowptr = d_rp; a.cols = d_cols; a.vals = d_vals; a.ids = d_ids; a.sc = d_sc; a.ld = ld; a.lam = d_lam;
    a.kk = kk; a.k = k; a.n_cols = n_cols; a.mode = mode;
    const size_t lds = lds_bytes(n_cols, kk);
    VS_HIP(hipFuncSetAttribute((const void*)mmr_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    {
        ProfScope prof("mmr_select", s);
        hipLaunchKernelGGL(mmr_select_kernel, dim3((unsigned)B), dim3(kThreads), lds, s, a);
        VS_HIP(hipGetLastError());
    }
    VS_STAGE("mmr_select", s);
    if (!dev)
        for (int i = 6; i < 11; ++i) VS_TRY(st[i].back(s));
    if (!stream || !dev) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}
