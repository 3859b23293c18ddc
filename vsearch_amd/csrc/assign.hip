// assign.hip -- clustering (vs_assign_plan, vs_index_assign, vs_centroid_half_norms, vs_label_bitmaps): for every row of a CSR-packet index the
// nearest of K dense centroids -- the transposed question of a search, answered in one pass over the index without a [K, N] score matrix -- the
// half norms that turn the dot product into the Euclidean distance, and the per-label bitmaps that hand the clusters to vs_index_term_sums.
// No reference counterpart.  Nothing here touches a search kernel.
//
// The sums have a FIXED ORDER so that a plain loop reproduces them bit for bit: one lane owns a centroid and adds that centroid's products
//   fp64(fl32(c'_j[col_t] * v_t))    (t: the row's cells in stored order, c': the centroid rounded to the index dtype)
// one after the other to an fp64 accumulator that starts at +0.0; the bias is added in fp64 and the sum rounded to fp32 once.
//
// (a) Prep: the centroids [K, ldc] are transposed and rounded into a slab Ct [n_cols + 1][Kp] through a 32 x 32 LDS tile (coalesced on both
//     sides).  Row n_cols -- the padding id of the packets -- and the slots j >= K are zero.  Every slot is written: no memset.
// (b) Assign: a workgroup of 4 waves owns a chunk of rows; a wave takes 64 rows at a time, reads their live and filter bits (wave-uniform words),
//     and gives every allowed row the whole wave: lane l holds packet p0 + l (8 column ids, 8 values) in registers, the cells are broadcast in stored
//     order by readlane, and every lane loads the weights of its W / 64 centroids at the cell's column -- one coalesced read of W * 4 bytes, the 8
//     reads of a packet in flight together.  K > W: the slices follow one another over the same registers (a row of more than 64 packets re-reads
//     its packets per slice).  The best key -- make_key(value, j): larger value, then lower j -- is reduced over the wave once a row; the slots
//     j >= K carry the lowest key, their value 0 never wins.  Lane r of the step keeps row r's answer: one coalesced store of 64 labels and values.
// (c) Half norms: one workgroup of 256 threads per centroid, strided partial sums and a halving tree in LDS.
// (d) Label bitmaps: a wave owns two output words, reads the 64 labels behind them (shifted by bit0), takes one ballot per value and writes the
//     two words of 64 values with one store each.
#include "agg_call.h"
#include "assign_check.h"
#include "topk_keys.h"

#include <algorithm>

using namespace vs;

namespace {

constexpr int kAssignThreads = 256;                   // 4 waves: a wave's registers hold a row's packets, nothing is shared
constexpr int kAssignWaves = kAssignThreads / 64;
constexpr int kNormThreads = 256;                     // the partial sums of the half-norm contract
constexpr int kBitmapThreads = 256;

struct AssignArgs {
    const uint32_t* pk_ptr;           // [n_rows + 1]
    const uint4* cols;                // packets of 8 uint16 column ids
    const void* vals;                 // 8 values a packet (fp32 | fp16), absent for a binary index
    int32_t n_cols;
    int64_t n_rows;
    const uint32_t* live;             // the handle's live bitmap at bit 0, or null
    const uint32_t* filt;             // the filter bitmap read from bit0 on, or null
    int64_t bit0;
    int64_t rows_per_chunk;
    const float* slab;                // [n_cols + 1][Kp]
    const float* bias;                // [K] or null
    int32_t K, Kp, slices;
    int32_t* out_labels;              // [n_rows]
    float* out_values;                // [n_rows] or null
};

__device__ __forceinline__ float round_to_store(float v, int round_f16) { return round_f16 ? __half2float(__float2half_rn(v)) : v; }

// ---- (a) prep ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void assign_prep_kernel(const float* c, int64_t ldc, int32_t K, int32_t Kp, int32_t n_cols, int round_f16,
                                                          float* slab) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    for (int k = ty; k < 32; k += 8) {
        const int j = j0 + k, col = c0 + tx;
        float x = 0.f;
        if (j < K && col < n_cols) x = round_to_store(c[(size_t)j * (size_t)ldc + col], round_f16);
        tile[k][tx] = x;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int col = c0 + k, j = j0 + tx;
        if (col <= n_cols && j < Kp) slab[(size_t)col * (size_t)Kp + j] = tile[tx][k];
    }
}

// ---- (b) assign ---------------------------------------------------------------------------------------------------------------------------------
// bits [p, p + 64) of a bitmap of n_words words (0 past its last word); p and the words are wave-uniform
__device__ __forceinline__ uint64_t bits64(const uint32_t* w, int64_t n_words, int64_t p) {
    const int64_t i = p >> 5;
    const int sh = (int)(p & 31);
    const uint32_t a = i < n_words ? w[i] : 0u, b = i + 1 < n_words ? w[i + 1] : 0u;
    uint64_t v = (((uint64_t)b << 32) | a) >> sh;
    if (sh) v |= (uint64_t)(i + 2 < n_words ? w[i + 2] : 0u) << (64 - sh);
    return v;
}
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// packet p: its 8 column ids and its 8 values widened to fp32 (packets.h)
template <int SD>
__device__ __forceinline__ void load_packet(const AssignArgs& a, uint64_t p, uint4& c, float (&v)[8]) {
    c = a.cols[p];
    load_vals<SD>(a.vals, p, v);
}

template <int CPL> struct SlabVec;
template <> struct SlabVec<1> { using type = float; };
template <> struct SlabVec<2> { using type = float2; };
template <> struct SlabVec<4> { using type = float4; };

// the cells of packets 0 .. n - 1 of the trip (packet i in lane i), in stored order: every lane adds the products of its CPL centroids
template <int SD, int CPL>
__device__ __forceinline__ void walk_packets(const AssignArgs& a, const uint4& c, const float (&v)[8], int n, const float* base, double (&acc)[CPL]) {
#pragma clang fp contract(off)
    using Vec = typename SlabVec<CPL>::type;
    const uint32_t pad = (uint32_t)a.n_cols;
    for (int i = 0; i < n; ++i) {                                // (i is wave-uniform: the broadcasts are scalar reads of lane i)
        const uint32_t cw[4] = {(uint32_t)__builtin_amdgcn_readlane((int)c.x, i), (uint32_t)__builtin_amdgcn_readlane((int)c.y, i),
                                (uint32_t)__builtin_amdgcn_readlane((int)c.z, i), (uint32_t)__builtin_amdgcn_readlane((int)c.w, i)};
        Vec wv[8];
        float vv[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {                             // the 8 reads of the packet are in flight together
            const uint32_t col = min((t & 1) ? (cw[t >> 1] >> 16) : (cw[t >> 1] & 0xFFFFu), pad);       // <= n_cols: the slab has that row, all zero
            wv[t] = *reinterpret_cast<const Vec*>(base + (size_t)col * (size_t)a.Kp);
            float x = 1.f;                                        // a binary index stores 1
            if constexpr (SD != VS_NONE) x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[t]), i));
            vv[t] = col == pad ? 0.f : x;                         // a padding cell adds +0.0 whatever stands in its value: skipped
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float* wq = reinterpret_cast<const float*>(&wv[t]);
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const float prod = wq[q] * vv[t];                 // rounded to fp32, then widened: the library's product
                acc[q] += (double)prod;
            }
        }
    }
}

// one wave, one row: the best key over all centroids, in every lane
template <int SD, int CPL>
__device__ __forceinline__ uint64_t assign_row(const AssignArgs& a, uint32_t p0, uint32_t p1, int lane) {
#pragma clang fp contract(off)
    constexpr int W = 64 * CPL;
    const uint32_t np = p1 - p0;
    const bool one_trip = np <= 64u;                              // the row's packets stay in registers across the slices
    uint4 c = make_uint4(0u, 0u, 0u, 0u);
    float v[8] = {};
    if (one_trip && (uint32_t)lane < np) load_packet<SD>(a, (uint64_t)p0 + lane, c, v);
    uint64_t best = 0ull;
    for (int s = 0; s < a.slices; ++s) {
        double acc[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) acc[q] = 0.0;
        const int j0 = s * W + lane * CPL;                        // this lane's centroids of the slice: j0 .. j0 + CPL - 1 (< Kp)
        const float* base = a.slab + j0;
        if (one_trip) {
            walk_packets<SD, CPL>(a, c, v, (int)np, base, acc);
        } else {
            for (uint64_t pb = p0; pb < p1; pb += 64) {           // (64-bit: no wrap next to 2^32 packets)
                const int n = (uint64_t)p1 - pb < 64 ? (int)((uint64_t)p1 - pb) : 64;
                if (lane < n) load_packet<SD>(a, pb + lane, c, v);
                walk_packets<SD, CPL>(a, c, v, n, base, acc);
            }
        }
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int j = j0 + q;
            uint64_t key = 0ull;                                  // a slot behind the last centroid: below every real key (the key of -inf is not 0)
            if (j < a.K) {
                double d = acc[q];
                if (a.bias) d += (double)a.bias[j];
                float f = (float)d;
                if (f != f) f = -INFINITY;                        // a NaN value counts as -inf
                key = make_key(canon_zero(f), (uint32_t)j);
            }
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)best, off, 64);
        best = o > best ? o : best;
    }
    return best;
}

template <int SD, int CPL>
__global__ __launch_bounds__(kAssignThreads) void assign_kernel(AssignArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * a.rows_per_chunk, r1 = min(a.n_rows, r0 + a.rows_per_chunk);
    const int64_t n_lw = (a.n_rows + 31) >> 5, n_fw = (a.bit0 + a.n_rows + 31) >> 5;
    for (int64_t row0 = r0 + (int64_t)w * 64; row0 < r1; row0 += (int64_t)kAssignWaves * 64) {
        const int64_t nvalid = r1 - row0;                                             // >= 1
        uint64_t m = nvalid >= 64 ? ~0ull : ((1ull << nvalid) - 1ull);                // bits at or past the last row are ignored
        if (a.live) m &= bits64(a.live, n_lw, row0);
        if (a.filt) m &= bits64(a.filt, n_fw, a.bit0 + row0);
        m = uniform64(m);
        uint32_t plo = 0u, phi = 0u;
        if ((m >> lane) & 1ull) {                                                     // (lane < nvalid: the bit is set)
            plo = a.pk_ptr[row0 + lane];
            phi = a.pk_ptr[row0 + lane + 1];
        }
        int32_t label = -1;                                                           // a row that is deleted or not allowed
        float value = -INFINITY;
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1ull;
            const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)plo, l), p1 = (uint32_t)__builtin_amdgcn_readlane((int)phi, l);
            const uint64_t best = assign_row<SD, CPL>(a, p0, p1, lane);
            if (lane == l) {
                label = (int32_t)key_row(best);
                value = key_score(best);
            }
        }
        if (lane < nvalid) {                                                          // row0 + lane < r1 <= n_rows
            a.out_labels[row0 + lane] = label;
            if (a.out_values) a.out_values[row0 + lane] = value;
        }
    }
}

template <int SD>
int assign_launch(const AssignArgs& a, int slice_w, dim3 grid, hipStream_t s) {
    if (slice_w == 64) hipLaunchKernelGGL((assign_kernel<SD, 1>), grid, dim3(kAssignThreads), 0, s, a);
    else if (slice_w == 128) hipLaunchKernelGGL((assign_kernel<SD, 2>), grid, dim3(kAssignThreads), 0, s, a);
    else hipLaunchKernelGGL((assign_kernel<SD, 4>), grid, dim3(kAssignThreads), 0, s, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// ---- (c) half norms -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNormThreads) void half_norms_kernel(const float* c, int64_t ldc, int32_t n_cols, int round_f16, float* out) {
#pragma clang fp contract(off)
    __shared__ double x[kNormThreads];
    const int tid = threadIdx.x;
    const float* cj = c + (size_t)blockIdx.x * (size_t)ldc;
    double sum = 0.0;
    for (int col = tid; col < n_cols; col += kNormThreads) {
        const float wgt = round_to_store(cj[col], round_f16);
        const float sq = wgt * wgt;
        sum += (double)sq;
    }
    x[tid] = sum;
    __syncthreads();
    for (int h = kNormThreads / 2; h > 0; h >>= 1) {
        if (tid < h) x[tid] += x[tid + h];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = (float)(0.5 * x[0]);
}

// ---- (d) label bitmaps --------------------------------------------------------------------------------------------------------------------------
struct BitmapArgs {
    const int32_t* labels;            // [n_rows]
    int64_t n_rows;
    const int32_t* values;            // [B]
    int32_t B;
    int64_t bit0, n_words;            // n_words = (bit0 + n_rows + 31) / 32 words of a row are written
    uint32_t* out;                    // [B, ld]
    int64_t ld;
};

__global__ __launch_bounds__(kBitmapThreads) void label_bitmaps_kernel(BitmapArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (kBitmapThreads / 64) + (threadIdx.x >> 6);      // this wave owns words 2 g and 2 g + 1 of every row
    const int64_t w0 = 2 * g;
    if (w0 >= a.n_words) return;                                                     // (wave-uniform)
    const int64_t r = 64 * g + lane - a.bit0;                                         // the row behind bit 64 g + lane
    const bool valid = r >= 0 && r < a.n_rows;
    const int32_t lab = valid ? a.labels[r] : 0;
    const bool two = w0 + 1 < a.n_words;
    for (int32_t b0 = 0; b0 < a.B; b0 += 64) {
        const int n = min(64, a.B - b0);
        const int32_t mine = lane < n ? a.values[b0 + lane] : 0;
        uint64_t bits = 0ull;
        for (int k = 0; k < n; ++k) {
            const int32_t val = __builtin_amdgcn_readlane(mine, k);
            const uint64_t m = __builtin_amdgcn_ballot_w64(valid && lab == val);
            if (lane == k) bits = m;
        }
        if (lane < n) {                                                               // value b0 + lane: its two words
            uint32_t* dst = a.out + (size_t)(b0 + lane) * (size_t)a.ld + w0;
            dst[0] = (uint32_t)bits;
            if (two) dst[1] = (uint32_t)(bits >> 32);
        }
    }
}

}  // namespace

extern "C" int vs_assign_plan(int64_t n_rows, int32_t K, int32_t n_cols, int64_t rows_per_chunk, int32_t* out_slice_w, int32_t* out_slices,
                              int64_t* out_chunks, int64_t* out_rows_per_chunk, int64_t* out_slab_bytes) {
    if (!out_slice_w || !out_slices || !out_chunks || !out_rows_per_chunk || !out_slab_bytes) return fail(VS_EINVAL, "NULL argument");
    AssignPlan p;
    char msg[256];
    VS_TRY(plan_or_fail(assign_plan(n_rows, K, n_cols, rows_per_chunk, &p, msg, sizeof msg), msg));
    *out_slice_w = p.slice_w;
    *out_slices = p.slices;
    *out_chunks = p.chunks;
    *out_rows_per_chunk = p.rows_per_chunk;
    *out_slab_bytes = p.slab_bytes;
    return VS_OK;
}

extern "C" int vs_centroid_half_norms(const float* c, int64_t ldc, int32_t K, int32_t n_cols, int round_f16, float* out, int device, void* stream) {
    char msg[256];
    VS_TRY(plan_or_fail(assign_check_norms(c && out, K, n_cols, ldc, msg, sizeof msg), msg));
    VS_TRY(device_in_range(device));
    const void* ptrs[2] = {c, out};
    const char* names[2] = {"c", "out"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 2, device, &dev));
    VS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    Staged st_c, st_o;
    float *d_c, *d_o;
    VS_TRY(st_c.in(c, (size_t)(K - 1) * (size_t)ldc + (size_t)n_cols, dev, true, s, &d_c));
    VS_TRY(st_o.in(out, (size_t)K, dev, false, s, &d_o));
    {
        ProfScope prof("half_norms", s);
        hipLaunchKernelGGL(half_norms_kernel, dim3((unsigned)K), dim3(kNormThreads), 0, s, d_c, ldc, n_cols, round_f16 != 0, d_o);
        VS_HIP(hipGetLastError());
    }
    return close_call("half_norms", dev, stream, s, Finish::kStream, [&] { return st_o.back(s); });
}

extern "C" int vs_index_assign(vs_index* idx, const float* centroids, int64_t ldc, int32_t K, const float* bias, const uint32_t* filter,
                               int64_t filter_bit0, int64_t rows_per_chunk, int32_t* out_labels, float* out_values, void* stream) {
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    if (idx->kind != VS_KIND_CSR) return fail(VS_EUNSUPPORTED, "assign reads the CSR packets: a dense index on the matrix cores has none");
    AssignPlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(assign_check_call(centroids && out_labels, K, ldc, filter_bit0, std::max<int64_t>(idx->n_rows, 1), idx->n_cols,
                                          rows_per_chunk, &plan, msg, sizeof msg), msg));
    const int32_t V = idx->n_cols;
    const void* ptrs[5] = {centroids, bias, filter, out_labels, out_values};
    const char* names[5] = {"centroids", "bias", "filter", "out_labels", "out_values"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 5, idx->device, &dev));
    if (!dev) VS_TRY(plan_or_fail(assign_check_finite_host(centroids, K, V, ldc, bias, msg, sizeof msg), msg));
    if (idx->n_rows == 0) return VS_OK;                              // no slot to write
    VS_HIP(hipSetDevice(idx->device));
    hipStream_t s = (hipStream_t)stream;
    Staged st_c, st_b, st_f, st_l, st_v;
    DevBuf slab;
    AssignArgs a{};
    float *d_c, *d_b;
    uint32_t* d_f;
    VS_TRY(st_c.in(centroids, (size_t)(K - 1) * (size_t)ldc + (size_t)V, dev, true, s, &d_c));
    VS_TRY(st_b.in(bias, (size_t)K, dev, true, s, &d_b));                                                     // (NULL stays NULL)
    VS_TRY(st_f.in(filter, (size_t)((filter_bit0 + idx->n_rows + 31) >> 5), dev, true, s, &d_f));
    VS_TRY(st_l.in(out_labels, (size_t)idx->n_rows, dev, false, s, &a.out_labels));
    VS_TRY(st_v.in(out_values, (size_t)idx->n_rows, dev, false, s, &a.out_values));
    VS_TRY(slab.alloc((size_t)plan.slab_bytes));
    const int32_t Kp = plan.slice_w * plan.slices;
    a.pk_ptr = idx->pk_ptr.as<uint32_t>();
    a.cols = idx->cols.as<uint4>();
    a.vals = idx->vals.p;
    a.n_cols = V;
    a.n_rows = idx->n_rows;
    a.live = live_words(idx);                                       // tombstones are ANDed in at bit 0 whatever filter_bit0 is
    a.filt = d_f;
    a.bit0 = filter_bit0;
    a.rows_per_chunk = plan.rows_per_chunk;
    a.slab = slab.as<float>();
    a.bias = d_b;
    a.K = K;
    a.Kp = Kp;
    a.slices = plan.slices;
    int rc = VS_OK;
    {
        ProfScope prof("assign_prep", s);
        const dim3 grid((unsigned)((V + 1 + 31) / 32), (unsigned)(Kp / 32));
        hipLaunchKernelGGL(assign_prep_kernel, grid, dim3(256), 0, s, d_c, ldc, K, Kp, V, idx->store_dtype == VS_F16, slab.as<float>());
        if (hipGetLastError() != hipSuccess) rc = fail(VS_EHIP, "the prep kernel's launch failed");
    }
    if (rc == VS_OK) {
        ProfScope prof("assign", s);
        const dim3 grid((unsigned)plan.chunks);
        const int sd = idx->store_dtype;
        rc = sd == VS_F32 ? assign_launch<VS_F32>(a, plan.slice_w, grid, s)
             : sd == VS_F16 ? assign_launch<VS_F16>(a, plan.slice_w, grid, s)
                            : assign_launch<VS_NONE>(a, plan.slice_w, grid, s);
    }
    if (rc != VS_OK) {
        (void)hipStreamSynchronize(s);                                // the slab and the staging buffers die here
        return rc;
    }
    return close_call("assign", dev, stream, s, Finish::kSync, [&] {      // (the slab is freed when the call returns)
        VS_TRY(st_l.back(s));
        return st_v.back(s);
    });
}

extern "C" int vs_label_bitmaps(const int32_t* labels, int64_t n_rows, const int32_t* values, int32_t B, int64_t bit0, uint32_t* out_words,
                                int64_t ld_words, int device, void* stream) {
    char msg[256];
    VS_TRY(plan_or_fail(assign_check_bitmaps(labels && values && out_words, n_rows, B, bit0, ld_words, msg, sizeof msg), msg));
    VS_TRY(device_in_range(device));
    const void* ptrs[3] = {labels, values, out_words};
    const char* names[3] = {"labels", "values", "out_words"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 3, device, &dev));
    VS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    BitmapArgs a{};
    a.n_rows = n_rows;
    a.B = B;
    a.bit0 = bit0;
    a.n_words = (bit0 + n_rows + 31) >> 5;
    Staged st_l, st_v, st_o;
    int32_t *d_l, *d_v;
    VS_TRY(st_l.in(labels, (size_t)n_rows, dev, true, s, &d_l));
    VS_TRY(st_v.in(values, (size_t)B, dev, true, s, &d_v));
    // (a host buffer's gaps between the rows come back as they went in: the staged copy starts from the caller's words)
    VS_TRY(st_o.in(out_words, (size_t)(B - 1) * (size_t)ld_words + (size_t)a.n_words, dev, true, s, &a.out));
    a.labels = d_l;
    a.values = d_v;
    a.ld = ld_words;
    {
        ProfScope prof("label_bitmaps", s);
        const int64_t waves = (a.n_words + 1) / 2;
        hipLaunchKernelGGL(label_bitmaps_kernel, dim3((unsigned)((waves + kBitmapThreads / 64 - 1) / (kBitmapThreads / 64))), dim3(kBitmapThreads), 0, s, a);
        VS_HIP(hipGetLastError());
    }
    return close_call("label_bitmaps", dev, stream, s, Finish::kStream, [&] { return st_o.back(s); });
}
