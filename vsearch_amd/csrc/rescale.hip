// rescale.hip -- the reweighted index: the per-row statistics of a stored CSR index (vs_index_row_stats) and a NEW index with the source's
// sparsity whose values are the source's times a scale per row and a scale per column, in fp32 or fp16 (vs_index_rescale; the arithmetic is
// pinned in vsearch_hip.h).  No reference counterpart: the reference's index is a tensor that is multiplied and rebuilt.  The sparsity is kept, so
// the row pointers and the packets' column ids are the source's bit for bit and only the value array is new: one bandwidth-bound stream in the
// shape of the gather of select.hip.  The scaffold of the call is new_index.h, the host-only part rescale_check.h.  Nothing here touches a
// walk or scan kernel.
#include "common.h"
#include "new_index.h"
#include "packets.h"
#include "rescale_check.h"

#include <algorithm>

using namespace vs;

namespace {

RescaleShape shape_of(const vs_index* a) {
    RescaleShape s;
    s.kind = a->kind;
    s.store_dtype = a->store_dtype;
    s.device = a->device;
    s.n_rows = a->n_rows;
    s.n_packets = a->n_packets;
    s.n_cols = a->n_cols;
    return s;
}

// ---- row stats ------------------------------------------------------------------------------------------------------------------------------
// A wave takes 64 consecutive rows, one after the other, in the shape of row_sum_f64 (csr_scan.h): lane l adds the cells of packets p0 + l,
// p0 + l + 64, ... cell by cell from +0.0, the 64 lane sums are combined by the xor butterfly o = 32 .. 1 -- the pinned order of the exact
// scores.  Lane i keeps the results of the run's row i, so that the five outputs leave as 64-entry runs (256 contiguous rows a workgroup).
struct StatsArgs {
    const uint32_t* pk;
    const uint4* cols;
    const void* vals;
    int64_t n_rows;
    int32_t n_cols;
    int32_t *cells, *nonzero;
    double *l1, *sumsq;
    float* max;
};

template <int SD>
__global__ __launch_bounds__(kStatsThreads) void row_stats_kernel(StatsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * (kStatsThreads / 64) + (threadIdx.x >> 6)) * kStatsRowsPerWave;
    if (r0 >= a.n_rows) return;
    const int n_run = (int)min((int64_t)kStatsRowsPerWave, a.n_rows - r0);
    const uint32_t pkl = a.pk[r0 + lane < a.n_rows ? r0 + lane : a.n_rows];
    const uint32_t pk_end = a.pk[r0 + n_run];
    int32_t k_cells = 0, k_nz = 0;
    double k_l1 = 0.0, k_sq = 0.0;
    float k_max = 0.f;
    for (int i = 0; i < n_run; ++i) {
        const uint32_t p0 = __shfl(pkl, i, 64);
        const uint32_t nx = __shfl(pkl, (i + 1) & 63, 64);
        const uint32_t p1 = i + 1 < n_run ? nx : pk_end;
        int32_t cells = 0, nz = 0;
        double l1 = 0.0, sq = 0.0;
        float mx = __uint_as_float(0x7FC00000u);              // "no value yet": fmaxf returns its other operand
        for (uint32_t p = p0 + lane; p < p1; p += 64) {
            const uint4 c = a.cols[p];
            float v[8];
            load_vals<SD>(a.vals, p, v);
            uint32_t real = 0u;
#pragma unroll
            for (int t = 0; t < 8; ++t) real |= (packet_col(c, t) != (uint32_t)a.n_cols ? 1u : 0u) << t;
            cells += __popc(real);
            nz += __popc(nonzero_cells<SD>(a.vals, p) & real);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if ((real >> t) & 1u) {
                    const float w = SD == VS_NONE ? 1.f : v[t];
                    const double x = (double)w;
                    l1 += fabs(x);
                    sq += x * x;                               // (the product is exact in fp64: contracted into an fma or not, the same sum)
                    mx = fmaxf(mx, w);                         // a NaN cell is skipped
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cells += __shfl_xor(cells, o, 64);
            nz += __shfl_xor(nz, o, 64);
            l1 += __shfl_xor(l1, o, 64);
            sq += __shfl_xor(sq, o, 64);
            mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        }
        if (mx == 0.f) mx = 0.f;                               // of -0.0 and +0.0: +0.0
        if (mx != mx) mx = __uint_as_float(0x7FC00000u);       // no non-NaN cell: the numeric fields' "no value"
        if (lane == i) {
            k_cells = cells;
            k_nz = nz;
            k_l1 = l1;
            k_sq = sq;
            k_max = mx;
        }
    }
    if (lane < n_run) {
        const int64_t r = r0 + lane;
        if (a.cells) a.cells[r] = k_cells;
        if (a.nonzero) a.nonzero[r] = k_nz;
        if (a.l1) a.l1[r] = k_l1;
        if (a.sumsq) a.sumsq[r] = k_sq;
        if (a.max) a.max[r] = k_max;
    }
}

// ---- rescale ----------------------------------------------------------------------------------------------------------------------------------
// A wave takes a run of 64 rows: one contiguous packet range, the same in source and result.  Lane p of it finds its row among the run's row
// pointers (held one a lane, searched with shuffles, as the gather of select.hip does: "the last row of the run whose first packet is <= p"),
// reads the packet's ids and values once, and writes ids and values once, 16 bytes a store; kRescaleSteps 64-packet steps are loaded before the
// first is stored.  Without a row scale no row is looked up; without any scale no scale is read.  CS: where a cell's column scale comes from
// -- the workgroup's LDS image (n_cols floats, loaded once by a persistent workgroup) or memory.
struct RescaleArgs {
    const uint32_t* pk;
    const uint4* cols;
    const void* vals;
    const float *rs, *cs;
    int64_t n_rows;
    int32_t n_cols;
    uint4* dcols;
    uint4* dvals;
};

struct RescalePacket {
    uint4 c, v0, v1;
    float rs;
};

template <int SD, int RS>
__device__ __forceinline__ RescalePacket rescale_load(int64_t q, int64_t p_end, uint32_t np, float rsl, const uint4* cols, const uint4* vals) {
    const int64_t p = q < p_end ? q : p_end - 1;                  // a lane past the run's end loads its last packet again and stores nothing
    RescalePacket r;
    r.rs = 1.f;
    if constexpr (RS != 0) {
        int i = 0;                                                // the last row of the run whose first packet is <= p: the row p belongs to
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) {
            const uint32_t t = __shfl(np, i + step, 64);
            if ((int64_t)t <= p) i += step;
        }
        r.rs = __shfl(rsl, i, 64);
    }
    r.c = cols[p];
    r.v0 = r.v1 = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (SD == VS_F16) r.v0 = vals[p];
    if constexpr (SD == VS_F32) {
        r.v0 = vals[(size_t)p * 2];
        r.v1 = vals[(size_t)p * 2 + 1];
    }
    return r;
}

__device__ __forceinline__ uint32_t half_bits(float f) { return (uint32_t)__half_as_ushort(__float2half_rn(f)); }

template <int SD, int OD, int CS, int RS>
__device__ __forceinline__ void rescale_store(const RescalePacket& r, int64_t p, int64_t p_end, int32_t n_cols, const float* cs, uint4* dcols, uint4* dvals) {
    if (p >= p_end) return;
    dcols[p] = r.c;
    if constexpr (CS == kColScaleNone && RS == 0 && SD == OD) {  // the value bits are copied
        if constexpr (OD == VS_F16) dvals[p] = r.v0;
        if constexpr (OD == VS_F32) {
            dvals[(size_t)p * 2] = r.v0;
            dvals[(size_t)p * 2 + 1] = r.v1;
        }
        return;
    }
    float w[8];
    if constexpr (SD == VS_F32) {
        const uint32_t b[8] = {r.v0.x, r.v0.y, r.v0.z, r.v0.w, r.v1.x, r.v1.y, r.v1.z, r.v1.w};
#pragma unroll
        for (int t = 0; t < 8; ++t) w[t] = __uint_as_float(b[t]);
    } else if constexpr (SD == VS_F16) {
        const uint32_t h[4] = {r.v0.x, r.v0.y, r.v0.z, r.v0.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w[2 * j] = __half2float(__ushort_as_half((unsigned short)(h[j] & 0xFFFFu)));
            w[2 * j + 1] = __half2float(__ushort_as_half((unsigned short)(h[j] >> 16)));
        }
    } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) w[t] = 1.f;
    }
    float f[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uint32_t col = packet_col(r.c, t);
        const bool pad = col == (uint32_t)n_cols;
        double x = (double)w[t];
        if constexpr (RS != 0) x *= (double)r.rs;
        if constexpr (CS != kColScaleNone) x *= (double)cs[pad ? 0u : col];     // (no scale applies to a padding cell: entry 0 is read in bounds, the value is set below)
        f[t] = pad ? 0.f : (float)x;
        // a fp16 result is fl16(fl32(x)), two roundings: the fp32 value has to exist.  Left to itself the compiler fuses a one-scale product and
        // the conversion into one v_fma_mixlo_f16, which rounds the exact product once (seen on the GPU: other bits on double-rounding cases;
        // "#pragma clang fp contract(off)" does not stop it) -- the empty statement makes the float opaque to that fold
        if constexpr (OD == VS_F16) asm volatile("" : "+v"(f[t]));
    }
    if constexpr (OD == VS_F32) {
        dvals[(size_t)p * 2] = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
        dvals[(size_t)p * 2 + 1] = make_uint4(__float_as_uint(f[4]), __float_as_uint(f[5]), __float_as_uint(f[6]), __float_as_uint(f[7]));
    } else {
        dvals[p] = make_uint4(half_bits(f[0]) | (half_bits(f[1]) << 16), half_bits(f[2]) | (half_bits(f[3]) << 16), half_bits(f[4]) | (half_bits(f[5]) << 16),
                              half_bits(f[6]) | (half_bits(f[7]) << 16));
    }
}

template <int SD, int OD, int CS, int RS>
__global__ __launch_bounds__(CS == kColScaleLds ? kRescaleImgThreads : kRescaleThreads) void rescale_kernel(RescaleArgs a) {
    static_assert(kRescaleSteps == 4, "the round below names its four packets");
    extern __shared__ __attribute__((aligned(16))) float rescale_img[];
    const float* cs = a.cs;
    if constexpr (CS == kColScaleLds) {
        for (int i = threadIdx.x; i < a.n_cols; i += kRescaleImgThreads) rescale_img[i] = a.cs[i];
        __syncthreads();
        cs = rescale_img;
    }
    constexpr int kWaves = (CS == kColScaleLds ? kRescaleImgThreads : kRescaleThreads) / 64;
    const int lane = threadIdx.x & 63;
    const int64_t n_runs = (a.n_rows + kRescaleRun - 1) / kRescaleRun;
    const uint4* svals = reinterpret_cast<const uint4*>(a.vals);
    for (int64_t run = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); run < n_runs; run += (int64_t)gridDim.x * kWaves) {
        const int64_t j = run * kRescaleRun + lane;
        const uint32_t np = a.pk[j < a.n_rows ? j : a.n_rows];
        float rsl = 1.f;
        if constexpr (RS != 0) rsl = j < a.n_rows ? a.rs[j] : 1.f;
        const int64_t j_end = (run * kRescaleRun + kRescaleRun < a.n_rows) ? run * kRescaleRun + kRescaleRun : a.n_rows;
        const int64_t p_begin = __shfl(np, 0, 64), p_end = a.pk[j_end];
        for (int64_t base = p_begin; base < p_end; base += 64 * kRescaleSteps) {
            const int64_t q = base + lane;
            const RescalePacket a0 = rescale_load<SD, RS>(q, p_end, np, rsl, a.cols, svals);
            const RescalePacket a1 = rescale_load<SD, RS>(q + 64, p_end, np, rsl, a.cols, svals);
            const RescalePacket a2 = rescale_load<SD, RS>(q + 128, p_end, np, rsl, a.cols, svals);
            const RescalePacket a3 = rescale_load<SD, RS>(q + 192, p_end, np, rsl, a.cols, svals);
            rescale_store<SD, OD, CS, RS>(a0, q, p_end, a.n_cols, cs, a.dcols, a.dvals);
            rescale_store<SD, OD, CS, RS>(a1, q + 64, p_end, a.n_cols, cs, a.dcols, a.dvals);
            rescale_store<SD, OD, CS, RS>(a2, q + 128, p_end, a.n_cols, cs, a.dcols, a.dvals);
            rescale_store<SD, OD, CS, RS>(a3, q + 192, p_end, a.n_cols, cs, a.dcols, a.dvals);
        }
    }
}

template <int SD, int OD, int CS, int RS>
int launch_rescale_one(const RescalePlan& plan, int cu_count, const RescaleArgs& a) {
    const auto kern = rescale_kernel<SD, OD, CS, RS>;
    if (plan.lds_bytes > 64 * 1024) VS_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, plan.lds_bytes));
    hipLaunchKernelGGL(kern, dim3((unsigned)rescale_grid(plan, cu_count)), dim3((unsigned)plan.threads), (size_t)plan.lds_bytes, 0, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}
template <int SD, int OD, int CS>
int launch_rescale_rs(const RescalePlan& plan, int cu_count, const RescaleArgs& a) {
    return a.rs ? launch_rescale_one<SD, OD, CS, 1>(plan, cu_count, a) : launch_rescale_one<SD, OD, CS, 0>(plan, cu_count, a);
}
template <int SD, int OD>
int launch_rescale_cs(const RescalePlan& plan, int cu_count, const RescaleArgs& a) {
    if (plan.col_route == kColScaleLds) return launch_rescale_rs<SD, OD, kColScaleLds>(plan, cu_count, a);
    if (plan.col_route == kColScaleMemory) return launch_rescale_rs<SD, OD, kColScaleMemory>(plan, cu_count, a);
    return launch_rescale_rs<SD, OD, kColScaleNone>(plan, cu_count, a);
}
template <int SD>
int launch_rescale_od(int od, const RescalePlan& plan, int cu_count, const RescaleArgs& a) {
    return od == VS_F32 ? launch_rescale_cs<SD, VS_F32>(plan, cu_count, a) : launch_rescale_cs<SD, VS_F16>(plan, cu_count, a);
}

}  // namespace

extern "C" int vs_rescale_plan(int64_t n_rows, int64_t n_packets, int32_t n_cols, int src_dtype, int out_dtype, int has_row_scale, int has_col_scale,
                               int64_t* out_scratch_bytes, int32_t* out_lds_bytes, int32_t* out_col_route) {
    char msg[512] = {0};
    RescalePlan p;
    const int rc = rescale_plan(n_rows, n_packets, n_cols, src_dtype, out_dtype, has_row_scale != 0, has_col_scale != 0, &p, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    if (out_scratch_bytes) *out_scratch_bytes = p.scratch_bytes;
    if (out_lds_bytes) *out_lds_bytes = p.lds_bytes;
    if (out_col_route) *out_col_route = p.col_route;
    return VS_OK;
}

extern "C" int vs_index_row_stats(const vs_index* src, int32_t* out_cells, int32_t* out_nonzero, double* out_l1, double* out_sumsq, float* out_max) {
    char msg[512] = {0};
    const void* outs[5] = {out_cells, out_nonzero, out_l1, out_sumsq, out_max};
    static const size_t width[5] = {4, 4, 8, 8, 4};
    static const char* const names[5] = {"out_cells", "out_nonzero", "out_l1", "out_sumsq", "out_max"};
    uint32_t have = 0u, on_dev = 0u;
    for (int i = 0; i < 5; ++i) {
        if (outs[i]) have |= 1u << i;
        if (src && is_device_ptr(outs[i])) on_dev |= 1u << i;
    }
    int rc = stats_check_outputs(src != nullptr, have, on_dev, msg, sizeof msg);
    if (rc == VS_OK) rc = rescale_check_source(shape_of(src), "take the statistics of", msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    VS_TRY(need_device());
    for (int i = 0; i < 5; ++i) VS_TRY(ptr_on(outs[i], ((on_dev >> i) & 1u) != 0u, src->device, names[i]));
    const int64_t n = src->n_rows;
    if (n == 0 || have == 0u) return VS_OK;
    VS_TRY(open_sources(src->device));
    const bool host = on_dev == 0u;
    DevBuf stage;
    void* dev[5] = {out_cells, out_nonzero, out_l1, out_sumsq, out_max};
    if (host) {                                                // the wanted outputs side by side on the device, the 8-byte ones first
        size_t bytes = 0;
        for (int i = 0; i < 5; ++i) bytes += (have >> i) & 1u ? (size_t)n * width[i] : 0;
        if (stage.alloc(bytes) != VS_OK) return fail(VS_ENOMEM, "the row statistics need %zu bytes of HBM to stage the outputs", bytes);
        size_t at = 0;
        static const int order[5] = {2, 3, 0, 1, 4};
        for (int k = 0; k < 5; ++k) {
            const int i = order[k];
            if (!((have >> i) & 1u)) continue;
            dev[i] = (char*)stage.p + at;
            at += (size_t)n * width[i];
        }
    }
    StatsArgs a;
    a.pk = src->pk_ptr.as<uint32_t>();
    a.cols = src->cols.as<uint4>();
    a.vals = src->vals.p;
    a.n_rows = n;
    a.n_cols = src->n_cols;
    a.cells = (int32_t*)dev[0];
    a.nonzero = (int32_t*)dev[1];
    a.l1 = (double*)dev[2];
    a.sumsq = (double*)dev[3];
    a.max = (float*)dev[4];
    const dim3 grid((unsigned)stats_grid(n));
    if (src->store_dtype == VS_F32) hipLaunchKernelGGL(row_stats_kernel<VS_F32>, grid, dim3(kStatsThreads), 0, 0, a);
    else if (src->store_dtype == VS_F16) hipLaunchKernelGGL(row_stats_kernel<VS_F16>, grid, dim3(kStatsThreads), 0, 0, a);
    else hipLaunchKernelGGL(row_stats_kernel<VS_NONE>, grid, dim3(kStatsThreads), 0, 0, a);
    VS_HIP(hipGetLastError());
    if (host)
        for (int i = 0; i < 5; ++i)
            if ((have >> i) & 1u) VS_HIP(hipMemcpy(const_cast<void*>(outs[i]), dev[i], (size_t)n * width[i], hipMemcpyDeviceToHost));
    VS_HIP(hipDeviceSynchronize());
    return VS_OK;
}

extern "C" int vs_index_rescale(const vs_index* src, const float* row_scale, const float* col_scale, int out_dtype, int64_t rows_extra,
                                int64_t packets_extra, int device, vs_index** out) {
    char msg[512] = {0};
    if (out) *out = nullptr;
    int rc = rescale_check_args(src != nullptr, out != nullptr, out_dtype, rows_extra, packets_extra, msg, sizeof msg);
    if (rc == VS_OK) rc = rescale_check_source(shape_of(src), "rescale", msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    VS_TRY(device_in_range(device));
    VS_TRY(ptr_on(row_scale, is_device_ptr(row_scale), src->device, "row_scale"));
    VS_TRY(ptr_on(col_scale, is_device_ptr(col_scale), src->device, "col_scale"));
    const int64_t n = src->n_rows, n_packets = src->n_packets;
    RescalePlan plan;
    rc = rescale_plan(n, n_packets, src->n_cols, src->store_dtype, out_dtype, row_scale != nullptr, col_scale != nullptr, &plan, msg, sizeof msg);
    if (rc == VS_OK) rc = new_index_check_capacity("rescaled", n, n_packets, rows_extra, packets_extra, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);

    VS_TRY(open_sources(src->device));
    DevBuf rs_stage, cs_stage;
    const void *d_rs = nullptr, *d_cs = nullptr;
    if (row_scale && n > 0) VS_TRY(to_device(row_scale, (size_t)n * 4, rs_stage, 0, &d_rs));
    if (col_scale) VS_TRY(to_device(col_scale, (size_t)src->n_cols * 4, cs_stage, 0, &d_cs));
    IndexGuard guard{nullptr};
    VS_TRY(new_csr_index("rescaling", "source's (drop the postings copy of the source)", n, n_packets, rows_extra, packets_extra, src->n_cols, out_dtype, src->device,
                         &guard));
    vs_index* idx = guard.p;
    VS_HIP(hipMemcpy(idx->pk_ptr.p, src->pk_ptr.p, (size_t)(n + 1) * 4, hipMemcpyDeviceToDevice));      // the row pointers are the source's
    if (n_packets > 0) {
        RescaleArgs a;
        a.pk = src->pk_ptr.as<uint32_t>();
        a.cols = src->cols.as<uint4>();
        a.vals = src->vals.p;
        a.rs = (const float*)d_rs;
        a.cs = (const float*)d_cs;
        a.n_rows = n;
        a.n_cols = src->n_cols;
        a.dcols = idx->cols.as<uint4>();
        a.dvals = idx->vals.as<uint4>();
        if (src->store_dtype == VS_F32) VS_TRY(launch_rescale_od<VS_F32>(out_dtype, plan, src->cu_count, a));
        else if (src->store_dtype == VS_F16) VS_TRY(launch_rescale_od<VS_F16>(out_dtype, plan, src->cu_count, a));
        else VS_TRY(launch_rescale_od<VS_NONE>(out_dtype, plan, src->cu_count, a));
    }
    set_csr_shape(idx, n, n_packets, src->nnz, src->logical_dense);
    return hand_over(guard, src->device, device, TombFrom::source_bits(src), out);
}
