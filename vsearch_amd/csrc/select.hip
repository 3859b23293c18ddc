// select.hip -- the sub-index: any rows of a stored index, in any order and with repeats, as a NEW index (vs_index_select_rows).  Packets are
// copied whole, so a row scores bit for bit what it scored in the source; the source's tombstones travel with the rows.  No reference
// counterpart: the reference's index is a tensor that is indexed and rebuilt (index.py:163-179).  The shape is vs_index_compact's (mutable.hip:
// scan, map, gather, recount) over an id list the caller gives instead of the live rows; the host-only part is select_check.h.
#include "block_scan.h"
#include "common.h"
#include "select_check.h"

#include <algorithm>

using namespace vs;

static_assert(kSelectScanRows == kScanRows, "the plan counts the scan blocks of block_scan.h");

namespace {

int need_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(VS_ENODEVICE, "no HIP device visible: libvsearch_hip has no CPU fallback");
    }
    return VS_OK;
}

int64_t bit_words(int64_t rows) { return (rows + 31) >> 5; }

unsigned grid_for(int64_t items, int per_block, int64_t cap) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, cap));
}

// what the first kernel leaves behind the block sums: read back in one copy
struct SelectTotals {
    uint2 total;                       // (ids, packets mod 2^32): scan_block_sums_kernel
    unsigned long long packets;        // the packets as a 64-bit sum (repeats can pass 2^32)
    uint32_t bad;                      // an id outside the source was seen
    uint32_t pad;
};

// the source row of id i, or -1
__device__ __forceinline__ int64_t row_of(const int64_t* ids, int64_t i, int64_t id_offset, int64_t n_rows) {
    const int64_t id = ids[i];
    const uint64_t row = (uint64_t)id - (uint64_t)id_offset;
    return (id < id_offset || row >= (uint64_t)n_rows) ? -1 : (int64_t)row;
}

// (1, packets of the source row) of id i; a position past the end counts nothing, an id outside the source raises *bad and counts no packets
__device__ __forceinline__ uint2 id_stat(const int64_t* ids, int64_t i, int64_t n, int64_t id_offset, int64_t n_rows, const uint32_t* pk, uint32_t* bad) {
    if (i >= n) return make_uint2(0u, 0u);
    const int64_t row = row_of(ids, i, id_offset, n_rows);
    if (row < 0) {
        *bad = 1u;
        return make_uint2(1u, 0u);
    }
    return make_uint2(1u, pk ? pk[row + 1] - pk[row] : 0u);
}

// step 1 (stat): the range check and the (ids, packets) of every block of kScanRows ids
__global__ __launch_bounds__(256) void select_stat_kernel(const int64_t* ids, int64_t n, int64_t id_offset, int64_t n_rows, const uint32_t* pk, uint2* sums,
                                                          SelectTotals* totals) {
    __shared__ uint2 sh[4];
    const int64_t i0 = (int64_t)blockIdx.x * kScanRows;
    uint2 acc = make_uint2(0u, 0u);
    for (int it = 0; it < kScanItems; ++it) acc = add2(acc, id_stat(ids, i0 + it * 256 + threadIdx.x, n, id_offset, n_rows, pk, &totals->bad));
    uint2 tot;
    (void)block_excl_scan<4>(acc, sh, &tot);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = tot;
        if (tot.y) atomicAdd(&totals->packets, (unsigned long long)tot.y);     // (a block's packets fit 32 bits: 4096 rows of at most 8192 packets)
    }
}

// step 2 (map): new_pk[j] = packets of the ids before position j.  With tombstones the live bits of the new rows as well: the 64 ids of a wave are
// two whole words of the new bitmap, written from a ballot with plain stores (bits past the last new row stay set: rows still to be appended are
// live); *dead counts the cleared ones
__global__ __launch_bounds__(256) void select_map_kernel(const int64_t* ids, int64_t n, int64_t id_offset, int64_t n_rows, const uint32_t* pk, const uint2* sums,
                                                         uint32_t* new_pk, const uint32_t* src_live, uint32_t* new_live, unsigned long long* dead) {
    __shared__ uint2 sh[4];
    const int lane = threadIdx.x & 63;
    const int64_t i0 = (int64_t)blockIdx.x * kScanRows;
    uint2 carry = sums[blockIdx.x];
    for (int it = 0; it < kScanItems; ++it) {
        const int64_t i = i0 + it * 256 + threadIdx.x;
        const int64_t row = i < n ? row_of(ids, i, id_offset, n_rows) : -1;     // (every id was checked by the stat kernel)
        const uint2 v = row >= 0 ? make_uint2(1u, pk ? pk[row + 1] - pk[row] : 0u) : make_uint2(0u, 0u);
        uint2 tot;
        const uint2 ex = block_excl_scan<4>(v, sh, &tot);
        if (row >= 0 && new_pk) new_pk[i] = carry.y + ex.y;
        if (src_live) {
            const bool is_dead = row >= 0 && !((src_live[row >> 5] >> (row & 31)) & 1u);
            const unsigned long long dead_bits = __ballot(is_dead);
            const int64_t w0 = i - lane;                                          // the wave's first position: a multiple of 64
            if (lane == 0 && w0 < n) new_live[w0 >> 5] = ~(uint32_t)dead_bits;
            if (lane == 32 && w0 + 32 < n) new_live[(w0 >> 5) + 1] = ~(uint32_t)(dead_bits >> 32);
            if (lane == 0 && dead_bits) atomicAdd(dead, (unsigned long long)__popcll(dead_bits));
        }
        carry = add2(carry, tot);
    }
}

// step 3 (gather).  A wave takes a run of 64 new rows: their packets are one contiguous range of the new index, lane p of it finds its row among
// the run's row pointers (held one a lane, searched with shuffles, as compact_gather_kernel of mutable.hip does) and copies the packet whole -- 16
// bytes of column ids, VB bytes of values; padding sits in a row's last packet and moves with it.  The source rows of a run are scattered, so a
// wave takes kSelectSteps 64-packet steps at a time and issues the loads of all of them before the first store; a lane past the run's end loads
// the run's last packet again (no branch around a load) and stores nothing.  A step's packet is a struct of its own, four named ones a round:
// written as arrays indexed by the step the compiler kept them in LDS and scratch, not in registers.
struct SelectPacket {
    uint4 c, v0, v1;
};

// packet q of the run (clamped to its last one), loaded from the source row it belongs to
template <int VB>
__device__ __forceinline__ SelectPacket select_load(int64_t q, int64_t p_end, uint32_t np, uint32_t sp, const uint4* src_cols, const uint4* src_vals) {
    const int64_t p = q < p_end ? q : p_end - 1;
    int i = 0;                                                    // the last row of the run whose first packet is <= p: the row p belongs to
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const uint32_t t = __shfl(np, i + step, 64);
        if ((int64_t)t <= p) i += step;
    }
    const uint32_t npi = __shfl(np, i, 64), spi = __shfl(sp, i, 64);
    const size_t s = (size_t)spi + (size_t)(p - (int64_t)npi);
    SelectPacket r;
    r.c = src_cols[s];
    r.v0 = r.v1 = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (VB == 16) r.v0 = src_vals[s];
    if constexpr (VB == 32) {
        r.v0 = src_vals[s * 2];
        r.v1 = src_vals[s * 2 + 1];
    }
    return r;
}

template <int VB>
__device__ __forceinline__ void select_store(const SelectPacket& r, int64_t p, int64_t p_end, uint4* dst_cols, uint4* dst_vals) {
    if (p >= p_end) return;
    dst_cols[p] = r.c;
    if constexpr (VB == 16) dst_vals[p] = r.v0;
    if constexpr (VB == 32) {
        dst_vals[(size_t)p * 2] = r.v0;
        dst_vals[(size_t)p * 2 + 1] = r.v1;
    }
}

template <int VB>
__global__ __launch_bounds__(256) void select_gather_kernel(const int64_t* ids, int64_t id_offset, const uint32_t* src_pk, const uint32_t* new_pk, int64_t n_new,
                                                            const uint4* src_cols, const uint4* src_vals, uint4* dst_cols, uint4* dst_vals) {
    static_assert(kSelectSteps == 4, "the round below names its four packets");
    const int lane = threadIdx.x & 63;
    const int64_t n_runs = (n_new + kSelectRun - 1) / kSelectRun;
    for (int64_t run = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); run < n_runs; run += (int64_t)gridDim.x * 4) {
        const int64_t j = run * kSelectRun + lane;
        const uint32_t np = new_pk[j < n_new ? j : n_new];
        const uint32_t sp = j < n_new ? src_pk[ids[j] - id_offset] : 0u;
        const int64_t j_end = (run * kSelectRun + kSelectRun < n_new) ? run * kSelectRun + kSelectRun : n_new;
        const int64_t p_begin = __shfl(np, 0, 64), p_end = new_pk[j_end];
        for (int64_t base = p_begin; base < p_end; base += 64 * kSelectSteps) {
            const int64_t q = base + lane;
            const SelectPacket a0 = select_load<VB>(q, p_end, np, sp, src_cols, src_vals);
            const SelectPacket a1 = select_load<VB>(q + 64, p_end, np, sp, src_cols, src_vals);
            const SelectPacket a2 = select_load<VB>(q + 128, p_end, np, sp, src_cols, src_vals);
            const SelectPacket a3 = select_load<VB>(q + 192, p_end, np, sp, src_cols, src_vals);
            select_store<VB>(a0, q, p_end, dst_cols, dst_vals);
            select_store<VB>(a1, q + 64, p_end, dst_cols, dst_vals);
            select_store<VB>(a2, q + 128, p_end, dst_cols, dst_vals);
            select_store<VB>(a3, q + 192, p_end, dst_cols, dst_vals);
        }
    }
}

// dense (matrix-core) index: row gather of the padded matrix, 16 bytes a lane (the padded row is a multiple of 32 floats)
__global__ __launch_bounds__(256) void select_dense_kernel(const int64_t* ids, int64_t id_offset, int64_t n_new, int64_t quads_per_row, const uint4* src, uint4* dst) {
    const int64_t n = n_new * quads_per_row;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t j = i / quads_per_row, c = i % quads_per_row;
        dst[i] = src[(size_t)(ids[j] - id_offset) * (size_t)quads_per_row + (size_t)c];
    }
}

// step 4: non-zeros of the new index (pads sit at the tail of a row's last packet only)
__global__ __launch_bounds__(256) void select_nnz_kernel(const uint32_t* pk, int64_t n_rows, const uint16_t* cols, int32_t n_cols, unsigned long long* out) {
    unsigned long long nnz = 0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * 256) {
        const uint32_t a = pk[r], b = pk[r + 1];
        if (b > a) {
            nnz += (unsigned long long)(b - a - 1) * 8ull;
#pragma unroll
            for (int i = 0; i < 8; ++i) nnz += cols[(size_t)(b - 1) * 8 + i] != (uint16_t)n_cols ? 1ull : 0ull;
        }
    }
    for (int o = 32; o > 0; o >>= 1) nnz += __shfl_xor(nnz, o, 64);
    if ((threadIdx.x & 63) == 0 && nnz) atomicAdd(out, nnz);
}

// the new handle's bitmap: every row it can ever hold live (the layout of mutable.hip: whole 16-byte quads over max(rows_cap, n_rows) rows)
int alloc_live(vs_index* idx, int64_t n_rows) {
    const int64_t words = (bit_words(std::max(idx->rows_cap, n_rows)) + 3) / 4 * 4;
    VS_TRY(idx->live.alloc(std::max<size_t>((size_t)words * 4, 16)));
    VS_TRY(idx->dead_cnt.alloc(8));
    VS_HIP(hipMemset(idx->live.p, 0xFF, idx->live.bytes));
    VS_HIP(hipMemset(idx->dead_cnt.p, 0, 8));
    return VS_OK;
}

}  // namespace

extern "C" int vs_select_plan(int64_t n_ids, int64_t* out_scratch_bytes) {
    char msg[512] = {0};
    SelectPlan p;
    const int rc = select_plan(n_ids, &p, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    if (out_scratch_bytes) *out_scratch_bytes = p.scratch_bytes;
    return VS_OK;
}

extern "C" int vs_select_split(const int64_t* ids, int64_t n, const int64_t* cuts, int32_t n_shards, int64_t* out_begin) {
    char msg[512] = {0};
    const int rc = select_split_by_shard(ids, n, cuts, n_shards, out_begin, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    return VS_OK;
}

extern "C" int vs_index_select_rows(const vs_index* src, const int64_t* ids, int64_t n, int64_t id_offset, int64_t rows_extra, int64_t packets_extra, int device,
                                    vs_index** out) {
    char msg[512] = {0};
    if (out) *out = nullptr;
    int rc = select_check_args(src != nullptr, ids != nullptr, out != nullptr, n, rows_extra, packets_extra, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    SelectPlan plan;
    rc = select_plan(n, &plan, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    VS_TRY(need_device());
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range (have %d)", device, ndev);
    SelectShape shape;
    shape.kind = src->kind;
    shape.device = src->device;
    shape.n_rows = src->n_rows;
    rc = select_check_dense(shape, rows_extra, packets_extra, device, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    const bool dense = src->kind != VS_KIND_CSR;
    const bool ids_dev = is_device_ptr(ids);
    if (ids_dev) {
        hipPointerAttribute_t attr;
        VS_HIP(hipPointerGetAttributes(&attr, ids));
        if (attr.device != src->device) return fail(VS_EINVAL, "ids lives on device %d, the index on device %d", attr.device, src->device);
    } else {
        rc = select_check_host_ids(ids, n, id_offset, src->n_rows, msg, sizeof msg);
        if (rc != VS_OK) return fail(rc, "%s", msg);
    }
    VS_HIP(hipSetDevice(src->device));
    VS_HIP(hipDeviceSynchronize());                            // deletions and ids enqueued on a caller's stream; everything below runs on the null stream
    const uint32_t* live = src->has_tomb ? src->live.as<uint32_t>() : nullptr;
    const uint32_t* pk = dense ? nullptr : src->pk_ptr.as<uint32_t>();
    DevBuf stage, sums, cnt;
    const void* d_ids_v = nullptr;
    VS_TRY(to_device(ids, (size_t)n * 8, stage, 0, &d_ids_v));
    const int64_t* d_ids = (const int64_t*)d_ids_v;
    // 1. stat and scan: the range check, the packets of the selection
    const int64_t n_blocks = plan.scan_blocks;
    VS_TRY(sums.alloc((size_t)n_blocks * 8 + sizeof(SelectTotals)));
    VS_TRY(cnt.alloc(16));                                     // [0] non-zeros, [1] dead rows
    uint2* d_sums = sums.as<uint2>();
    SelectTotals* d_tot = reinterpret_cast<SelectTotals*>(d_sums + n_blocks);
    VS_HIP(hipMemset(d_tot, 0, sizeof(SelectTotals)));
    VS_HIP(hipMemset(cnt.p, 0, 16));
    hipLaunchKernelGGL(select_stat_kernel, dim3((unsigned)n_blocks), dim3(256), 0, 0, d_ids, n, id_offset, src->n_rows, pk, d_sums, d_tot);
    hipLaunchKernelGGL(scan_block_sums_kernel<0>, dim3(1), dim3(1024), 0, 0, d_sums, n_blocks, &d_tot->total);
    VS_HIP(hipGetLastError());
    SelectTotals tot;
    VS_HIP(hipMemcpy(&tot, d_tot, sizeof tot, hipMemcpyDeviceToHost));
    if (tot.bad) return fail(VS_EINVAL, "the selection holds a document id outside [%lld, %lld)", (long long)id_offset, (long long)(id_offset + src->n_rows));
    const int64_t p_new = (int64_t)tot.packets;
    unsigned long long* d_nnz = cnt.as<unsigned long long>();
    unsigned long long* d_dead = d_nnz + 1;
    vs_index* idx = nullptr;
    struct Guard { vs_index* p; ~Guard() { if (p) vs_index_destroy(p); } } guard{nullptr};
    if (!dense) {
        rc = select_check_capacity(n, p_new, rows_extra, packets_extra, msg, sizeof msg);
        if (rc != VS_OK) return fail(rc, "%s", msg);
        const size_t vb = src->store_dtype == VS_F32 ? 32 : (src->store_dtype == VS_F16 ? 16 : 0);
        if (vs_index_create_reserved(n + rows_extra, p_new + packets_extra, src->n_cols, src->store_dtype, src->device, &idx) != VS_OK) {
            const size_t need = (size_t)(p_new + packets_extra) * (16 + vb) + (size_t)(n + rows_extra + 1) * 4;
            return fail(VS_ENOMEM, "the selection needs %zu bytes of HBM for the new index next to the source's (drop the postings copy of the source, or select onto fewer rows)", need);
        }
        guard.p = idx;
        if (live) VS_TRY(alloc_live(idx, n));
        // 2. map
        hipLaunchKernelGGL(select_map_kernel, dim3((unsigned)n_blocks), dim3(256), 0, 0, d_ids, n, id_offset, src->n_rows, pk, (const uint2*)d_sums,
                           idx->pk_ptr.as<uint32_t>(), live, idx->live.as<uint32_t>(), d_dead);
        VS_HIP(hipGetLastError());
        const uint32_t last = (uint32_t)p_new;
        VS_HIP(hipMemcpy(idx->pk_ptr.as<uint32_t>() + n, &last, 4, hipMemcpyHostToDevice));
        // 3. gather
        if (p_new > 0) {
            const unsigned grid = grid_for((n + kSelectRun - 1) / kSelectRun, 4, (int64_t)src->cu_count * 32);
            const uint4 *sc = src->cols.as<uint4>(), *sv = src->vals.as<uint4>();
            uint4 *dc = idx->cols.as<uint4>(), *dv = idx->vals.as<uint4>();
            const uint32_t* npk = idx->pk_ptr.as<uint32_t>();
            if (vb == 32) hipLaunchKernelGGL(select_gather_kernel<32>, dim3(grid), dim3(256), 0, 0, d_ids, id_offset, pk, npk, n, sc, sv, dc, dv);
            else if (vb == 16) hipLaunchKernelGGL(select_gather_kernel<16>, dim3(grid), dim3(256), 0, 0, d_ids, id_offset, pk, npk, n, sc, sv, dc, dv);
            else hipLaunchKernelGGL(select_gather_kernel<0>, dim3(grid), dim3(256), 0, 0, d_ids, id_offset, pk, npk, n, sc, sv, dc, dv);
            VS_HIP(hipGetLastError());
        }
        // 4. non-zeros
        hipLaunchKernelGGL(select_nnz_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, 0, idx->pk_ptr.as<uint32_t>(), n, idx->cols.as<uint16_t>(), src->n_cols, d_nnz);
        VS_HIP(hipGetLastError());
        unsigned long long counts[2] = {0ull, 0ull};
        VS_HIP(hipMemcpy(counts, cnt.p, 16, hipMemcpyDeviceToHost));
        idx->n_rows = n;
        idx->n_packets = p_new;
        idx->nnz = (int64_t)counts[0];
        idx->logical_dense = src->logical_dense;
        idx->lanes_per_row = pick_lanes(p_new, n);
    } else {
        idx = new (std::nothrow) vs_index();
        if (!idx) return fail(VS_ENOMEM, "host allocation failed");
        guard.p = idx;
        idx->kind = VS_KIND_DENSE;
        idx->device = src->device;
        idx->cu_count = src->cu_count;
        idx->store_dtype = src->store_dtype;
        idx->n_rows = n;
        idx->n_cols = src->n_cols;
        idx->nnz = n * (int64_t)src->n_cols;
        const size_t row_bytes = src->mat.bytes / (size_t)src->n_rows;     // the padded row (dense.hip: a multiple of 32 floats)
        if (idx->mat.alloc((size_t)n * row_bytes) != VS_OK)
            return fail(VS_ENOMEM, "the selection needs %zu bytes of HBM for the new matrix next to the source's", (size_t)n * row_bytes);
        if (live) {
            VS_TRY(alloc_live(idx, n));
            hipLaunchKernelGGL(select_map_kernel, dim3((unsigned)n_blocks), dim3(256), 0, 0, d_ids, n, id_offset, src->n_rows, pk, (const uint2*)d_sums,
                               (uint32_t*)nullptr, live, idx->live.as<uint32_t>(), d_dead);
        }
        const int64_t qpr = (int64_t)(row_bytes / 16);
        hipLaunchKernelGGL(select_dense_kernel, dim3(grid_for(n * qpr, 256, (int64_t)src->cu_count * 32)), dim3(256), 0, 0, d_ids, id_offset, n, qpr,
                           src->mat.as<uint4>(), idx->mat.as<uint4>());
        VS_HIP(hipGetLastError());
    }
    if (live) {                                                 // the dead count the map kernel found
        unsigned long long dead = 0;
        VS_HIP(hipMemcpy(&dead, d_dead, 8, hipMemcpyDeviceToHost));
        if (dead > 0) {
            VS_HIP(hipMemcpy(idx->dead_cnt.p, &dead, 8, hipMemcpyHostToDevice));
            idx->has_tomb = true;
        } else {                                                // no selected row is deleted: a handle without a live bitmap, as from a source without tombstones
            VS_HIP(hipDeviceSynchronize());
            idx->live.release();
            idx->dead_cnt.release();
        }
    }
    VS_HIP(hipDeviceSynchronize());
    if (device != src->device) {                                // the new index moves to its GPU, its tombstones behind it; the copy on the source's GPU is dropped
        vs_index* moved = nullptr;
        VS_TRY(move_csr(idx, device, &moved));
        struct Guard moved_guard{moved};
        VS_TRY(tomb_from_bits(moved, idx, 0));
        VS_HIP(hipSetDevice(src->device));
        vs_index_destroy(idx);
        guard.p = nullptr;
        idx = moved;
        moved_guard.p = nullptr;
    }
    guard.p = nullptr;
    *out = idx;
    return VS_OK;
}
