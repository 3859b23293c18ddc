// select.hip -- the sub-index: any rows of a stored index, in any order and with repeats, as a NEW index (vs_index_select_rows).  Packets are
// copied whole, so a row scores bit for bit what it scored in the source; the source's tombstones travel with the rows.  No reference
// counterpart: the reference's index is a tensor that is indexed and rebuilt (index.py:163-179).  Four steps: stat and scan, map, gather, recount
// (the last one and the scaffold of the call: new_index.h).  vs_index_compact (mutable.hip) is the same call over the live rows: it runs the
// gather of this file (launch_packet_gather).  The host-only part is select_check.h.
#include "block_scan.h"
#include "common.h"
#include "new_index.h"
#include "select_check.h"

#include <algorithm>

using namespace vs;

static_assert(kSelectScanRows == kScanRows, "the plan counts the scan blocks of block_scan.h");

namespace {

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
// two whole words of the new bitmap (live_words_from_ballot); *dead counts the cleared ones
__global__ __launch_bounds__(256) void select_map_kernel(const int64_t* ids, int64_t n, int64_t id_offset, int64_t n_rows, const uint32_t* pk, const uint2* sums,
                                                         uint32_t* new_pk, const uint32_t* src_live, uint32_t* new_live, unsigned long long* dead) {
    __shared__ uint2 sh[4];
    const int64_t i0 = (int64_t)blockIdx.x * kScanRows;
    uint2 carry = sums[blockIdx.x];
    for (int it = 0; it < kScanItems; ++it) {
        const int64_t i = i0 + it * 256 + threadIdx.x;
        const int64_t row = i < n ? row_of(ids, i, id_offset, n_rows) : -1;     // (every id was checked by the stat kernel)
        const uint2 v = row >= 0 ? make_uint2(1u, pk ? pk[row + 1] - pk[row] : 0u) : make_uint2(0u, 0u);
        uint2 tot;
        const uint2 ex = block_excl_scan<4>(v, sh, &tot);
        if (row >= 0 && new_pk) new_pk[i] = carry.y + ex.y;
        if (src_live) live_words_from_ballot(row >= 0 && !((src_live[row >> 5] >> (row & 31)) & 1u), i, n, new_live, dead);
        carry = add2(carry, tot);
    }
}

// step 3 (gather).  A wave takes a run of 64 new rows: their packets are one contiguous range of the new index, lane p of it finds its row among
// the run's row pointers (held one a lane, searched with shuffles) and copies the packet whole -- 16
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

}  // namespace

namespace vs {

int launch_packet_gather(const vs_index* src, const int64_t* d_ids, int64_t id_offset, const uint32_t* new_pk, int64_t n_new, uint4* dst_cols, uint4* dst_vals) {
    const unsigned grid = grid_for((n_new + kSelectRun - 1) / kSelectRun, 4, (int64_t)src->cu_count * 32);
    const uint32_t* pk = src->pk_ptr.as<uint32_t>();
    const uint4 *sc = src->cols.as<uint4>(), *sv = src->vals.as<uint4>();
    const size_t vb = value_bytes(src->store_dtype);
    if (vb == 32) hipLaunchKernelGGL(select_gather_kernel<32>, dim3(grid), dim3(256), 0, 0, d_ids, id_offset, pk, new_pk, n_new, sc, sv, dst_cols, dst_vals);
    else if (vb == 16) hipLaunchKernelGGL(select_gather_kernel<16>, dim3(grid), dim3(256), 0, 0, d_ids, id_offset, pk, new_pk, n_new, sc, sv, dst_cols, dst_vals);
    else hipLaunchKernelGGL(select_gather_kernel<0>, dim3(grid), dim3(256), 0, 0, d_ids, id_offset, pk, new_pk, n_new, sc, sv, dst_cols, dst_vals);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

}  // namespace vs

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
    VS_TRY(device_in_range(device));
    SelectShape shape;
    shape.kind = src->kind;
    shape.device = src->device;
    shape.n_rows = src->n_rows;
    rc = select_check_dense(shape, rows_extra, packets_extra, device, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    const bool dense = src->kind != VS_KIND_CSR;
    const bool ids_dev = is_device_ptr(ids);
    VS_TRY(ptr_on(ids, ids_dev, src->device, "ids"));
    if (!ids_dev) {
        rc = select_check_host_ids(ids, n, id_offset, src->n_rows, msg, sizeof msg);
        if (rc != VS_OK) return fail(rc, "%s", msg);
    }
    VS_TRY(open_sources(src->device));
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
    IndexGuard guard{nullptr};
    if (!dense) {
        rc = new_index_check_capacity("selected", n, p_new, rows_extra, packets_extra, msg, sizeof msg);
        if (rc != VS_OK) return fail(rc, "%s", msg);
        VS_TRY(new_csr_index("the selection", "source's (drop the postings copy of the source, or select onto fewer rows)", n, p_new, rows_extra, packets_extra,
                             src->n_cols, src->store_dtype, src->device, &guard));
    } else {
        VS_TRY(new_dense_rows("the selection", src, d_ids, id_offset, n, &guard));
    }
    vs_index* idx = guard.p;
    if (live) VS_TRY(alloc_live(idx, n));
    // 2. map (a dense matrix has no row pointers: only the live words, when there are tombstones)
    if (!dense || live)
        hipLaunchKernelGGL(select_map_kernel, dim3((unsigned)n_blocks), dim3(256), 0, 0, d_ids, n, id_offset, src->n_rows, pk, (const uint2*)d_sums,
                           dense ? (uint32_t*)nullptr : idx->pk_ptr.as<uint32_t>(), live, idx->live.as<uint32_t>(), d_dead);
    VS_HIP(hipGetLastError());
    if (!dense) {
        const uint32_t last = (uint32_t)p_new;
        VS_HIP(hipMemcpy(idx->pk_ptr.as<uint32_t>() + n, &last, 4, hipMemcpyHostToDevice));
        // 3. gather
        if (p_new > 0) VS_TRY(launch_packet_gather(src, d_ids, id_offset, idx->pk_ptr.as<uint32_t>(), n, idx->cols.as<uint4>(), idx->vals.as<uint4>()));
        // 4. non-zeros
        VS_TRY(launch_nnz_recount(idx, n, d_nnz));
        unsigned long long nnz = 0;
        VS_HIP(hipMemcpy(&nnz, d_nnz, 8, hipMemcpyDeviceToHost));
        set_csr_shape(idx, n, p_new, (int64_t)nnz, src->logical_dense);
    }
    if (live) VS_TRY(settle_dead(idx, d_dead));
    return hand_over(guard, src->device, device, TombFrom::own_bits(), out);   // the tombstones travel behind the index
}
