// new_index.hip -- the host scaffold and the kernels the calls that return a NEW index share (new_index.h).  No reference
// counterpart: the reference's index is a tensor that is rebuilt (index.py:163-179).  Nothing here touches a walk or scan kernel.
#include "new_index.h"

#include "block_scan.h"

namespace vs {

int need_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(VS_ENODEVICE, "no HIP device visible: libvsearch_hip has no CPU fallback");
    }
    return VS_OK;
}

int device_in_range(int device) {
    VS_TRY(need_device());
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range (have %d)", device, ndev);
    return VS_OK;
}

int ptr_on(const void* p, bool on_device, int device, const char* what) {
    if (!on_device) return VS_OK;
    hipPointerAttribute_t attr;
    VS_HIP(hipPointerGetAttributes(&attr, p));
    if (attr.device != device) return fail(VS_EINVAL, "%s lives on device %d, the index on device %d", what, attr.device, device);
    return VS_OK;
}

int open_sources(int device_of_sources) {
    VS_HIP(hipSetDevice(device_of_sources));
    VS_HIP(hipDeviceSynchronize());
    return VS_OK;
}

int new_csr_index(const char* verb, const char* hint, int64_t rows, int64_t packets, int64_t rows_extra, int64_t packets_extra, int32_t n_cols, int dtype,
                  int device, IndexGuard* guard) {
    if (vs_index_create_reserved(rows + rows_extra, packets + packets_extra, n_cols, dtype, device, &guard->p) != VS_OK)
        return fail(VS_ENOMEM, "%s needs %zu bytes of HBM for the new index next to the %s", verb,
                    new_index_bytes(rows + rows_extra, packets + packets_extra, value_bytes(dtype)), hint);
    return VS_OK;
}

void set_csr_shape(vs_index* idx, int64_t rows, int64_t packets, int64_t nnz, bool logical_dense) {
    idx->n_rows = rows;
    idx->n_packets = packets;
    idx->nnz = nnz;
    idx->logical_dense = logical_dense;
    idx->lanes_per_row = pick_lanes(packets, rows);
}

int pick_lanes(int64_t n_packets, int64_t n_rows) {             // (csr_index.hip: pick_lanes_per_row)
    const double mp = n_rows > 0 ? (double)n_packets / (double)n_rows : 1.0;
    int g = 4;
    while (g < 64 && mp / g > 4.0) g <<= 1;
    return g;
}

// peer copies: a call across devices works on the sources' GPU first
int move_csr(const vs_index* a, int device, vs_index** out) {
    IndexGuard guard{nullptr};
    VS_TRY(vs_index_create_reserved(a->rows_cap, a->packets_cap, a->n_cols, a->store_dtype, device, &guard.p));
    vs_index* idx = guard.p;
    const size_t vb = value_bytes(a->store_dtype);
    VS_HIP(hipMemcpyPeer(idx->pk_ptr.p, device, a->pk_ptr.p, a->device, (size_t)(a->n_rows + 1) * 4));
    if (a->n_packets) VS_HIP(hipMemcpyPeer(idx->cols.p, device, a->cols.p, a->device, (size_t)a->n_packets * 16));
    if (a->n_packets && vb) VS_HIP(hipMemcpyPeer(idx->vals.p, device, a->vals.p, a->device, (size_t)a->n_packets * vb));
    idx->n_rows = a->n_rows;
    idx->n_packets = a->n_packets;
    idx->nnz = a->nnz;
    idx->logical_dense = a->logical_dense;
    idx->lanes_per_row = a->lanes_per_row;
    guard.p = nullptr;
    *out = idx;
    return VS_OK;
}

int alloc_live(vs_index* idx, int64_t rows) {
    const int64_t words = (bit_words(std::max(idx->rows_cap, rows)) + 3) / 4 * 4;
    VS_TRY(idx->live.alloc(std::max<size_t>((size_t)words * 4, 16)));
    VS_TRY(idx->dead_cnt.alloc(8));
    VS_HIP(hipMemset(idx->live.p, 0xFF, idx->live.bytes));
    VS_HIP(hipMemset(idx->dead_cnt.p, 0, 8));
    return VS_OK;
}

int settle_dead(vs_index* idx, const unsigned long long* d_dead) {
    unsigned long long dead = 0;
    VS_HIP(hipMemcpy(&dead, d_dead, 8, hipMemcpyDeviceToHost));
    if (dead > 0) {
        VS_HIP(hipMemcpy(idx->dead_cnt.p, &dead, 8, hipMemcpyHostToDevice));
        idx->has_tomb = true;
    } else {                                                    // no new row is deleted: a handle without a live bitmap, as from sources without tombstones
        VS_HIP(hipDeviceSynchronize());
        idx->live.release();
        idx->dead_cnt.release();
    }
    return VS_OK;
}

int hand_over(IndexGuard& guard, int src_device, int device, const TombFrom& tomb, vs_index** out) {
    VS_HIP(hipDeviceSynchronize());
    if (device != src_device) {
        vs_index* moved = nullptr;
        VS_TRY(move_csr(guard.p, device, &moved));
        IndexGuard moved_guard{moved};
        if (tomb.kind == TombFrom::kOwnBits) VS_TRY(tomb_from_bits(moved, guard.p, 0));
        VS_HIP(hipSetDevice(src_device));
        vs_index_destroy(guard.p);
        guard.p = moved;
        moved_guard.p = nullptr;
    }
    // rows 1:1 with a source's: deleted rows stay deleted, restore() brings them back as the call made them
    if (tomb.kind == TombFrom::kSourceBits) VS_TRY(tomb_from_bits(guard.p, tomb.src, 0));
    if (tomb.kind == TombFrom::kHostWords) VS_TRY(tomb_from_host(guard.p, tomb.words));
    *out = guard.p;
    guard.p = nullptr;
    return VS_OK;
}

// =================================================================================================
// kernels more than one call runs
// =================================================================================================
namespace {

__global__ __launch_bounds__(256) void nnz_recount_kernel(const uint32_t* pk, int64_t n_rows, const uint16_t* cols, int32_t n_cols, unsigned long long* out) {
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

// dense (matrix-core) index: row gather of the padded matrix, 16 bytes a lane (the padded row is a multiple of 32 floats)
__global__ __launch_bounds__(256) void dense_gather_kernel(const int64_t* ids, int64_t id_offset, int64_t n_new, int64_t quads_per_row, const uint4* src, uint4* dst) {
    const int64_t n = n_new * quads_per_row;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t j = i / quads_per_row, c = i % quads_per_row;
        dst[i] = src[(size_t)(ids[j] - id_offset) * (size_t)quads_per_row + (size_t)c];
    }
}

// (cells, packets) of row r; a row past the end counts nothing
__device__ __forceinline__ uint2 cells_stat(const int32_t* cells, int64_t r, int64_t n_rows) {
    if (r >= n_rows) return make_uint2(0u, 0u);
    const uint32_t k = (uint32_t)cells[r] & 0x7FFFFFFFu;
    return make_uint2(k, (k + 7u) >> 3);
}

// (a block's cells fit 32 bits: 4096 rows x 65535; their sum over the index goes to *nnz, the scanned .x of the block sums is not used)
__global__ __launch_bounds__(256) void cells_sums_kernel(const int32_t* cells, int64_t n_rows, uint2* sums, unsigned long long* nnz) {
    __shared__ uint2 sh[4];
    const int64_t r0 = (int64_t)blockIdx.x * kScanRows;
    uint2 acc = make_uint2(0u, 0u);
    for (int it = 0; it < kScanItems; ++it) acc = add2(acc, cells_stat(cells, r0 + it * 256 + threadIdx.x, n_rows));
    uint2 tot;
    (void)block_excl_scan<4>(acc, sh, &tot);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = tot;
        if (tot.x) atomicAdd(nnz, (unsigned long long)tot.x);
    }
}

__global__ __launch_bounds__(256) void cells_map_kernel(const int32_t* cells, int64_t n_rows, const uint2* sums, uint32_t* new_pk) {
    __shared__ uint2 sh[4];
    const int64_t r0 = (int64_t)blockIdx.x * kScanRows;
    uint2 carry = sums[blockIdx.x];
    for (int it = 0; it < kScanItems; ++it) {
        const int64_t r = r0 + it * 256 + threadIdx.x;
        const uint2 v = cells_stat(cells, r, n_rows);
        uint2 tot;
        const uint2 ex = block_excl_scan<4>(v, sh, &tot);
        if (r < n_rows) new_pk[r] = carry.y + ex.y;
        carry = add2(carry, tot);
    }
}

}  // namespace

int launch_nnz_recount(const vs_index* idx, int64_t rows, unsigned long long* d_nnz) {
    if (rows > 0)
        hipLaunchKernelGGL(nnz_recount_kernel, dim3(grid_for(rows, 256, 4096)), dim3(256), 0, 0, idx->pk_ptr.as<uint32_t>(), rows, idx->cols.as<uint16_t>(), idx->n_cols,
                           d_nnz);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int new_dense_rows(const char* verb, const vs_index* src, const int64_t* ids, int64_t id_offset, int64_t rows, IndexGuard* guard) {
    vs_index* idx = new (std::nothrow) vs_index();
    if (!idx) return fail(VS_ENOMEM, "host allocation failed");
    guard->p = idx;
    idx->kind = VS_KIND_DENSE;
    idx->device = src->device;
    idx->cu_count = src->cu_count;
    idx->store_dtype = src->store_dtype;
    idx->n_rows = rows;
    idx->n_cols = src->n_cols;
    idx->nnz = rows * (int64_t)src->n_cols;
    const size_t row_bytes = src->mat.bytes / (size_t)src->n_rows;         // the padded row (dense.hip: a multiple of 32 floats)
    if (idx->mat.alloc((size_t)rows * row_bytes) != VS_OK)
        return fail(VS_ENOMEM, "%s needs %zu bytes of HBM for the new matrix next to the source's", verb, (size_t)rows * row_bytes);
    const int64_t qpr = (int64_t)(row_bytes / 16);
    hipLaunchKernelGGL(dense_gather_kernel, dim3(grid_for(rows * qpr, 256, (int64_t)src->cu_count * 32)), dim3(256), 0, 0, ids, id_offset, rows, qpr,
                       src->mat.as<uint4>(), idx->mat.as<uint4>());
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int cells_scan(const int32_t* d_cells, int64_t n_rows, int64_t scan_blocks, uint2* d_sums, unsigned long long* d_nnz, int64_t* packets) {
    hipLaunchKernelGGL(cells_sums_kernel, dim3((unsigned)scan_blocks), dim3(256), 0, 0, d_cells, n_rows, d_sums, d_nnz);
    hipLaunchKernelGGL(scan_block_sums_kernel<0>, dim3(1), dim3(1024), 0, 0, d_sums, scan_blocks, d_sums + scan_blocks);
    VS_HIP(hipGetLastError());
    uint32_t tot[2] = {0u, 0u};
    VS_HIP(hipMemcpy(tot, d_sums + scan_blocks, 8, hipMemcpyDeviceToHost));
    *packets = tot[1];
    return VS_OK;
}

int cells_row_pointers(const int32_t* d_cells, int64_t n_rows, int64_t scan_blocks, const uint2* d_sums, int64_t packets, uint32_t* new_pk) {
    hipLaunchKernelGGL(cells_map_kernel, dim3((unsigned)scan_blocks), dim3(256), 0, 0, d_cells, n_rows, d_sums, new_pk);
    VS_HIP(hipGetLastError());
    const uint32_t last = (uint32_t)packets;
    VS_HIP(hipMemcpy(new_pk + n_rows, &last, 4, hipMemcpyHostToDevice));
    return VS_OK;
}

}  // namespace vs
