// mutable.hip -- the writable index: tombstones kept in the handle (delete / restore rows, applied by every search as a document filter)
// and compaction (a new index of the live rows, with spare capacity for appends: the scan and the map that finds the live rows are here, the
// rest is the scaffold and the shared kernels of new_index.h -- the packets move by the gather of select.hip).  No reference counterpart: the reference's index is
// a tensor that is rebuilt (index.py:163-179).  Nothing here touches a walk or scan kernel: deletion reaches them as FilterArgs.
#include "block_scan.h"
#include "common.h"
#include "new_index.h"

#include <algorithm>

using namespace vs;

namespace {

// words of the handle's live bitmap: the rows it can ever hold, rounded to whole 16-byte quads (the AND kernel reads and writes quads)
int64_t live_words(const vs_index* idx) { return (bit_words(std::max(idx->rows_cap, idx->n_rows)) + 3) / 4 * 4; }

// ---- bit clear / set from an id list: one thread an id; the dead count moves by what the atomic found (duplicates count once) --------
template <int DEL>
__global__ __launch_bounds__(256) void tomb_update_kernel(const int64_t* ids, int64_t n, int64_t id_offset, int64_t n_rows, uint32_t* live,
                                                          unsigned long long* dead) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t id = ids[i], row = id - id_offset;
        if (id == -1 || row < 0 || row >= n_rows) continue;              // (never dereferenced: not a row of this index)
        const uint32_t bit = 1u << (row & 31);
        if (DEL) {
            const uint32_t old = atomicAnd(&live[row >> 5], ~bit);
            if (old & bit) atomicAdd(dead, 1ull);
        } else {
            const uint32_t old = atomicOr(&live[row >> 5], bit);
            if (!(old & bit)) atomicAdd(dead, ~0ull);                     // (- 1)
        }
    }
}

// ---- effective filter: out[b][w] = live[w] & (user bitmap of query b from bit `bit0` on), re-based to bit 0 --------------------------
// A lane takes four output words (16-byte load of `live`, 16-byte store); the user's words start at an arbitrary word and bit -- a shard of
// a group reads the global bitmap from its first row -- so five neighbouring words are funnel-shifted into four.  live == nullptr: all
// ones (a plain re-base).  Words of the user's bitmap past `span` (what it is promised to hold) are not read.
struct AndArgs {
    const uint32_t* live;
    const uint32_t* user;
    int64_t user_ld, bit0, span;
    uint32_t* out;
    int64_t out_ld, n_quads;
};
__global__ __launch_bounds__(256) void live_and_kernel(AndArgs a) {
    const uint32_t* u = a.user + (size_t)blockIdx.y * (size_t)a.user_ld;
    uint4* o = reinterpret_cast<uint4*>(a.out + (size_t)blockIdx.y * (size_t)a.out_ld);
    const int64_t w0 = a.bit0 >> 5;
    const uint32_t sh = (uint32_t)(a.bit0 & 31);
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < a.n_quads; q += (int64_t)gridDim.x * 256) {
        uint4 lv = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (a.live) lv = reinterpret_cast<const uint4*>(a.live)[q];
        uint32_t x[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int64_t w = w0 + 4 * q + i;
            x[i] = w < a.span ? u[w] : 0u;
        }
        uint4 r;
        r.x = lv.x & __funnelshift_r(x[0], x[1], sh);
        r.y = lv.y & __funnelshift_r(x[1], x[2], sh);
        r.z = lv.z & __funnelshift_r(x[2], x[3], sh);
        r.w = lv.w & __funnelshift_r(x[3], x[4], sh);
        o[q] = r;
    }
}

// set bits among rows [0, n_rows) of a bitmap
__global__ __launch_bounds__(256) void count_bits_kernel(const uint32_t* words, int64_t n_rows, unsigned long long* out) {
    const int64_t nw = (n_rows + 31) >> 5;
    unsigned long long c = 0;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < nw; w += (int64_t)gridDim.x * 256) {
        uint32_t v = words[w];
        if (w == nw - 1 && (n_rows & 31)) v &= (1u << (n_rows & 31)) - 1u;
        c += __popc(v);
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// the bitmap a caller inspects: bits of rows [0, n_rows), zeros behind them (live == nullptr: every row live)
__global__ __launch_bounds__(256) void live_out_kernel(const uint32_t* live, int64_t n_rows, uint32_t* out, int64_t n_words) {
    const int64_t nw = (n_rows + 31) >> 5;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * 256) {
        uint32_t v = w < nw ? (live ? live[w] : ~0u) : 0u;
        if (w == nw - 1 && (n_rows & 31)) v &= (1u << (n_rows & 31)) - 1u;
        out[w] = v;
    }
}

// the handle's bitmap, allocated on the first deletion: every row (and every row still to be appended) live
int ensure_live(vs_index* idx, hipStream_t s) {
    const size_t bytes = (size_t)live_words(idx) * 4;
    if (idx->live.p && idx->live.bytes >= bytes && idx->dead_cnt.p) return VS_OK;
    VS_TRY(idx->live.alloc(std::max<size_t>(bytes, 16)));
    VS_TRY(idx->dead_cnt.alloc(8));
    VS_HIP(hipMemsetAsync(idx->live.p, 0xFF, idx->live.bytes, s));
    VS_HIP(hipMemsetAsync(idx->dead_cnt.p, 0, 8, s));
    return VS_OK;
}

int tomb_update(vs_index* idx, const int64_t* ids, int64_t n, int64_t id_offset, void* stream, bool del) {
    VS_TRY(need_device());
    if (!idx) return fail(VS_EINVAL, "NULL index");
    if (n < 0) return fail(VS_EINVAL, "n must be >= 0");
    if (!ids && n > 0 && del) return fail(VS_EINVAL, "ids is NULL");
    VS_HIP(hipSetDevice(idx->device));
    hipStream_t s = (hipStream_t)stream;
    if (!del && !ids) {                                        // restore all: the bitmap is kept for the next deletion, searches go back to FL = 0
        if (idx->live.p) {
            VS_HIP(hipMemsetAsync(idx->live.p, 0xFF, idx->live.bytes, s));
            VS_HIP(hipMemsetAsync(idx->dead_cnt.p, 0, 8, s));
        }
        idx->has_tomb = false;
        if (!stream) VS_HIP(hipStreamSynchronize(s));
        return VS_OK;
    }
    if (n == 0) return VS_OK;
    const bool dev_ids = is_device_ptr(ids);
    VS_TRY(ptr_on(ids, dev_ids, idx->device, "ids"));
    if (!dev_ids)
        for (int64_t i = 0; i < n; ++i) {
            const int64_t row = ids[i] - id_offset;
            if (ids[i] != -1 && (row < 0 || row >= idx->n_rows))
                return fail(VS_EINVAL, "document id %lld is outside [%lld, %lld)", (long long)ids[i], (long long)id_offset, (long long)(id_offset + idx->n_rows));
        }
    if (!del && !idx->live.p) return VS_OK;                    // nothing was ever deleted
    VS_TRY(ensure_live(idx, s));
    DevBuf stage;
    const void* d_ids = nullptr;
    VS_TRY(to_device(ids, (size_t)n * 8, stage, s, &d_ids));
    if (del)
        hipLaunchKernelGGL(tomb_update_kernel<1>, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, (const int64_t*)d_ids, n, id_offset, idx->n_rows, idx->live.as<uint32_t>(),
                           idx->dead_cnt.as<unsigned long long>());
    else
        hipLaunchKernelGGL(tomb_update_kernel<0>, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, (const int64_t*)d_ids, n, id_offset, idx->n_rows, idx->live.as<uint32_t>(),
                           idx->dead_cnt.as<unsigned long long>());
    VS_HIP(hipGetLastError());
    if (del) idx->has_tomb = true;
    if (!stream || stage.p) VS_HIP(hipStreamSynchronize(s));   // blocking call / the staged ids die here
    return VS_OK;
}

}  // namespace

// =================================================================================================
// what the rest of the library asks of the tombstones (common.h)
// =================================================================================================
namespace vs {

int tomb_effective_filter(vs_index* idx, const FilterArgs& user, int32_t B, hipStream_t s, FilterArgs* out) {
    if (!idx->has_tomb) { *out = user; return VS_OK; }
    if (!user.words) {                                         // the live bitmap itself: no copy
        *out = FilterArgs{idx->live.as<uint32_t>(), 0, 0};
        return VS_OK;
    }
    AndArgs a;
    a.live = idx->live.as<uint32_t>();
    a.user = user.words;
    a.user_ld = user.ld;
    a.bit0 = user.bit0;
    a.span = (user.bit0 + idx->n_rows + 31) >> 5;
    a.n_quads = (bit_words(idx->n_rows) + 3) / 4;
    a.out_ld = a.n_quads * 4;
    const int64_t nb = user.ld > 0 ? B : 1;
    if (nb > 65535) return fail(VS_EUNSUPPORTED, "a per-query filter on an index with deleted rows takes at most 65535 queries a call (got %d)", B);
    const size_t bytes = (size_t)nb * (size_t)a.out_ld * 4;
    if (idx->ws_live.reserve(bytes) != VS_OK)
        return fail(VS_ENOMEM, "no room for the %zu bytes of (live rows AND filter) of %lld queries x %lld rows: compact the index, or search in smaller batches",
                    bytes, (long long)nb, (long long)idx->n_rows);
    a.out = idx->ws_live.as<uint32_t>();
    hipLaunchKernelGGL(live_and_kernel, dim3(grid_for(a.n_quads, 256, 4096), (unsigned)nb), dim3(256), 0, s, a);
    VS_HIP(hipGetLastError());
    *out = FilterArgs{a.out, 0, user.ld > 0 ? a.out_ld : 0};
    return VS_OK;
}

int tomb_dead_count(const vs_index* idx, int64_t* out) {
    *out = 0;
    if (!idx->has_tomb) return VS_OK;
    VS_HIP(hipSetDevice(idx->device));
    VS_HIP(hipDeviceSynchronize());
    VS_HIP(hipMemcpy(out, idx->dead_cnt.p, 8, hipMemcpyDeviceToHost));
    return VS_OK;
}

// after new bits were written into idx->live on the null stream: the dead count they imply
static int recount(vs_index* idx) {
    DevBuf cnt;
    VS_TRY(cnt.alloc(8));
    VS_HIP(hipMemset(cnt.p, 0, 8));
    if (idx->n_rows > 0)
        hipLaunchKernelGGL(count_bits_kernel, dim3(grid_for(bit_words(idx->n_rows), 256, 8192)), dim3(256), 0, 0, idx->live.as<uint32_t>(), idx->n_rows,
                           cnt.as<unsigned long long>());
    VS_HIP(hipGetLastError());
    int64_t live = 0;
    VS_HIP(hipMemcpy(&live, cnt.p, 8, hipMemcpyDeviceToHost));
    const int64_t dead = idx->n_rows - live;
    VS_HIP(hipMemcpy(idx->dead_cnt.p, &dead, 8, hipMemcpyHostToDevice));
    idx->has_tomb = dead > 0;
    return VS_OK;
}

int tomb_from_bits(vs_index* dst, const vs_index* src, int64_t row0) {
    if (!src->has_tomb || dst->n_rows == 0) return VS_OK;
    // re-based on the source's device (live_and_kernel with no `live` operand), then copied to the new index's
    VS_HIP(hipSetDevice(src->device));
    AndArgs a;
    a.live = nullptr;
    a.user = src->live.as<uint32_t>();
    a.user_ld = 0;
    a.bit0 = row0;
    a.span = (row0 + dst->n_rows + 31) >> 5;
    a.n_quads = (bit_words(dst->n_rows) + 3) / 4;
    a.out_ld = a.n_quads * 4;
    DevBuf tmp;
    VS_TRY(tmp.alloc((size_t)a.out_ld * 4));
    a.out = tmp.as<uint32_t>();
    hipLaunchKernelGGL(live_and_kernel, dim3(grid_for(a.n_quads, 256, 4096), 1), dim3(256), 0, 0, a);
    VS_HIP(hipGetLastError());
    VS_HIP(hipDeviceSynchronize());
    VS_HIP(hipSetDevice(dst->device));
    VS_TRY(ensure_live(dst, 0));
    VS_HIP(hipDeviceSynchronize());
    if (dst->device == src->device) VS_HIP(hipMemcpy(dst->live.p, tmp.p, (size_t)bit_words(dst->n_rows) * 4, hipMemcpyDeviceToDevice));
    else VS_HIP(hipMemcpyPeer(dst->live.p, dst->device, tmp.p, src->device, (size_t)bit_words(dst->n_rows) * 4));
    // (bits past the slice's last row came from the source's next rows: a slice holds exactly its rows, so they are never read or appended to)
    return recount(dst);
}

int tomb_from_host(vs_index* idx, const uint32_t* words) {
    VS_HIP(hipSetDevice(idx->device));
    VS_TRY(ensure_live(idx, 0));
    VS_HIP(hipDeviceSynchronize());
    VS_HIP(hipMemcpy(idx->live.p, words, (size_t)bit_words(idx->n_rows) * 4, hipMemcpyHostToDevice));
    return recount(idx);
}

int tomb_to_host(const vs_index* idx, std::vector<uint32_t>& words) {
    words.assign((size_t)bit_words(idx->n_rows), 0u);
    if (words.empty()) return VS_OK;
    VS_HIP(hipSetDevice(idx->device));
    DevBuf tmp;
    VS_TRY(tmp.alloc(words.size() * 4));
    hipLaunchKernelGGL(live_out_kernel, dim3(grid_for((int64_t)words.size(), 256, 8192)), dim3(256), 0, 0, idx->has_tomb ? idx->live.as<uint32_t>() : nullptr, idx->n_rows,
                       tmp.as<uint32_t>(), (int64_t)words.size());
    VS_HIP(hipGetLastError());
    VS_HIP(hipMemcpy(words.data(), tmp.p, words.size() * 4, hipMemcpyDeviceToHost));
    return VS_OK;
}

}  // namespace vs

// =================================================================================================
// C entry points: delete / restore / live count / live bitmap
// =================================================================================================
extern "C" int vs_index_delete_rows(vs_index* idx, const int64_t* ids, int64_t n, int64_t id_offset, void* stream) {
    VS_TRY(need_device());
    if (!idx || (!ids && n > 0)) return fail(VS_EINVAL, "NULL argument");
    return tomb_update(idx, ids, n, id_offset, stream, true);
}

extern "C" int vs_index_restore_rows(vs_index* idx, const int64_t* ids, int64_t n, int64_t id_offset, void* stream) {
    VS_TRY(need_device());
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    return tomb_update(idx, ids, n, id_offset, stream, false);
}

extern "C" int vs_index_live_rows(const vs_index* idx, int64_t* out) {
    VS_TRY(need_device());
    if (!idx || !out) return fail(VS_EINVAL, "NULL argument");
    int64_t dead = 0;
    VS_TRY(tomb_dead_count(idx, &dead));
    *out = idx->n_rows - dead;
    return VS_OK;
}

extern "C" int vs_index_live_bitmap(const vs_index* idx, uint32_t* out_words, int64_t n_words) {
    VS_TRY(need_device());
    if (!idx || !out_words) return fail(VS_EINVAL, "NULL argument");
    if (n_words < bit_words(idx->n_rows)) return fail(VS_EINVAL, "n_words = %lld is shorter than the %lld words of %lld rows", (long long)n_words,
                                                      (long long)bit_words(idx->n_rows), (long long)idx->n_rows);
    if (n_words == 0) return VS_OK;
    const bool out_dev = is_device_ptr(out_words);
    VS_TRY(ptr_on(out_words, out_dev, idx->device, "out_words"));
    VS_TRY(open_sources(idx->device));
    DevBuf tmp;
    uint32_t* d = out_words;
    if (!out_dev) {
        VS_TRY(tmp.alloc((size_t)n_words * 4));
        d = tmp.as<uint32_t>();
    }
    hipLaunchKernelGGL(live_out_kernel, dim3(grid_for(n_words, 256, 8192)), dim3(256), 0, 0, idx->has_tomb ? idx->live.as<uint32_t>() : nullptr, idx->n_rows, d, n_words);
    VS_HIP(hipGetLastError());
    if (!out_dev) VS_HIP(hipMemcpy(out_words, d, (size_t)n_words * 4, hipMemcpyDeviceToHost));
    VS_HIP(hipDeviceSynchronize());
    return VS_OK;
}

// =================================================================================================
// compaction
// =================================================================================================
namespace {

// (the scan: block_scan.h -- blocks of kScanRows rows, block_excl_scan inside a block, scan_block_sums_kernel over the block sums)
// (live?, packets) of row r; a dead row and a row past the end count nothing.  pk == nullptr (dense matrix): no packets
__device__ __forceinline__ uint2 row_stat(const uint32_t* live, const uint32_t* pk, int64_t r, int64_t n_rows) {
    if (r >= n_rows) return make_uint2(0u, 0u);
    if (live && !((live[r >> 5] >> (r & 31)) & 1u)) return make_uint2(0u, 0u);
    return make_uint2(1u, pk ? pk[r + 1] - pk[r] : 0u);
}

// step 1a: (live rows, their packets) of every block of kScanRows rows
__global__ __launch_bounds__(256) void compact_sums_kernel(const uint32_t* live, const uint32_t* pk, int64_t n_rows, uint2* sums) {
    __shared__ uint2 sh[4];
    const int64_t r0 = (int64_t)blockIdx.x * kScanRows;
    uint2 acc = make_uint2(0u, 0u);
    for (int it = 0; it < kScanItems; ++it) acc = add2(acc, row_stat(live, pk, r0 + it * 256 + threadIdx.x, n_rows));
    uint2 tot;
    (void)block_excl_scan<4>(acc, sh, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// step 1c: every live row learns its new row id j and first packet: old_ids[j] = row, new_pk[j] = packets of the live rows before it
__global__ __launch_bounds__(256) void compact_map_kernel(const uint32_t* live, const uint32_t* pk, int64_t n_rows, const uint2* sums, int64_t* old_ids,
                                                          uint32_t* new_pk) {
    __shared__ uint2 sh[4];
    const int64_t r0 = (int64_t)blockIdx.x * kScanRows;
    uint2 carry = sums[blockIdx.x];
    for (int it = 0; it < kScanItems; ++it) {
        const int64_t r = r0 + it * 256 + threadIdx.x;
        const uint2 v = row_stat(live, pk, r, n_rows);
        uint2 tot;
        const uint2 ex = block_excl_scan<4>(v, sh, &tot);
        if (v.x) {
            const int64_t j = (int64_t)carry.x + ex.x;
            old_ids[j] = r;
            if (new_pk) new_pk[j] = carry.y + ex.y;
        }
        carry = add2(carry, tot);
    }
}

}  // namespace

extern "C" int vs_index_compact(const vs_index* src, int64_t rows_extra, int64_t packets_extra, int device, vs_index** out, int64_t* out_old_ids) {
    char msg[512] = {0};
    VS_TRY(need_device());
    if (!src || !out) return fail(VS_EINVAL, "NULL argument");
    *out = nullptr;
    if (new_index_check_extra(rows_extra, packets_extra, msg, sizeof msg) != VS_OK) return fail(VS_EINVAL, "%s", msg);
    VS_TRY(device_in_range(device));
    const bool dense = src->kind != VS_KIND_CSR;
    if (dense && (rows_extra || packets_extra)) return fail(VS_EINVAL, "a dense (matrix) index has no append: rows_extra and packets_extra must be 0");
    if (dense && device != src->device) return fail(VS_EUNSUPPORTED, "a dense (matrix) index compacts on its own device");
    const bool ids_dev = is_device_ptr(out_old_ids);
    VS_TRY(ptr_on(out_old_ids, ids_dev, src->device, "out_old_ids"));
    VS_TRY(open_sources(src->device));
    const int64_t n = src->n_rows;
    const uint32_t* live = src->has_tomb ? src->live.as<uint32_t>() : nullptr;
    const uint32_t* pk = dense ? nullptr : src->pk_ptr.as<uint32_t>();
    // 1. scan: live rows and their packets
    const int64_t n_blocks = std::max<int64_t>(1, (n + kScanRows - 1) / kScanRows);
    DevBuf sums;
    VS_TRY(sums.alloc((size_t)(n_blocks + 1) * 8));
    uint2* d_sums = sums.as<uint2>();
    hipLaunchKernelGGL(compact_sums_kernel, dim3((unsigned)n_blocks), dim3(256), 0, 0, live, pk, n, d_sums);
    hipLaunchKernelGGL(scan_block_sums_kernel<0>, dim3(1), dim3(1024), 0, 0, d_sums, n_blocks, d_sums + n_blocks);
    VS_HIP(hipGetLastError());
    uint32_t tot[2] = {0u, 0u};
    VS_HIP(hipMemcpy(tot, d_sums + n_blocks, 8, hipMemcpyDeviceToHost));
    const int64_t n_new = tot[0], p_new = tot[1];
    if (dense && n_new == 0) return fail(VS_EINVAL, "every row is deleted: a dense (matrix) index cannot be empty");
    DevBuf old_buf;
    int64_t* d_old = out_old_ids;
    if (!ids_dev) {
        VS_TRY(old_buf.alloc(std::max<size_t>((size_t)n_new * 8, 8)));
        d_old = old_buf.as<int64_t>();
    }
    IndexGuard guard{nullptr};
    if (!dense) {
        const int rc = new_index_check_capacity("compacted", n_new, p_new, rows_extra, packets_extra, msg, sizeof msg);
        if (rc != VS_OK) return fail(rc, "%s", msg);
        VS_TRY(new_csr_index("compaction", "source's (drop the postings copy of the source, or compact onto another GPU)", n_new, p_new, rows_extra, packets_extra,
                             src->n_cols, src->store_dtype, src->device, &guard));
        vs_index* idx = guard.p;
        hipLaunchKernelGGL(compact_map_kernel, dim3((unsigned)n_blocks), dim3(256), 0, 0, live, pk, n, (const uint2*)d_sums, d_old, idx->pk_ptr.as<uint32_t>());
        VS_HIP(hipGetLastError());
        const uint32_t last = (uint32_t)p_new;
        VS_HIP(hipMemcpy(idx->pk_ptr.as<uint32_t>() + n_new, &last, 4, hipMemcpyHostToDevice));
        // 2. gather: the live rows are a selection, old_ids its id list
        if (p_new > 0) VS_TRY(launch_packet_gather(src, d_old, 0, idx->pk_ptr.as<uint32_t>(), n_new, idx->cols.as<uint4>(), idx->vals.as<uint4>()));
        // 3. non-zeros
        DevBuf cnt;
        VS_TRY(cnt.alloc(8));
        VS_HIP(hipMemset(cnt.p, 0, 8));
        VS_TRY(launch_nnz_recount(idx, n_new, cnt.as<unsigned long long>()));
        unsigned long long nnz = 0;
        VS_HIP(hipMemcpy(&nnz, cnt.p, 8, hipMemcpyDeviceToHost));
        set_csr_shape(idx, n_new, p_new, (int64_t)nnz, src->logical_dense);
    } else {
        hipLaunchKernelGGL(compact_map_kernel, dim3((unsigned)n_blocks), dim3(256), 0, 0, live, pk, n, (const uint2*)d_sums, d_old, (uint32_t*)nullptr);
        VS_TRY(new_dense_rows("compaction", src, d_old, 0, n_new, &guard));
    }
    if (out_old_ids && !ids_dev && n_new > 0) VS_HIP(hipMemcpy(out_old_ids, d_old, (size_t)n_new * 8, hipMemcpyDeviceToHost));
    return hand_over(guard, src->device, device, TombFrom::none(), out);   // the live rows alone: nothing is deleted in the new index
}
