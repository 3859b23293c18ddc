// concat.hip -- the joined index: the rows of several stored indexes, one source behind the other, as a NEW index (vs_index_concat; the contract is
// pinned in vsearch_hip.h).  The reference's counterpart is its load step, vstack(shards) of host matrices (index.py:172-175); here the sources
// are already on the GPU.  Packets are copied whole, so a row scores bit for bit what it scored in a source of the result's dtype; a source of
// another store is converted in registers under vs_index_rescale's rule with no scale; the sources' tombstones travel with the rows.  Two
// launches for ALL sources -- map (row pointers, live words) and copy (packets) -- over a device table of per-source entries that every workgroup
// reads into LDS once and searches.  The scaffold of the call is new_index.h, the host-only part concat_check.h.  Nothing here touches a walk or
// scan kernel.
#include "common.h"
#include "new_index.h"
#include "packets.h"
#include "concat_check.h"

#include <algorithm>
#include <vector>

using namespace vs;

namespace {

ConcatShape shape_of(const vs_index* a) {
    ConcatShape s;
    s.kind = a->kind;
    s.store_dtype = a->store_dtype;
    s.device = a->device;
    s.n_rows = a->n_rows;
    s.n_packets = a->n_packets;
    s.n_cols = a->n_cols;
    return s;
}

// the last table slot whose base is <= x: concat_find of concat_check.h on the LDS image, no branch
__device__ __forceinline__ int find_source(const uint32_t* base, uint32_t x) {
    int i = 0;
#pragma unroll
    for (int step = kConcatMaxSources / 2; step > 0; step >>= 1) i += base[i + step] <= x ? step : 0;
    return i;
}

// The table's pointers come out of LDS, where the compiler no longer knows that they point to global memory: loaded through as they are they
// become flat loads, whose counter is shared with the LDS reads of the next step's search -- every step then waits for its own loads.  The LDS
// image holds them as integers, and these two read through them as global pointers.
typedef uint32_t ConcatQuad __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 global_quad(uint64_t at) {
    const ConcatQuad v = *(const ConcatQuad __attribute__((address_space(1)))*)at;
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint32_t global_word(uint64_t base, size_t i) { return ((const uint32_t __attribute__((address_space(1)))*)base)[i]; }

// ---- map ---------------------------------------------------------------------------------------------------------------------------------------
// A thread a result row: it finds its source among the row bases and writes the rebased row pointer; thread n_rows writes the last pointer.  With
// tombstones on any source the live bits of the new rows as well: the 64 rows of a wave are two whole words of the new bitmap
// (live_words_from_ballot); *dead counts the cleared ones.
struct ConcatMapLds {
    uint64_t pk[kConcatMaxSources];                               // const uint32_t*
    uint64_t live[kConcatMaxSources];                             // const uint32_t*, or 0
    uint32_t row_base[kConcatMaxSources + 1];
    uint32_t pk_base[kConcatMaxSources];
};
static_assert(sizeof(ConcatMapLds) == kConcatMapLds, "the plan counts these bytes");

__global__ __launch_bounds__(kConcatThreads) void concat_map_kernel(const ConcatEntry* table, int32_t n_src, int64_t n_rows, uint32_t n_packets, uint32_t* new_pk,
                                                                    uint32_t* new_live, unsigned long long* dead) {
    __shared__ ConcatMapLds t;
    for (int s = threadIdx.x; s <= kConcatMaxSources; s += kConcatThreads) {
        const bool have = s < n_src;
        t.row_base[s] = have ? table[s].row_base : kConcatNoBase;
        if (s < kConcatMaxSources) {
            t.pk_base[s] = have ? table[s].pk_base : kConcatNoBase;
            t.pk[s] = have ? (uint64_t)table[s].pk : 0ull;
            t.live[s] = have ? (uint64_t)table[s].live : 0ull;
        }
    }
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * kConcatThreads + threadIdx.x;
    bool is_dead = false;
    if (r < n_rows) {
        const int s = find_source(t.row_base, (uint32_t)r);
        const uint32_t local = (uint32_t)r - t.row_base[s];
        new_pk[r] = global_word(t.pk[s], local) + t.pk_base[s];
        const uint64_t live = t.live[s];
        if (new_live && live) is_dead = !((global_word(live, local >> 5) >> (local & 31u)) & 1u);
    } else if (r == n_rows) {
        new_pk[r] = n_packets;
    }
    if (new_live) live_words_from_ballot(is_dead, r, n_rows, new_live, dead);
}

// ---- copy --------------------------------------------------------------------------------------------------------------------------------------
// A wave takes a round of kConcatRound contiguous result packets, a lane a packet of each 64-packet step.  The source of a packet is the last
// table slot whose packet base is <= it.  A step whose first and last packet fall into one source -- all of them but the few that straddle a
// boundary -- takes that source for every lane, decided wave-uniformly: the source's pointers and store are then scalars and the store's branch
// is uniform.  A step that crosses a boundary searches a lane at a time.  The loads of all four steps are issued before the first store; a lane
// past the last packet loads the last packet again (no branch around a load) and stores nothing.  A step's packet is a struct of its own, four
// named ones a round (select.hip: written as arrays indexed by the step the compiler kept them in LDS and scratch, not in registers).
// hipcc 7, gfx950: <VB, WS> = <32, 32> 81 VGPRs, <32, 16> 70, <32, 0> 54, <16, 32> 80, <16, 16> 68, <16, 0> 52, <0, 0> 43; the map kernel 12;
// no scratch, 6 152 bytes of LDS (the table) each.
struct ConcatCopyLds {
    uint64_t cols[kConcatMaxSources];                             // const uint4*
    uint64_t vals[kConcatMaxSources];                             // const uint4*; of a binary source its cols
    uint32_t pk_base[kConcatMaxSources + 1];
    int32_t dtype[kConcatMaxSources];
};
static_assert(sizeof(ConcatCopyLds) == kConcatCopyLds, "the plan counts these bytes");

struct ConcatPacket {
    uint4 c, v0, v1;
    int sd;                                                       // the store of the source the packet came from
};

// WS: the widest store among the sources (32: one is fp32, 16: fp16 and binary ones only, 0: all binary).  No branch goes around a load: the
// compiler waited for a load inside the branch that issued it, so that no two steps were in flight.  Instead every lane loads the quads its
// instantiation can need, from an address picked without a branch: a source narrower than WS gives its first quad twice (fp16 under WS = 32)
// or its column ids again (binary: the table's value pointer of such a source is its id pointer) -- lines the lane has just touched --, and
// the store ignores them.
template <int WS>
__device__ __forceinline__ ConcatPacket concat_load(const ConcatCopyLds& t, int64_t q, int64_t p_total) {
    const uint32_t p = (uint32_t)(q < p_total ? q : p_total - 1);
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(q - (threadIdx.x & 63)));   // the step's first packet (below p_total: the round starts there)
    const uint32_t last = (uint32_t)min((int64_t)first + 63, p_total - 1);
    const int s0 = __builtin_amdgcn_readfirstlane(find_source(t.pk_base, first));
    int s = s0;
    if (last >= t.pk_base[s0 + 1]) s = find_source(t.pk_base, p);               // (wave-uniform: the step crosses into the next source)
    const size_t sp = (size_t)(p - t.pk_base[s]);
    const uint64_t at_c = t.cols[s] + sp * 16;
    ConcatPacket r;
    r.sd = t.dtype[s];
    r.c = global_quad(at_c);
    r.v0 = r.v1 = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (WS != 0) {
        const uint64_t at_v = t.vals[s] + sp * (r.sd == VS_F32 ? 32 : 16);
        r.v0 = global_quad(at_v);
        if constexpr (WS == 32) r.v1 = global_quad(r.sd == VS_F32 ? at_v + 16 : at_v);
    }
    return r;
}

__device__ __forceinline__ uint32_t concat_half_bits(float f) { return (uint32_t)__half_as_ushort(__float2half_rn(f)); }

// VB: the value bytes of a result packet (32: fp32, 16: fp16, 0: binary -- every source is binary then)
template <int VB>
__device__ __forceinline__ void concat_store(const ConcatPacket& r, int64_t p, int64_t p_total, int32_t n_cols, uint4* dst_cols, uint4* dst_vals) {
    if (p >= p_total) return;
    dst_cols[p] = r.c;
    if constexpr (VB == 32) {
        uint4 lo = r.v0, hi = r.v1;
        if (r.sd != VS_F32) {                                     // fp16 widens exactly; a binary source's real cell is 1, its padding cell +0
            float f[8];
            const uint32_t h[4] = {r.v0.x, r.v0.y, r.v0.z, r.v0.w};
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const bool pad = packet_col(r.c, t) == (uint32_t)n_cols;
                const unsigned short hb = (unsigned short)((t & 1) ? (h[t >> 1] >> 16) : (h[t >> 1] & 0xFFFFu));
                const float w = r.sd == VS_F16 ? __half2float(__ushort_as_half(hb)) : 1.f;
                f[t] = pad ? 0.f : w;
            }
            lo = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
            hi = make_uint4(__float_as_uint(f[4]), __float_as_uint(f[5]), __float_as_uint(f[6]), __float_as_uint(f[7]));
        }
        dst_vals[(size_t)p * 2] = lo;
        dst_vals[(size_t)p * 2 + 1] = hi;
    }
    if constexpr (VB == 16) {
        uint4 v = r.v0;
        if (r.sd != VS_F16) {                                     // fp32 rounds once to nearest even; a binary source's real cell is 1, its padding cell +0
            const uint32_t b[8] = {r.v0.x, r.v0.y, r.v0.z, r.v0.w, r.v1.x, r.v1.y, r.v1.z, r.v1.w};
            uint32_t h[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const bool pad = packet_col(r.c, t) == (uint32_t)n_cols;
                const float w = r.sd == VS_F32 ? __uint_as_float(b[t]) : 1.f;
                h[t] = pad ? 0u : concat_half_bits(w);
            }
            v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
        }
        dst_vals[p] = v;
    }
}

template <int VB, int WS>
__global__ __launch_bounds__(kConcatThreads) void concat_copy_kernel(const ConcatEntry* table, int32_t n_src, int64_t p_total, int32_t n_cols, uint4* dst_cols,
                                                                     uint4* dst_vals) {
    static_assert(kConcatSteps == 4, "the round below names its four packets");
    __shared__ ConcatCopyLds t;
    for (int s = threadIdx.x; s <= kConcatMaxSources; s += kConcatThreads) {
        const bool have = s < n_src;
        t.pk_base[s] = have ? table[s].pk_base : kConcatNoBase;
        if (s < kConcatMaxSources) {
            t.cols[s] = have ? (uint64_t)table[s].cols : 0ull;
            t.vals[s] = have ? (uint64_t)(table[s].vals ? table[s].vals : table[s].cols) : 0ull;   // (a binary source: its ids stand in, see concat_load)
            t.dtype[s] = have ? table[s].store_dtype : VS_NONE;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t n_rounds = (p_total + kConcatRound - 1) / kConcatRound;
    for (int64_t round = (int64_t)blockIdx.x * kConcatWaves + (threadIdx.x >> 6); round < n_rounds; round += (int64_t)gridDim.x * kConcatWaves) {
        const int64_t q = round * kConcatRound + lane;
        // (a step that starts past the last packet is clamped to it as a whole: its first packet is the last packet, every lane loads that one)
        const ConcatPacket a0 = concat_load<WS>(t, q, p_total);
        const ConcatPacket a1 = concat_load<WS>(t, min(q + 64, p_total - 1 + lane), p_total);
        const ConcatPacket a2 = concat_load<WS>(t, min(q + 128, p_total - 1 + lane), p_total);
        const ConcatPacket a3 = concat_load<WS>(t, min(q + 192, p_total - 1 + lane), p_total);
        concat_store<VB>(a0, q, p_total, n_cols, dst_cols, dst_vals);
        concat_store<VB>(a1, q + 64, p_total, n_cols, dst_cols, dst_vals);
        concat_store<VB>(a2, q + 128, p_total, n_cols, dst_cols, dst_vals);
        concat_store<VB>(a3, q + 192, p_total, n_cols, dst_cols, dst_vals);
    }
}

}  // namespace

extern "C" int vs_concat_plan(int32_t n_src, const int64_t* rows, const int64_t* packets, int32_t n_cols, const int* dtypes, int out_dtype, int64_t* out_rows,
                              int64_t* out_packets, int64_t* out_scratch_bytes, int32_t* out_lds_bytes) {
    char msg[512] = {0};
    ConcatPlan p;
    const int rc = concat_plan(n_src, rows, packets, n_cols, dtypes, out_dtype, &p, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    if (out_rows) *out_rows = p.rows;
    if (out_packets) *out_packets = p.packets;
    if (out_scratch_bytes) *out_scratch_bytes = p.scratch_bytes;
    if (out_lds_bytes) *out_lds_bytes = p.lds_bytes;
    return VS_OK;
}

extern "C" int vs_index_concat(const vs_index* const* srcs, int32_t n_src, int out_dtype, int64_t rows_extra, int64_t packets_extra, int device, vs_index** out) {
    char msg[512] = {0};
    if (out) *out = nullptr;
    int rc = concat_check_args(srcs != nullptr, out != nullptr, n_src, rows_extra, packets_extra, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    for (int32_t s = 0; s < n_src; ++s)
        if (!srcs[s]) return fail(VS_EINVAL, "NULL argument: source %d", s);
    std::vector<ConcatShape> shapes((size_t)n_src);
    std::vector<int64_t> rows((size_t)n_src), packets((size_t)n_src);
    std::vector<int> dtypes((size_t)n_src);
    for (int32_t s = 0; s < n_src; ++s) {
        shapes[(size_t)s] = shape_of(srcs[s]);
        rc = concat_check_source(shapes[0], shapes[(size_t)s], s, msg, sizeof msg);
        if (rc != VS_OK) return fail(rc, "%s", msg);
        rows[(size_t)s] = srcs[s]->n_rows;
        packets[(size_t)s] = srcs[s]->n_packets;
        dtypes[(size_t)s] = srcs[s]->store_dtype;
    }
    ConcatPlan plan;
    rc = concat_plan(n_src, rows.data(), packets.data(), shapes[0].n_cols, dtypes.data(), out_dtype, &plan, msg, sizeof msg);
    if (rc == VS_OK) rc = new_index_check_capacity("joined", plan.rows, plan.packets, rows_extra, packets_extra, msg, sizeof msg);
    if (rc != VS_OK) return fail(rc, "%s", msg);
    VS_TRY(device_in_range(device));
    const int src_device = shapes[0].device;
    const int64_t n = plan.rows, p_new = plan.packets;

    VS_TRY(open_sources(src_device));
    std::vector<ConcatEntry> table((size_t)n_src);
    concat_fill_bases(shapes.data(), n_src, table.data());
    bool any_tomb = false, all_dense = true;
    int64_t nnz = 0;
    for (int32_t s = 0; s < n_src; ++s) {
        const vs_index* a = srcs[s];
        ConcatEntry& e = table[(size_t)s];
        e.pk = a->pk_ptr.p;
        e.cols = a->cols.p;
        e.vals = a->vals.p;
        e.live = a->has_tomb && a->n_rows > 0 ? a->live.p : nullptr;
        any_tomb = any_tomb || e.live != nullptr;
        all_dense = all_dense && a->logical_dense;
        nnz += a->nnz;
    }
    DevBuf scratch;
    const size_t table_bytes = (size_t)n_src * sizeof(ConcatEntry);
    VS_TRY(scratch.alloc((size_t)plan.scratch_bytes));
    VS_HIP(hipMemcpy(scratch.p, table.data(), table_bytes, hipMemcpyHostToDevice));
    const ConcatEntry* d_table = scratch.as<ConcatEntry>();
    unsigned long long* d_dead = reinterpret_cast<unsigned long long*>((char*)scratch.p + table_bytes);
    VS_HIP(hipMemset(d_dead, 0, kConcatCounterBytes));

    const size_t vb = value_bytes(out_dtype);
    IndexGuard guard{nullptr};
    VS_TRY(new_csr_index("the join", "sources' (drop the postings copies of the sources, or join fewer rows)", n, p_new, rows_extra, packets_extra, shapes[0].n_cols,
                         out_dtype, src_device, &guard));
    vs_index* idx = guard.p;
    if (any_tomb) VS_TRY(alloc_live(idx, n));
    // 1. map
    hipLaunchKernelGGL(concat_map_kernel, dim3((unsigned)concat_map_grid(n)), dim3(kConcatThreads), 0, 0, d_table, n_src, n, (uint32_t)p_new,
                       idx->pk_ptr.as<uint32_t>(), any_tomb ? idx->live.as<uint32_t>() : (uint32_t*)nullptr, d_dead);
    VS_HIP(hipGetLastError());
    // 2. copy
    if (p_new > 0) {
        const dim3 grid((unsigned)concat_copy_grid(p_new, srcs[0]->cu_count));
        uint4 *dc = idx->cols.as<uint4>(), *dv = idx->vals.as<uint4>();
        const int32_t n_cols = shapes[0].n_cols;
        int ws = 0;                                             // the widest store among the sources that hold packets
        for (int32_t s = 0; s < n_src; ++s)
            if (srcs[s]->n_packets > 0) ws = std::max(ws, srcs[s]->store_dtype == VS_F32 ? 32 : (srcs[s]->store_dtype == VS_F16 ? 16 : 0));
#define VS_CONCAT_LAUNCH(VB, WS) hipLaunchKernelGGL((concat_copy_kernel<VB, WS>), grid, dim3(kConcatThreads), 0, 0, d_table, n_src, p_new, n_cols, dc, dv)
        if (vb == 32 && ws == 32) VS_CONCAT_LAUNCH(32, 32);
        else if (vb == 32 && ws == 16) VS_CONCAT_LAUNCH(32, 16);
        else if (vb == 32) VS_CONCAT_LAUNCH(32, 0);
        else if (vb == 16 && ws == 32) VS_CONCAT_LAUNCH(16, 32);
        else if (vb == 16 && ws == 16) VS_CONCAT_LAUNCH(16, 16);
        else if (vb == 16) VS_CONCAT_LAUNCH(16, 0);
        else VS_CONCAT_LAUNCH(0, 0);
#undef VS_CONCAT_LAUNCH
        VS_HIP(hipGetLastError());
    }
    set_csr_shape(idx, n, p_new, nnz, all_dense);
    if (any_tomb) VS_TRY(settle_dead(idx, d_dead));
    return hand_over(guard, src_device, device, TombFrom::own_bits(), out);   // the tombstones travel behind the index
}
