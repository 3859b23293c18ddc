// label_terms.hip -- per-label term aggregations (vs_label_term_plan, vs_label_order, vs_index_label_term_sums, vs_index_label_term_counts): for
// ONE set of rows and one int32 label a row, the term sums / term counts of every label's rows at once -- the centroids of all clusters,
// categories or articles in one visit per stored cell, whatever the number of labels.  No reference counterpart.  Nothing here
// touches a search kernel; the set arrives as for vs_index_term_sums with B = 1, the fixed point is term_fx, the cells go through term_cells.h.
//
// (a) Label order: the set rows grouped by label.  A count pass walks the set (walk_rows, set_walk.h) and counts the labels -- a uint32 LDS
//     histogram a workgroup up to VS_FACET_LDS_BINS labels, flushed with one 64-bit atomicAdd a non-zero bin; 64-bit global atomics above.  One
//     workgroup turns the counts into exclusive bases (block_excl_scan, block_scan.h) -- ptr, total, and the bases of the item table.  A
//     place pass walks the set again: LDS regime -- histogram of the chunk, one global atomicAdd a non-zero label reserves the chunk's range in
//     the label's segment, and the rows are placed by LDS ranks; global regime -- one global atomicAdd a set row.  The order inside a label is
//     unspecified.
// (b) Item table: a wave a label cuts its segment into items (label, e0, e1) of at most rows_per_item rows.
// (c) Segmented sums: a workgroup of 16 waves owns an item and a column tile (work item i: tile i % tiles of item i / tiles -- resident
//     workgroups sweep the same packets).  It zeroes the tile's bins in LDS, resolves 64 list entries a wave to packet ranges (the listed rows
//     are live and in the set by construction: no membership test), streams them through sum_packets and adds the non-zero bins to row `label`
//     of the output with 64-bit atomics.  Items behind the real count leave at once: no device-to-host read between the stages.
//     The counts variant: the same on uint32 bins, a cell counting when its value is not zero (term_agg.hip's test).
#include "agg_call.h"
#include "block_scan.h"
#include "label_term_check.h"
#include "term_cells.h"

#include <algorithm>

using namespace vs;

namespace {

constexpr int kOrderThreads = 256;
constexpr int kOrderWaves = kOrderThreads / 64;
constexpr int kScanThreads = 1024;
constexpr int kItemThreads = 256;
constexpr int kSumThreads = 1024;                     // 16 waves: a workgroup with a full tile has the CU to itself
constexpr int kSumWaves = kSumThreads / 64;
static_assert((size_t)VS_FACET_LDS_BINS * 4 + 1024 <= 160 * 1024, "the label histogram and the counters fit a CU's LDS");
static_assert((uint64_t)VS_LABEL_TERM_MAX_WORK_ITEMS * kSumThreads < (1ull << 32), "the plan's work items are a launch of fewer than 2^32 threads");

struct OrderArgs {
    RowSet set;                       // one set (B = 1); rows_per_chunk: the rows of a workgroup
    const int32_t* labels;            // [n_rows]
    uint32_t L;
    unsigned long long* cnt;          // [L + 1], zeroed: the set rows of each label; [L]: the set rows whose label is outside [0, L)
    uint32_t* cursor;                 // [L] (place pass): the next free slot of each label's segment, starting at its base
    uint32_t* rows;                   // [n_rows] (place pass)
};

// PLACE = 0: count the labels of the set rows into cnt; PLACE = 1: write the set rows into their labels' segments of rows.
// GLOBAL = 0: a uint32 LDS bin a label; GLOBAL = 1: global atomics.
template <int GLOBAL, int PLACE>
__global__ __launch_bounds__(kOrderThreads) void label_order_kernel(OrderArgs a) {
    extern __shared__ uint32_t label_hist[];                     // [L] (LDS regime)
    __shared__ uint32_t s_oth;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * a.set.rows_per_chunk;
    const int64_t r1 = min(a.set.n_rows, r0 + a.set.rows_per_chunk);
    const uint32_t L = a.L;
    if constexpr (!GLOBAL)
        for (uint32_t i = tid; i < L; i += kOrderThreads) label_hist[i] = 0u;
    if (tid == 0) s_oth = 0u;
    __syncthreads();
    uint32_t oth = 0u;                                           // wave-uniform: a chunk holds fewer than 2^32 rows
    if constexpr (!(GLOBAL && PLACE)) {                          // the labels of the chunk's set rows, counted
        walk_rows<kOrderWaves>(a.set, 0, r0, r1, w, lane, [&](int64_t row0, uint64_t m, int64_t) {
            const bool in = (m >> lane) & 1ull;
            const int32_t label = in ? a.labels[row0 + lane] : -1;
            const bool ok = in && (uint32_t)label < L;                               // -1 and anything too large: `other`
            oth += (uint32_t)(__popcll(m) - __popcll(__builtin_amdgcn_ballot_w64(ok)));
            if (ok) {
                if constexpr (GLOBAL) atomicAdd(a.cnt + label, 1ull);
                else atomicAdd(label_hist + label, 1u);
            }
        }, [] {});
    }
    if constexpr (!PLACE) {
        if (lane == 0 && oth) atomicAdd(&s_oth, oth);
        __syncthreads();
        if constexpr (!GLOBAL) {
            for (uint32_t i = tid; i < L; i += kOrderThreads) {
                const uint32_t v = label_hist[i];
                if (v) atomicAdd(a.cnt + i, (unsigned long long)v);
            }
        }
        if (tid == 0 && s_oth) atomicAdd(a.cnt + L, (unsigned long long)s_oth);
    } else {
        if constexpr (!GLOBAL) {                                 // a non-zero bin becomes the first slot of the chunk's range in the label's segment
            __syncthreads();
            for (uint32_t i = tid; i < L; i += kOrderThreads) {
                const uint32_t v = label_hist[i];
                if (v) label_hist[i] = atomicAdd(a.cursor + i, v);
            }
            __syncthreads();
        }
        walk_rows<kOrderWaves>(a.set, 0, r0, r1, w, lane, [&](int64_t row0, uint64_t m, int64_t) {
            const bool in = (m >> lane) & 1ull;
            const int32_t label = in ? a.labels[row0 + lane] : -1;
            if (in && (uint32_t)label < L) {
                uint32_t pos;
                if constexpr (GLOBAL) pos = atomicAdd(a.cursor + label, 1u);
                else pos = atomicAdd(label_hist + label, 1u);
                if ((int64_t)pos < a.set.n_rows) a.rows[pos] = (uint32_t)(row0 + lane);   // (always, while labels and set are those of the count pass)
            }
        }, [] {});
    }
}

struct ScanArgs {
    const unsigned long long* cnt;    // [L + 1]
    uint32_t L;
    uint64_t R;                       // rows of an item at most
    long long* ptr;                   // [L + 1]: the exclusive bases of the counts
    uint32_t* cursor;                 // [L]: the same, for the place pass
    uint32_t* item_base;              // [L + 1]: the exclusive bases of ceil(cnt / R), or null
    long long* total;                 // [L]: the counts, or null
    long long* other;                 // [1]
};

// one workgroup walks the labels 1024 at a time (a set holds fewer than 2^32 rows: the bases fit uint32)
__global__ __launch_bounds__(kScanThreads) void label_scan_kernel(ScanArgs a) {
    __shared__ uint2 sh[kScanThreads / 64];
    uint2 carry = make_uint2(0u, 0u);
    for (uint32_t l0 = 0; l0 < a.L; l0 += kScanThreads) {
        const uint32_t l = l0 + threadIdx.x;
        const uint32_t c = l < a.L ? (uint32_t)a.cnt[l] : 0u;
        const uint2 v = make_uint2(c, (uint32_t)(((uint64_t)c + a.R - 1) / a.R));
        uint2 tot;
        const uint2 ex = block_excl_scan<kScanThreads / 64>(v, sh, &tot);
        if (l < a.L) {
            a.ptr[l] = (long long)(carry.x + ex.x);
            a.cursor[l] = carry.x + ex.x;
            if (a.item_base) a.item_base[l] = carry.y + ex.y;
            if (a.total) a.total[l] = (long long)c;
        }
        carry = add2(carry, tot);
    }
    if (threadIdx.x == 0) {
        a.ptr[a.L] = (long long)carry.x;
        if (a.item_base) a.item_base[a.L] = carry.y;
        a.other[0] = (long long)a.cnt[a.L];
    }
}

struct ItemArgs {
    const long long* ptr;             // [L + 1]
    const uint32_t* item_base;        // [L + 1]
    uint32_t L;
    uint64_t R;
    uint4* items;                     // [max_items]: (label, e0, e1, 0) -- entries [e0, e1) of rows
    uint32_t max_items;
};

// a wave a label
__global__ __launch_bounds__(kItemThreads) void label_items_kernel(ItemArgs a) {
    const uint32_t l = blockIdx.x * (kItemThreads / 64) + (threadIdx.x >> 6);
    if (l >= a.L) return;
    const uint64_t e0 = (uint64_t)a.ptr[l], e1 = (uint64_t)a.ptr[l + 1];
    const uint32_t base = a.item_base[l], n = a.item_base[l + 1] - base;
    for (uint32_t j = threadIdx.x & 63; j < n; j += 64) {
        const uint64_t b = e0 + (uint64_t)j * a.R;
        if (base + j < a.max_items) a.items[base + j] = make_uint4(l, (uint32_t)b, (uint32_t)(b + a.R < e1 ? b + a.R : e1), 0u);
    }
}

struct LabelSumArgs {
    TermSetArgs t;                    // the packets; set.n_rows: the index's rows
    const uint32_t* rows;             // the set rows grouped by label
    const uint4* items;
    const uint32_t* n_items;          // [1] on the device
    int32_t tiles, tile_cols;         // work item i of the grid: tile i % tiles of item i / tiles
    unsigned long long* out;          // [L, ld], zeroed by the caller
    int64_t ld;
};

// one wave: every cell of packets [p0, p1) whose column lies in the tile and whose value is not zero adds 1 to the column's bin
template <int SD>
__device__ __forceinline__ void count_tile_packets(const TermSetArgs& a, uint32_t p0, uint32_t p1, int lane, uint32_t tile0, uint32_t lim,
                                                   uint32_t* bins) {
    for (uint64_t pb = p0; pb < p1; pb += 128) {                  // (64-bit: no wrap next to 2^32 packets)
        const uint64_t pa = pb + lane, pc = pb + 64 + lane;
        const bool oa = pa < p1, oc = pc < p1;
        uint4 ca = make_uint4(0u, 0u, 0u, 0u), cc = ca;
        if (oa) ca = a.cols[pa];
        if (oc) cc = a.cols[pc];
        uint32_t ha = oa ? tile_hits(ca, tile0, lim) : 0u, hc = oc ? tile_hits(cc, tile0, lim) : 0u;
        if (ha) ha &= nonzero_cells<SD>(a.vals, pa);              // no id in the tile: the values are not read
        if (hc) hc &= nonzero_cells<SD>(a.vals, pc);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if ((ha >> t) & 1u) atomicAdd(bins + (packet_col(ca, t) - tile0), 1u);
            if ((hc >> t) & 1u) atomicAdd(bins + (packet_col(cc, t) - tile0), 1u);
        }
    }
}

// COUNTS = 0: 64-bit bins of fixed-point sums; COUNTS = 1: uint32 bins of counts
template <int SD, int COUNTS>
__global__ __launch_bounds__(kSumThreads) void label_term_kernel(LabelSumArgs a) {
    extern __shared__ uint4 label_bins4[];                       // [ceil(tile_cols / 2)] 64-bit bins, [ceil(tile_cols / 4)] uint32 bins
    const uint32_t item = blockIdx.x / (uint32_t)a.tiles;        // the tile runs fastest: resident workgroups sweep the same packets
    if (item >= a.n_items[0]) return;                            // (uniform) the grid is sized by the bound
    const uint32_t tile = blockIdx.x % (uint32_t)a.tiles;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t tile0 = tile * (uint32_t)a.tile_cols;         // < n_cols: no tile of the plan is empty
    const uint32_t lim = min((uint32_t)a.tile_cols, (uint32_t)a.t.n_cols - tile0);   // the padding id n_cols is never inside
    const int n16 = COUNTS ? (a.tile_cols + 3) / 4 : (a.tile_cols + 1) / 2;
    for (int i = tid; i < n16; i += kSumThreads) label_bins4[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const uint4 it = a.items[item];                              // (label, e0, e1)
    for (uint64_t eb = (uint64_t)it.y + (uint64_t)w * 64; eb < it.z; eb += (uint64_t)kSumWaves * 64) {
        const uint64_t e = eb + lane;
        bool ok = e < it.z;
        uint32_t plo = 0u, phi = 0u;
        if (ok) {
            const uint32_t row = a.rows[e];
            ok = (int64_t)row < a.t.set.n_rows;                  // (always: the order lists rows of the index)
            if (ok) {
                plo = a.t.pk_ptr[row];
                phi = a.t.pk_ptr[row + 1];
            }
        }
        unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1ull;
            const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)plo, l), p1 = (uint32_t)__builtin_amdgcn_readlane((int)phi, l);
            if constexpr (COUNTS) count_tile_packets<SD>(a.t, p0, p1, lane, tile0, lim, reinterpret_cast<uint32_t*>(label_bins4));
            else sum_packets<SD>(a.t, p0, p1, lane, tile0, lim, reinterpret_cast<unsigned long long*>(label_bins4));
        }
    }
    __syncthreads();
    unsigned long long* dst = a.out + (size_t)it.x * (size_t)a.ld + tile0;
    for (uint32_t i = tid; i < lim; i += kSumThreads) {
        unsigned long long v;
        if constexpr (COUNTS) v = reinterpret_cast<const uint32_t*>(label_bins4)[i];
        else v = reinterpret_cast<const unsigned long long*>(label_bins4)[i];
        if (v) atomicAdd(dst + i, v);
    }
}

template <int GLOBAL, int PLACE>
int order_launch(const OrderArgs& a, dim3 grid, hipStream_t s) {
    const size_t lds = GLOBAL ? 0 : (size_t)a.L * 4;
    if (lds) VS_HIP(hipFuncSetAttribute((const void*)label_order_kernel<GLOBAL, PLACE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((label_order_kernel<GLOBAL, PLACE>), grid, dim3(kOrderThreads), lds, s, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

template <int SD, int COUNTS>
int term_launch(const LabelSumArgs& a, dim3 grid, hipStream_t s) {
    const size_t lds = (size_t)(COUNTS ? (a.tile_cols + 3) / 4 : (a.tile_cols + 1) / 2) * 16;
    VS_HIP(hipFuncSetAttribute((const void*)label_term_kernel<SD, COUNTS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((label_term_kernel<SD, COUNTS>), grid, dim3(kSumThreads), lds, s, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// the handle's workspace of a call (grow-only, so that a call with device pointers only enqueues)
struct LabelWork {
    unsigned long long* cnt = nullptr;   // [L + 1]
    long long* ptr = nullptr;            // [L + 1] (vs_label_order writes the caller's instead)
    uint32_t *cursor = nullptr, *item_base = nullptr, *rows = nullptr;
    uint4* items = nullptr;
    int bind(vs_index* idx, int32_t L, int64_t max_items, bool own_order) {
        const size_t n_cnt = up16((size_t)(L + 1) * 8), n_cur = up16((size_t)L * 4), n_ib = up16((size_t)(L + 1) * 4);
        const size_t n_rows = own_order ? up16((size_t)idx->n_rows * 4) : 0, n_items = up16((size_t)max_items * 16);
        VS_TRY(idx->ws_label.reserve(2 * n_cnt + n_cur + n_ib + n_rows + n_items));
        char* p = idx->ws_label.as<char>();
        cnt = reinterpret_cast<unsigned long long*>(p), p += n_cnt;
        ptr = reinterpret_cast<long long*>(p), p += n_cnt;
        cursor = reinterpret_cast<uint32_t*>(p), p += n_cur;
        item_base = reinterpret_cast<uint32_t*>(p), p += n_ib;
        rows = reinterpret_cast<uint32_t*>(p), p += n_rows;
        items = reinterpret_cast<uint4*>(p);
        return VS_OK;
    }
};

// the order of the set rows on the stream: counts, bases, placement.  total / item_base may be null.
int order_on_stream(const RowSet& set0, const int32_t* labels, int32_t L, uint64_t R, const LabelWork& wk, long long* ptr, uint32_t* rows,
                    uint32_t* item_base, long long* total, long long* other, hipStream_t s) {
    OrderArgs a{set0, labels, (uint32_t)L, wk.cnt, wk.cursor, rows};
    a.set.rows_per_chunk = label_order_chunk(set0.n_rows, L);
    const dim3 grid((unsigned)ceil_div64(set0.n_rows, a.set.rows_per_chunk));
    const bool global = L > VS_FACET_LDS_BINS;
    VS_HIP(hipMemsetAsync(wk.cnt, 0, (size_t)(L + 1) * 8, s));
    VS_TRY((global ? order_launch<1, 0>(a, grid, s) : order_launch<0, 0>(a, grid, s)));
    const ScanArgs sc{wk.cnt, (uint32_t)L, R, ptr, wk.cursor, item_base, total, other};
    hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, sc);
    VS_HIP(hipGetLastError());
    VS_TRY((global ? order_launch<1, 1>(a, grid, s) : order_launch<0, 1>(a, grid, s)));
    return VS_OK;
}

// One call on the index's device: counts = false -> sums
int label_term_call(vs_index* idx, const uint32_t* words, int64_t bit0, const int32_t* labels, int32_t L, const LabelTermPlan& plan, bool counts,
                    int64_t* out, int64_t ld_out, int64_t* total, int64_t* other, void* stream) {
    const void* ptrs[5] = {words, labels, out, total, other};
    const char* names[5] = {"words", "labels", counts ? "counts" : "sums", "total", "other"};
    const char* prof_name = counts ? "label_term_counts" : "label_term_sums";
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 5, idx->device, &dev));
    VS_HIP(hipSetDevice(idx->device));
    hipStream_t s = (hipStream_t)stream;
    Staged st_w, st_l, st_o;
    CountsOut o;
    uint32_t* d_w;
    int32_t* d_l;
    int64_t* d_other;
    VS_TRY(st_w.in(words, (size_t)((bit0 + idx->n_rows + 31) >> 5), dev, true, s, &d_w));
    VS_TRY(st_l.in(labels, (size_t)idx->n_rows, dev, true, s, &d_l));
    VS_TRY(st_o.in(other, 1, dev, false, s, &d_other));
    VS_TRY(o.bind(dev, out, ld_out, idx->n_cols, L, {total}, s));
    VS_HIP(hipMemsetAsync(d_other, 0, 8, s));
    if (idx->n_rows > 0) {
        ProfScope prof(prof_name, s);
        LabelWork wk;
        VS_TRY(launch_rc(wk.bind(idx, L, plan.max_items, true), s));
        const RowSet set{d_w, bit0, 0, live_words(idx), 0, idx->n_rows, 1, 0};
        const uint64_t R = (uint64_t)plan.rows_per_item;
        VS_TRY(launch_rc(order_on_stream(set, d_l, L, R, wk, wk.ptr, wk.rows, wk.item_base, reinterpret_cast<long long*>(o.vec[0]),
                                         reinterpret_cast<long long*>(d_other), s), s));
        const ItemArgs ia{wk.ptr, wk.item_base, (uint32_t)L, R, wk.items, (uint32_t)plan.max_items};
        hipLaunchKernelGGL(label_items_kernel, dim3((unsigned)ceil_div64(L, kItemThreads / 64)), dim3(kItemThreads), 0, s, ia);
        if (hipGetLastError() != hipSuccess) return launch_rc(fail(VS_EHIP, "the item kernel's launch failed"), s);
        LabelSumArgs a{};
        a.t.pk_ptr = idx->pk_ptr.as<uint32_t>();
        a.t.cols = idx->cols.as<uint4>();
        a.t.vals = idx->vals.p;
        a.t.n_cols = idx->n_cols;
        a.t.set = set;
        a.rows = wk.rows;
        a.items = wk.items;
        a.n_items = wk.item_base + L;
        a.tiles = plan.tiles;
        a.tile_cols = plan.tile_cols;
        a.out = o.mat;
        a.ld = o.ld;
        const dim3 grid((unsigned)(plan.max_items * plan.tiles));
        VS_TRY(launch_rc(dispatch_store(idx->store_dtype, counts, [&](auto sd, auto is_counts) {
            return term_launch<decltype(sd)::value, decltype(is_counts)::value>(a, grid, s);
        }), s));
    }
    return close_call(prof_name, dev, stream, s, Finish::kStream, [&] {
        VS_TRY(o.back(s));
        return st_o.back(s);
    });
}

}  // namespace

extern "C" int vs_label_term_plan(int64_t n_rows, int32_t n_labels, int32_t n_cols, int64_t rows_per_item, int32_t tile_cols, int32_t* out_tiles,
                                  int32_t* out_tile_cols, int64_t* out_rows_per_item, int64_t* out_max_items) {
    if (!out_tiles || !out_tile_cols || !out_rows_per_item || !out_max_items) return fail(VS_EINVAL, "NULL argument");
    LabelTermPlan p;
    char msg[256];
    VS_TRY(plan_or_fail(label_term_plan(n_rows, n_labels, n_cols, rows_per_item, tile_cols, &p, msg, sizeof msg), msg));
    *out_tiles = p.tiles;
    *out_tile_cols = p.tile_cols;
    *out_rows_per_item = p.rows_per_item;
    *out_max_items = p.max_items;
    return VS_OK;
}

extern "C" int vs_label_order(vs_index* idx, const uint32_t* words, int64_t bit0, const int32_t* labels, int32_t n_labels, int64_t* ptr,
                              uint32_t* rows, int64_t* other, void* stream) {
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    char msg[256];
    VS_TRY(plan_or_fail(label_order_check(bit0, std::max<int64_t>(idx->n_rows, 1), labels != nullptr, n_labels, ptr && rows && other, msg, sizeof msg),
                        msg));
    VS_TRY(need_device());
    const void* ptrs[5] = {words, labels, ptr, rows, other};
    const char* names[5] = {"words", "labels", "ptr", "rows", "other"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 5, idx->device, &dev));
    VS_HIP(hipSetDevice(idx->device));
    hipStream_t s = (hipStream_t)stream;
    Staged st_w, st_l, st_p, st_r, st_o;
    uint32_t *d_w, *d_rows;
    int32_t* d_l;
    int64_t *d_ptr, *d_other;
    VS_TRY(st_w.in(words, (size_t)((bit0 + idx->n_rows + 31) >> 5), dev, true, s, &d_w));
    VS_TRY(st_l.in(labels, (size_t)idx->n_rows, dev, true, s, &d_l));
    VS_TRY(st_p.in(ptr, (size_t)n_labels + 1, dev, false, s, &d_ptr));
    VS_TRY(st_r.in(rows, (size_t)idx->n_rows, dev, false, s, &d_rows));
    VS_TRY(st_o.in(other, 1, dev, false, s, &d_other));
    if (!dev && st_r.bytes) VS_HIP(hipMemsetAsync(d_rows, 0, st_r.bytes, s));     // (the slots behind the set's rows are copied back too)
    if (idx->n_rows > 0) {
        ProfScope prof("label_order", s);
        LabelWork wk;
        VS_TRY(launch_rc(wk.bind(idx, n_labels, 0, false), s));
        const RowSet set{d_w, bit0, 0, live_words(idx), 0, idx->n_rows, 1, 0};
        VS_TRY(launch_rc(order_on_stream(set, d_l, n_labels, 1, wk, reinterpret_cast<long long*>(d_ptr), d_rows, nullptr, nullptr,
                                         reinterpret_cast<long long*>(d_other), s), s));
    } else {
        VS_HIP(hipMemsetAsync(d_ptr, 0, ((size_t)n_labels + 1) * 8, s));
        VS_HIP(hipMemsetAsync(d_other, 0, 8, s));
    }
    return close_call("label_order", dev, stream, s, Finish::kStream, [&] {
        VS_TRY(st_p.back(s));
        VS_TRY(st_r.back(s));
        return st_o.back(s);
    });
}

extern "C" int vs_index_label_term_sums(vs_index* idx, const uint32_t* words, int64_t bit0, const int32_t* labels, int32_t n_labels,
                                        int64_t rows_per_item, int32_t tile_cols, int64_t* sums, int64_t ld_sums, int64_t* total, int64_t* other,
                                        void* stream) {
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    VS_TRY(csr_index_ok(idx, "per-label term sums"));
    LabelTermPlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(label_term_check(bit0, std::max<int64_t>(idx->n_rows, 1), idx->n_cols, labels != nullptr, n_labels, rows_per_item, tile_cols,
                                         sums && total && other, ld_sums, "sums", &plan, msg, sizeof msg), msg));
    VS_TRY(need_device());
    return label_term_call(idx, words, bit0, labels, n_labels, plan, false, sums, ld_sums, total, other, stream);
}

extern "C" int vs_index_label_term_counts(vs_index* idx, const uint32_t* words, int64_t bit0, const int32_t* labels, int32_t n_labels,
                                          int64_t rows_per_item, int32_t tile_cols, int64_t* counts, int64_t ld_counts, int64_t* total,
                                          int64_t* other, void* stream) {
    if (!idx) return fail(VS_EINVAL, "NULL argument");
    VS_TRY(csr_index_ok(idx, "per-label term counts"));
    LabelTermPlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(label_term_check(bit0, std::max<int64_t>(idx->n_rows, 1), idx->n_cols, labels != nullptr, n_labels, rows_per_item, tile_cols,
                                         counts && total && other, ld_counts, "counts", &plan, msg, sizeof msg), msg));
    VS_TRY(need_device());
    return label_term_call(idx, words, bit0, labels, n_labels, plan, true, counts, ld_counts, total, other, stream);
}
