// grouped.hip -- grouped search (field collapsing): the top k GROUPS of a ranking, each with its best m rows (vs_topk_collapse,
// vs_group_filter).  No reference counterpart: the reference searches a larger k on a guess and de-duplicates on the host.  Nothing here
// touches a search kernel: the collapse runs behind a search, the filter in front of the next one.
//
// (a) Collapse: one wave per query continues the serial walk of the contract over a ranked list, 64 entries a step.  The query's open groups
//     sit in an LDS open-addressing table (group -> slot) beside the slots' kept counts.  Inside a step the lanes of one group are found
//     with the leader loop (the first pending lane's group is broadcast, the equal lanes balloted and ranked by their position under the
//     mask); ranks continue from the table's counts, new groups take slots from a prefix count of "first of its group in the step and
//     absent from the table".  Both limits -- k groups, m rows a group -- are applied in rank order, which is the order of the serial walk:
//     a new group opens iff fewer than k are open before it, and the new first lanes ahead of it are exactly the groups opened ahead of it.
//     The state lives in the caller's output buffers, so a later call (the next round's list) goes on where this one stopped.
// (b) Filter: the rows a later round still has to rank, F = caller's filter AND group not full AND (fewer than k open OR group open) AND not
//     kept.  A workgroup owns a run of rows and a tile of queries; a lane loads its row's group id once and probes every query's LDS table;
//     a wave ballot is two bitmap words.  Kept rows of open, non-full groups are cleared by id afterwards (atomicAnd, as the tombstones).
#include "common.h"
#include "staging.h"

#include <algorithm>

using namespace vs;

namespace {

constexpr int kMaxK = 1024;               // groups a query may ask for (the LDS table holds 2 k keys)
constexpr int kMaxM = 64;                 // rows kept per group
constexpr int kMaxKM = 8192;              // k * m: the state rows of a query
constexpr int kMaxKK = 16384;             // entries of a list a call walks
constexpr int kFiltThreads = 256;
constexpr int kFiltChunks = 8;            // 64-row steps a wave of the filter kernel takes
constexpr int kFiltMaxTile = 16;          // queries a workgroup of the filter kernel serves
constexpr int kFiltLds = 48 * 1024;

__device__ __forceinline__ uint32_t table_hash(int32_t g, int shift) { return ((uint32_t)g * 2654435761u) >> shift; }

// the slot of group g in the table, -1 when absent (the table is never more than half full: an empty key ends every probe)
__device__ __forceinline__ int table_find(const int32_t* tkey, uint32_t tmask, int shift, int32_t g) {
    uint32_t h = table_hash(g, shift);
    for (;;) {
        const int32_t key = tkey[h];
        if (key == g) return (int)h;
        if (key == -1) return -1;
        h = (h + 1) & tmask;
    }
}

// claims a cell for group g (distinct groups only: no lane inserts a key another lane inserts) -> the cell
__device__ __forceinline__ int table_insert(int32_t* tkey, uint32_t tmask, int shift, int32_t g) {
    uint32_t h = table_hash(g, shift);
    for (;;) {
        const int32_t old = atomicCAS(&tkey[h], -1, g);
        if (old == -1 || old == g) return (int)h;
        h = (h + 1) & tmask;
    }
}

// ---- (a) collapse ------------------------------------------------------------------------------------------------------------------
struct CollapseArgs {
    const int64_t* ids;
    const float* sc;
    int32_t kk;
    int64_t ld;
    const int32_t* qmap;
    const int32_t* groups;
    int64_t n_rows;
    int32_t B, k, m;
    int32_t* og;         // [B, k] group of slot j, -1 = unused
    int32_t* oc;         // [B, k] rows kept of slot j
    int64_t* oi;         // [B, k, m]
    float* os;           // [B, k, m]
    int32_t* status;     // [B] 1 = complete
    int32_t* incomplete; // [1] listed queries left incomplete by this call
    int init, exhausted;
    uint32_t tmask;      // table cells - 1 (a power of two >= 2 k)
    int shift;           // 32 - log2(table cells)
};

__global__ __launch_bounds__(64) void topk_collapse_kernel(CollapseArgs a) {
    extern __shared__ int32_t coll_sh[];
    int32_t* tkey = coll_sh;                         // [cells] group, -1 = empty
    int32_t* tslot = coll_sh + (a.tmask + 1);        // [cells] its slot
    int32_t* cnt = tslot + (a.tmask + 1);            // [k] rows kept of a slot
    const int lane = threadIdx.x;
    const size_t i = blockIdx.x;
    const int64_t bq = a.qmap ? (int64_t)a.qmap[i] : (int64_t)i;
    if (bq < 0 || bq >= a.B) return;                                         // (a device qmap is not read on the host)
    const size_t b = (size_t)bq;
    if (!a.init && a.status[b] == 1) return;                                 // complete already: its state is final
    const int k = a.k, m = a.m;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t j = lane; j <= a.tmask; j += 64) tkey[j] = -1;
    for (int j = lane; j < k; j += 64) cnt[j] = 0;
    __syncthreads();
    int n_open = 0, n_full = 0;
    if (!a.init) {                                                           // the state so far: slots are dealt in order, so the open ones lead
        for (int j0 = 0; j0 < k; j0 += 64) {
            const int j = j0 + lane;
            const int32_t g = j < k ? a.og[b * k + j] : -1;
            const int32_t c = g >= 0 ? min(max(a.oc[b * k + j], 0), m) : 0;          // (clamped: a count indexes the member slots)
            if (g >= 0) {
                tslot[table_insert(tkey, a.tmask, a.shift, g)] = j;
                cnt[j] = c;
            }
            n_open += __popcll(__ballot(g >= 0));
            n_full += __popcll(__ballot(g >= 0 && c >= m));
        }
        __syncthreads();
    }
    bool ended = false;
    for (int i0 = 0; i0 < a.kk && n_full < k && !ended; i0 += 64) {
        const int e = i0 + lane;
        int64_t id = -1;
        float s = -INFINITY;
        if (e < a.kk) {
            id = a.ids[i * a.ld + e];
            s = a.sc[i * a.ld + e];
        }
        bool ok = e < a.kk && id >= 0 && id < a.n_rows;
        const unsigned long long bad = __ballot(e < a.kk && !ok);            // padding (or an id that is no row) ends the list
        if (bad) {
            ended = true;
            ok = ok && lane < __ffsll((long long)bad) - 1;
        }
        int32_t g = ok ? a.groups[id] : -1;
        ok = ok && g >= 0;                                                   // (a negative group id: the row is never kept)
        int slot = -1, base = 0;
        if (ok) {
            const int h = table_find(tkey, a.tmask, a.shift, g);
            if (h >= 0) {
                slot = tslot[h];
                base = cnt[slot];
            }
        }
        // leader loop: rank of a lane among the lanes of its group in this step, the first of them, and how many they are
        int rank = 0, first = lane, tot = 0;
        unsigned long long pending = __ballot(ok);
        while (pending) {
            const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)pending) - 1);
            const int32_t lg = __builtin_amdgcn_readlane(g, l);
            const bool mine = ok && g == lg;
            const unsigned long long eq = __ballot(mine);
            if (mine) {
                rank = __popcll(eq & lt);
                first = l;
                tot = __popcll(eq);
            }
            pending &= ~eq;
        }
        // new groups open in list order while fewer than k are open
        const bool newfirst = ok && slot < 0 && rank == 0;
        const int p = __popcll(__ballot(newfirst) & lt);
        if (newfirst && n_open + p < k) slot = n_open + p;
        const int lead_slot = __shfl(slot, first);
        if (ok && rank > 0) slot = lead_slot;                                // (the table's slot, or the one its first lane was just dealt)
        const bool opened = newfirst && slot >= 0;
        if (ok && slot >= 0 && base + rank < m) {
            const size_t o = (b * k + slot) * (size_t)m + (size_t)(base + rank);
            a.oi[o] = id;
            a.os[o] = s;
        }
        bool fills = false;
        if (ok && rank == 0 && slot >= 0) {
            const int nc = min(m, base + tot);
            cnt[slot] = nc;
            fills = base < m && nc >= m;
            if (opened) {
                tslot[table_insert(tkey, a.tmask, a.shift, g)] = slot;
                a.og[b * k + slot] = g;
            }
        }
        n_open += __popcll(__ballot(opened));
        n_full += __popcll(__ballot(fills));
        __syncthreads();
    }
    for (int j = lane; j < k; j += 64) {
        a.oc[b * k + j] = cnt[j];
        if (a.init && j >= n_open) a.og[b * k + j] = -1;
    }
    if (a.init)                                                              // unused member slots: id -1, score -inf
        for (int t = lane; t < k * m; t += 64)
            if (t % m >= cnt[t / m]) {
                a.oi[b * k * m + t] = -1;
                a.os[b * k * m + t] = -INFINITY;
            }
    if (lane == 0) {
        const bool complete = ended || a.exhausted || n_full >= k;
        a.status[b] = complete ? 1 : 0;
        if (!complete) atomicAdd(a.incomplete, 1);
    }
}

// ---- (b) filter --------------------------------------------------------------------------------------------------------------------
struct GroupFilterArgs {
    const int32_t* groups;
    int64_t n_rows;
    int32_t Bp, B;
    const int32_t* qmap;
    int32_t k, m;
    const int32_t* sg;   // state: [B, k] groups, [B, k] counts, [B, k, m] ids
    const int32_t* sc;
    const int64_t* si;
    const uint32_t* filt;
    int64_t filt_ld;
    uint32_t* out;
    int64_t ld_words, W;
    int32_t tile;        // queries a workgroup serves
    uint32_t tmask;
    int shift;
};

__global__ __launch_bounds__(kFiltThreads) void group_filter_kernel(GroupFilterArgs a) {
    extern __shared__ int32_t filt_sh[];
    const uint32_t cells = a.tmask + 1;
    int32_t* tkey = filt_sh;                                                 // [tile][cells]
    uint32_t* tfull = reinterpret_cast<uint32_t*>(filt_sh + (size_t)a.tile * cells);   // [tile][cells / 32] bit of a cell: its group is full
    int32_t* nopen = reinterpret_cast<int32_t*>(tfull + (size_t)a.tile * (cells / 32));  // [tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.y * a.tile;
    const int nq = min(a.tile, a.Bp - q0);
    for (uint32_t j = tid; j < (uint32_t)a.tile * cells; j += kFiltThreads) tkey[j] = -1;
    for (uint32_t j = tid; j < (uint32_t)a.tile * (cells / 32); j += kFiltThreads) tfull[j] = 0u;
    if (tid < a.tile) nopen[tid] = 0;
    __syncthreads();
    for (int q = 0; q < nq; ++q) {
        const int64_t b = a.qmap ? (int64_t)a.qmap[q0 + q] : (int64_t)(q0 + q);
        if (b < 0 || b >= a.B) continue;                                     // (no state: every group reads as absent, none open)
        for (int j = tid; j < a.k; j += kFiltThreads) {
            const int32_t g = a.sg[b * a.k + j];
            if (g < 0) continue;
            const int h = table_insert(tkey + (size_t)q * cells, a.tmask, a.shift, g);
            if (a.sc[b * a.k + j] >= a.m) atomicOr(&tfull[(size_t)q * (cells / 32) + (h >> 5)], 1u << (h & 31));
            atomicAdd(&nopen[q], 1);
        }
    }
    __syncthreads();
    const int64_t run0 = (int64_t)blockIdx.x * (kFiltThreads / 64) * kFiltChunks * 64;
    for (int c = 0; c < kFiltChunks; ++c) {
        const int64_t r0 = run0 + ((int64_t)c * (kFiltThreads / 64) + wave) * 64;
        if (r0 >= a.n_rows) break;
        const int64_t r = r0 + lane;
        const int32_t g = r < a.n_rows ? a.groups[r] : -1;
        unsigned long long mine = 0ull;
        for (int q = 0; q < nq; ++q) {
            bool allow = false;
            if (g >= 0) {
                const int h = table_find(tkey + (size_t)q * cells, a.tmask, a.shift, g);
                allow = h >= 0 ? ((tfull[(size_t)q * (cells / 32) + (h >> 5)] >> (h & 31)) & 1u) == 0u : nopen[q] < a.k;
            }
            const unsigned long long mk = __ballot(allow);
            if (lane == q) mine = mk;
        }
        if (lane < nq) {
            const int64_t w0 = r0 >> 5;
            uint32_t lo = (uint32_t)mine, hi = (uint32_t)(mine >> 32);
            if (a.filt) {
                const int64_t b = a.qmap ? (int64_t)a.qmap[q0 + lane] : (int64_t)(q0 + lane);
                const uint32_t* f = a.filt + (b >= 0 && b < a.B ? (size_t)b : 0) * (size_t)a.filt_ld;
                lo &= f[w0];
                if (w0 + 1 < a.W) hi &= f[w0 + 1];
            }
            uint32_t* o = a.out + (size_t)(q0 + lane) * (size_t)a.ld_words;
            o[w0] = lo;
            if (w0 + 1 < a.W) o[w0 + 1] = hi;
        }
    }
}

// kept rows of open groups that are not full: their bits go (one workgroup per listed query)
__global__ __launch_bounds__(256) void group_filter_kept_kernel(GroupFilterArgs a) {
    const int64_t b = a.qmap ? (int64_t)a.qmap[blockIdx.x] : (int64_t)blockIdx.x;
    if (b < 0 || b >= a.B) return;
    uint32_t* o = a.out + (size_t)blockIdx.x * (size_t)a.ld_words;
    for (int t = threadIdx.x; t < a.k * a.m; t += 256) {
        const int j = t / a.m, p = t % a.m;
        if (a.sg[b * a.k + j] < 0) continue;
        const int32_t c = a.sc[b * a.k + j];
        if (c >= a.m || p >= c) continue;
        const int64_t id = a.si[((size_t)b * a.k + j) * (size_t)a.m + p];
        if (id < 0 || id >= a.n_rows) continue;
        atomicAnd(&o[id >> 5], ~(1u << (id & 31)));
    }
}

// ---- host helpers ------------------------------------------------------------------------------------------------------------------
int table_cells(int k) { return (int)pow2_ceil((uint32_t)std::max(2 * k, 64)); }
int log2_of(uint32_t p) {
    int l = 0;
    while ((1u << l) < p) ++l;
    return l;
}

int check_km(int32_t k, int32_t m) {
    if (k < 1 || k > kMaxK) return fail(VS_EINVAL, "k must be in 1..%d (got %d)", kMaxK, k);
    if (m < 1 || m > kMaxM) return fail(VS_EINVAL, "per_group must be in 1..%d (got %d)", kMaxM, m);
    if ((int64_t)k * m > kMaxKM) return fail(VS_EINVAL, "k * per_group must be at most %d (got %d x %d)", kMaxKM, k, m);
    return VS_OK;
}

}  // namespace

extern "C" int vs_topk_collapse(const int64_t* ids, const float* scores, int32_t Bp, int32_t kk, int64_t ld, const int32_t* qmap, const int32_t* groups,
                                int64_t n_rows, int32_t B, int32_t k, int32_t m, int32_t* out_group, int32_t* out_count, int64_t* out_ids,
                                float* out_scores, int32_t* out_status, int32_t* out_incomplete, int init, int exhausted_hint, int device, void* stream) {
    VS_TRY(need_device());
    if (!ids || !scores || !groups || !out_group || !out_count || !out_ids || !out_scores || !out_status || !out_incomplete)
        return fail(VS_EINVAL, "NULL argument");
    if (Bp <= 0 || B <= 0 || n_rows <= 0) return fail(VS_EINVAL, "the list count, B and n_rows must be positive");
    VS_TRY(check_km(k, m));
    if (kk < 1 || kk > kMaxKK) return fail(VS_EINVAL, "kk must be in 1..%d (got %d)", kMaxKK, kk);
    if (ld < kk) return fail(VS_EINVAL, "ld = %lld is shorter than kk = %d", (long long)ld, kk);
    if (!qmap && Bp > B) return fail(VS_EINVAL, "%d lists but state for %d queries", Bp, B);
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range", device);
    const void* ptrs[10] = {ids, scores, qmap, groups, out_group, out_count, out_ids, out_scores, out_status, out_incomplete};
    const char* names[10] = {"ids", "scores", "qmap", "groups", "out_group", "out_count", "out_ids", "out_scores", "out_status", "out_incomplete"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 10, device, &dev));
    const size_t n_in = (size_t)(Bp - 1) * ld + kk;
    if (!dev) {                                                              // host lists are checked here; device lists end at such an id
        for (int32_t i = 0; i < Bp; ++i) {
            if (qmap && (qmap[i] < 0 || qmap[i] >= B)) return fail(VS_EINVAL, "qmap[%d] = %d is outside [0, %d)", i, qmap[i], B);
            for (int32_t j = 0; j < kk; ++j) {
                const int64_t id = ids[(size_t)i * ld + j];
                if (id < -1 || id >= n_rows) return fail(VS_EINVAL, "document id %lld is outside [-1, %lld)", (long long)id, (long long)n_rows);
            }
        }
    }
    VS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    Staged st[10];
    CollapseArgs a{};
    int64_t* d_ids;
    float* d_sc;
    int32_t *d_qmap, *d_groups;
    VS_TRY(st[0].in(ids, n_in, dev, true, s, &d_ids));
    VS_TRY(st[1].in(scores, n_in, dev, true, s, &d_sc));
    VS_TRY(st[2].in(qmap, (size_t)Bp, dev, true, s, &d_qmap));
    VS_TRY(st[3].in(groups, (size_t)n_rows, dev, true, s, &d_groups));
    const size_t nk = (size_t)B * k;
    VS_TRY(st[4].in(out_group, nk, dev, true, s, &a.og));                     // (the state goes in as well: a continuing round reads it, and the
    VS_TRY(st[5].in(out_count, nk, dev, true, s, &a.oc));                     //  queries the call does not list keep theirs)
    VS_TRY(st[6].in(out_ids, nk * m, dev, true, s, &a.oi));
    VS_TRY(st[7].in(out_scores, nk * m, dev, true, s, &a.os));
    VS_TRY(st[8].in(out_status, (size_t)B, dev, true, s, &a.status));
    VS_TRY(st[9].in(out_incomplete, (size_t)1, dev, false, s, &a.incomplete));
    VS_HIP(hipMemsetAsync(a.incomplete, 0, 4, s));
    a.ids = d_ids; a.sc = d_sc; a.kk = kk; a.ld = ld; a.qmap = d_qmap; a.groups = d_groups; a.n_rows = n_rows;
    a.B = B; a.k = k; a.m = m; a.init = init ? 1 : 0; a.exhausted = exhausted_hint ? 1 : 0;
    const int cells = table_cells(k);
    a.tmask = (uint32_t)cells - 1u;
    a.shift = 32 - log2_of((uint32_t)cells);
    {
        ProfScope prof("topk_collapse", s);
        hipLaunchKernelGGL(topk_collapse_kernel, dim3((unsigned)Bp), dim3(64), (size_t)(2 * cells + k) * 4, s, a);
        VS_HIP(hipGetLastError());
    }
    VS_STAGE("topk_collapse", s);
    if (!dev)
        for (int i = 4; i < 10; ++i) VS_TRY(st[i].back(s));
    if (!stream || !dev) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}

extern "C" int vs_group_filter(const int32_t* groups, int64_t n_rows, int32_t Bp, const int32_t* qmap, int32_t B, int32_t k, int32_t m,
                               const int32_t* state_group, const int32_t* state_count, const int64_t* state_ids, const uint32_t* filter,
                               int64_t filter_ld, uint32_t* out_words, int64_t ld_words, int device, void* stream) {
    VS_TRY(need_device());
    if (!groups || !state_group || !state_count || !state_ids || !out_words) return fail(VS_EINVAL, "NULL argument");
    if (Bp <= 0 || B <= 0 || n_rows <= 0) return fail(VS_EINVAL, "the query count, B and n_rows must be positive");
    VS_TRY(check_km(k, m));
    const int64_t W = (n_rows + 31) / 32;
    if (ld_words < W) return fail(VS_EINVAL, "ld_words = %lld is shorter than the %lld words of %lld rows", (long long)ld_words, (long long)W, (long long)n_rows);
    if (filter && filter_ld != 0 && filter_ld < W) return fail(VS_EINVAL, "filter_ld = %lld is shorter than the %lld words of a bitmap", (long long)filter_ld, (long long)W);
    if (!qmap && Bp > B) return fail(VS_EINVAL, "%d queries but state for %d", Bp, B);
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range", device);
    const void* ptrs[7] = {groups, qmap, state_group, state_count, state_ids, filter, out_words};
    const char* names[7] = {"groups", "qmap", "state_group", "state_count", "state_ids", "filter", "out_words"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 7, device, &dev));
    if (!dev && qmap)
        for (int32_t i = 0; i < Bp; ++i)
            if (qmap[i] < 0 || qmap[i] >= B) return fail(VS_EINVAL, "qmap[%d] = %d is outside [0, %d)", i, qmap[i], B);
    VS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    Staged st[7];
    GroupFilterArgs a{};
    int32_t *d_groups, *d_qmap, *d_sg, *d_sc;
    int64_t* d_si;
    uint32_t* d_f;
    const size_t nk = (size_t)B * k;
    const size_t out_n = (size_t)(Bp - 1) * ld_words + W;
    VS_TRY(st[0].in(groups, (size_t)n_rows, dev, true, s, &d_groups));
    VS_TRY(st[1].in(qmap, (size_t)Bp, dev, true, s, &d_qmap));
    VS_TRY(st[2].in(state_group, nk, dev, true, s, &d_sg));
    VS_TRY(st[3].in(state_count, nk, dev, true, s, &d_sc));
    VS_TRY(st[4].in(state_ids, nk * m, dev, true, s, &d_si));
    VS_TRY(st[5].in(filter, filter_ld ? (size_t)(B - 1) * filter_ld + W : (size_t)W, dev, true, s, &d_f));
    if (!dev) {
        if (st[6].buf.alloc(out_n * 4) != VS_OK)
            return fail(VS_ENOMEM, "the per-query bitmaps of %d queries over %lld rows take %zu bytes of device memory", Bp, (long long)n_rows, out_n * 4);
        st[6].host = out_words;
        st[6].bytes = out_n * 4;
        VS_HIP(hipMemcpyAsync(st[6].buf.p, out_words, out_n * 4, hipMemcpyHostToDevice, s));   // (words past W of a row stay the caller's)
        a.out = st[6].buf.as<uint32_t>();
    } else {
        a.out = out_words;
    }
    a.groups = d_groups; a.n_rows = n_rows; a.Bp = Bp; a.B = B; a.qmap = d_qmap; a.k = k; a.m = m; a.sg = d_sg; a.sc = d_sc; a.si = d_si;
    a.filt = d_f; a.filt_ld = filter_ld; a.ld_words = ld_words; a.W = W;
    const int cells = table_cells(k);
    a.tmask = (uint32_t)cells - 1u;
    a.shift = 32 - log2_of((uint32_t)cells);
    const size_t per_q = (size_t)cells * 4 + (size_t)cells / 8 + 4;
    a.tile = (int32_t)std::min<size_t>(std::min<size_t>(kFiltMaxTile, kFiltLds / per_q), (size_t)Bp);
    const int64_t run = (int64_t)(kFiltThreads / 64) * kFiltChunks * 64;
    const int64_t gx = ceil_div64(n_rows, run);
    if (gx > 0x7FFFFFFF || ceil_div(Bp, a.tile) > 65535) return fail(VS_EINVAL, "n_rows = %lld / %d queries are too many for one call", (long long)n_rows, Bp);
    {
        ProfScope prof("group_filter", s);
        hipLaunchKernelGGL(group_filter_kernel, dim3((unsigned)gx, (unsigned)ceil_div(Bp, a.tile)), dim3(kFiltThreads), per_q * a.tile, s, a);
        VS_HIP(hipGetLastError());
        hipLaunchKernelGGL(group_filter_kept_kernel, dim3((unsigned)Bp), dim3(256), 0, s, a);
        VS_HIP(hipGetLastError());
    }
    VS_STAGE("group_filter", s);
    if (!dev) VS_TRY(st[6].back(s));
    if (!stream || !dev) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}
