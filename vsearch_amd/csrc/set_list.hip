// set_list.hip -- set egress (vs_set_list_plan, vs_set_count, vs_set_ids, vs_set_sample, vs_set_from_ids and their vs_index_* variants): the
// size of a document set, its members as a sorted id list or a page of it, a uniform sample of it, and the way back from id lists to a bitmap
// (DESIGN.md 3.1s).  No reference counterpart (the reference only has topk, index.py:92).  Nothing here touches a search kernel: a set arrives
// as a packed bitmap in the layout of vs_index_search_filtered.  No atomic decides a position and no float is involved, so every result is exact
// and independent of the launch.
//
// (a) Count: a wave owns a 2048-row span of one query.  Lane s forms the 64 rows of step s out of the set's and the and-bitmap's words (three
//     lane reads each, whatever bit the rows start at) and the wave adds the popcounts: span_count uint32 [B, spans], plain stores.
// (b) Scan: one workgroup per query turns the span counts into exclusive int64 bases, 256 spans a step, and writes the size of the set.
// (c) Write: a wave per span again.  A span whose ranks [base, base + count) miss the window is left without reading the bitmap.  Otherwise
//     lane s holds the popcount of step s, a wave-exclusive scan gives the step bases, and a row's rank is base + step base + the set rows below
//     it in its step; rows inside the window are stored at rank - offset.  A fourth launch writes -1 behind the last member.
// (d) Sample: the shape of vs_value_topk with the key computed instead of loaded.  A workgroup owns a chunk and one query, walks the set with
//     walk_rows and pushes (~hash << 32 | ~row) above the threshold into the buffer of topn_stream.h; per-chunk lists and per-chunk counts go
//     to scratch, and one workgroup per query merges them (stream_topn) and adds the counts.
// (e) From ids: the bitmaps are cleared, every listed id ORs its bit in (a vector atomicOr), and an invert pass gives the complement.
#include "agg_call.h"
#include "set_list_check.h"
#include "set_walk.h"
#include "topn_stream.h"

using namespace vs;

namespace {

static_assert(kTopCap - kTopKeep >= kSpanRows, "a span adds up to kSpanRows candidates");

// a value every lane of the wave holds alike, in scalar registers: the branches on it are uniform for the compiler as well
__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// bits [64 s + sh, 64 s + sh + 64) of the span for a step s of the lane's own (0..31): window64 of bitmap_span.h with the lane reads as shuffles
__device__ __forceinline__ uint64_t lane_window64(const Span& sp, int s, int sh) {
    const uint32_t a = (uint32_t)__shfl((int)sp.lo, 2 * s, 64);
    const uint32_t b = (uint32_t)__shfl((int)sp.hi, 2 * s, 64);
    const uint32_t c = (uint32_t)__shfl((int)sp.hi, 2 * s + 1, 64);
    uint64_t v = (((uint64_t)b << 32) | a) >> sh;
    if (sh) v |= (uint64_t)c << (64 - sh);
    return v;
}

// The set rows of the span at row rb for query b: lane s < 32 -> the rows of step s (bit l: row rb + 64 s + l), lanes 32..63 -> 0.  Every lane
// of the wave calls it.
__device__ __forceinline__ uint64_t span_steps(const RowSet& a, size_t b, int64_t rb, int lane) {
    const int64_t n_w = (a.bit0 + a.n_rows + 31) >> 5, n_aw = (a.and_bit0 + a.n_rows + 31) >> 5;
    const int s = lane & 31;
    uint64_t m = ~0ull;
    if (a.and_words) {
        const int64_t p = a.and_bit0 + rb;
        const Span an = load_span(a.and_words, p >> 5, n_aw, lane);
        if (__builtin_amdgcn_ballot_w64((an.lo | an.hi) != 0u) == 0ull) return 0ull;
        m &= lane_window64(an, s, (int)(p & 31));
    }
    if (a.words) {
        const int64_t p = a.bit0 + rb;
        const Span sp = load_span(a.words + b * (size_t)a.ld_words, p >> 5, n_w, lane);
        if (__builtin_amdgcn_ballot_w64((sp.lo | sp.hi) != 0u) == 0ull) return 0ull;
        m &= lane_window64(sp, s, (int)(p & 31));
    }
    const int64_t nvalid = a.n_rows - (rb + (int64_t)s * 64);                          // rows from the step's first to the last of all
    if (lane >= 32 || nvalid <= 0) return 0ull;
    return m & valid_mask(nvalid);
}

// ---- (a) - (c) count and list --------------------------------------------------------------------------------------------------------------
struct ListArgs {
    RowSet set;
    int64_t spans;
    uint32_t* span_count;             // [B, spans]
    int64_t* span_base;               // [B, spans] or null (count only)
    const int64_t* offsets;           // [B] or null (0)
    int64_t limit, id_offset;
    int64_t* out_ids;                 // [B, limit]
    int64_t* out_counts;              // [B]
};

__global__ __launch_bounds__(kSetThreads) void set_count_kernel(ListArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t b = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * a.set.rows_per_chunk;                    // (whole spans)
    const int64_t r1 = min(a.set.n_rows, r0 + a.set.rows_per_chunk);
    for (int64_t rb = r0 + (int64_t)w * kSpanRows; rb < r1; rb += (int64_t)kSetWaves * kSpanRows) {
        uint32_t c = (uint32_t)__popcll(span_steps(a.set, b, rb, lane));
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);      // (lanes 32..63 hold 0)
        if (lane == 0) a.span_count[b * (size_t)a.spans + (size_t)(rb / kSpanRows)] = c;
    }
}

__global__ __launch_bounds__(kSetThreads) void set_scan_kernel(ListArgs a) {
    __shared__ uint64_t s_wave[kSetWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t b = blockIdx.x;
    const uint32_t* cnt = a.span_count + b * (size_t)a.spans;
    int64_t* base = a.span_base ? a.span_base + b * (size_t)a.spans : nullptr;
    uint64_t carry = 0ull;                                                            // (uniform)
    for (int64_t t0 = 0; t0 < a.spans; t0 += kSetThreads) {
        const int64_t i = t0 + tid;
        const uint64_t v = i < a.spans ? (uint64_t)cnt[i] : 0ull;
        uint64_t x = v;                                                               // inclusive over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_wave[w] = x;
        __syncthreads();
        uint64_t before = 0ull, all = 0ull;
#pragma unroll
        for (int k = 0; k < kSetWaves; ++k) {
            const uint64_t t = s_wave[k];
            if (k < w) before += t;
            all += t;
        }
        if (base && i < a.spans) base[i] = (int64_t)(carry + before + x - v);
        carry += all;
        __syncthreads();
    }
    if (tid == 0) a.out_counts[b] = (int64_t)carry;
}

__global__ __launch_bounds__(kSetThreads) void set_write_kernel(ListArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t b = blockIdx.y;
    const int64_t off = set_window_offset(uniform64(a.offsets ? a.offsets[b] : 0));
    const int64_t r0 = (int64_t)blockIdx.x * a.set.rows_per_chunk;
    const int64_t r1 = min(a.set.n_rows, r0 + a.set.rows_per_chunk);
    int64_t* dst = a.out_ids + b * (size_t)a.limit;
    for (int64_t rb = r0 + (int64_t)w * kSpanRows; rb < r1; rb += (int64_t)kSetWaves * kSpanRows) {
        const size_t si = b * (size_t)a.spans + (size_t)(rb / kSpanRows);
        const int64_t cnt = uniform64((int64_t)a.span_count[si]), base = uniform64(a.span_base[si]);
        if (set_span_misses(base, cnt, off, a.limit)) continue;                       // (uniform) left without reading the bitmap
        const uint64_t m = span_steps(a.set, b, rb, lane);
        const uint32_t pc = (uint32_t)__popcll(m);
        uint32_t x = pc;                                                              // inclusive over the wave (lanes 32..63 add 0)
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64);
            if (lane >= o) x += y;
        }
        const uint32_t sb = x - pc;                                                   // the set rows of the span before the lane's step
        const int nsub = (int)((min(a.set.n_rows, rb + kSpanRows) - rb + 63) >> 6);
        for (int s = 0; s < nsub; ++s) {
            const uint64_t ms = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(m >> 32), s) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)m, s);
            if (ms == 0ull) continue;                                                 // (uniform)
            const int64_t rank0 = base + (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)sb, s);
            if ((ms >> lane) & 1ull) {
                const int64_t rank = rank0 + __popcll(ms & ((1ull << lane) - 1ull));
                if (set_rank_in_window(rank, off, a.limit)) dst[rank - off] = rb + (int64_t)s * 64 + lane + a.id_offset;
            }
        }
    }
}

// -1 behind the last member: slot j of query b when offset + j is at or past the count
__global__ __launch_bounds__(kSetThreads) void set_tail_kernel(ListArgs a) {
    const size_t b = blockIdx.y;
    const int64_t off = set_window_offset(a.offsets ? a.offsets[b] : 0);
    const int64_t count = a.out_counts[b];
    int64_t* dst = a.out_ids + b * (size_t)a.limit;
    for (int64_t j = (int64_t)blockIdx.x * kSetThreads + threadIdx.x; j < a.limit; j += (int64_t)gridDim.x * kSetThreads)
        if (set_slot_is_tail(j, off, count)) dst[j] = -1;
}

// ---- (d) sample ------------------------------------------------------------------------------------------------------------------------------
struct SampleArgs {
    RowSet set;
    const uint64_t* seeds;            // [B]
    int32_t n;
    int64_t chunks;
    uint64_t* scratch;                // [B, chunks, n]
    uint32_t* chunk_count;            // [B, chunks]
    int64_t id_offset;
    int64_t* out_ids;                 // [B, n]
    uint32_t* out_hash;               // [B, n] or null
    int64_t* out_counts;              // [B]
};

__global__ __launch_bounds__(kSetThreads) void set_sample_chunk_kernel(SampleArgs a) {
    __shared__ uint64_t cand[kTopCap];
    __shared__ int cnt_sh;
    __shared__ uint32_t s_rows[kSetWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t c = blockIdx.x;
    const size_t b = blockIdx.y;
    const int K = a.n;
    const int64_t r0 = c * a.set.rows_per_chunk;
    const int64_t r1 = min(a.set.n_rows, r0 + a.set.rows_per_chunk);
    const uint64_t qk = set_sample_seed_key(a.seeds[b]);
    if (tid == 0) cnt_sh = 0;
    __syncthreads();
    uint64_t tau = 0ull;
    uint32_t rows = 0u;                                           // set rows this wave saw (uniform: a chunk holds fewer than 2^32 rows)
    walk_rows<kSetWaves>(a.set, b, r0, r1, w, lane, [&](int64_t row0, uint64_t m, int64_t) {
        rows += (uint32_t)__popcll(m);
        uint64_t key = 0ull;
        if ((m >> lane) & 1ull) {
            const int64_t row = row0 + lane;
            key = set_sample_key(set_sample_hash_keyed(qk, (uint64_t)(row + a.id_offset)), (uint32_t)row);      // never 0: row < 2^32 - 1
        }
        top_push(cand, &cnt_sh, key > tau, key, lane);
    }, [&] {                                                     // (the walk leaves a span for the whole workgroup or not at all)
        __syncthreads();
        tau = top_cut<kSetThreads>(cand, &cnt_sh, K, false, tau, tid);
    });
    if (lane == 0) s_rows[w] = rows;
    __syncthreads();
    (void)top_cut<kSetThreads>(cand, &cnt_sh, K, true, tau, tid);
    uint64_t* dst = a.scratch + (b * (size_t)a.chunks + (size_t)c) * (size_t)K;
    for (int i = tid; i < K; i += kSetThreads) dst[i] = cand[i];                      // sorted, zeros behind the last
    if (tid == 0) {
        uint32_t t = 0u;
        for (int k = 0; k < kSetWaves; ++k) t += s_rows[k];
        a.chunk_count[b * (size_t)a.chunks + (size_t)c] = t;
    }
}

__global__ __launch_bounds__(kSetThreads) void set_sample_merge_kernel(SampleArgs a) {
    __shared__ uint64_t cand[kTopCap];
    __shared__ int cnt_sh;
    __shared__ unsigned long long s_sum[kSetWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int K = a.n;
    const size_t b = blockIdx.x;
    const uint64_t* src = a.scratch + b * (size_t)a.chunks * (size_t)K;
    stream_topn<kSetThreads>(a.chunks * K, K, [&](int64_t i) { return src[i]; }, cand, &cnt_sh);
    for (int i = tid; i < K; i += kSetThreads) {                  // every slot is written: id -1 / hash 0xFFFFFFFF behind the last
        const uint64_t key = cand[i];
        a.out_ids[b * (size_t)K + i] = key ? (int64_t)set_sample_key_row(key) + a.id_offset : -1;
        if (a.out_hash) a.out_hash[b * (size_t)K + i] = key ? set_sample_key_hash(key) : 0xFFFFFFFFu;
    }
    uint64_t sum = 0ull;                                          // the size of the set: the chunks' counts added
    for (int64_t c = tid; c < a.chunks; c += kSetThreads) sum += a.chunk_count[b * (size_t)a.chunks + (size_t)c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += (uint64_t)__shfl_xor((unsigned long long)sum, o, 64);
    if (lane == 0) s_sum[w] = sum;
    __syncthreads();
    if (tid == 0) {
        uint64_t t = 0ull;
        for (int k = 0; k < kSetWaves; ++k) t += s_sum[k];
        a.out_counts[b] = (int64_t)t;
    }
}

// ---- (e) from ids ----------------------------------------------------------------------------------------------------------------------------
struct FromIdsArgs {
    const int64_t* ids;               // [B, ld_ids]
    int64_t m, ld_ids, n_rows, bit0, n_words;
    uint32_t* out;                    // [B, ld_words], words [0, n_words) of a row zeroed by the caller
    int64_t ld_words;
};

__global__ __launch_bounds__(kSetThreads) void set_scatter_kernel(FromIdsArgs a) {
    const size_t b = blockIdx.y;
    const int64_t* src = a.ids + b * (size_t)a.ld_ids;
    uint32_t* dst = a.out + b * (size_t)a.ld_words;
    for (int64_t j = (int64_t)blockIdx.x * kSetThreads + threadIdx.x; j < a.m; j += (int64_t)gridDim.x * kSetThreads) {
        const int64_t id = src[j];
        if (id < 0 || id >= a.n_rows) continue;                   // padding, or no row of these: never written anywhere
        const int64_t bit = a.bit0 + id;                          // (bit >> 5 < n_words)
        atomicOr(dst + (bit >> 5), 1u << (bit & 31));
    }
}

__global__ __launch_bounds__(kSetThreads) void set_invert_kernel(FromIdsArgs a) {
    uint32_t* dst = a.out + (size_t)blockIdx.y * (size_t)a.ld_words;
    for (int64_t w = (int64_t)blockIdx.x * kSetThreads + threadIdx.x; w < a.n_words; w += (int64_t)gridDim.x * kSetThreads)
        dst[w] = ~dst[w] & set_row_bits_of_word(w, a.bit0, a.n_rows);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------
unsigned grid_over(int64_t items) { return (unsigned)std::min<int64_t>(std::max<int64_t>(1, ceil_div64(items, kSetThreads)), 65535 * 16); }

// vs_set_count (limit = 0, out_ids NULL), vs_set_ids and their vs_index_* forms: one call on the set's device.  Host arrays are looked at before
// the device is (a pointer the runtime does not know, or no runtime at all: a host pointer).
int set_ids(const SetSrc& src, const int64_t* offsets, int64_t limit, int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids,
            int64_t* out_counts, void* stream) {
    SetListPlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(set_list_check_set(out_counts != nullptr, src.words != nullptr, src.bit0, src.ld_words, src.B, src.n_rows, rows_per_chunk, &plan,
                                           msg, sizeof msg), msg));
    VS_TRY(plan_or_fail(set_list_check_ids(limit, src.B, out_ids != nullptr, msg, sizeof msg), msg));
    if (offsets && !is_device_ptr(offsets)) VS_TRY(plan_or_fail(set_list_check_offsets_host(offsets, src.B, msg, sizeof msg), msg));
    VS_TRY(src.device_ok());
    if (!limit) out_ids = nullptr;
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"offsets", offsets}, {"out_ids", out_ids},
                                       {"out_counts", out_counts}}));
    const int32_t B = src.B;
    BitmapStage st;
    Staged st_off, st_ids, st_cnt;
    DevBuf scratch;
    const char* name = limit ? "set_ids" : "set_count";
    return c.run(name, Finish::kSync, [&] {
        ListArgs a{};
        int64_t* d_off;
        VS_TRY(st.in(src, plan.rows_per_chunk, c.dev, c.s, &a.set));
        VS_TRY(st_off.in(offsets, (size_t)B, c.dev, true, c.s, &d_off));
        VS_TRY(st_ids.in(out_ids, (size_t)B * (size_t)limit, c.dev, false, c.s, &a.out_ids));
        VS_TRY(st_cnt.in(out_counts, (size_t)B, c.dev, false, c.s, &a.out_counts));
        const size_t cells = (size_t)B * (size_t)plan.spans;
        VS_TRY(scratch.alloc(cells * (limit ? 12 : 4)));           // the bases (8-byte aligned: first), then the counts
        a.span_base = limit ? scratch.as<int64_t>() : nullptr;
        a.span_count = reinterpret_cast<uint32_t*>(scratch.as<char>() + (limit ? cells * 8 : 0));
        a.spans = plan.spans;
        a.offsets = d_off;
        a.limit = limit;
        a.id_offset = id_offset;
        ProfScope prof(name, c.s);
        const dim3 grid((unsigned)plan.chunks, (unsigned)B);
        hipLaunchKernelGGL(set_count_kernel, grid, dim3(kSetThreads), 0, c.s, a);
        hipLaunchKernelGGL(set_scan_kernel, dim3((unsigned)B), dim3(kSetThreads), 0, c.s, a);
        if (limit) {
            hipLaunchKernelGGL(set_write_kernel, grid, dim3(kSetThreads), 0, c.s, a);
            hipLaunchKernelGGL(set_tail_kernel, dim3(grid_over(limit), (unsigned)B), dim3(kSetThreads), 0, c.s, a);
        }
        return VS_OK;
    }, [&] {
        VS_TRY(st_ids.back(c.s));
        return st_cnt.back(c.s);
    });
}

// vs_set_sample and vs_index_set_sample
int set_sample(const SetSrc& src, const uint64_t* seeds, int32_t n, int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids, uint32_t* out_hash,
               int64_t* out_counts, void* stream) {
    SetListPlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(set_list_check_set(seeds && out_ids && out_counts, src.words != nullptr, src.bit0, src.ld_words, src.B, src.n_rows,
                                           rows_per_chunk, &plan, msg, sizeof msg), msg));
    VS_TRY(plan_or_fail(set_list_check_sample(n, src.B, plan, msg, sizeof msg), msg));
    VS_TRY(src.device_ok());
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"seeds", seeds}, {"out_ids", out_ids},
                                       {"out_hash", out_hash}, {"out_counts", out_counts}}));
    const int32_t B = src.B;
    BitmapStage st;
    Staged st_seed, st_ids, st_hash, st_cnt;
    DevBuf scratch;
    return c.run("set_sample", Finish::kSync, [&] {
        SampleArgs a{};
        uint64_t* d_seed;
        VS_TRY(st.in(src, plan.rows_per_chunk, c.dev, c.s, &a.set));
        VS_TRY(st_seed.in(seeds, (size_t)B, c.dev, true, c.s, &d_seed));
        VS_TRY(st_ids.in(out_ids, (size_t)B * n, c.dev, false, c.s, &a.out_ids));
        VS_TRY(st_hash.in(out_hash, (size_t)B * n, c.dev, false, c.s, &a.out_hash));
        VS_TRY(st_cnt.in(out_counts, (size_t)B, c.dev, false, c.s, &a.out_counts));
        const size_t lists = (size_t)B * (size_t)plan.chunks;
        VS_TRY(scratch.alloc(lists * (size_t)n * 8 + lists * 4));  // the keys, then the chunks' counts
        a.seeds = d_seed;
        a.n = n;
        a.chunks = plan.chunks;
        a.scratch = scratch.as<uint64_t>();
        a.chunk_count = reinterpret_cast<uint32_t*>(a.scratch + lists * (size_t)n);
        a.id_offset = id_offset;
        ProfScope prof("set_sample", c.s);
        hipLaunchKernelGGL(set_sample_chunk_kernel, dim3((unsigned)plan.chunks, (unsigned)B), dim3(kSetThreads), 0, c.s, a);
        hipLaunchKernelGGL(set_sample_merge_kernel, dim3((unsigned)B), dim3(kSetThreads), 0, c.s, a);
        return VS_OK;
    }, [&] {
        VS_TRY(st_ids.back(c.s));
        VS_TRY(st_hash.back(c.s));
        return st_cnt.back(c.s);
    });
}

}  // namespace

extern "C" uint32_t vs_set_sample_hash(uint64_t seed, int64_t id) { return set_sample_hash(seed, (uint64_t)id); }

extern "C" int vs_set_list_plan(int64_t n_rows, int32_t B, int per_query, int64_t rows_per_chunk, int64_t* out_chunks, int64_t* out_rows_per_chunk,
                                int64_t* out_spans) {
    if (!out_chunks || !out_rows_per_chunk || !out_spans) return fail(VS_EINVAL, "NULL argument");
    SetListPlan p;
    char msg[256];
    VS_TRY(plan_or_fail(set_list_plan(n_rows, B, per_query != 0, rows_per_chunk, &p, msg, sizeof msg), msg));
    *out_chunks = p.chunks;
    *out_rows_per_chunk = p.rows_per_chunk;
    *out_spans = p.spans;
    return VS_OK;
}

extern "C" int vs_set_count(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, int64_t n_rows,
                            int64_t rows_per_chunk, int64_t* out_counts, int device, void* stream) {
    return set_ids(free_set(words, bit0, ld_words, and_words, B, n_rows, device), nullptr, 0, 0, rows_per_chunk, nullptr, out_counts, stream);
}

extern "C" int vs_index_set_count(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, int64_t rows_per_chunk,
                                  int64_t* out_counts, void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return set_ids(src, nullptr, 0, 0, rows_per_chunk, nullptr, out_counts, stream);
}

extern "C" int vs_set_ids(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, int64_t n_rows,
                          const int64_t* offsets, int64_t limit, int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids, int64_t* out_counts,
                          int device, void* stream) {
    return set_ids(free_set(words, bit0, ld_words, and_words, B, n_rows, device), offsets, limit, id_offset, rows_per_chunk, out_ids, out_counts, stream);
}

extern "C" int vs_index_set_ids(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const int64_t* offsets, int64_t limit,
                                int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids, int64_t* out_counts, void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return set_ids(src, offsets, limit, id_offset, rows_per_chunk, out_ids, out_counts, stream);
}

extern "C" int vs_set_sample(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, int64_t n_rows,
                             const uint64_t* seeds, int32_t n, int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids, uint32_t* out_hash,
                             int64_t* out_counts, int device, void* stream) {
    return set_sample(free_set(words, bit0, ld_words, and_words, B, n_rows, device), seeds, n, id_offset, rows_per_chunk, out_ids, out_hash, out_counts,
                      stream);
}

extern "C" int vs_index_set_sample(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const uint64_t* seeds, int32_t n,
                                   int64_t id_offset, int64_t rows_per_chunk, int64_t* out_ids, uint32_t* out_hash, int64_t* out_counts,
                                   void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return set_sample(src, seeds, n, id_offset, rows_per_chunk, out_ids, out_hash, out_counts, stream);
}

extern "C" int vs_set_from_ids(const int64_t* ids, int32_t B, int64_t m, int64_t ld_ids, int64_t n_rows, int64_t bit0, int allow, uint32_t* out_words,
                               int64_t ld_words, int device, void* stream) {
    char msg[256];
    VS_TRY(plan_or_fail(set_list_check_from_ids(ids != nullptr, out_words != nullptr, B, m, ld_ids, n_rows, bit0, ld_words, msg, sizeof msg), msg));
    if (m > 0 && !is_device_ptr(ids)) VS_TRY(plan_or_fail(set_list_check_id_lists_host(ids, B, m, ld_ids, n_rows, msg, sizeof msg), msg));
    VS_TRY(device_in_range(device));
    Call c;
    VS_TRY(c.open(device, stream, {{"ids", m > 0 ? ids : nullptr}, {"out_words", out_words}}));
    Staged st_i, st_o;
    return c.run("set_from_ids", Finish::kStream, [&] {
        FromIdsArgs a{};
        a.m = m;
        a.ld_ids = ld_ids;
        a.n_rows = n_rows;
        a.bit0 = bit0;
        a.n_words = (bit0 + n_rows + 31) >> 5;
        a.ld_words = ld_words;
        int64_t* d_i = nullptr;
        if (m > 0) VS_TRY(st_i.in(ids, (size_t)(B - 1) * (size_t)ld_ids + (size_t)m, c.dev, true, c.s, &d_i));
        // (a host buffer's gaps between the rows come back as they went in: the staged copy starts from the caller's words)
        VS_TRY(st_o.in(out_words, (size_t)(B - 1) * (size_t)ld_words + (size_t)a.n_words, c.dev, true, c.s, &a.out));
        a.ids = d_i;
        if (ld_words == a.n_words || B == 1) VS_HIP(hipMemsetAsync(a.out, 0, ((size_t)(B - 1) * (size_t)ld_words + (size_t)a.n_words) * 4, c.s));
        else VS_HIP(hipMemset2DAsync(a.out, (size_t)ld_words * 4, 0, (size_t)a.n_words * 4, (size_t)B, c.s));
        ProfScope prof("set_from_ids", c.s);
        if (m > 0) hipLaunchKernelGGL(set_scatter_kernel, dim3(std::min(grid_over(m), 65535u), (unsigned)B), dim3(kSetThreads), 0, c.s, a);
        if (!allow) hipLaunchKernelGGL(set_invert_kernel, dim3(std::min(grid_over(a.n_words), 65535u), (unsigned)B), dim3(kSetThreads), 0, c.s, a);
        return VS_OK;
    }, [&] { return st_o.back(c.s); });
}
