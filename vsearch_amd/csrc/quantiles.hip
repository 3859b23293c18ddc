// quantiles.hip -- percentiles (vs_value_quantile_plan, vs_value_quantiles, vs_value_radix_counts, vs_value_radix_step and the vs_index_*
// variants): exact order statistics of a numeric field over any document set.  No reference counterpart.  A most-significant-
// digit radix select on the uint32 order keys of value_check.h, three levels (bits 31..21, 20..10, 9..0: quantile_check.h), every level one
// counting pass over bitmaps and values and one tiny step.  All integer: shards add their counts between the levels.
//
// (a) Counting (value_radix_kernel): a workgroup owns a chunk of rows and a tile of QT queries and walks the bitmaps with walk_tile (set_walk.h) as the
//     histogram of values.hip does.  LDS: one uint32 histogram of `bins` per (query, slot).  Level 0 has one slot a query and counts the missing
//     rows; at levels 1 and 2 a query's slots are the sorted distinct key prefixes its ranks resolved to (padded to 16 in LDS), a row's slot is
//     radix_find_slot (branch-free, 4 steps and a compare), a row of no slot costs no atomic.  When every counted row of a 64-row step falls
//     into one bin, one lane adds the popcount.  Only the slots in use are zeroed and flushed (64-bit atomics on the non-zero bins); a tile none
//     of whose ranks resolved leaves at once.
// (b) Step (value_radix_step_kernel): one workgroup a query.  Per slot a block prefix scan of its bins into LDS, per rank radix_find_bin; then
//     the ranks' extended prefixes are deduplicated and sorted into the next level's slots (R <= 16: counted, not sorted).  Level 0 forms count
//     and the ranks (quantile_rank), level 2 writes the values.
#include "agg_call.h"
#include "value_check.h"
#include "quantile_check.h"

using namespace vs;

namespace {

constexpr int kMaxRanks = VS_VALUE_MAX_RANKS;
constexpr int kStepThreads = 256;

struct RadixArgs {
    SetArgs s;
    int level;
    int32_t R;
    const uint32_t* slot_prefix;      // [B, R] (levels 1, 2)
    const int32_t* n_slots;           // [B]    (levels 1, 2)
    unsigned long long* counts;       // [B, S, bins], zeroed by the caller
    unsigned long long* missing;      // [B], zeroed by the caller (level 0)
};

struct StepArgs {
    int level, method, dtype;
    int32_t B, R;
    const int64_t* counts;            // [B, S, bins]
    const double* q;                  // [R] or null (level 0)
    const int64_t* ranks;             // [B, R] (level 0, q == null)
    int64_t* rank_res;                // [B, R]
    int32_t* rank_slot;               // [B, R]
    uint32_t* rank_prefix;            // [B, R]
    uint32_t* slot_prefix;            // [B, R]
    int32_t* n_slots;                 // [B]
    int64_t* count;                   // [B]    (level 0)
    int64_t* out_ranks;               // [B, R] (level 0)
    uint32_t* out_values;             // [B, R] (level 2)
};

// ---- (a) counting ----------------------------------------------------------------------------------------------------------------------------------
template <int QT, bool TOP>
__global__ __launch_bounds__(kValThreads) void value_radix_kernel(RadixArgs a) {
    extern __shared__ uint32_t rad_lds[];                        // the histograms [QT][S][bins]
    __shared__ uint32_t s_pre[QT * kMaxRanks];                   // a query's slot prefixes, ascending, kRadixNoSlot behind the last
    __shared__ uint32_t s_mis[QT];
    __shared__ int s_ns[QT];                                     // slots in use
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q0 = (int)blockIdx.y * QT;
    const int nq = min(QT, a.s.set.B - q0);
    const int64_t r0 = (int64_t)blockIdx.x * a.s.set.rows_per_chunk;
    const int64_t r1 = min(a.s.set.n_rows, r0 + a.s.set.rows_per_chunk);
    const int level = TOP ? 0 : a.level;
    const uint32_t bins = (uint32_t)radix_bins(level);
    const uint32_t qstride = (TOP ? 1u : (uint32_t)a.R) * bins;  // uint32 words of a query's histograms
    if (tid < QT) {
        s_mis[tid] = 0u;
        s_ns[tid] = tid >= nq ? 0 : TOP ? 1 : min(max(a.n_slots[q0 + tid], 0), a.R);
    }
    if (!TOP && tid < QT * kMaxRanks) {
        const int q = tid / kMaxRanks, j = tid % kMaxRanks;
        uint32_t p = kRadixNoSlot;
        if (q < nq && j < min(max(a.n_slots[q0 + q], 0), a.R)) p = a.slot_prefix[(size_t)(q0 + q) * (size_t)a.R + j];
        s_pre[tid] = p;
    }
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int q = 0; q < QT; ++q) any |= s_ns[q];
    if (!any) return;                                            // (uniform) no rank of the tile resolved: nothing to count
    for (int q = 0; q < nq; ++q)
        for (uint32_t i = tid; i < (uint32_t)s_ns[q] * bins; i += kValThreads) rad_lds[(size_t)q * qstride + i] = 0u;
    __syncthreads();
    uint32_t mis[QT];                                            // wave-uniform: a chunk holds fewer than 2^32 rows
#pragma unroll
    for (int q = 0; q < QT; ++q) mis[q] = 0u;
    const int shift = radix_shift(level);
    walk_tile<QT, kValWaves>(a.s.set, q0, nq, r0, r1, w, lane, [&](int64_t row0, uint64_t many, const Span* sp, int s, int sh, uint64_t live) {
        const uint32_t key = (many >> lane) & 1ull ? value_key(a.s.values[row0 + lane], a.s.dtype) : 0u;      // once for the tile
        const uint32_t dig = (key >> shift) & (bins - 1u);                            // once for the tile
        const uint32_t pre = TOP ? 0u : radix_prefix(key, level);
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            if (q >= nq) continue;
            const uint64_t m = window64(sp[q], s, sh) & live;
            if (m == 0ull) continue;
            const bool in = (m >> lane) & 1ull;
            bool has = in && key != 0u;
            uint32_t idx = dig;
            if (!TOP) {
                const int slot = radix_find_slot(s_pre + q * kMaxRanks, pre);
                has = has && slot >= 0;
                idx = (uint32_t)max(slot, 0) * bins + dig;
            }
            const uint64_t mh = __builtin_amdgcn_ballot_w64(has);
            if (TOP) mis[q] += (uint32_t)__popcll(m) - (uint32_t)__popcll(mh);
            if (mh == 0ull) continue;                                                 // no row of a slot: no atomic
            const int first = __builtin_ctzll(mh);
            const uint32_t i0 = (uint32_t)__builtin_amdgcn_readlane((int)idx, first);
            const bool one = __builtin_amdgcn_ballot_w64(has && idx == i0) == mh;     // every counted row of the step in one bin: add once
            uint32_t* dst = rad_lds + (size_t)q * qstride;
            if (one) {
                if (lane == first) atomicAdd(dst + i0, (uint32_t)__popcll(mh));
            } else if (has) {
                atomicAdd(dst + idx, 1u);
            }
        }
    });
    if (TOP) {
#pragma unroll
        for (int q = 0; q < QT; ++q)
            if (q < nq && lane == 0 && mis[q]) atomicAdd(&s_mis[q], mis[q]);
    }
    __syncthreads();
    for (int q = 0; q < nq; ++q) {
        const size_t b = (size_t)(q0 + q);
        unsigned long long* dst = a.counts + b * (size_t)qstride;
        for (uint32_t i = tid; i < (uint32_t)s_ns[q] * bins; i += kValThreads) {
            const uint32_t v = rad_lds[(size_t)q * qstride + i];
            if (v) atomicAdd(dst + i, (unsigned long long)v);
        }
    }
    if (TOP && tid < nq && s_mis[tid]) atomicAdd(&a.missing[q0 + tid], (unsigned long long)s_mis[tid]);
}

// ---- (b) the step ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kStepThreads) void value_radix_step_kernel(StepArgs a) {
    __shared__ int64_t cum[VS_VALUE_RADIX_BINS + 1];             // exclusive prefix sums of the slot's bins, the total behind them
    __shared__ int64_t part[kStepThreads];
    __shared__ int64_t s_res[kMaxRanks], s_newres[kMaxRanks];
    __shared__ int s_slot[kMaxRanks], s_first[kMaxRanks];
    __shared__ uint32_t s_oldpre[kMaxRanks], s_newpre[kMaxRanks];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int R = a.R, level = a.level;
    const int bins = radix_bins(level), per = bins / kStepThreads;                    // 8 or 4 bins a thread
    const int S = level == 0 ? 1 : R;
    const int ns_in = level == 0 ? 1 : min(max(a.n_slots[b], 0), R);                  // (uniform)
    if (tid < kMaxRanks) {
        int sl = -1;
        int64_t r = -1;
        if (tid < R) {
            if (level == 0) {
                sl = 0;                                                               // the rank itself is formed below, once count is known
            } else {
                sl = a.rank_slot[b * R + tid];
                r = a.rank_res[b * R + tid];
                if (sl < 0 || sl >= ns_in || r < 0) {
                    sl = -1;
                    r = -1;
                }
            }
        }
        s_slot[tid] = sl;
        s_res[tid] = r;
        s_newres[tid] = -1;
        s_newpre[tid] = 0u;
        s_oldpre[tid] = level > 0 && tid < ns_in ? a.slot_prefix[b * R + tid] : 0u;
    }
    __syncthreads();
    for (int s = 0; s < ns_in; ++s) {
        const int64_t* c = a.counts + (b * (size_t)S + (size_t)s) * (size_t)bins;
        int64_t loc[8], sum = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            loc[i] = i < per ? c[tid * per + i] : 0;
            sum += loc[i];
        }
        part[tid] = sum;
        __syncthreads();
        for (int o = 1; o < kStepThreads; o <<= 1) {                                  // block scan of the threads' sums
            const int64_t v = tid >= o ? part[tid - o] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        int64_t run = part[tid] - sum;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < per) {
                cum[tid * per + i] = run;
                run += loc[i];
            }
        if (tid == kStepThreads - 1) cum[bins] = run;
        __syncthreads();
        if (level == 0 && tid < R) {
            const int64_t total = cum[bins];
            const int64_t r = a.q ? quantile_rank(a.q[tid], total, a.method) : quantile_rank_given(a.ranks[b * R + tid], total);
            s_res[tid] = r;
            if (r < 0) s_slot[tid] = -1;
            a.out_ranks[b * R + tid] = r;
            if (tid == 0) a.count[b] = total;
        }
        if (tid < R && s_slot[tid] == s) {
            const int d = radix_find_bin(cum, bins, s_res[tid]);
            if (d >= 0) {
                s_newpre[tid] = radix_extend(s_oldpre[s], level, (uint32_t)d);
                s_newres[tid] = s_res[tid] - cum[d];
            }
        }
        __syncthreads();                                                              // cum is rewritten by the next slot
    }
    // the next level's slots: the distinct prefixes of the ranks with an answer, ascending
    if (tid < kMaxRanks) {
        int first = tid < R && s_newres[tid] >= 0;
        for (int k = 0; k < tid; ++k)
            if (s_newres[k] >= 0 && s_newpre[k] == s_newpre[tid]) first = 0;
        s_first[tid] = first;
    }
    __syncthreads();
    if (tid < R) {
        const bool valid = s_newres[tid] >= 0;
        const uint32_t p = valid ? s_newpre[tid] : 0u;
        int slot = 0, n = 0;
        for (int k = 0; k < R; ++k) {
            n += s_first[k];
            slot += s_first[k] && s_newpre[k] < p;
        }
        a.rank_res[b * R + tid] = s_newres[tid];
        a.rank_slot[b * R + tid] = valid ? slot : -1;
        a.rank_prefix[b * R + tid] = p;
        if (level == VS_VALUE_RADIX_LEVELS - 1) a.out_values[b * R + tid] = value_unkey(p, a.dtype);      // p = 0: the sentinel
        if (s_first[tid]) a.slot_prefix[b * R + slot] = p;                            // slot < n
        if (tid >= n) a.slot_prefix[b * R + tid] = kRadixNoSlot;
        if (tid == 0) a.n_slots[b] = n;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
size_t level_counts(int32_t B, int32_t R, int level) { return (size_t)B * (size_t)(level == 0 ? 1 : R) * (size_t)radix_bins(level); }

template <int QT, bool TOP>
int radix_launch_qt(const RadixArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    VS_HIP(hipFuncSetAttribute((const void*)value_radix_kernel<QT, TOP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((value_radix_kernel<QT, TOP>), grid, dim3(kValThreads), lds, s, a);
    return VS_OK;
}

template <bool TOP>
int radix_launch_top(const RadixArgs& a, int32_t qt, dim3 grid, size_t lds, hipStream_t s) {
    return launch_by_qt(qt, [&](auto t) { return radix_launch_qt<decltype(t)::value, TOP>(a, grid, lds, s); });
}

// zero a level's counts (and missing at level 0) and count; everything on the device
int radix_counts_launch(const RadixArgs& a, const ValuePlan& plan, hipStream_t s) {
    const int32_t B = a.s.set.B;
    VS_HIP(hipMemsetAsync(a.counts, 0, level_counts(B, a.R, a.level) * 8, s));
    if (a.level == 0) VS_HIP(hipMemsetAsync(a.missing, 0, (size_t)B * 8, s));
    ProfScope prof("value_radix_counts", s);
    const dim3 grid((unsigned)plan.chunks, (unsigned)ceil_div64(B, plan.qt));
    const size_t lds = quantile_lds_bytes(plan.qt, a.R, a.level);                     // 128 KiB at most
    return a.level == 0 ? radix_launch_top<true>(a, plan.qt, grid, lds, s) : radix_launch_top<false>(a, plan.qt, grid, lds, s);
}

int radix_step_launch(const StepArgs& a, hipStream_t s) {
    ProfScope prof("value_radix_step", s);
    hipLaunchKernelGGL(value_radix_step_kernel, dim3((unsigned)a.B), dim3(kStepThreads), 0, s, a);
    return VS_OK;
}

// the set, R and the scratch of a call -> the plan
int check_quant_set(const SetSrc& src, const void* values, int dtype, int32_t R, int64_t rows_per_chunk, bool have_outputs, ValuePlan* plan) {
    char msg[256];
    VS_TRY(plan_or_fail(quantile_check_ranks(R, msg, sizeof msg), msg));
    VS_TRY(plan_or_fail(value_check_set(values && have_outputs, src.words != nullptr, src.bit0, src.ld_words, src.B, dtype, src.n_rows, 0,
                                        rows_per_chunk, quantile_qt(R, true), plan, msg, sizeof msg), msg));
    return plan_or_fail(quantile_check_scratch(src.B, R, msg, sizeof msg), msg);
}

// q with its method, or ranks: host arrays are looked at before the device is
int check_ranks_arg(const double* q, int method, const int64_t* ranks, int32_t B, int32_t R) {
    char msg[256];
    if (q) {
        VS_TRY(plan_or_fail(quantile_check_method(method, msg, sizeof msg), msg));
        if (!is_device_ptr(q)) VS_TRY(plan_or_fail(quantile_check_q_host(q, R, msg, sizeof msg), msg));
        return VS_OK;
    }
    if (!ranks) return fail(VS_EINVAL, "NULL argument: q [R] or ranks [B, R] must be given");
    if (!is_device_ptr(ranks)) VS_TRY(plan_or_fail(quantile_check_ranks_host(ranks, (int64_t)B * R, msg, sizeof msg), msg));
    return VS_OK;
}

int check_counts_arg(int level, const uint32_t* slot_prefix, const int32_t* n_slots, const int64_t* missing) {
    char msg[256];
    VS_TRY(plan_or_fail(quantile_check_level(level, msg, sizeof msg), msg));
    if (level == 0 ? !missing : (!slot_prefix || !n_slots)) return fail(VS_EINVAL, "NULL argument: level %d needs %s", level,
                                                                        level == 0 ? "missing" : "slot_prefix and n_slots");
    return VS_OK;
}

// vs_value_radix_counts and vs_index_value_radix_counts: one level's counts on the set's device
int radix_counts(const SetSrc& src, const void* values, int dtype, int level, int32_t R, const uint32_t* slot_prefix, const int32_t* n_slots,
                 int64_t rows_per_chunk, int64_t* counts, int64_t* missing, void* stream) {
    ValuePlan plan;
    VS_TRY(check_quant_set(src, values, dtype, R, rows_per_chunk, counts != nullptr, &plan));
    VS_TRY(check_counts_arg(level, slot_prefix, n_slots, missing));
    VS_TRY(src.device_ok());
    if (level != 0) missing = nullptr;
    else slot_prefix = nullptr, n_slots = nullptr;
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"values", values}, {"slot_prefix", slot_prefix},
                                       {"n_slots", n_slots}, {"counts", counts}, {"missing", missing}}));
    const int32_t B = src.B;
    SetStage st;
    Staged st_p, st_n, st_c, st_m;
    return c.run("value_radix_counts", Finish::kStream, [&] {
        RadixArgs a{};
        VS_TRY(st.in(src, values, dtype, plan.rows_per_chunk, c.dev, c.s, &a.s));
        uint32_t* d_p;
        int32_t* d_n;
        int64_t *d_c, *d_m;
        VS_TRY(st_p.in(slot_prefix, (size_t)B * R, c.dev, true, c.s, &d_p));
        VS_TRY(st_n.in(n_slots, (size_t)B, c.dev, true, c.s, &d_n));
        VS_TRY(st_c.in(counts, level_counts(B, R, level), c.dev, false, c.s, &d_c));
        VS_TRY(st_m.in(missing, (size_t)B, c.dev, false, c.s, &d_m));
        a.level = level;
        a.R = R;
        a.slot_prefix = d_p;
        a.n_slots = d_n;
        a.counts = reinterpret_cast<unsigned long long*>(d_c);
        a.missing = reinterpret_cast<unsigned long long*>(d_m);
        return radix_counts_launch(a, plan, c.s);
    }, [&] {
        VS_TRY(st_c.back(c.s));
        return st_m.back(c.s);
    });
}

// vs_value_quantiles and vs_index_value_quantiles: every level's counts and steps on the set's device
int value_quantiles(const SetSrc& src, const void* values, int dtype, const double* q, int method, const int64_t* ranks, int32_t R,
                    int64_t rows_per_chunk, void* out_values, int64_t* out_ranks, int64_t* count, int64_t* missing, void* stream) {
    ValuePlan plan;
    VS_TRY(check_quant_set(src, values, dtype, R, rows_per_chunk, out_values && out_ranks && count && missing, &plan));
    VS_TRY(check_ranks_arg(q, method, ranks, src.B, R));
    VS_TRY(src.device_ok());
    if (q) ranks = nullptr;
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"values", values}, {"q", q}, {"ranks", ranks},
                                       {"out_values", out_values}, {"out_ranks", out_ranks}, {"count", count}, {"missing", missing}}));
    const int32_t B = src.B;
    SetStage st;
    Staged st_q, st_r, st_v, st_o, st_c, st_m;
    DevBuf scratch;                                               // the counts of a level, then the step's state
    return c.run("value_quantiles", Finish::kSync, [&] {
        RadixArgs ca{};
        StepArgs sa{};
        VS_TRY(st.in(src, values, dtype, plan.rows_per_chunk, c.dev, c.s, &ca.s));
        double* d_q;
        int64_t *d_r, *d_m;
        VS_TRY(st_q.in(q, (size_t)R, c.dev, true, c.s, &d_q));
        VS_TRY(st_r.in(ranks, (size_t)B * R, c.dev, true, c.s, &d_r));
        VS_TRY(st_v.in(static_cast<uint32_t*>(out_values), (size_t)B * R, c.dev, false, c.s, &sa.out_values));
        VS_TRY(st_o.in(out_ranks, (size_t)B * R, c.dev, false, c.s, &sa.out_ranks));
        VS_TRY(st_c.in(count, (size_t)B, c.dev, false, c.s, &sa.count));
        VS_TRY(st_m.in(missing, (size_t)B, c.dev, false, c.s, &d_m));
        const size_t n_cnt = (size_t)B * (size_t)R * VS_VALUE_RADIX_BINS, n_br = (size_t)B * (size_t)R;
        VS_TRY(scratch.alloc(n_cnt * 8 + n_br * 8 + 3 * n_br * 4 + (size_t)B * 4));
        unsigned long long* d_counts = scratch.as<unsigned long long>();
        sa.rank_res = reinterpret_cast<int64_t*>(d_counts + n_cnt);
        sa.rank_slot = reinterpret_cast<int32_t*>(sa.rank_res + n_br);
        sa.rank_prefix = reinterpret_cast<uint32_t*>(sa.rank_slot + n_br);
        sa.slot_prefix = sa.rank_prefix + n_br;
        sa.n_slots = reinterpret_cast<int32_t*>(sa.slot_prefix + n_br);
        sa.method = method;
        sa.dtype = dtype;
        sa.B = B;
        sa.R = R;
        sa.counts = reinterpret_cast<const int64_t*>(d_counts);
        sa.q = d_q;
        sa.ranks = d_r;
        ca.R = R;
        ca.slot_prefix = sa.slot_prefix;
        ca.n_slots = sa.n_slots;
        ca.counts = d_counts;
        ca.missing = reinterpret_cast<unsigned long long*>(d_m);
        for (int level = 0; level < VS_VALUE_RADIX_LEVELS; ++level) {
            ca.level = sa.level = level;
            VS_TRY(radix_counts_launch(ca, plan, c.s));
            VS_TRY(radix_step_launch(sa, c.s));
        }
        return VS_OK;
    }, [&] {
        VS_TRY(st_v.back(c.s));
        VS_TRY(st_o.back(c.s));
        VS_TRY(st_c.back(c.s));
        return st_m.back(c.s);
    });
}

}  // namespace

extern "C" int vs_value_quantile_plan(int64_t n_rows, int32_t B, int32_t R, int per_query, int64_t rows_per_chunk, int32_t* out_qt,
                                      int64_t* out_chunks, int64_t* out_rows_per_chunk) {
    if (!out_qt || !out_chunks || !out_rows_per_chunk) return fail(VS_EINVAL, "NULL argument");
    ValuePlan p;
    char msg[256];
    VS_TRY(plan_or_fail(quantile_plan(n_rows, B, R, per_query != 0, rows_per_chunk, &p, msg, sizeof msg), msg));
    *out_qt = p.qt;
    *out_chunks = p.chunks;
    *out_rows_per_chunk = p.rows_per_chunk;
    return VS_OK;
}

extern "C" int vs_value_quantiles(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const void* values,
                                  int dtype, int64_t n_rows, const double* q, int method, const int64_t* ranks, int32_t R, int64_t rows_per_chunk,
                                  void* out_values, int64_t* out_ranks, int64_t* count, int64_t* missing, int device, void* stream) {
    return value_quantiles(free_set(words, bit0, ld_words, and_words, B, n_rows, device), values, dtype, q, method, ranks, R, rows_per_chunk, out_values,
                           out_ranks, count, missing, stream);
}

extern "C" int vs_index_value_quantiles(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const void* values,
                                        int dtype, const double* q, int method, const int64_t* ranks, int32_t R, int64_t rows_per_chunk,
                                        void* out_values, int64_t* out_ranks, int64_t* count, int64_t* missing, void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return value_quantiles(src, values, dtype, q, method, ranks, R, rows_per_chunk, out_values, out_ranks, count, missing, stream);
}

extern "C" int vs_value_radix_counts(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B, const void* values,
                                     int dtype, int64_t n_rows, int level, int32_t R, const uint32_t* slot_prefix, const int32_t* n_slots,
                                     int64_t rows_per_chunk, int64_t* counts, int64_t* missing, int device, void* stream) {
    return radix_counts(free_set(words, bit0, ld_words, and_words, B, n_rows, device), values, dtype, level, R, slot_prefix, n_slots, rows_per_chunk,
                        counts, missing, stream);
}

extern "C" int vs_index_value_radix_counts(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const void* values,
                                           int dtype, int level, int32_t R, const uint32_t* slot_prefix, const int32_t* n_slots,
                                           int64_t rows_per_chunk, int64_t* counts, int64_t* missing, void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return radix_counts(src, values, dtype, level, R, slot_prefix, n_slots, rows_per_chunk, counts, missing, stream);
}

extern "C" int vs_value_radix_step(int level, const int64_t* counts, int32_t B, int32_t R, const double* q, int method, const int64_t* ranks,
                                   int64_t* rank_res, int32_t* rank_slot, uint32_t* rank_prefix, uint32_t* slot_prefix, int32_t* n_slots,
                                   int64_t* count, int64_t* out_ranks, void* out_values, int dtype, int device, void* stream) {
    char msg[256];
    VS_TRY(plan_or_fail(quantile_check_level(level, msg, sizeof msg), msg));
    VS_TRY(plan_or_fail(quantile_check_ranks(R, msg, sizeof msg), msg));
    VS_TRY(plan_or_fail(value_check_dtype(dtype, msg, sizeof msg), msg));
    if (B < 1) return fail(VS_EINVAL, "B must be positive (got %d)", B);
    VS_TRY(plan_or_fail(quantile_check_scratch(B, R, msg, sizeof msg), msg));
    if (!counts || !rank_res || !rank_slot || !rank_prefix || !slot_prefix || !n_slots) return fail(VS_EINVAL, "NULL argument");
    if (level == 0) {
        if (!count || !out_ranks || (!q && !ranks)) return fail(VS_EINVAL, "NULL argument: level 0 needs count, out_ranks and q or ranks");
        if (q) VS_TRY(plan_or_fail(quantile_check_method(method, msg, sizeof msg), msg));
    }
    if (level == VS_VALUE_RADIX_LEVELS - 1 && !out_values) return fail(VS_EINVAL, "NULL argument: the last level needs out_values");
    VS_TRY(device_in_range(device));
    if (q || level != 0) ranks = nullptr;
    if (level != 0) q = nullptr, count = nullptr, out_ranks = nullptr;
    if (level != VS_VALUE_RADIX_LEVELS - 1) out_values = nullptr;
    const void* ptrs[11] = {counts, q, ranks, rank_res, rank_slot, rank_prefix, slot_prefix, n_slots, count, out_ranks, out_values};
    const char* names[11] = {"counts", "q", "ranks", "rank_res", "rank_slot", "rank_prefix", "slot_prefix", "n_slots", "count", "out_ranks", "out_values"};
    bool dev = false;
    VS_TRY(pointers_kind(ptrs, names, 11, device, &dev));
    if (!dev) return fail(VS_EINVAL, "vs_value_radix_step works on device buffers (the counts of vs_value_radix_counts, summed over the shards)");
    VS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    StepArgs a{};
    a.level = level;
    a.method = method;
    a.dtype = dtype;
    a.B = B;
    a.R = R;
    a.counts = counts;
    a.q = q;
    a.ranks = ranks;
    a.rank_res = rank_res;
    a.rank_slot = rank_slot;
    a.rank_prefix = rank_prefix;
    a.slot_prefix = slot_prefix;
    a.n_slots = n_slots;
    a.count = count;
    a.out_ranks = out_ranks;
    a.out_values = static_cast<uint32_t*>(out_values);
    VS_TRY(radix_step_launch(a, s));
    return close_call("value_radix_step", true, stream, s, Finish::kStream, [] { return VS_OK; });
}
