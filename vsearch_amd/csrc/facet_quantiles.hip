// facet_quantiles.hip -- per-label percentiles (vs_facet_value_quantile_plan, vs_facet_value_quantiles, vs_facet_value_radix_counts and the
// vs_index_* variants): exact order statistics of a numeric field per facet label over any document set, in one pass a radix level (DESIGN.md
// 3.1t).  No reference counterpart.  The radix select of quantiles.hip with a (query, label) cell where that has a query: the keys, the digits,
// the slots and the step (vs_value_radix_step over B x n_labels cells, unchanged) are its; only the counting kernel is new.
//
// Counting (facet_radix_kernel): a workgroup owns a chunk of rows and a tile of QT queries and walks the bitmaps with walk_tile (set_walk.h).
// A lane whose row is in SOME query's set loads its label once for the tile.  All integer.
//   LDS regime     the workgroup also owns a tile of tile_labels labels (the grid's z dimension); one unsigned compare label - tile0 <
//                  tile_labels picks the tile's rows (and drops -1 and anything out of range), only those load their value.  LDS: one uint32
//                  histogram of `bins` per (query, label, slot), the cells' slot prefixes (padded to 16) next to them.  Only the slots in use
//                  are zeroed and flushed (64-bit atomics on the non-zero bins).  total and other are counted by the first label tile alone;
//                  a label's missing rows by the tile that owns the label (the only one that loads their values).
//   global regime  64-bit atomics straight into counts; a cell's slot prefixes are read from global memory (R words at most a row).
// Both keep the rule of value_radix_kernel: when every counted row of a 64-row step falls into one (label, slot, bin), one lane adds the popcount.
#include "agg_call.h"
#include "facet_quantile_check.h"

using namespace vs;

namespace {

constexpr int kMaxRanks = VS_VALUE_MAX_RANKS;
// Threads of a counting workgroup.  Its LDS (up to 128 KiB) leaves one workgroup a CU, and a wave of the walk has one label load in flight a
// 64-row step: 16 waves instead of the 4 of the percentiles hide that latency (measured: DESIGN.md 3.1t).
constexpr int kFqThreads = 1024;
constexpr int kFqWaves = kFqThreads / 64;

struct FqArgs {
    SetArgs s;
    const int32_t* labels;            // [n_rows]
    int32_t n_labels, tile_labels;
    int level;
    int32_t R;
    const uint32_t* slot_prefix;      // [B, n_labels, R] (levels 1, 2)
    const int32_t* n_slots;           // [B, n_labels]    (levels 1, 2)
    unsigned long long* counts;       // [B, n_labels, S, bins], zeroed by the caller
    unsigned long long* missing;      // [B, n_labels], zeroed by the caller (level 0)
    unsigned long long *total, *other;             // [B], zeroed by the caller (level 0)
};

template <int QT, bool TOP, bool GLOBAL>
__global__ __launch_bounds__(kFqThreads) void facet_radix_kernel(FqArgs a) {
    extern __shared__ uint32_t fq_lds[];                         // the histograms [cell][S][bins], cell = q x tile_labels + label - tile0
    __shared__ uint32_t s_pre[GLOBAL ? 1 : kFqMaxCells * kMaxRanks];      // a cell's slot prefixes, ascending, kRadixNoSlot behind the last
    __shared__ uint32_t s_mis[GLOBAL ? 1 : kFqMaxCells];
    __shared__ int s_ns[GLOBAL ? 1 : kFqMaxCells];               // slots in use
    __shared__ uint32_t s_tot[QT], s_oth[QT];
    __shared__ int s_any;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q0 = (int)blockIdx.y * QT;
    const int nq = min(QT, a.s.set.B - q0);
    const int64_t r0 = (int64_t)blockIdx.x * a.s.set.rows_per_chunk;
    const int64_t r1 = min(a.s.set.n_rows, r0 + a.s.set.rows_per_chunk);
    const int level = TOP ? 0 : a.level;
    const uint32_t bins = (uint32_t)radix_bins(level);
    const int R = a.R;
    const uint32_t S = TOP ? 1u : (uint32_t)R;
    const uint32_t L = (uint32_t)a.n_labels;
    const uint32_t t0 = GLOBAL ? 0u : blockIdx.z * (uint32_t)a.tile_labels;            // the tile's first label
    const uint32_t tl = GLOBAL ? L : min((uint32_t)a.tile_labels, L - t0);             // its labels
    const uint32_t cstride = S * bins;                                                 // uint32 words of a cell's histograms
    const bool first_tile = GLOBAL || blockIdx.z == 0;
    const int ncell = GLOBAL ? 0 : nq * (int)tl;                                       // <= kFqMaxCells: the plan's rule
    if (tid < QT) s_tot[tid] = s_oth[tid] = 0u;
    if (tid == 0) s_any = TOP ? 1 : 0;
    if constexpr (!GLOBAL) {
        __syncthreads();
        if (tid < ncell) {
            const size_t g = (size_t)(q0 + tid / (int)tl) * L + t0 + (uint32_t)(tid % (int)tl);
            const int ns = TOP ? 1 : min(max(a.n_slots[g], 0), R);
            s_mis[tid] = 0u;
            s_ns[tid] = ns;
            if (!TOP && ns) s_any = 1;
        }
        if (!TOP) {
            for (int i = tid; i < ncell * kMaxRanks; i += kFqThreads) {
                const int c = i / kMaxRanks, j = i % kMaxRanks;
                const size_t g = (size_t)(q0 + c / (int)tl) * L + t0 + (uint32_t)(c % (int)tl);
                uint32_t p = kRadixNoSlot;
                if (j < min(max(a.n_slots[g], 0), R)) p = a.slot_prefix[g * (size_t)R + j];
                s_pre[i] = p;
            }
        }
        __syncthreads();
        if (!s_any) return;                                      // (uniform) no rank of the tile resolved: nothing to count
        for (int c = 0; c < ncell; ++c)
            for (uint32_t i = tid; i < (uint32_t)s_ns[c] * bins; i += kFqThreads) fq_lds[(size_t)c * cstride + i] = 0u;
    }
    __syncthreads();
    uint32_t tot[QT], oth[QT];                                   // wave-uniform: a chunk holds fewer than 2^32 rows
#pragma unroll
    for (int q = 0; q < QT; ++q) tot[q] = oth[q] = 0u;
    const int shift = radix_shift(level);
    walk_tile<QT, kFqWaves>(a.s.set, q0, nq, r0, r1, w, lane, [&](int64_t row0, uint64_t many, const Span* sp, int s, int sh, uint64_t live) {
        int32_t label = -1;
        if ((many >> lane) & 1ull) label = a.labels[row0 + lane];                      // once for the tile
        const uint32_t rel = (uint32_t)label - t0;
        const bool in_tile = rel < tl;                                                 // -1, out of range, another tile's: not ours
        const uint32_t key = in_tile ? value_key(a.s.values[row0 + lane], a.s.dtype) : 0u;       // a lane outside the tile never loads its value
        const uint32_t dig = (key >> shift) & (bins - 1u);
        const uint32_t pre = TOP ? 0u : radix_prefix(key, level);
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            if (q >= nq) continue;
            const uint64_t m = window64(sp[q], s, sh) & live;
            if (m == 0ull) continue;
            const bool in = (m >> lane) & 1ull;
            if (TOP && first_tile) {
                tot[q] += (uint32_t)__popcll(m);
                oth[q] += (uint32_t)(__popcll(m) - __popcll(__builtin_amdgcn_ballot_w64(in && (uint32_t)label < L)));
            }
            const bool ok = in && in_tile;
            bool has = ok && key != 0u;
            uint32_t idx = 0u;                                                         // the bin among the workgroup's (LDS) / the call's (global): < 2^27
            if constexpr (GLOBAL) {
                const size_t g = (size_t)(q0 + q) * L + rel;
                if (TOP) {
                    if (ok && !has) atomicAdd(a.missing + g, 1ull);
                    idx = (uint32_t)g * bins + dig;
                } else if (has) {
                    const int ns = min(max(a.n_slots[g], 0), R);
                    const uint32_t* gp = a.slot_prefix + g * (size_t)R;
                    int slot = -1;
                    for (int j = 0; j < ns; ++j) slot = gp[j] == pre ? j : slot;
                    has = slot >= 0;
                    idx = ((uint32_t)g * S + (uint32_t)max(slot, 0)) * bins + dig;
                }
            } else {
                const uint32_t c = ok ? (uint32_t)q * tl + rel : 0u;
                if (TOP) {
                    if (ok && !has) atomicAdd(&s_mis[c], 1u);
                    idx = c * bins + dig;
                } else {
                    const int slot = radix_find_slot(s_pre + c * kMaxRanks, pre);
                    has = has && slot >= 0;
                    idx = (c * S + (uint32_t)max(slot, 0)) * bins + dig;
                }
            }
            const uint64_t mh = __builtin_amdgcn_ballot_w64(has);
            if (mh == 0ull) continue;                                                  // no row of a slot: no atomic
            const int first = __builtin_ctzll(mh);
            const uint32_t i0 = (uint32_t)__builtin_amdgcn_readlane((int)idx, first);
            const bool one = __builtin_amdgcn_ballot_w64(has && idx == i0) == mh;      // every counted row of the step in one bin: add once
            if constexpr (GLOBAL) {
                if (one) {
                    if (lane == first) atomicAdd(a.counts + i0, (unsigned long long)__popcll(mh));
                } else if (has) {
                    atomicAdd(a.counts + idx, 1ull);
                }
            } else {
                if (one) {
                    if (lane == first) atomicAdd(fq_lds + i0, (uint32_t)__popcll(mh));
                } else if (has) {
                    atomicAdd(fq_lds + idx, 1u);
                }
            }
        }
    });
    if (TOP && first_tile && lane == 0) {
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            if (tot[q]) atomicAdd(&s_tot[q], tot[q]);
            if (oth[q]) atomicAdd(&s_oth[q], oth[q]);
        }
    }
    __syncthreads();
    if (TOP && first_tile && tid < nq) {
        if (s_tot[tid]) atomicAdd(&a.total[q0 + tid], (unsigned long long)s_tot[tid]);
        if (s_oth[tid]) atomicAdd(&a.other[q0 + tid], (unsigned long long)s_oth[tid]);
    }
    if constexpr (!GLOBAL) {
        for (int c = 0; c < ncell; ++c) {
            const size_t g = (size_t)(q0 + c / (int)tl) * L + t0 + (uint32_t)(c % (int)tl);
            unsigned long long* dst = a.counts + g * (size_t)cstride;
            for (uint32_t i = tid; i < (uint32_t)s_ns[c] * bins; i += kFqThreads) {
                const uint32_t v = fq_lds[(size_t)c * cstride + i];
                if (v) atomicAdd(dst + i, (unsigned long long)v);
            }
            if (TOP && tid == 0 && s_mis[c]) atomicAdd(a.missing + g, (unsigned long long)s_mis[c]);
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
size_t level_counts(int32_t B, int32_t L, int32_t R, int level) {
    return (size_t)B * (size_t)L * (size_t)(level == 0 ? 1 : R) * (size_t)radix_bins(level);
}

template <int QT, bool TOP>
int fq_launch_qt(const FqArgs& a, const FacetQuantilePlan& p, dim3 grid, size_t lds, hipStream_t s) {
    if (p.regime) {                                               // (the global regime only has the tiles 8 and 1)
        if constexpr (QT == 8 || QT == 1) hipLaunchKernelGGL((facet_radix_kernel<QT, TOP, true>), grid, dim3(kFqThreads), 0, s, a);
        else return fail(VS_EINVAL, "no global-regime kernel for a tile of %d queries", QT);
    } else {
        VS_HIP(hipFuncSetAttribute((const void*)facet_radix_kernel<QT, TOP, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((facet_radix_kernel<QT, TOP, false>), grid, dim3(kFqThreads), lds, s, a);
    }
    return VS_OK;
}

template <bool TOP>
int fq_launch_top(const FqArgs& a, const FacetQuantilePlan& p, dim3 grid, size_t lds, hipStream_t s) {
    return launch_by_qt(p.qt, [&](auto t) { return fq_launch_qt<decltype(t)::value, TOP>(a, p, grid, lds, s); });
}

// zero a level's counts (and missing, total, other at level 0) and count; everything on the device
int fq_counts_launch(FqArgs a, const FacetQuantilePlan& plan, hipStream_t s) {
    const int32_t B = a.s.set.B;
    VS_HIP(hipMemsetAsync(a.counts, 0, level_counts(B, a.n_labels, a.R, a.level) * 8, s));
    if (a.level == 0) {
        VS_HIP(hipMemsetAsync(a.missing, 0, (size_t)B * (size_t)a.n_labels * 8, s));
        VS_HIP(hipMemsetAsync(a.total, 0, (size_t)B * 8, s));
        VS_HIP(hipMemsetAsync(a.other, 0, (size_t)B * 8, s));
    }
    ProfScope prof("facet_value_radix_counts", s);
    a.s.set.rows_per_chunk = plan.rows_per_chunk;
    a.tile_labels = plan.tile_labels;
    const dim3 grid((unsigned)plan.chunks, (unsigned)ceil_div64(B, plan.qt), (unsigned)plan.label_tiles);
    const size_t lds = facet_quantile_lds_bytes(plan, a.R, a.level);                  // 128 KiB at most
    return a.level == 0 ? fq_launch_top<true>(a, plan, grid, lds, s) : fq_launch_top<false>(a, plan, grid, lds, s);
}

// the set, the labels, R and the scratch of a call -> the plan of `level`
int check_fq_set(const SetSrc& src, const int32_t* labels, int32_t n_labels, const void* values, int dtype, int32_t R, int level,
                 int64_t rows_per_chunk, bool have_outputs, FacetQuantilePlan* plan) {
    char msg[256];
    return plan_or_fail(facet_quantile_check_set(labels && values && have_outputs, src.words != nullptr, src.bit0, src.ld_words, src.B, dtype, src.n_rows,
                                                 n_labels, R, level, rows_per_chunk, plan, msg, sizeof msg), msg);
}

// q with its method, or ranks [B, n_labels, R]: host arrays are looked at before the device is
int check_ranks_arg(const double* q, int method, const int64_t* ranks, int64_t cells, int32_t R) {
    char msg[256];
    if (q) {
        VS_TRY(plan_or_fail(quantile_check_method(method, msg, sizeof msg), msg));
        if (!is_device_ptr(q)) VS_TRY(plan_or_fail(quantile_check_q_host(q, R, msg, sizeof msg), msg));
        return VS_OK;
    }
    if (!ranks) return fail(VS_EINVAL, "NULL argument: q [R] or ranks [B, n_labels, R] must be given");
    if (!is_device_ptr(ranks)) VS_TRY(plan_or_fail(quantile_check_ranks_host(ranks, cells * R, msg, sizeof msg), msg));
    return VS_OK;
}

// vs_facet_value_radix_counts and vs_index_facet_value_radix_counts: one level's counts on the set's device
int facet_radix_counts(const SetSrc& src, const int32_t* labels, int32_t n_labels, const void* values, int dtype, int level, int32_t R,
                       const uint32_t* slot_prefix, const int32_t* n_slots, int64_t rows_per_chunk, int64_t* counts, int64_t* missing, int64_t* total,
                       int64_t* other, void* stream) {
    FacetQuantilePlan plan;
    char msg[256];
    VS_TRY(check_fq_set(src, labels, n_labels, values, dtype, R, level, rows_per_chunk, counts != nullptr, &plan));
    VS_TRY(plan_or_fail(facet_quantile_check_level_args(level, slot_prefix && n_slots, missing && total && other, msg, sizeof msg), msg));
    VS_TRY(src.device_ok());
    if (level != 0) missing = total = other = nullptr;
    else slot_prefix = nullptr, n_slots = nullptr;
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"labels", labels}, {"values", values},
                                       {"slot_prefix", slot_prefix}, {"n_slots", n_slots}, {"counts", counts}, {"missing", missing}, {"total", total},
                                       {"other", other}}));
    const int32_t B = src.B;
    SetStage st;
    Staged st_l, st_p, st_n, st_c, st_m, st_t, st_o;
    return c.run("facet_value_radix_counts", Finish::kStream, [&] {
        FqArgs a{};
        const size_t cells = (size_t)B * (size_t)n_labels;
        VS_TRY(st.in(src, values, dtype, plan.rows_per_chunk, c.dev, c.s, &a.s));
        int32_t *d_l, *d_n;
        uint32_t* d_p;
        int64_t *d_c, *d_m, *d_t, *d_o;
        VS_TRY(st_l.in(labels, (size_t)src.n_rows, c.dev, true, c.s, &d_l));
        VS_TRY(st_p.in(slot_prefix, cells * R, c.dev, true, c.s, &d_p));
        VS_TRY(st_n.in(n_slots, cells, c.dev, true, c.s, &d_n));
        VS_TRY(st_c.in(counts, level_counts(B, n_labels, R, level), c.dev, false, c.s, &d_c));
        VS_TRY(st_m.in(missing, cells, c.dev, false, c.s, &d_m));
        VS_TRY(st_t.in(total, (size_t)B, c.dev, false, c.s, &d_t));
        VS_TRY(st_o.in(other, (size_t)B, c.dev, false, c.s, &d_o));
        a.labels = d_l;
        a.n_labels = n_labels;
        a.level = level;
        a.R = R;
        a.slot_prefix = d_p;
        a.n_slots = d_n;
        a.counts = reinterpret_cast<unsigned long long*>(d_c);
        a.missing = reinterpret_cast<unsigned long long*>(d_m);
        a.total = reinterpret_cast<unsigned long long*>(d_t);
        a.other = reinterpret_cast<unsigned long long*>(d_o);
        return fq_counts_launch(a, plan, c.s);
    }, [&] {
        VS_TRY(st_c.back(c.s));
        VS_TRY(st_m.back(c.s));
        VS_TRY(st_t.back(c.s));
        return st_o.back(c.s);
    });
}

// vs_facet_value_quantiles and vs_index_facet_value_quantiles: every level's counts and steps on the set's device
int facet_value_quantiles(const SetSrc& src, const int32_t* labels, int32_t n_labels, const void* values, int dtype, const double* q, int method,
                          const int64_t* ranks, int32_t R, int64_t rows_per_chunk, void* out_values, int64_t* out_ranks, int64_t* count,
                          int64_t* missing, int64_t* total, int64_t* other, void* stream) {
    FacetQuantilePlan plans[VS_VALUE_RADIX_LEVELS];
    for (int level = 0; level < VS_VALUE_RADIX_LEVELS; ++level)
        VS_TRY(check_fq_set(src, labels, n_labels, values, dtype, R, level, rows_per_chunk, out_values && out_ranks && count && missing && total && other,
                            plans + level));
    VS_TRY(check_ranks_arg(q, method, ranks, (int64_t)src.B * n_labels, R));
    VS_TRY(src.device_ok());
    if (q) ranks = nullptr;
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"labels", labels}, {"values", values}, {"q", q},
                                       {"ranks", ranks}, {"out_values", out_values}, {"out_ranks", out_ranks}, {"count", count}, {"missing", missing},
                                       {"total", total}, {"other", other}}));
    SetStage st;
    Staged st_l, st_q, st_r, st_v, st_o, st_c, st_m, st_t, st_x;
    DevBuf scratch;                                               // the counts of a level, then the step's state
    return c.run("facet_value_quantiles", Finish::kSync, [&] {
        FqArgs ca{};
        const size_t cells = (size_t)src.B * (size_t)n_labels, n_br = cells * (size_t)R, n_cnt = n_br * VS_VALUE_RADIX_BINS;
        VS_TRY(st.in(src, values, dtype, plans[0].rows_per_chunk, c.dev, c.s, &ca.s));
        int32_t* d_l;
        double* d_q;
        uint32_t* d_v;
        int64_t *d_r, *d_or, *d_c, *d_m, *d_t, *d_x;
        VS_TRY(st_l.in(labels, (size_t)src.n_rows, c.dev, true, c.s, &d_l));
        VS_TRY(st_q.in(q, (size_t)R, c.dev, true, c.s, &d_q));
        VS_TRY(st_r.in(ranks, n_br, c.dev, true, c.s, &d_r));
        VS_TRY(st_v.in(static_cast<uint32_t*>(out_values), n_br, c.dev, false, c.s, &d_v));
        VS_TRY(st_o.in(out_ranks, n_br, c.dev, false, c.s, &d_or));
        VS_TRY(st_c.in(count, cells, c.dev, false, c.s, &d_c));
        VS_TRY(st_m.in(missing, cells, c.dev, false, c.s, &d_m));
        VS_TRY(st_t.in(total, (size_t)src.B, c.dev, false, c.s, &d_t));
        VS_TRY(st_x.in(other, (size_t)src.B, c.dev, false, c.s, &d_x));
        VS_TRY(scratch.alloc(n_cnt * 8 + n_br * 8 + 3 * n_br * 4 + cells * 4));
        unsigned long long* d_counts = scratch.as<unsigned long long>();
        int64_t* rank_res = reinterpret_cast<int64_t*>(d_counts + n_cnt);
        int32_t* rank_slot = reinterpret_cast<int32_t*>(rank_res + n_br);
        uint32_t* rank_prefix = reinterpret_cast<uint32_t*>(rank_slot + n_br);
        uint32_t* slot_prefix = rank_prefix + n_br;
        int32_t* n_slots = reinterpret_cast<int32_t*>(slot_prefix + n_br);
        ca.labels = d_l;
        ca.n_labels = n_labels;
        ca.R = R;
        ca.slot_prefix = slot_prefix;
        ca.n_slots = n_slots;
        ca.counts = d_counts;
        ca.missing = reinterpret_cast<unsigned long long*>(d_m);
        ca.total = reinterpret_cast<unsigned long long*>(d_t);
        ca.other = reinterpret_cast<unsigned long long*>(d_x);
        for (int level = 0; level < VS_VALUE_RADIX_LEVELS; ++level) {
            ca.level = level;
            VS_TRY(fq_counts_launch(ca, plans[level], c.s));
            VS_TRY(launch_failed("facet_value_radix_counts", c.s));
            // the step of the percentiles, a (query, label) cell as one of its queries (on the null stream it synchronises, which costs nothing here)
            VS_TRY(vs_value_radix_step(level, reinterpret_cast<const int64_t*>(d_counts), (int32_t)cells, R, d_q, method, d_r, rank_res, rank_slot,
                                       rank_prefix, slot_prefix, n_slots, d_c, d_or, d_v, dtype, src.device, stream));
        }
        return VS_OK;
    }, [&] {
        VS_TRY(st_v.back(c.s));
        VS_TRY(st_o.back(c.s));
        VS_TRY(st_c.back(c.s));
        VS_TRY(st_m.back(c.s));
        VS_TRY(st_t.back(c.s));
        return st_x.back(c.s);
    });
}

}  // namespace

extern "C" int vs_facet_value_quantile_plan(int64_t n_rows, int32_t B, int32_t n_labels, int32_t R, int level, int per_query, int64_t rows_per_chunk,
                                            int32_t* out_regime, int32_t* out_qt, int32_t* out_tile_labels, int32_t* out_label_tiles,
                                            int64_t* out_chunks, int64_t* out_rows_per_chunk) {
    if (!out_regime || !out_qt || !out_tile_labels || !out_label_tiles || !out_chunks || !out_rows_per_chunk) return fail(VS_EINVAL, "NULL argument");
    FacetQuantilePlan p;
    char msg[256];
    VS_TRY(plan_or_fail(facet_quantile_plan(n_rows, B, n_labels, R, level, per_query != 0, rows_per_chunk, &p, msg, sizeof msg), msg));
    *out_regime = p.regime;
    *out_qt = p.qt;
    *out_tile_labels = p.tile_labels;
    *out_label_tiles = p.label_tiles;
    *out_chunks = p.chunks;
    *out_rows_per_chunk = p.rows_per_chunk;
    return VS_OK;
}

extern "C" int vs_facet_value_quantiles(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B,
                                        const int32_t* labels, int32_t n_labels, const void* values, int dtype, int64_t n_rows, const double* q,
                                        int method, const int64_t* ranks, int32_t R, int64_t rows_per_chunk, void* out_values, int64_t* out_ranks,
                                        int64_t* count, int64_t* missing, int64_t* total, int64_t* other, int device, void* stream) {
    return facet_value_quantiles(free_set(words, bit0, ld_words, and_words, B, n_rows, device), labels, n_labels, values, dtype, q, method, ranks, R,
                                 rows_per_chunk, out_values, out_ranks, count, missing, total, other, stream);
}

extern "C" int vs_index_facet_value_quantiles(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const int32_t* labels,
                                              int32_t n_labels, const void* values, int dtype, const double* q, int method, const int64_t* ranks,
                                              int32_t R, int64_t rows_per_chunk, void* out_values, int64_t* out_ranks, int64_t* count,
                                              int64_t* missing, int64_t* total, int64_t* other, void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return facet_value_quantiles(src, labels, n_labels, values, dtype, q, method, ranks, R, rows_per_chunk, out_values, out_ranks, count, missing, total,
                                 other, stream);
}

extern "C" int vs_facet_value_radix_counts(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B,
                                           const int32_t* labels, int32_t n_labels, const void* values, int dtype, int64_t n_rows, int level, int32_t R,
                                           const uint32_t* slot_prefix, const int32_t* n_slots, int64_t rows_per_chunk, int64_t* counts,
                                           int64_t* missing, int64_t* total, int64_t* other, int device, void* stream) {
    return facet_radix_counts(free_set(words, bit0, ld_words, and_words, B, n_rows, device), labels, n_labels, values, dtype, level, R, slot_prefix,
                              n_slots, rows_per_chunk, counts, missing, total, other, stream);
}

extern "C" int vs_index_facet_value_radix_counts(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B,
                                                 const int32_t* labels, int32_t n_labels, const void* values, int dtype, int level, int32_t R,
                                                 const uint32_t* slot_prefix, const int32_t* n_slots, int64_t rows_per_chunk, int64_t* counts,
                                                 int64_t* missing, int64_t* total, int64_t* other, void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return facet_radix_counts(src, labels, n_labels, values, dtype, level, R, slot_prefix, n_slots, rows_per_chunk, counts, missing, total, other,
                              stream);
}
