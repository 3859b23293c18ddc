// facet_values.hip -- breakdowns (vs_facet_value_plan, vs_facet_value_stats, vs_facet_value_histogram and their vs_index_* variants): a numeric
// field's stats and histogram per facet label in one pass over (set bitmaps, labels, values).  No reference counterpart (the
// reference only has topk, index.py:92).  Nothing here touches a search kernel: a set arrives as a packed bitmap in the layout of
// vs_index_search_filtered, the labels as int32 [n_rows], the values as fp32 or int32 [n_rows].  Everything is decided on the uint32 order keys
// of value_check.h (0 = the row has no value), so every result is exact and independent of the launch.
//
// Both kernels are walk_tile bodies (set_walk.h): a workgroup owns a chunk of rows and a tile of QT queries; a lane whose row is in SOME
// query's set loads its label and its raw value once for the tile and computes in_range, the key and the sum addend (the histogram: the
// composite slot label x (n_edges + 2) + value slot) once.  total / other are kept as facet_counts_kernel keeps them: wave-uniform counters,
// one LDS add a wave, one global add a workgroup.
//   stats      LDS regime: the records of the tile's queries as arrays in dynamic LDS -- sum[] (64-bit, first for alignment), cnt[], mis[],
//              kmin[], kmax[] -- flushed at the end of the chunk, only records with cnt | mis != 0.  Global regime: the same body with the
//              atomics straight into the output matrices.  out_min / out_max hold KEYS until facet_value_finish_kernel turns them into values.
//   histogram  LDS regime: the edge keys, then uint32 bins [nq][n_labels][n_edges + 2]; the flush routes a slot to below / bin / above /
//              missing of its label.  Global regime: 64-bit atomics straight into the outputs.
// A step whose in-range rows of a query all carry one label (one slot) is reduced across the wave and added by one lane: labels in long runs
// -- article ids, sorted clusters, a compacted corpus -- would otherwise put 64 lanes on one LDS address, five times over for the stats.  The
// stats take that path from VS_FV_ONE_LABEL_MIN rows of a step on (its reduction is not free); the histogram's is a popcount and always taken.
#include "agg_call.h"
#include "facet_value_check.h"
#include "term_sum_check.h"

using namespace vs;

// Rows of a step on one label from which the stats kernel reduces them across the wave and lets one lane add; below it every lane adds for
// itself.  The reduction costs the same whatever the rows (24 ds_bpermute a query), the lanes' own atomics on one LDS address grow with them:
// measured at 21 M rows, 12 labels in runs, B = 8, the two meet between 16 and 32 rows.  make EXTRA=-DVS_FV_ONE_LABEL_MIN=65
// takes the path out, =1 takes it always (A/B runs on the GPU box).
#ifndef VS_FV_ONE_LABEL_MIN
#define VS_FV_ONE_LABEL_MIN 32
#endif

namespace {

struct FvStatsArgs {
    SetArgs s;
    const int32_t* labels;            // [n_rows]
    int32_t n_labels;
    unsigned long long *count, *missing, *sum;     // [B, ld], columns [0, n_labels) zeroed by the caller
    uint32_t *min_key, *max_key;                   // [B, ld], columns [0, n_labels) set to 0xFFFFFFFF / 0 by the caller
    int64_t ld;
    unsigned long long *total, *other;             // [B], zeroed by the caller
};

struct FvHistArgs {
    SetArgs s;
    const int32_t* labels;            // [n_rows]
    int32_t n_labels;
    const uint32_t* edges;            // [n_edges] raw
    int32_t n_edges;
    unsigned long long* counts;       // [B x n_labels, ld_counts], columns [0, n_edges - 1) zeroed by the caller
    int64_t ld_counts;
    unsigned long long *below, *above, *missing;   // [B x n_labels], zeroed by the caller
    unsigned long long *total, *other;             // [B], zeroed by the caller
};

// what c rows with a value (min key lo, max key hi, addends sm) and m rows without one add to record i; no-ops are skipped and no result is used
template <class C>
__device__ __forceinline__ void record_add(C* cnt, C* mis, uint32_t* kmin, uint32_t* kmax, unsigned long long* sum, size_t i, uint32_t c, uint32_t m,
                                           uint32_t lo, uint32_t hi, uint64_t sm) {
    if (c) {
        atomicAdd(cnt + i, (C)c);
        atomicMin(kmin + i, lo);
        atomicMax(kmax + i, hi);
        if (sm) atomicAdd(sum + i, (unsigned long long)sm);
    }
    if (m) atomicAdd(mis + i, (C)m);
}

// the workgroup's total / other of its tile, from the waves' counters
template <int QT>
__device__ __forceinline__ void flush_total_other(const uint32_t* tot, const uint32_t* oth, uint32_t* s_tot, uint32_t* s_oth, int lane, int tid, int q0,
                                                  int nq, unsigned long long* total, unsigned long long* other) {
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            if (tot[q]) atomicAdd(&s_tot[q], tot[q]);
            if (oth[q]) atomicAdd(&s_oth[q], oth[q]);
        }
    }
    __syncthreads();
    if (tid < nq) {
        if (s_tot[tid]) atomicAdd(&total[q0 + tid], (unsigned long long)s_tot[tid]);
        if (s_oth[tid]) atomicAdd(&other[q0 + tid], (unsigned long long)s_oth[tid]);
    }
}

// ---- stats ---------------------------------------------------------------------------------------------------------------------------------------
template <int QT, int GLOBAL>
__global__ __launch_bounds__(kValThreads) void facet_value_stats_kernel(FvStatsArgs a) {
    extern __shared__ unsigned long long fv_lds[];               // sum [R], then cnt, mis, kmin, kmax [R] (LDS regime); R = min(QT, B) x n_labels
    __shared__ uint32_t s_tot[QT], s_oth[QT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q0 = (int)blockIdx.y * QT;
    const int nq = min(QT, a.s.set.B - q0);
    const int64_t r0 = (int64_t)blockIdx.x * a.s.set.rows_per_chunk;
    const int64_t r1 = min(a.s.set.n_rows, r0 + a.s.set.rows_per_chunk);
    const uint32_t L = (uint32_t)a.n_labels;
    const uint32_t R = (uint32_t)min(QT, a.s.set.B) * L;
    unsigned long long* l_sum = fv_lds;
    uint32_t* l_cnt = reinterpret_cast<uint32_t*>(fv_lds + R);
    uint32_t *l_mis = l_cnt + R, *l_min = l_mis + R, *l_max = l_min + R;
    if constexpr (!GLOBAL) {
        for (uint32_t i = tid; i < (uint32_t)nq * L; i += kValThreads) {
            l_sum[i] = 0ull;
            l_cnt[i] = l_mis[i] = 0u;
            l_min[i] = 0xFFFFFFFFu;
            l_max[i] = 0u;
        }
    }
    if (tid < QT) s_tot[tid] = s_oth[tid] = 0u;
    __syncthreads();
    uint32_t tot[QT], oth[QT];                                   // wave-uniform: a chunk holds fewer than 2^32 rows
#pragma unroll
    for (int q = 0; q < QT; ++q) tot[q] = oth[q] = 0u;
    const bool f32 = a.s.dtype == VS_VAL_F32;
    walk_tile<QT, kValWaves>(a.s.set, q0, nq, r0, r1, w, lane, [&](int64_t row0, uint64_t many, const Span* sp, int s, int sh, uint64_t live) {
        int32_t label = -1;
        uint32_t raw = 0u, key = 0u;
        if ((many >> lane) & 1ull) {                                                 // once for the tile
            label = a.labels[row0 + lane];
            raw = a.s.values[row0 + lane];
            key = value_key(raw, a.s.dtype);
        }
        const bool in_range = (uint32_t)label < L;                                   // -1 and anything too large: `other`
        uint64_t add = 0ull;                                                         // what value_stats adds; nothing without a value
        if (key != 0u) add = f32 ? term_fx(__uint_as_float(raw)) : (uint64_t)(int64_t)(int32_t)raw;
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            if (q >= nq) continue;
            const uint64_t m = window64(sp[q], s, sh) & live;
            if (m == 0ull) continue;
            const bool ok = ((m >> lane) & 1ull) && in_range;
            const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
            tot[q] += (uint32_t)__popcll(m);
            oth[q] += (uint32_t)(__popcll(m) - __popcll(okm));
            if (okm == 0ull) continue;
            const bool has = ok && key != 0u;
            const int first = __builtin_ctzll(okm);
            const int32_t l0 = __builtin_amdgcn_readlane(label, first);
            // enough rows, all on one label: reduce and add once
            const bool one = __popcll(okm) >= VS_FV_ONE_LABEL_MIN && __builtin_amdgcn_ballot_w64(ok && label == l0) == okm;
            uint32_t c = has ? 1u : 0u, mi = (ok && !has) ? 1u : 0u, lo = key, hi = key;
            uint64_t sm = add;
            bool mine = ok;
            size_t at = (uint32_t)label;
            if (one) {
                c = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(has));
                mi = (uint32_t)__popcll(okm) - c;
                if (c) {                                                             // (uniform)
                    lo = has ? key : 0xFFFFFFFFu;
                    hi = has ? key : 0u;
                    sm = has ? add : 0ull;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
                        hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, 64));
                        sm += (uint64_t)__shfl_xor((unsigned long long)sm, o, 64);
                    }
                }
                mine = lane == first;
                at = (uint32_t)l0;
            }
            if (!mine) continue;
            if constexpr (GLOBAL) {
                at += (size_t)(q0 + q) * (size_t)a.ld;
                record_add(a.count, a.missing, a.min_key, a.max_key, a.sum, at, c, mi, lo, hi, sm);
            } else {
                at += (size_t)q * L;
                record_add(l_cnt, l_mis, l_min, l_max, l_sum, at, c, mi, lo, hi, sm);
            }
        }
    });
    flush_total_other<QT>(tot, oth, s_tot, s_oth, lane, tid, q0, nq, a.total, a.other);      // (its barrier: the records are complete)
    if constexpr (!GLOBAL) {
        for (int q = 0; q < nq; ++q) {
            const size_t row = (size_t)(q0 + q) * (size_t)a.ld;
            for (uint32_t i = tid; i < L; i += kValThreads) {
                const size_t j = (size_t)q * L + i;
                const uint32_t c = l_cnt[j], mi = l_mis[j];
                if ((c | mi) == 0u) continue;
                record_add(a.count, a.missing, a.min_key, a.max_key, a.sum, row + i, c, mi, l_min[j], l_max[j], l_sum[j]);
            }
        }
    }
}

// keys -> raw values, in place, over the n_labels columns of [B, ld]; a cell without a value: the missing sentinel
__global__ void facet_value_finish_kernel(uint32_t* min_key, uint32_t* max_key, const unsigned long long* count, int64_t cells, int32_t n_labels,
                                          int64_t ld, int dtype) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    const size_t at = (size_t)(i / n_labels) * (size_t)ld + (size_t)(i % n_labels);
    const bool any = count[at] != 0ull;
    min_key[at] = value_unkey(any ? min_key[at] : 0u, dtype);
    max_key[at] = value_unkey(any ? max_key[at] : 0u, dtype);
}

// ---- histogram -------------------------------------------------------------------------------------------------------------------------------------
template <int QT, int GLOBAL>
__global__ __launch_bounds__(kValThreads) void facet_value_hist_kernel(FvHistArgs a) {
    extern __shared__ uint32_t fv_bins[];                        // edge keys [n_edges], then the bins [nq][n_labels][n_edges + 2] (LDS regime)
    __shared__ uint32_t s_tot[QT], s_oth[QT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q0 = (int)blockIdx.y * QT;
    const int nq = min(QT, a.s.set.B - q0);
    const int64_t r0 = (int64_t)blockIdx.x * a.s.set.rows_per_chunk;
    const int64_t r1 = min(a.s.set.n_rows, r0 + a.s.set.rows_per_chunk);
    const int E = a.n_edges;
    const uint32_t L = (uint32_t)a.n_labels, S = (uint32_t)E + 2u;         // slots of a label
    const uint32_t cells = L * S;                                           // of a query: at most 2^22
    uint32_t* ekeys = fv_bins;
    uint32_t* bins = fv_bins + E;
    for (int i = tid; i < E; i += kValThreads) ekeys[i] = value_key(a.edges[i], a.s.dtype);
    if constexpr (!GLOBAL)
        for (uint32_t i = tid; i < (uint32_t)nq * cells; i += kValThreads) bins[i] = 0u;
    if (tid < QT) s_tot[tid] = s_oth[tid] = 0u;
    __syncthreads();
    uint32_t tot[QT], oth[QT];                                   // wave-uniform: a chunk holds fewer than 2^32 rows
#pragma unroll
    for (int q = 0; q < QT; ++q) tot[q] = oth[q] = 0u;
    // where value slot vs of (query b, label l) is counted
    auto cell = [&](size_t b, uint32_t l, uint32_t vs) -> unsigned long long* {
        const size_t r = b * L + l;
        return vs == 0u ? a.below + r : vs == (uint32_t)E ? a.above + r : vs == (uint32_t)E + 1u ? a.missing + r : a.counts + r * (size_t)a.ld_counts + (vs - 1u);
    };
    walk_tile<QT, kValWaves>(a.s.set, q0, nq, r0, r1, w, lane, [&](int64_t row0, uint64_t many, const Span* sp, int s, int sh, uint64_t live) {
        int32_t label = -1;
        uint32_t key = 0u;
        if ((many >> lane) & 1ull) {                                                 // once for the tile
            label = a.labels[row0 + lane];
            key = value_key(a.s.values[row0 + lane], a.s.dtype);
        }
        const bool in_range = (uint32_t)label < L;
        const uint32_t vslot = key == 0u ? (uint32_t)E + 1u : (uint32_t)value_bin(ekeys, E, key);
        const uint32_t slot = in_range ? (uint32_t)label * S + vslot : 0u;           // the composite slot, below `cells`
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            if (q >= nq) continue;
            const uint64_t m = window64(sp[q], s, sh) & live;
            if (m == 0ull) continue;
            const bool ok = ((m >> lane) & 1ull) && in_range;
            const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
            tot[q] += (uint32_t)__popcll(m);
            oth[q] += (uint32_t)(__popcll(m) - __popcll(okm));
            if (okm == 0ull) continue;
            const int first = __builtin_ctzll(okm);
            const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)slot, first);
            const bool one = __builtin_amdgcn_ballot_w64(ok && slot == s0) == okm;      // every row of the step in one slot: add once
            if constexpr (GLOBAL) {
                if (one) {
                    if (lane == first) atomicAdd(cell((size_t)(q0 + q), s0 / S, s0 % S), (unsigned long long)__popcll(okm));
                } else if (ok) {
                    atomicAdd(cell((size_t)(q0 + q), (uint32_t)label, vslot), 1ull);
                }
            } else {
                uint32_t* dst = bins + (size_t)q * cells;
                if (one) {
                    if (lane == first) atomicAdd(dst + s0, (uint32_t)__popcll(okm));
                } else if (ok) {
                    atomicAdd(dst + slot, 1u);
                }
            }
        }
    });
    flush_total_other<QT>(tot, oth, s_tot, s_oth, lane, tid, q0, nq, a.total, a.other);      // (its barrier: the bins are complete)
    if constexpr (!GLOBAL) {
        for (int q = 0; q < nq; ++q) {
            for (uint32_t i = tid; i < cells; i += kValThreads) {
                const uint32_t v = bins[(size_t)q * cells + i];
                if (v) atomicAdd(cell((size_t)(q0 + q), i / S, i % S), (unsigned long long)v);
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
// Up to two zeroed int64 vectors [B] next to a CountsOut whose three are taken: the sibling the histogram's total / other need.
struct VecsOut {
    DevBuf buf;
    unsigned long long* vec[2] = {};
    int bind(bool dev, int64_t* u0, int64_t* u1, int32_t B, hipStream_t s) {
        u_[0] = u0, u_[1] = u1, B_ = B;
        if (dev) {
            for (int i = 0; i < 2; ++i) {
                vec[i] = reinterpret_cast<unsigned long long*>(u_[i]);
                VS_HIP(hipMemsetAsync(vec[i], 0, (size_t)B * 8, s));
            }
        } else {
            VS_TRY(buf.alloc((size_t)B * 16));
            vec[0] = buf.as<unsigned long long>();
            vec[1] = vec[0] + B;
            VS_HIP(hipMemsetAsync(buf.p, 0, buf.bytes, s));
        }
        return VS_OK;
    }
    // host outputs only
    int back(hipStream_t s) {
        for (int i = 0; i < 2; ++i) VS_HIP(hipMemcpyAsync(u_[i], vec[i], (size_t)B_ * 8, hipMemcpyDeviceToHost, s));
        return VS_OK;
    }

private:
    int64_t* u_[2] = {};
    int32_t B_ = 0;
};

// The two [B, n] key matrices of the stats: preset to 0xFFFFFFFF / 0 over the n columns.  Device outputs in place (their spare columns are not
// touched), host outputs in one dense device buffer that back() copies out.
struct KeysOut {
    DevBuf buf;
    uint32_t *lo = nullptr, *hi = nullptr;
    int64_t ld = 0;
    int bind(bool dev, void* u_lo, void* u_hi, int64_t u_ld, int64_t n, int32_t B, hipStream_t s) {
        u_lo_ = u_lo, u_hi_ = u_hi, u_ld_ = u_ld, n_ = n, B_ = B;
        const size_t cells = (size_t)B * (size_t)n;
        if (dev) {
            lo = static_cast<uint32_t*>(u_lo);
            hi = static_cast<uint32_t*>(u_hi);
            ld = u_ld;
            if (u_ld == n || B == 1) {
                VS_HIP(hipMemsetAsync(lo, 0xFF, cells * 4, s));
                VS_HIP(hipMemsetAsync(hi, 0, cells * 4, s));
            } else {
                VS_HIP(hipMemset2DAsync(lo, (size_t)u_ld * 4, 0xFF, (size_t)n * 4, (size_t)B, s));
                VS_HIP(hipMemset2DAsync(hi, (size_t)u_ld * 4, 0, (size_t)n * 4, (size_t)B, s));
            }
        } else {
            VS_TRY(buf.alloc(cells * 8));
            lo = buf.as<uint32_t>();
            hi = lo + cells;
            ld = n;
            VS_HIP(hipMemsetAsync(lo, 0xFF, cells * 4, s));
            VS_HIP(hipMemsetAsync(hi, 0, cells * 4, s));
        }
        return VS_OK;
    }
    // host outputs only
    int back(hipStream_t s) {
        VS_HIP(hipMemcpy2DAsync(u_lo_, (size_t)u_ld_ * 4, lo, (size_t)n_ * 4, (size_t)n_ * 4, (size_t)B_, hipMemcpyDeviceToHost, s));
        VS_HIP(hipMemcpy2DAsync(u_hi_, (size_t)u_ld_ * 4, hi, (size_t)n_ * 4, (size_t)n_ * 4, (size_t)B_, hipMemcpyDeviceToHost, s));
        return VS_OK;
    }

private:
    void *u_lo_ = nullptr, *u_hi_ = nullptr;
    int64_t u_ld_ = 0, n_ = 0;
    int32_t B_ = 0;
};

template <int QT>
int stats_launch_qt(const FacetValuePlan& p, const FvStatsArgs& a, dim3 grid, hipStream_t s) {
    if (p.regime) {                                               // (the global regime only has the tiles 8 and 1)
        if constexpr (QT == 8 || QT == 1) hipLaunchKernelGGL((facet_value_stats_kernel<QT, 1>), grid, dim3(kValThreads), 0, s, a);
        else return fail(VS_EINVAL, "no global-regime kernel for a tile of %d queries", QT);
    } else {
        const size_t lds = (size_t)std::min<int32_t>(QT, a.s.set.B) * (size_t)a.n_labels * 24;      // the actual records: a 12-label field takes a few hundred bytes
        VS_HIP(hipFuncSetAttribute((const void*)facet_value_stats_kernel<QT, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((facet_value_stats_kernel<QT, 0>), grid, dim3(kValThreads), lds, s, a);
    }
    VS_HIP(hipGetLastError());
    return VS_OK;
}

template <int QT>
int hist_launch_qt(const FacetValuePlan& p, const FvHistArgs& a, dim3 grid, hipStream_t s) {
    if (p.regime) {                                               // (the global regime only has the tiles 8 and 1; its LDS: the edge keys)
        if constexpr (QT == 8 || QT == 1) hipLaunchKernelGGL((facet_value_hist_kernel<QT, 1>), grid, dim3(kValThreads), (size_t)a.n_edges * 4, s, a);
        else return fail(VS_EINVAL, "no global-regime kernel for a tile of %d queries", QT);
    } else {
        const size_t lds = ((size_t)a.n_edges + (size_t)std::min<int32_t>(QT, a.s.set.B) * (size_t)a.n_labels * ((size_t)a.n_edges + 2)) * 4;
        VS_HIP(hipFuncSetAttribute((const void*)facet_value_hist_kernel<QT, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((facet_value_hist_kernel<QT, 0>), grid, dim3(kValThreads), lds, s, a);
    }
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// vs_facet_value_stats and vs_index_facet_value_stats: one call on the set's device
int facet_value_stats(const SetSrc& src, const int32_t* labels, int32_t n_labels, const void* values, int dtype, int64_t rows_per_chunk,
                      int64_t* count, int64_t* missing, void* out_min, void* out_max, int64_t* sum, int64_t ld_out, int64_t* total, int64_t* other,
                      void* stream) {
    FacetValuePlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(facet_value_check_stats(labels && values && count && missing && out_min && out_max && sum && total && other,
                                                src.words != nullptr, src.bit0, src.ld_words, src.B, dtype, src.n_rows, n_labels, rows_per_chunk, ld_out,
                                                &plan, msg, sizeof msg), msg));
    VS_TRY(src.device_ok());
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"labels", labels}, {"values", values}, {"count", count},
                                       {"missing", missing}, {"out_min", out_min}, {"out_max", out_max}, {"sum", sum}, {"total", total},
                                       {"other", other}}));
    const int32_t B = src.B;
    SetStage st;
    Staged st_l;
    CountsOut o_cnt, o_mis, o_sum;                                // (host outputs: three dense matrices, total and other behind the first)
    KeysOut o_key;
    return c.run("facet_value_stats", Finish::kStream, [&] {
        FvStatsArgs a{};
        int32_t* d_l;
        VS_TRY(st.in(src, values, dtype, plan.rows_per_chunk, c.dev, c.s, &a.s));
        VS_TRY(st_l.in(labels, (size_t)src.n_rows, c.dev, true, c.s, &d_l));
        a.labels = d_l;
        a.n_labels = n_labels;
        VS_TRY(o_cnt.bind(c.dev, count, ld_out, n_labels, B, {total, other}, c.s));
        VS_TRY(o_mis.bind(c.dev, missing, ld_out, n_labels, B, {}, c.s));
        VS_TRY(o_sum.bind(c.dev, sum, ld_out, n_labels, B, {}, c.s));
        VS_TRY(o_key.bind(c.dev, out_min, out_max, ld_out, n_labels, B, c.s));
        a.count = o_cnt.mat;
        a.missing = o_mis.mat;
        a.sum = o_sum.mat;
        a.min_key = o_key.lo;
        a.max_key = o_key.hi;
        a.ld = o_cnt.ld;
        a.total = o_cnt.vec[0];
        a.other = o_cnt.vec[1];
        ProfScope prof("facet_value_stats", c.s);
        const dim3 grid((unsigned)plan.chunks, (unsigned)ceil_div64(B, plan.qt));
        VS_TRY(launch_by_qt(plan.qt, [&](auto qt) { return stats_launch_qt<decltype(qt)::value>(plan, a, grid, c.s); }));
        const int64_t cells = (int64_t)B * n_labels;
        hipLaunchKernelGGL(facet_value_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c.s, a.min_key, a.max_key, a.count, cells,
                           n_labels, a.ld, dtype);
        return VS_OK;
    }, [&] {
        VS_TRY(o_cnt.back(c.s));
        VS_TRY(o_mis.back(c.s));
        VS_TRY(o_sum.back(c.s));
        return o_key.back(c.s);
    });
}

// vs_facet_value_histogram and vs_index_facet_value_histogram (a host edges array is looked at before the device is, as vs_value_histogram does)
int facet_value_histogram(const SetSrc& src, const int32_t* labels, int32_t n_labels, const void* values, int dtype, const void* edges,
                          int32_t n_edges, int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts, int64_t* below, int64_t* above,
                          int64_t* missing, int64_t* total, int64_t* other, void* stream) {
    FacetValuePlan plan;
    char msg[256];
    VS_TRY(plan_or_fail(facet_value_check_hist(labels && values && edges && counts && below && above && missing && total && other, src.words != nullptr,
                                               src.bit0, src.ld_words, src.B, dtype, src.n_rows, n_labels, n_edges, rows_per_chunk, ld_counts, &plan, msg,
                                               sizeof msg), msg));
    if (!is_device_ptr(edges)) VS_TRY(plan_or_fail(value_check_edges_host(static_cast<const uint32_t*>(edges), n_edges, dtype, msg, sizeof msg), msg));
    VS_TRY(src.device_ok());
    Call c;
    VS_TRY(c.open(src.device, stream, {{"words", src.words}, {"and_words", src.and_user}, {"labels", labels}, {"values", values}, {"edges", edges},
                                       {"counts", counts}, {"below", below}, {"above", above}, {"missing", missing}, {"total", total},
                                       {"other", other}}));
    const int32_t B = src.B;
    SetStage st;
    Staged st_l, st_e;
    CountsOut out;                                                // B x n_labels rows of n_edges - 1 columns, three [B x n_labels] vectors
    VecsOut tail;
    return c.run("facet_value_histogram", Finish::kStream, [&] {
        FvHistArgs a{};
        int32_t* d_l;
        uint32_t* d_e;
        VS_TRY(st.in(src, values, dtype, plan.rows_per_chunk, c.dev, c.s, &a.s));
        VS_TRY(st_l.in(labels, (size_t)src.n_rows, c.dev, true, c.s, &d_l));
        VS_TRY(st_e.in(static_cast<const uint32_t*>(edges), (size_t)n_edges, c.dev, true, c.s, &d_e));
        a.labels = d_l;
        a.n_labels = n_labels;
        a.edges = d_e;
        a.n_edges = n_edges;
        VS_TRY(out.bind(c.dev, counts, ld_counts, n_edges - 1, B * n_labels, {below, above, missing}, c.s));
        VS_TRY(tail.bind(c.dev, total, other, B, c.s));
        a.counts = out.mat;
        a.ld_counts = out.ld;
        a.below = out.vec[0];
        a.above = out.vec[1];
        a.missing = out.vec[2];
        a.total = tail.vec[0];
        a.other = tail.vec[1];
        ProfScope prof("facet_value_histogram", c.s);
        const dim3 grid((unsigned)plan.chunks, (unsigned)ceil_div64(B, plan.qt));
        return launch_by_qt(plan.qt, [&](auto qt) { return hist_launch_qt<decltype(qt)::value>(plan, a, grid, c.s); });
    }, [&] {
        VS_TRY(out.back(c.s));
        return tail.back(c.s);
    });
}

}  // namespace

extern "C" int vs_facet_value_plan(int64_t n_rows, int32_t B, int32_t n_labels, int32_t n_slots, int per_query, int64_t rows_per_chunk,
                                   int32_t* out_regime, int32_t* out_qt, int64_t* out_chunks, int64_t* out_rows_per_chunk) {
    if (!out_regime || !out_qt || !out_chunks || !out_rows_per_chunk) return fail(VS_EINVAL, "NULL argument");
    FacetValuePlan p;
    char msg[256];
    VS_TRY(plan_or_fail(facet_value_plan(n_rows, B, n_labels, n_slots, per_query != 0, rows_per_chunk, &p, msg, sizeof msg), msg));
    *out_regime = p.regime;
    *out_qt = p.qt;
    *out_chunks = p.chunks;
    *out_rows_per_chunk = p.rows_per_chunk;
    return VS_OK;
}

extern "C" int vs_facet_value_stats(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B,
                                    const int32_t* labels, int32_t n_labels, const void* values, int dtype, int64_t n_rows, int64_t rows_per_chunk,
                                    int64_t* count, int64_t* missing, void* out_min, void* out_max, int64_t* sum, int64_t ld_out, int64_t* total,
                                    int64_t* other, int device, void* stream) {
    return facet_value_stats(free_set(words, bit0, ld_words, and_words, B, n_rows, device), labels, n_labels, values, dtype, rows_per_chunk, count,
                             missing, out_min, out_max, sum, ld_out, total, other, stream);
}

extern "C" int vs_index_facet_value_stats(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const int32_t* labels,
                                          int32_t n_labels, const void* values, int dtype, int64_t rows_per_chunk, int64_t* count, int64_t* missing,
                                          void* out_min, void* out_max, int64_t* sum, int64_t ld_out, int64_t* total, int64_t* other, void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return facet_value_stats(src, labels, n_labels, values, dtype, rows_per_chunk, count, missing, out_min, out_max, sum, ld_out, total, other, stream);
}

extern "C" int vs_facet_value_histogram(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_words, int32_t B,
                                        const int32_t* labels, int32_t n_labels, const void* values, int dtype, int64_t n_rows, const void* edges,
                                        int32_t n_edges, int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts, int64_t* below, int64_t* above,
                                        int64_t* missing, int64_t* total, int64_t* other, int device, void* stream) {
    return facet_value_histogram(free_set(words, bit0, ld_words, and_words, B, n_rows, device), labels, n_labels, values, dtype, edges, n_edges,
                                 rows_per_chunk, counts, ld_counts, below, above, missing, total, other, stream);
}

extern "C" int vs_index_facet_value_histogram(vs_index* idx, const uint32_t* words, int64_t bit0, int64_t ld_words, int32_t B, const int32_t* labels,
                                              int32_t n_labels, const void* values, int dtype, const void* edges, int32_t n_edges,
                                              int64_t rows_per_chunk, int64_t* counts, int64_t ld_counts, int64_t* below, int64_t* above,
                                              int64_t* missing, int64_t* total, int64_t* other, void* stream) {
    SetSrc src;
    VS_TRY(index_set(idx, words, bit0, ld_words, B, &src));
    return facet_value_histogram(src, labels, n_labels, values, dtype, edges, n_edges, rows_per_chunk, counts, ld_counts, below, above, missing, total,
                                 other, stream);
}
