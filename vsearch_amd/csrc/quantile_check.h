// quantile_check.h -- the host-only part of the percentiles (vs_value_quantiles, vs_value_radix_counts, vs_value_radix_step,
// vs_value_quantile_plan): the digit geometry of the three radix levels, the quantile -> rank rule, the bin search of the step,
// the plan rule and the argument checks.  The rank rule, the digit functions and the bin search are what the kernels of quantiles.hip run,
// __host__ __device__, so that the stand-alone check (quantile_check_main.cpp, built under the host sanitizers by tests/test_quantile_cpu.py)
// exercises the very code.  Plain C++ with no HIP in it.
#pragma once

#include <cmath>

#include "value_check.h"

namespace vs {

static_assert(VS_VALUE_RADIX_LEVELS == 3 && VS_VALUE_RADIX_BINS == 2048, "digits: bits 31..21, 20..10, 9..0");
static_assert(VS_VALUE_MAX_RANKS == 16, "the slot search takes 4 steps");

// ---- the digits: level 0 = bits 31..21, level 1 = bits 20..10, level 2 = bits 9..0 of a key ------------------------------------------------------
VS_VALUE_HD inline int radix_bins(int level) { return level == 2 ? 1024 : 2048; }
VS_VALUE_HD inline int radix_shift(int level) { return level == 0 ? 21 : level == 1 ? 10 : 0; }                  // where the level's digit starts
VS_VALUE_HD inline uint32_t radix_digit(uint32_t key, int level) { return (key >> radix_shift(level)) & (uint32_t)(radix_bins(level) - 1); }
// the digits above the level's, right-aligned: what a slot of the level is named by (level 0: nothing, 0)
VS_VALUE_HD inline uint32_t radix_prefix(uint32_t key, int level) { return level == 0 ? 0u : key >> (radix_shift(level) + (level == 1 ? 11 : 10)); }
// a slot's prefix extended by the digit found at `level`: the prefix of the next level, the key itself after level 2
VS_VALUE_HD inline uint32_t radix_extend(uint32_t prefix, int level, uint32_t digit) { return (prefix << (level == 2 ? 10 : 11)) | digit; }
constexpr uint32_t kRadixNoSlot = 0xFFFFFFFFu;        // pads the slot prefixes behind the last: no prefix has more than 22 bits

// ---- quantile -> rank: pos = q * (count - 1) in one fp64 multiplication; -1 = no answer (count = 0, q outside [0, 1] or NaN) --------------------
VS_VALUE_HD inline int64_t quantile_rank(double q, int64_t count, int method) {
    if (count <= 0 || !(q >= 0.0 && q <= 1.0)) return -1;
    const double pos = q * (double)(count - 1);
    const double r = method == VS_QUANTILE_LOWER ? floor(pos) : method == VS_QUANTILE_HIGHER ? ceil(pos) : rint(pos);      // rint: half to even
    return (int64_t)r;
}
// an explicit rank: itself inside 0..count - 1, else -1
VS_VALUE_HD inline int64_t quantile_rank_given(int64_t rank, int64_t count) { return rank >= 0 && rank < count ? rank : -1; }

// The step's bin search.  cum [n_bins + 1] is the exclusive prefix sum of a slot's bins (cum[0] = 0, cum[n_bins] = the slot's total), n_bins a
// power of two; -> the bin d with cum[d] <= r < cum[d + 1], or -1 when r is outside 0..total - 1.  Branch-free: log2(n_bins) steps.
VS_VALUE_HD inline int radix_find_bin(const int64_t* cum, int n_bins, int64_t r) {
    if (r < 0 || r >= cum[n_bins]) return -1;
    int d = 0;                                        // cum[d] <= r throughout
    for (int step = n_bins >> 1; step > 0; step >>= 1) d = cum[d + step] <= r ? d + step : d;
    return d;                                         // the largest d < n_bins with cum[d] <= r: bins of count 0 are stepped over
}

// The slot of a prefix among a query's sorted slot prefixes sp [16] (padded with kRadixNoSlot): its index, or -1.  4 steps and a compare.
VS_VALUE_HD inline int radix_find_slot(const uint32_t* sp, uint32_t prefix) {
    int pos = 0;
    pos += sp[pos + 8] <= prefix ? 8 : 0;
    pos += sp[pos + 4] <= prefix ? 4 : 0;
    pos += sp[pos + 2] <= prefix ? 2 : 0;
    pos += sp[pos + 1] <= prefix ? 1 : 0;
    return sp[pos] == prefix ? pos : -1;
}

// ---- the plan: queries a workgroup serves by the number of ranks, the chunks by value_plan's rule -------------------------------------------------
inline int32_t quantile_qt(int32_t R, bool per_query) { return !per_query ? 1 : R <= 2 ? 8 : R <= 4 ? 4 : R <= 8 ? 2 : 1; }

inline int quantile_check_ranks(int32_t R, char* msg, size_t cap) {
    if (R < 1 || R > VS_VALUE_MAX_RANKS) return snprintf(msg, cap, "R must be in 1..%d ranks (got %d)", VS_VALUE_MAX_RANKS, R), VS_EINVAL;
    return VS_OK;
}

inline int quantile_plan(int64_t n_rows, int32_t B, int32_t R, bool per_query, int64_t rows_per_chunk, ValuePlan* out, char* msg, size_t cap) {
    const int rc = quantile_check_ranks(R, msg, cap);
    if (rc != VS_OK) return rc;
    return value_plan(n_rows, B, 0, per_query, rows_per_chunk, quantile_qt(R, per_query), out, msg, cap);
}
// LDS bytes of the counting kernel at a level: qt x slots x bins uint32 (level 0 has one slot a query)
inline size_t quantile_lds_bytes(int32_t qt, int32_t R, int level) { return (size_t)qt * (size_t)(level == 0 ? 1 : R) * (size_t)radix_bins(level) * 4; }

// ---- the checks of the calls --------------------------------------------------------------------------------------------------------------------------
inline int quantile_check_level(int level, char* msg, size_t cap) {
    if (level < 0 || level >= VS_VALUE_RADIX_LEVELS) return snprintf(msg, cap, "level must be in 0..%d (got %d)", VS_VALUE_RADIX_LEVELS - 1, level), VS_EINVAL;
    return VS_OK;
}
inline int quantile_check_method(int method, char* msg, size_t cap) {
    if (method != VS_QUANTILE_LOWER && method != VS_QUANTILE_HIGHER && method != VS_QUANTILE_NEAREST)
        return snprintf(msg, cap, "method must be VS_QUANTILE_LOWER (0), VS_QUANTILE_HIGHER (1) or VS_QUANTILE_NEAREST (2), got %d", method), VS_EINVAL;
    return VS_OK;
}
// the int64 counts [B, R, 2048] a call holds on the device
inline int quantile_check_scratch(int32_t B, int32_t R, char* msg, size_t cap) {
    if ((int64_t)B * R * VS_VALUE_RADIX_BINS > kValueMaxScratchKeys)
        return snprintf(msg, cap, "%d queries x %d ranks x %d bins are more than 2^27 counts: take fewer queries a call", B, R, VS_VALUE_RADIX_BINS), VS_EINVAL;
    return VS_OK;
}
// a host q array: every entry in [0, 1]
inline int quantile_check_q_host(const double* q, int32_t R, char* msg, size_t cap) {
    for (int32_t j = 0; j < R; ++j)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return snprintf(msg, cap, "q[%d] = %g is outside [0, 1]", j, q[j]), VS_EINVAL;
    return VS_OK;
}
// a host ranks array [B, R]: none negative (a rank at or past the count is answered with the sentinel)
inline int quantile_check_ranks_host(const int64_t* ranks, int64_t n, char* msg, size_t cap) {
    for (int64_t i = 0; i < n; ++i)
        if (ranks[i] < 0) return snprintf(msg, cap, "ranks[%lld] = %lld is negative", (long long)i, (long long)ranks[i]), VS_EINVAL;
    return VS_OK;
}

}  // namespace vs
