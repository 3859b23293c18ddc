// value_check.h -- the order keys, the bin search, the plan rule and the argument checks of the numeric fields (vs_value_range_bitmaps,
// vs_value_plan, vs_value_stats, vs_value_histogram, vs_value_topk) that need no device.  The key functions and the bin search are what the
// kernels of values.hip run, __host__ __device__, so that the stand-alone check exercises the very code.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_value_cpu.py builds one).
#pragma once

#include "set_check.h"

namespace vs {

#if defined(__HIPCC__)
#define VS_VALUE_HD __host__ __device__
#else
#define VS_VALUE_HD
#endif

constexpr int64_t kValueMaxRows = 0xFFFFFFFFll;       // a chunk's count fits a uint32 bin, a row fits the low half of a top-k key
constexpr int kValThreads = 256;                      // threads of the workgroups that walk a set of values (values.hip, quantiles.hip)
constexpr int kValWaves = kValThreads / 64;
constexpr int64_t kValueMaxScratchKeys = 1ll << 27;   // keys of vs_value_topk's per-chunk lists (1 GiB)
constexpr uint32_t kValueNanF32 = 0x7FC00000u;        // the missing sentinels the calls WRITE (any NaN is read as missing)
constexpr uint32_t kValueMissI32 = 0x80000000u;

// ---- order keys: raw 32-bit value -> uint32, 0 = missing ---------------------------------------------------------------------------------
// fp32: flip_f32(canon_zero(v)) of topk_keys.h spelled on the bits; a NaN of either sign is missing.  -inf (0xFF800000) -> 0x007FFFFF is the
// smallest key of a value: the negative NaNs, which would flip below it, are taken out first.
VS_VALUE_HD inline uint32_t value_key_f32(uint32_t u) {
    const uint32_t mag = u & 0x7FFFFFFFu;
    if (mag > 0x7F800000u) return 0u;                 // NaN
    if (mag == 0u) u = 0u;                            // -0.0 -> +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
VS_VALUE_HD inline uint32_t value_key_i32(uint32_t u) { return u ^ 0x80000000u; }     // INT32_MIN -> 0
VS_VALUE_HD inline uint32_t value_key(uint32_t raw, int dtype) { return dtype == VS_VAL_F32 ? value_key_f32(raw) : value_key_i32(raw); }
// key -> the raw value it stands for (key 0 -> the missing sentinel)
VS_VALUE_HD inline uint32_t value_unkey(uint32_t key, int dtype) {
    if (dtype == VS_VAL_F32) return key == 0u ? kValueNanF32 : ((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
    return key ^ 0x80000000u;
}

// The edges of `key` = how many of the n ascending edge keys are <= key (numpy's searchsorted(side = "right")): 0 = below the first edge,
// i in 1..n - 1 = bin i - 1, n = at or above the last.  Branch-free: 11 steps for the 1025 edges at most, every step one load and a select.
VS_VALUE_HD inline int value_bin(const uint32_t* edges, int n, uint32_t key) {
    int pos = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int step = 1024; step > 0; step >>= 1) {
        const int idx = pos + step;                   // edges [0, pos) are <= key
        const int at = (idx <= n ? idx : n) - 1;      // (n >= 1: never negative)
        const bool take = idx <= n && edges[at] <= key;
        pos = take ? idx : pos;
    }
    return pos;
}
static_assert(VS_VALUE_MAX_EDGES <= 2047, "value_bin starts at a step of 1024");

// ---- the plan rule: pure host arithmetic ----------------------------------------------------------------------------------------------------
struct ValuePlan {
    int32_t qt = 1;                   // queries a workgroup serves
    int64_t chunks = 1, rows_per_chunk = kSpanRows;
};

// qt_max: 8 for stats and histograms, 1 for the top-k (one query a workgroup)
inline int value_plan(int64_t n_rows, int32_t B, int32_t n_bins, bool per_query, int64_t rows_per_chunk, int32_t qt_max, ValuePlan* out, char* msg,
                      size_t cap) {
    int rc = check_n_rows(n_rows, msg, cap);
    if (rc == VS_OK) rc = check_batch(B, msg, cap);
    if (rc != VS_OK) return rc;
    if (n_bins < 0 || n_bins > VS_VALUE_MAX_EDGES + 2)
        return snprintf(msg, cap, "n_bins must be in 0..%d (got %d)", VS_VALUE_MAX_EDGES + 2, n_bins), VS_EINVAL;
    rc = check_chunking(per_query, B, rows_per_chunk, "bitmap", msg, cap);
    if (rc != VS_OK) return rc;
    ValuePlan p;
    p.qt = per_query ? qt_max : 1;
    const int64_t tiles = (B + p.qt - 1) / p.qt;
    // enough workgroups to fill the chip, chunks long enough that zeroing and flushing the histograms stays a sixteenth of the bit tests
    if (rows_per_chunk == 0) rows_per_chunk = auto_chunk(n_rows, tiles, std::max<int64_t>(kMinChunk, (int64_t)16 * n_bins));
    p.rows_per_chunk = rows_per_chunk;
    p.chunks = (n_rows + rows_per_chunk - 1) / rows_per_chunk;
    if (p.chunks > 0x7FFFFFFF || tiles > 65535)
        return snprintf(msg, cap, "%lld chunks x %d queries are too many for one call", (long long)p.chunks, B), VS_EINVAL;
    *out = p;
    return VS_OK;
}

inline int value_check_dtype(int dtype, char* msg, size_t cap) {
    if (dtype != VS_VAL_F32 && dtype != VS_VAL_I32)
        return snprintf(msg, cap, "dtype must be VS_VAL_F32 (0) or VS_VAL_I32 (1), got %d", dtype), VS_EINVAL;
    return VS_OK;
}

// the set of a stats / histogram / top-k call: the bitmap's geometry, and the plan
inline int value_check_set(bool have_pointers, bool have_words, int64_t bit0, int64_t ld_words, int32_t B, int dtype, int64_t n_rows, int32_t n_bins,
                           int64_t rows_per_chunk, int32_t qt_max, ValuePlan* plan, char* msg, size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    int rc = value_check_dtype(dtype, msg, cap);
    if (rc != VS_OK) return rc;
    rc = check_bit0(bit0, msg, cap);
    if (rc == VS_OK) rc = value_plan(n_rows, B, n_bins, have_words && ld_words != 0, rows_per_chunk, qt_max, plan, msg, cap);
    if (rc == VS_OK) rc = check_ld_words(have_words, bit0, ld_words, n_rows, msg, cap);
    return rc;
}

// vs_value_histogram: the edge count and the stride of counts
inline int value_check_hist(int32_t n_edges, int64_t ld_counts, char* msg, size_t cap) {
    if (n_edges < 2 || n_edges > VS_VALUE_MAX_EDGES)
        return snprintf(msg, cap, "n_edges must be in 2..%d (got %d)", VS_VALUE_MAX_EDGES, n_edges), VS_EINVAL;
    if (ld_counts < n_edges - 1) return snprintf(msg, cap, "ld_counts = %lld is shorter than the %d bins", (long long)ld_counts, n_edges - 1), VS_EINVAL;
    return VS_OK;
}

// a host edges array: no missing sentinel, keys strictly ascending
inline int value_check_edges_host(const uint32_t* edges, int32_t n_edges, int dtype, char* msg, size_t cap) {
    uint32_t prev = 0u;
    for (int32_t i = 0; i < n_edges; ++i) {
        const uint32_t k = value_key(edges[i], dtype);
        if (k == 0u) return snprintf(msg, cap, "edges[%d] is the missing sentinel (NaN / INT32_MIN)", i), VS_EINVAL;
        if (i && k <= prev) return snprintf(msg, cap, "edges must be strictly ascending: edges[%d] is not above edges[%d]", i, i - 1), VS_EINVAL;
        prev = k;
    }
    return VS_OK;
}

// vs_value_topk: k and the scratch the per-chunk lists take
inline int value_check_topk(int32_t k, int32_t B, const ValuePlan& plan, char* msg, size_t cap) {
    if (k < 1 || k > VS_VALUE_MAX_TOPK) return snprintf(msg, cap, "k must be in 1..%d (got %d)", VS_VALUE_MAX_TOPK, k), VS_EINVAL;
    if (plan.chunks > kValueMaxScratchKeys / ((int64_t)B * k))
        return snprintf(msg, cap, "%lld chunks x %d queries x k = %d are more than 2^27 scratch keys: take longer chunks", (long long)plan.chunks, B, k),
               VS_EINVAL;
    return VS_OK;
}

// vs_value_range_bitmaps
inline int value_check_ranges(bool have_pointers, int dtype, int64_t n_rows, int32_t B, int64_t bit0, int64_t ld_words, char* msg, size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    const int rc = value_check_dtype(dtype, msg, cap);
    if (rc != VS_OK) return rc;
    if (n_rows < 1 || n_rows > kValueMaxRows) return snprintf(msg, cap, "n_rows must be in 1..2^32 - 1 (got %lld)", (long long)n_rows), VS_EINVAL;
    if (B < 1 || B > VS_VALUE_MAX_RANGES) return snprintf(msg, cap, "B must be in 1..%d ranges (got %d)", VS_VALUE_MAX_RANGES, B), VS_EINVAL;
    if (bit0 < 0 || bit0 > (1ll << 32)) return snprintf(msg, cap, "bit0 must be in 0..2^32 (got %lld)", (long long)bit0), VS_EINVAL;
    const int64_t span = (bit0 + n_rows + 31) >> 5;
    if (ld_words < span)
        return snprintf(msg, cap, "ld_words = %lld is shorter than the %lld words a bitmap spans", (long long)ld_words, (long long)span), VS_EINVAL;
    return VS_OK;
}

// host bounds: none missing
inline int value_check_bounds_host(const uint32_t* lo, const uint32_t* hi, int32_t B, int dtype, char* msg, size_t cap) {
    for (int32_t b = 0; b < B; ++b)
        if (value_key(lo[b], dtype) == 0u || value_key(hi[b], dtype) == 0u)
            return snprintf(msg, cap, "range %d has a missing bound (NaN / INT32_MIN): pass -inf / +inf or INT32_MIN + 1 / INT32_MAX for an open end", b),
                   VS_EINVAL;
    return VS_OK;
}

}  // namespace vs
