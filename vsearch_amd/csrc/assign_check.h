// assign_check.h -- the plan rule and the argument checks of the clustering calls (vs_assign_plan, vs_index_assign, vs_centroid_half_norms,
// vs_label_bitmaps) that need no device: slice width, slices, chunks, the slab's size, strides, and the finiteness of host centroids and bias.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_cluster_cpu.py builds one).
#pragma once

#include <cmath>

#include "term_agg_check.h"

namespace vs {

constexpr int kAssignAutoChunks = 4096;               // workgroups the automatic plan aims at (16 a CU: a workgroup is 4 waves)
constexpr int64_t kAssignMaxBit0 = (int64_t)1 << 32;  // the first bit of a bitmap: its words stay inside a 1-D grid
constexpr int kAssignMinChunkRows = 256;              // ... each with at least one 64-row step a wave

struct AssignPlan {
    int32_t slice_w = 64, slices = 1;                 // a lane owns slice_w / 64 centroids of a slice; Kp = slice_w * slices >= K
    int64_t chunks = 1, rows_per_chunk = kAssignMinChunkRows;
    int64_t slab_bytes = 0;                           // (n_cols + 1) * Kp * 4: the transposed centroids, row n_cols zero
};

// The plan rule: pure host arithmetic.
inline int assign_plan(int64_t n_rows, int32_t K, int32_t n_cols, int64_t rows_per_chunk, AssignPlan* out, char* msg, size_t cap) {
    if (n_rows < 1 || n_rows > kTermMaxRows) return snprintf(msg, cap, "n_rows must be in 1..2^32 - 1 (got %lld)", (long long)n_rows), VS_EINVAL;
    if (K < 1 || K > VS_ASSIGN_MAX_K) return snprintf(msg, cap, "K must be in 1..%d centroids (got %d)", VS_ASSIGN_MAX_K, K), VS_EINVAL;
    if (n_cols < 1 || n_cols > kTermMaxCols) return snprintf(msg, cap, "n_cols must be in 1..%d (got %d)", kTermMaxCols, n_cols), VS_EINVAL;
    if (rows_per_chunk < 0 || rows_per_chunk % 64 != 0 || rows_per_chunk > kTermMaxRows)
        return snprintf(msg, cap, "rows_per_chunk must be 0 (automatic) or a positive multiple of 64 below 2^32 (got %lld)", (long long)rows_per_chunk),
               VS_EINVAL;
    AssignPlan p;
    p.slice_w = K <= 64 ? 64 : (K <= 128 ? 128 : 256);                            // 1, 2 or 4 centroids a lane: a 256 / 512 / 1024-byte read a cell
    p.slices = (K + p.slice_w - 1) / p.slice_w;
    if (rows_per_chunk == 0) {
        rows_per_chunk = std::max<int64_t>((n_rows + kAssignAutoChunks - 1) / kAssignAutoChunks, kAssignMinChunkRows);
        rows_per_chunk = (rows_per_chunk + 63) / 64 * 64;
    }
    p.rows_per_chunk = rows_per_chunk;
    p.chunks = (n_rows + rows_per_chunk - 1) / rows_per_chunk;                     // <= 2^26: a 1-D grid holds them
    p.slab_bytes = ((int64_t)n_cols + 1) * p.slice_w * p.slices * 4;              // <= 2^16 * 2^12 * 4 = 1 GiB
    *out = p;
    return VS_OK;
}

// vs_index_assign: the geometry (n_rows, n_cols: the index's)
inline int assign_check_call(bool have_pointers, int32_t K, int64_t ldc, int64_t filter_bit0, int64_t n_rows, int32_t n_cols, int64_t rows_per_chunk,
                             AssignPlan* plan, char* msg, size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    if (filter_bit0 < 0 || filter_bit0 > kAssignMaxBit0)
        return snprintf(msg, cap, "filter_bit0 must be in 0..2^32 (got %lld)", (long long)filter_bit0), VS_EINVAL;
    const int rc = assign_plan(n_rows, K, n_cols, rows_per_chunk, plan, msg, cap);
    if (rc != VS_OK) return rc;
    if (ldc < n_cols) return snprintf(msg, cap, "ldc = %lld is shorter than n_cols = %d", (long long)ldc, n_cols), VS_EINVAL;
    return VS_OK;
}

// host centroids [K, ldc] (columns [0, n_cols) of a row are read, nothing behind the last row's) and a host bias [K] (may be absent) are finite
inline int assign_check_finite_host(const float* c, int32_t K, int32_t n_cols, int64_t ldc, const float* bias, char* msg, size_t cap) {
    for (int32_t j = 0; j < K; ++j)
        for (int32_t i = 0; i < n_cols; ++i)
            if (!std::isfinite(c[(size_t)j * (size_t)ldc + (size_t)i]))
                return snprintf(msg, cap, "centroid %d is not finite at column %d", j, i), VS_EINVAL;
    if (bias)
        for (int32_t j = 0; j < K; ++j)
            if (!std::isfinite(bias[j])) return snprintf(msg, cap, "bias[%d] is not finite", j), VS_EINVAL;
    return VS_OK;
}

// vs_centroid_half_norms
inline int assign_check_norms(bool have_pointers, int32_t K, int32_t n_cols, int64_t ldc, char* msg, size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    if (K < 1 || K > VS_ASSIGN_MAX_K) return snprintf(msg, cap, "K must be in 1..%d centroids (got %d)", VS_ASSIGN_MAX_K, K), VS_EINVAL;
    if (n_cols < 1 || n_cols > kTermMaxCols) return snprintf(msg, cap, "n_cols must be in 1..%d (got %d)", kTermMaxCols, n_cols), VS_EINVAL;
    if (ldc < n_cols) return snprintf(msg, cap, "ldc = %lld is shorter than n_cols = %d", (long long)ldc, n_cols), VS_EINVAL;
    return VS_OK;
}

// vs_label_bitmaps
inline int assign_check_bitmaps(bool have_pointers, int64_t n_rows, int32_t B, int64_t bit0, int64_t ld_words, char* msg, size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    if (n_rows < 1 || n_rows > kTermMaxRows) return snprintf(msg, cap, "n_rows must be in 1..2^32 - 1 (got %lld)", (long long)n_rows), VS_EINVAL;
    if (B < 1 || B > VS_LABEL_MAX_VALUES) return snprintf(msg, cap, "B must be in 1..%d values (got %d)", VS_LABEL_MAX_VALUES, B), VS_EINVAL;
    if (bit0 < 0 || bit0 > kAssignMaxBit0) return snprintf(msg, cap, "bit0 must be in 0..2^32 (got %lld)", (long long)bit0), VS_EINVAL;
    const int64_t span = (bit0 + n_rows + 31) >> 5;
    if (ld_words < span)
        return snprintf(msg, cap, "ld_words = %lld is shorter than the %lld words a bitmap spans", (long long)ld_words, (long long)span), VS_EINVAL;
    return VS_OK;
}

}  // namespace vs
