// term_agg_check.h -- the plan rule and the argument checks of the term aggregations (vs_term_plan, vs_index_term_counts,
// vs_index_term_counts_ids, vs_term_topn) that need no device: sizes and strides, and a host id list before it is staged.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_term_agg_cpu.py builds one).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "vsearch_hip.h"

namespace vs {

constexpr int64_t kTermMaxRows = 0xFFFFFFFFll;        // a chunk's count fits a uint32 bin
constexpr int32_t kTermMaxCols = 65535;               // the packets hold uint16 column ids; n_cols itself is the padding id
constexpr int kTermSpanRows = 2048;                   // rows a workgroup loads the bitmap words of at a time: 64 lanes x 32 bits
constexpr int kTermAutoItems = 1024;                  // workgroups the automatic plan aims at (4 a CU)

struct TermPlan {
    int32_t regime = 0;               // 0 = one LDS histogram of all columns per workgroup, 1 = global atomics
    int64_t chunks = 1, rows_per_chunk = kTermSpanRows;
};

// The plan rule: pure host arithmetic.  n_rows: the rows of the index (bitmap driven) or the entries of a query's id list (id-list driven).
inline int term_plan(int64_t n_rows, int32_t B, int32_t n_cols, bool per_query, int64_t rows_per_chunk, TermPlan* out, char* msg, size_t cap) {
    if (n_rows < 1 || n_rows > kTermMaxRows) return snprintf(msg, cap, "n_rows must be in 1..2^32 - 1 (got %lld)", (long long)n_rows), VS_EINVAL;
    if (B < 1) return snprintf(msg, cap, "B must be positive (got %d)", B), VS_EINVAL;
    if (n_cols < 1 || n_cols > kTermMaxCols) return snprintf(msg, cap, "n_cols must be in 1..%d (got %d)", kTermMaxCols, n_cols), VS_EINVAL;
    if (!per_query && B > 1) return snprintf(msg, cap, "one set for all queries (ld_words = 0) takes B = 1, got B = %d", B), VS_EINVAL;
    if (rows_per_chunk < 0 || rows_per_chunk % 64 != 0 || rows_per_chunk > kTermMaxRows)
        return snprintf(msg, cap, "rows_per_chunk must be 0 (automatic) or a positive multiple of 64 below 2^32 (got %lld)", (long long)rows_per_chunk),
               VS_EINVAL;
    TermPlan p;
    p.regime = n_cols > VS_TERM_LDS_COLS ? 1 : 0;
    if (rows_per_chunk == 0) {
        // a few workgroups per CU over the batch; a chunk is at least one span, so zeroing and flushing the histogram (n_cols bins) stays
        // small against the cells of the chunk's rows
        const int64_t want = std::max<int64_t>(1, kTermAutoItems / B);
        rows_per_chunk = std::max<int64_t>((n_rows + want - 1) / want, kTermSpanRows);
        rows_per_chunk = (rows_per_chunk + kTermSpanRows - 1) / kTermSpanRows * kTermSpanRows;
    }
    p.rows_per_chunk = rows_per_chunk;
    p.chunks = (n_rows + rows_per_chunk - 1) / rows_per_chunk;
    if (p.chunks > 0x7FFFFFFF / B)                                                // (one work item a chunk and query: a 1-D grid of 31 bits)
        return snprintf(msg, cap, "%lld chunks x %d queries are too many for one call", (long long)p.chunks, B), VS_EINVAL;
    *out = p;
    return VS_OK;
}

// vs_index_term_counts: the bitmap's geometry and the outputs (n_rows, n_cols: the index's)
inline int term_check_counts(bool have_words, int64_t bit0, int64_t ld_words, int32_t B, int64_t n_rows, int32_t n_cols, int64_t rows_per_chunk,
                             bool have_outputs, int64_t ld_counts, TermPlan* plan, char* msg, size_t cap) {
    if (!have_outputs) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    if (bit0 < 0) return snprintf(msg, cap, "bit0 must be >= 0 (got %lld)", (long long)bit0), VS_EINVAL;
    const bool per_query = have_words && ld_words != 0;
    const int rc = term_plan(n_rows, B, n_cols, per_query, rows_per_chunk, plan, msg, cap);
    if (rc != VS_OK) return rc;
    const int64_t span = (bit0 + n_rows + 31) >> 5;
    if (have_words && (ld_words < 0 || (ld_words > 0 && ld_words < span)))
        return snprintf(msg, cap, "ld_words = %lld is shorter than the %lld words a query's bitmap spans", (long long)ld_words, (long long)span), VS_EINVAL;
    if (ld_counts < n_cols) return snprintf(msg, cap, "ld_counts = %lld is shorter than n_cols = %d", (long long)ld_counts, n_cols), VS_EINVAL;
    return VS_OK;
}

// vs_index_term_counts_ids: the list's geometry and the outputs; the plan is taken over the m entries of a query
inline int term_check_ids(bool have_ids, int32_t B, int64_t m, int64_t ld, int32_t n_cols, bool have_outputs, int64_t ld_counts, TermPlan* plan,
                          char* msg, size_t cap) {
    if (!have_ids || !have_outputs) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    if (m < 1 || m > kTermMaxRows) return snprintf(msg, cap, "m must be in 1..2^32 - 1 entries a query (got %lld)", (long long)m), VS_EINVAL;
    if (ld < m) return snprintf(msg, cap, "ld = %lld is shorter than m = %lld", (long long)ld, (long long)m), VS_EINVAL;
    const int rc = term_plan(m, B, n_cols, true, 0, plan, msg, cap);
    if (rc != VS_OK) return rc;
    if (ld_counts < n_cols) return snprintf(msg, cap, "ld_counts = %lld is shorter than n_cols = %d", (long long)ld_counts, n_cols), VS_EINVAL;
    return VS_OK;
}

// a host id list under strict = 1: every id is -1 or names a row of the index.  Reads ids [(B - 1) * ld + m] and nothing behind them.
inline int term_check_ids_host(const int64_t* ids, int32_t B, int64_t m, int64_t ld, int64_t id_offset, int64_t n_rows, char* msg, size_t cap) {
    for (int32_t b = 0; b < B; ++b)
        for (int64_t j = 0; j < m; ++j) {
            const int64_t id = ids[(size_t)b * (size_t)ld + (size_t)j];
            if (id == -1) continue;
            const uint64_t row = (uint64_t)id - (uint64_t)id_offset;               // (unsigned: no overflow at the ends of int64; the kernel's test)
            if (id < id_offset || row >= (uint64_t)n_rows)
                return snprintf(msg, cap, "id %lld (query %d, position %lld) is outside the index: %lld rows from id %lld on", (long long)id, b,
                                (long long)j, (long long)n_rows, (long long)id_offset), VS_EINVAL;
        }
    return VS_OK;
}

// vs_term_topn
inline int term_check_topn(bool have_pointers, int32_t B, int32_t n_cols, int64_t ld_counts, int32_t n, int method, char* msg, size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    if (B < 1) return snprintf(msg, cap, "B must be positive (got %d)", B), VS_EINVAL;
    if (n_cols < 1 || n_cols > kTermMaxCols) return snprintf(msg, cap, "n_cols must be in 1..%d (got %d)", kTermMaxCols, n_cols), VS_EINVAL;
    if (n < 1 || n > VS_TERM_MAX_TOPN) return snprintf(msg, cap, "n must be in 1..%d (got %d)", VS_TERM_MAX_TOPN, n), VS_EINVAL;
    if (ld_counts < n_cols) return snprintf(msg, cap, "ld_counts = %lld is shorter than n_cols = %d", (long long)ld_counts, n_cols), VS_EINVAL;
    if (method != VS_TERM_LIFT && method != VS_TERM_JLH)
        return snprintf(msg, cap, "method must be VS_TERM_LIFT or VS_TERM_JLH (got %d)", method), VS_EINVAL;
    return VS_OK;
}

}  // namespace vs
