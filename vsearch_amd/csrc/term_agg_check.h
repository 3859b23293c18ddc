// term_agg_check.h -- the plan rule and the argument checks of the term aggregations (vs_term_plan, vs_index_term_counts,
// vs_index_term_counts_ids, vs_term_topn) that need no device: sizes and strides, and a host id list before it is staged.
// What every aggregation over a row set checks alike (rows, batch, chunking, bitmap and id-list geometry, auto_chunk) is set_check.h's.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_term_agg_cpu.py builds one).
#pragma once

#include "set_check.h"

namespace vs {

constexpr int64_t kTermMaxRows = kSetMaxRows;         // (the names the stand-alone check programs and assign_check.h use)
constexpr int kTermSpanRows = kSpanRows;

struct TermPlan {
    int32_t regime = 0;               // 0 = one LDS histogram of all columns per workgroup, 1 = global atomics
    int64_t chunks = 1, rows_per_chunk = kSpanRows;
};

// The plan rule: pure host arithmetic.  n_rows: the rows of the index (bitmap driven) or the entries of a query's id list (id-list driven).
inline int term_plan(int64_t n_rows, int32_t B, int32_t n_cols, bool per_query, int64_t rows_per_chunk, TermPlan* out, char* msg, size_t cap) {
    const int rc = check_term_set(n_rows, B, n_cols, per_query, rows_per_chunk, msg, cap);
    if (rc != VS_OK) return rc;
    TermPlan p;
    p.regime = n_cols > VS_TERM_LDS_COLS ? 1 : 0;
    p.rows_per_chunk = rows_per_chunk ? rows_per_chunk : auto_chunk(n_rows, B);
    p.chunks = (n_rows + p.rows_per_chunk - 1) / p.rows_per_chunk;
    if (p.chunks > 0x7FFFFFFF / B)                                                // (one work item a chunk and query: a 1-D grid of 31 bits)
        return snprintf(msg, cap, "%lld chunks x %d queries are too many for one call", (long long)p.chunks, B), VS_EINVAL;
    *out = p;
    return VS_OK;
}

// vs_index_term_counts: the bitmap's geometry and the outputs (n_rows, n_cols: the index's)
inline int term_check_counts(bool have_words, int64_t bit0, int64_t ld_words, int32_t B, int64_t n_rows, int32_t n_cols, int64_t rows_per_chunk,
                             bool have_outputs, int64_t ld_counts, TermPlan* plan, char* msg, size_t cap) {
    return check_bitmap_call(have_words, bit0, ld_words, n_rows, n_cols, have_outputs, ld_counts, "counts",
                             [&](bool per_query) { return term_plan(n_rows, B, n_cols, per_query, rows_per_chunk, plan, msg, cap); }, msg, cap);
}

// vs_index_term_counts_ids: the list's geometry and the outputs; the plan is taken over the m entries of a query
inline int term_check_ids(bool have_ids, int32_t B, int64_t m, int64_t ld, int32_t n_cols, bool have_outputs, int64_t ld_counts, TermPlan* plan,
                          char* msg, size_t cap) {
    return check_ids_call(have_ids, m, ld, n_cols, have_outputs, ld_counts, "counts",
                          [&] { return term_plan(m, B, n_cols, true, 0, plan, msg, cap); }, msg, cap);
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
    int rc = check_term_topn(have_pointers, B, n_cols, n, msg, cap);
    if (rc == VS_OK) rc = check_ld_out(ld_counts, n_cols, "counts", msg, cap);
    if (rc != VS_OK) return rc;
    if (method != VS_TERM_LIFT && method != VS_TERM_JLH)
        return snprintf(msg, cap, "method must be VS_TERM_LIFT or VS_TERM_JLH (got %d)", method), VS_EINVAL;
    return VS_OK;
}

}  // namespace vs
