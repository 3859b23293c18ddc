// facet_value_check.h -- the plan rule, the limits and the argument checks of the breakdowns (vs_facet_value_plan, vs_facet_value_stats,
// vs_facet_value_histogram and their vs_index_* variants) that need no device.  A breakdown is a numeric field's stats or
// histogram per facet label: the set and the chunking are checked by set_check.h, the automatic chunk included; the dtype and the edges are
// value_check.h's.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_facet_value_cpu.py builds one).
#pragma once

#include "set_check.h"
#include "value_check.h"

namespace vs {

static_assert(VS_FACET_VALUE_LDS_RECORDS * 24 <= 48 * 1024, "a record is 24 bytes: sum 8, count, missing, min key, max key 4 each");
static_assert((int64_t)VS_FACET_LDS_BINS * 4 + (int64_t)VS_VALUE_MAX_EDGES * 4 + 256 <= 160 * 1024, "the bins, the edge keys and the counters fit a CU's LDS");

struct FacetValuePlan {
    int32_t regime = 0, qt = 1;       // regime: 0 = LDS records / bins, 1 = global atomics; qt: queries a workgroup serves
    int64_t chunks = 1, rows_per_chunk = kSpanRows;
    int64_t lds_slots = 0;            // the LDS records (stats) or bins (histogram) a query takes; 0 in the global regime
};

// n_slots: 0 = stats (a query takes n_labels records), n_edges + 2 = histogram (a query takes n_labels x n_slots bins)
inline int facet_value_plan(int64_t n_rows, int32_t B, int32_t n_labels, int32_t n_slots, bool per_query, int64_t rows_per_chunk, FacetValuePlan* out,
                            char* msg, size_t cap) {
    int rc = check_n_rows(n_rows, msg, cap);
    if (rc == VS_OK) rc = check_batch(B, msg, cap);
    if (rc != VS_OK) return rc;
    if (n_labels < 1) return snprintf(msg, cap, "n_labels must be at least 1 (got %d)", n_labels), VS_EINVAL;
    if (n_slots != 0 && (n_slots < 4 || n_slots > VS_VALUE_MAX_EDGES + 2))
        return snprintf(msg, cap, "n_slots must be 0 (stats) or n_edges + 2 in 4..%d (got %d)", VS_VALUE_MAX_EDGES + 2, n_slots), VS_EINVAL;
    const int64_t cells = (int64_t)n_labels * (n_slots ? n_slots : 1);         // a query's records / bins
    if (n_slots != 0 && cells > VS_FACET_VALUE_MAX_CELLS)
        return snprintf(msg, cap, "n_labels x (n_edges + 2) = %lld is more than the %d cells a query takes", (long long)cells, VS_FACET_VALUE_MAX_CELLS),
               VS_EINVAL;
    if ((int64_t)B * n_labels > 0x7FFFFFFFll)
        return snprintf(msg, cap, "B x n_labels = %lld is more than 2^31 - 1 (query, label) cells", (long long)B * n_labels), VS_EINVAL;
    rc = check_chunking(per_query, B, rows_per_chunk, "bitmap", msg, cap);
    if (rc != VS_OK) return rc;
    const int64_t lds_cap = n_slots ? VS_FACET_LDS_BINS : VS_FACET_VALUE_LDS_RECORDS;
    FacetValuePlan p;
    p.regime = cells > lds_cap ? 1 : 0;
    p.qt = per_query ? 8 : 1;                                     // (global regime: the tile only shares the loads)
    if (!p.regime)
        while (p.qt > 1 && (int64_t)p.qt * cells > lds_cap) p.qt >>= 1;
    p.lds_slots = p.regime ? 0 : cells;
    const int64_t tiles = (B + p.qt - 1) / p.qt;
    // value_plan's rule: enough workgroups to fill the chip, chunks long enough that zeroing and flushing the LDS stays a sixteenth of the walk
    if (rows_per_chunk == 0) rows_per_chunk = auto_chunk(n_rows, tiles, std::max<int64_t>(kMinChunk, (int64_t)16 * p.lds_slots));
    p.rows_per_chunk = rows_per_chunk;
    p.chunks = (n_rows + rows_per_chunk - 1) / rows_per_chunk;
    if (p.chunks > 0x7FFFFFFF || tiles > 65535)
        return snprintf(msg, cap, "%lld chunks x %d queries are too many for one call", (long long)p.chunks, B), VS_EINVAL;
    *out = p;
    return VS_OK;
}

// the set of either call: the pointers, the dtype, the bitmap's geometry, and the plan
inline int facet_value_check_set(bool have_pointers, bool have_words, int64_t bit0, int64_t ld_words, int32_t B, int dtype, int64_t n_rows,
                                 int32_t n_labels, int32_t n_slots, int64_t rows_per_chunk, FacetValuePlan* plan, char* msg, size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    int rc = value_check_dtype(dtype, msg, cap);
    if (rc == VS_OK) rc = check_bit0(bit0, msg, cap);
    if (rc == VS_OK) rc = facet_value_plan(n_rows, B, n_labels, n_slots, have_words && ld_words != 0, rows_per_chunk, plan, msg, cap);
    if (rc == VS_OK) rc = check_ld_words(have_words, bit0, ld_words, n_rows, msg, cap);
    return rc;
}

// vs_facet_value_stats: the set and the stride of the five [B, ld_out] matrices
inline int facet_value_check_stats(bool have_pointers, bool have_words, int64_t bit0, int64_t ld_words, int32_t B, int dtype, int64_t n_rows,
                                   int32_t n_labels, int64_t rows_per_chunk, int64_t ld_out, FacetValuePlan* plan, char* msg, size_t cap) {
    const int rc = facet_value_check_set(have_pointers, have_words, bit0, ld_words, B, dtype, n_rows, n_labels, 0, rows_per_chunk, plan, msg, cap);
    if (rc != VS_OK) return rc;
    if (ld_out < n_labels) return snprintf(msg, cap, "ld_out = %lld is shorter than n_labels = %d", (long long)ld_out, n_labels), VS_EINVAL;
    return VS_OK;
}

// vs_facet_value_histogram: the edge count and the stride of counts (value_check_hist), then the set (a host edges array: value_check_edges_host)
inline int facet_value_check_hist(bool have_pointers, bool have_words, int64_t bit0, int64_t ld_words, int32_t B, int dtype, int64_t n_rows,
                                  int32_t n_labels, int32_t n_edges, int64_t rows_per_chunk, int64_t ld_counts, FacetValuePlan* plan, char* msg,
                                  size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    const int rc = value_check_hist(n_edges, ld_counts, msg, cap);
    if (rc != VS_OK) return rc;
    return facet_value_check_set(true, have_words, bit0, ld_words, B, dtype, n_rows, n_labels, n_edges + 2, rows_per_chunk, plan, msg, cap);
}

}  // namespace vs
