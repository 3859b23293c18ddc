// label_term_check.h -- the plan rule, the limits and the argument checks of the per-label term aggregations (vs_label_term_plan,
// vs_label_order, vs_index_label_term_sums, vs_index_label_term_counts) that need no device: column tiles, the rows of a work item, the item
// bound, sizes and strides.  The fixed point is term_fx of term_sum_check.h, unchanged.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_label_term_cpu.py builds one).
#pragma once

#include "term_sum_check.h"

namespace vs {

constexpr int64_t kLabelOrderMinChunk = kMinChunk;    // rows of a chunk of the label order at least (a workgroup keeps a bin a label)

struct LabelTermPlan {
    int32_t tiles = 1, tile_cols = 1;  // column tile t holds columns [t * tile_cols, min(n_cols, (t + 1) * tile_cols)): never empty
    int64_t rows_per_item = kSpanRows; // a label's rows are cut into work items of at most this many
    int64_t max_items = 1;             // the bound the grid is sized by: ceil(n_rows / rows_per_item) + n_labels >= sum over labels of ceil(cnt / R)
};

inline int check_n_labels(int32_t n_labels, char* msg, size_t cap) {
    if (n_labels < 1 || n_labels > VS_LABEL_TERM_MAX_LABELS)
        return snprintf(msg, cap, "n_labels must be in 1..%d (got %d)", VS_LABEL_TERM_MAX_LABELS, n_labels), VS_EINVAL;
    return VS_OK;
}

// The plan rule: pure host arithmetic.  The tiles are those of term_sum_plan; the automatic item follows the chunk rule over `tiles` work items
// (auto_chunk: ~ kAutoItems workgroups over the rows, an item at least one span), so that zeroing and flushing a tile stays small against
// the packets of the item's rows.  Every label adds at most one short item, hence the bound.
inline int label_term_plan(int64_t n_rows, int32_t n_labels, int32_t n_cols, int64_t rows_per_item, int32_t tile_cols, LabelTermPlan* out, char* msg,
                           size_t cap) {
    int rc = check_n_rows(n_rows, msg, cap);
    if (rc == VS_OK) rc = check_n_labels(n_labels, msg, cap);
    if (rc == VS_OK) rc = check_n_cols(n_cols, msg, cap);
    if (rc != VS_OK) return rc;
    if (rows_per_item < 0 || rows_per_item % 64 != 0 || rows_per_item > kSetMaxRows)
        return snprintf(msg, cap, "rows_per_item must be 0 (automatic) or a positive multiple of 64 below 2^32 (got %lld)", (long long)rows_per_item),
               VS_EINVAL;
    if (tile_cols < 0 || tile_cols > VS_TERM_SUM_TILE_COLS)
        return snprintf(msg, cap, "tile_cols must be 0 (automatic) or in 1..%d (got %d)", VS_TERM_SUM_TILE_COLS, tile_cols), VS_EINVAL;
    LabelTermPlan p;
    if (tile_cols == 0) {                                                         // as few tiles as fit the LDS, balanced
        p.tiles = (n_cols + VS_TERM_SUM_TILE_COLS - 1) / VS_TERM_SUM_TILE_COLS;
        p.tile_cols = (n_cols + p.tiles - 1) / p.tiles;
    } else {                                                                      // taken as given (more columns than the index has: one tile)
        p.tile_cols = tile_cols;
        p.tiles = (n_cols + tile_cols - 1) / tile_cols;
    }
    p.rows_per_item = rows_per_item ? rows_per_item : auto_chunk(n_rows, p.tiles);
    p.max_items = (n_rows + p.rows_per_item - 1) / p.rows_per_item + n_labels;
    if (p.max_items > VS_LABEL_TERM_MAX_WORK_ITEMS / p.tiles)                     // (one 1024-thread workgroup an item and tile: a launch holds fewer than 2^32 threads)
        return snprintf(msg, cap, "%lld items x %d column tiles are too many for one call (at most %d work items)", (long long)p.max_items, p.tiles,
                        VS_LABEL_TERM_MAX_WORK_ITEMS), VS_EINVAL;
    *out = p;
    return VS_OK;
}

// the rows a workgroup of the label order takes: the automatic chunk of the aggregations with the kMinChunk floor, in both regimes.  A
// floor that grows with the labels (the facet counts' 16 rows a bin, then 4) was measured and dropped: it left 16 workgroups over 1 M rows at
// 16 384 labels and made the LDS regime slower there than the global one.  Zeroing and scanning a workgroup's bins is 64 steps
// of its 256 threads at most, and it reserves at most one range a row of its chunk -- what the global regime pays for every row.
inline int64_t label_order_chunk(int64_t n_rows, int32_t n_labels) {
    (void)n_labels;
    return auto_chunk(n_rows, 1, kLabelOrderMinChunk);
}

// vs_label_order: n_rows the index's
inline int label_order_check(int64_t bit0, int64_t n_rows, bool have_labels, int32_t n_labels, bool have_outputs, char* msg, size_t cap) {
    if (!have_labels || !have_outputs) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    int rc = check_bit0(bit0, msg, cap);
    if (rc == VS_OK) rc = check_n_rows(n_rows, msg, cap);
    if (rc == VS_OK) rc = check_n_labels(n_labels, msg, cap);
    return rc;
}

// vs_index_label_term_sums / vs_index_label_term_counts: out names the matrix ("sums" | "counts"); n_rows, n_cols: the index's
inline int label_term_check(int64_t bit0, int64_t n_rows, int32_t n_cols, bool have_labels, int32_t n_labels, int64_t rows_per_item,
                            int32_t tile_cols, bool have_outputs, int64_t ld_out, const char* out, LabelTermPlan* plan, char* msg, size_t cap) {
    if (!have_labels || !have_outputs) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    int rc = check_bit0(bit0, msg, cap);
    if (rc == VS_OK) rc = label_term_plan(n_rows, n_labels, n_cols, rows_per_item, tile_cols, plan, msg, cap);
    if (rc == VS_OK) rc = check_ld_out(ld_out, n_cols, out, msg, cap);
    if (rc == VS_OK && (int64_t)n_labels * ld_out > VS_LABEL_TERM_MAX_CELLS)
        rc = (snprintf(msg, cap, "n_labels x ld_%s = %lld is more than %lld cells (1 GiB of int64)", out, (long long)((int64_t)n_labels * ld_out),
                       (long long)VS_LABEL_TERM_MAX_CELLS), VS_EINVAL);
    return rc;
}

}  // namespace vs
