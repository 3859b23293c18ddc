// term_sum_check.h -- the plan rule and the argument checks of the term sums (vs_term_sum_plan, vs_index_term_sums, vs_index_term_sums_ids,
// vs_term_sum_topn) that need no device: column tiles, chunks, sizes and strides -- and term_fx, the fixed-point image of a value, which the kernel and
// the stand-alone check share.  A host id list is checked by term_check_ids_host of
// term_agg_check.h, whose limits (rows, columns, span, the automatic plan's aim) hold here as well.
// What every aggregation over a row set checks alike (rows, batch, chunking, bitmap and id-list geometry, auto_chunk) is set_check.h's.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_term_sum_cpu.py builds one).
#pragma once

#include "term_agg_check.h"

namespace vs {

#if defined(__HIPCC__)
#define VS_TERM_HD __host__ __device__
#else
#define VS_TERM_HD
#endif

// The fixed-point image of a stored value, fx(v) = llrint(double(clamp(v, -2^20, +2^20)) * 2^24) with NaN -> 0, as the bits of an int64.
// x = double(c) * 2^24 is exact (a power of two, no underflow in fp64) and |x| <= 2^44.  Adding 1.5 * 2^52 rounds x to an integer, to nearest
// even -- the one rounding of the chain, llrint's -- and leaves it in the low mantissa bits: the sum lies in [2^52, 2^53), where doubles are the
// integers, so its bits minus the bits of 1.5 * 2^52 are the integer itself, sign included.  The product being exact, the fma rounds once,
// exactly as a separate multiplication and addition would.  7 instructions a cell on the device instead of the 14 of rint and a conversion.
static_assert(VS_TERM_FX_SHIFT == 24 && VS_TERM_FX_CLAMP_LOG2 == 20, "term_fx spells the two constants out");
VS_TERM_HD inline uint64_t term_fx(float v) {
    if (v != v) return 0;                                                         // NaN adds nothing
    const float c = v < -1048576.0f ? -1048576.0f : (v > 1048576.0f ? 1048576.0f : v);
    const double d = __builtin_fma((double)c, 16777216.0, 6755399441055744.0);
    uint64_t bits;
    __builtin_memcpy(&bits, &d, sizeof bits);
    return bits - 0x4338000000000000ull;                                          // (the bits of 1.5 * 2^52)
}

struct TermSumPlan {
    int32_t tiles = 1, tile_cols = 1;  // column tile t holds columns [t * tile_cols, min(n_cols, (t + 1) * tile_cols)): never empty
    int64_t chunks = 1, rows_per_chunk = kSpanRows;
};

// The plan rule: pure host arithmetic.  n_rows: the rows of the index (bitmap driven) or the entries of a query's id list (id-list driven).
inline int term_sum_plan(int64_t n_rows, int32_t B, int32_t n_cols, bool per_query, int64_t rows_per_chunk, int32_t tile_cols, TermSumPlan* out,
                         char* msg, size_t cap) {
    const int rc = check_term_set(n_rows, B, n_cols, per_query, rows_per_chunk, msg, cap);
    if (rc != VS_OK) return rc;
    if (tile_cols < 0 || tile_cols > VS_TERM_SUM_TILE_COLS)
        return snprintf(msg, cap, "tile_cols must be 0 (automatic) or in 1..%d (got %d)", VS_TERM_SUM_TILE_COLS, tile_cols), VS_EINVAL;
    TermSumPlan p;
    if (tile_cols == 0) {                                                         // as few tiles as fit the LDS, balanced
        p.tiles = (n_cols + VS_TERM_SUM_TILE_COLS - 1) / VS_TERM_SUM_TILE_COLS;
        p.tile_cols = (n_cols + p.tiles - 1) / p.tiles;
    } else {                                                                      // taken as given (more columns than the index has: one tile)
        p.tile_cols = tile_cols;
        p.tiles = (n_cols + tile_cols - 1) / tile_cols;
    }
    const int64_t items = (int64_t)B * p.tiles;                                   // work items a chunk
    p.rows_per_chunk = rows_per_chunk ? rows_per_chunk : auto_chunk(n_rows, items);
    p.chunks = (n_rows + p.rows_per_chunk - 1) / p.rows_per_chunk;
    if (p.chunks > 0x7FFFFFFF / items)                                            // (one work item a chunk, query and tile: a 1-D grid of 31 bits)
        return snprintf(msg, cap, "%lld chunks x %d queries x %d column tiles are too many for one call", (long long)p.chunks, B, p.tiles), VS_EINVAL;
    *out = p;
    return VS_OK;
}

// vs_index_term_sums: the bitmap's geometry and the outputs (n_rows, n_cols: the index's)
inline int term_sum_check_sums(bool have_words, int64_t bit0, int64_t ld_words, int32_t B, int64_t n_rows, int32_t n_cols, int64_t rows_per_chunk,
                               int32_t tile_cols, bool have_outputs, int64_t ld_sums, TermSumPlan* plan, char* msg, size_t cap) {
    return check_bitmap_call(have_words, bit0, ld_words, n_rows, n_cols, have_outputs, ld_sums, "sums",
                             [&](bool per_query) { return term_sum_plan(n_rows, B, n_cols, per_query, rows_per_chunk, tile_cols, plan, msg, cap); },
                             msg, cap);
}

// vs_index_term_sums_ids: the list's geometry and the outputs; the plan is taken over the m entries of a query
inline int term_sum_check_ids(bool have_ids, int32_t B, int64_t m, int64_t ld, int32_t n_cols, int32_t tile_cols, bool have_outputs, int64_t ld_sums,
                              TermSumPlan* plan, char* msg, size_t cap) {
    return check_ids_call(have_ids, m, ld, n_cols, have_outputs, ld_sums, "sums",
                          [&] { return term_sum_plan(m, B, n_cols, true, 0, tile_cols, plan, msg, cap); }, msg, cap);
}

// vs_term_sum_topn (counts may be absent: then ld_counts is not looked at)
inline int term_sum_check_topn(bool have_pointers, bool have_counts, int32_t B, int32_t n_cols, int64_t ld_sums, int64_t ld_counts, int32_t n,
                               char* msg, size_t cap) {
    int rc = check_term_topn(have_pointers, B, n_cols, n, msg, cap);
    if (rc == VS_OK) rc = check_ld_out(ld_sums, n_cols, "sums", msg, cap);
    if (rc == VS_OK && have_counts) rc = check_ld_out(ld_counts, n_cols, "counts", msg, cap);
    return rc;
}

}  // namespace vs
