// facet_quantile_check.h -- the host-only part of the per-label percentiles (vs_facet_value_quantile_plan, vs_facet_value_quantiles,
// vs_facet_value_radix_counts and their vs_index_* variants): the plan rule, the limits and the argument checks.  The digits, the
// rank rule and the searches are quantile_check.h's, the label limits facet_value_check.h's.  Plain C++ with no HIP in it, so that the
// stand-alone check (facet_quantile_check_main.cpp, built under the host sanitizers by tests/test_facet_quantile_cpu.py) runs the very code.
#pragma once

#include "facet_value_check.h"
#include "quantile_check.h"

namespace vs {

constexpr int64_t kFqLdsBytes = 128 * 1024;           // the histograms of a workgroup, as the percentiles: 16 of 2048 uint32 bins
constexpr int kFqMaxCells = 32;                       // (query, label) cells a workgroup holds at most: level 2, R = 1 (1024 bins a slot)
// Label tiles the LDS regime takes at most (VS_FACET_QUANTILE_MAX_LABEL_TILES = 16).  A label tile walks the bitmaps and reads the labels of
// the whole chunk again, so T tiles read the labels T times where the global regime reads them once and pays one 64-bit atomic a counted row
// instead.  Measured (tools/probe_facet_quantiles.py --ours-only on a build of either regime; 21 M rows, every row set, B = 1, random labels;
// DESIGN.md 3.1t): a tile pass costs 0.06 ms, a global level 0.5 ms (uniform float32, 256 labels or more) to 5 ms (years, 32 labels: every row
// of a label on one address).  The two builds meet at 8 tiles a level on the uniform field (L = 128, R = 1: 2.33 against 2.29 ms) and at 16
// on years (L = 256, R = 1: 3.85 against 3.60 ms); 16 costs the uniform field up to 1.75 times between 129 and 256 labels, 8 would cost years
// twice at 32 labels and 7 ranks.
// make EXTRA=-DVS_FQ_MAX_LABEL_TILES=0 takes the LDS regime out beyond one tile, =65535 the global regime (the A/B builds).
#ifndef VS_FQ_MAX_LABEL_TILES
#define VS_FQ_MAX_LABEL_TILES VS_FACET_QUANTILE_MAX_LABEL_TILES
#endif
static_assert(VS_FQ_MAX_LABEL_TILES >= 0 && VS_FQ_MAX_LABEL_TILES <= 65535, "the label tiles are the grid's z dimension");

struct FacetQuantilePlan {
    int32_t regime = 0, qt = 1;       // regime: 0 = LDS histograms, 1 = global atomics; qt: queries a workgroup serves
    int32_t tile_labels = 1, label_tiles = 1;         // labels of a workgroup's tile, tiles (global regime: n_labels, 1)
    int64_t chunks = 1, rows_per_chunk = kSpanRows;
};

// (query, label) cells whose histograms fit a workgroup's LDS at a level: 16 at level 0, 16 / R at level 1, 32 / R at level 2
inline int32_t facet_quantile_lds_cells(int32_t R, int level) {
    return (int32_t)(kFqLdsBytes / ((int64_t)(level == 0 ? 1 : R) * radix_bins(level) * 4));
}
inline size_t facet_quantile_lds_bytes(const FacetQuantilePlan& p, int32_t R, int level) {
    return p.regime ? 0 : (size_t)p.qt * (size_t)p.tile_labels * (size_t)(level == 0 ? 1 : R) * (size_t)radix_bins(level) * 4;
}
inline int facet_quantile_check_scratch(int32_t B, int32_t n_labels, int32_t R, char* msg, size_t cap) {
    if ((int64_t)B * n_labels * R * VS_VALUE_RADIX_BINS > kValueMaxScratchKeys)
        return snprintf(msg, cap, "%d queries x %d labels x %d ranks x %d bins are more than 2^27 counts: take fewer queries or ranks a call", B,
                        n_labels, R, VS_VALUE_RADIX_BINS), VS_EINVAL;
    return VS_OK;
}

// The rule.  cap = facet_quantile_lds_cells(R, level).  A workgroup serves qt queries x tile_labels labels, qt x tile_labels <= cap; qt is the
// power of two in 1..8 (1 for a shared bitmap) that needs the fewest passes over the rows, ceil(B / qt) x ceil(n_labels / tile_labels) with
// tile_labels = min(n_labels, cap / qt), among those with at most VS_FQ_MAX_LABEL_TILES label tiles; of equal ones the smallest qt.  None:
// the global regime, qt = 8 (1 for a shared bitmap), one "tile" of all labels.  Chunks by value_plan's rule over qtiles x label tiles items.
inline int facet_quantile_plan(int64_t n_rows, int32_t B, int32_t n_labels, int32_t R, int level, bool per_query, int64_t rows_per_chunk,
                               FacetQuantilePlan* out, char* msg, size_t cap) {
    int rc = check_n_rows(n_rows, msg, cap);
    if (rc == VS_OK) rc = check_batch(B, msg, cap);
    if (rc != VS_OK) return rc;
    if (n_labels < 1) return snprintf(msg, cap, "n_labels must be at least 1 (got %d)", n_labels), VS_EINVAL;
    if ((int64_t)B * n_labels > 0x7FFFFFFFll)
        return snprintf(msg, cap, "B x n_labels = %lld is more than 2^31 - 1 (query, label) cells", (long long)B * n_labels), VS_EINVAL;
    rc = quantile_check_ranks(R, msg, cap);
    if (rc == VS_OK) rc = quantile_check_level(level, msg, cap);
    if (rc == VS_OK) rc = check_chunking(per_query, B, rows_per_chunk, "bitmap", msg, cap);
    if (rc != VS_OK) return rc;
    const int32_t cells = facet_quantile_lds_cells(R, level);
    FacetQuantilePlan p;
    int64_t best = -1;
    for (int32_t qt = 1; qt <= (per_query ? 8 : 1) && qt <= cells; qt <<= 1) {
        const int32_t tl = std::min<int32_t>(n_labels, cells / qt);
        const int64_t lt = ((int64_t)n_labels + tl - 1) / tl;
        if (lt > std::max(1, VS_FQ_MAX_LABEL_TILES)) continue;
        const int64_t passes = (((int64_t)B + qt - 1) / qt) * lt;
        if (best < 0 || passes < best) {
            best = passes;
            p.qt = qt;
            p.tile_labels = tl;
            p.label_tiles = (int32_t)lt;
        }
    }
    if (best < 0) {
        p.regime = 1;
        p.qt = per_query ? 8 : 1;
        p.tile_labels = n_labels;
        p.label_tiles = 1;
    }
    const int64_t qtiles = ((int64_t)B + p.qt - 1) / p.qt;
    if (rows_per_chunk == 0) rows_per_chunk = auto_chunk(n_rows, qtiles * p.label_tiles, kMinChunk);
    p.rows_per_chunk = rows_per_chunk;
    p.chunks = (n_rows + rows_per_chunk - 1) / rows_per_chunk;
    if (p.chunks > 0x7FFFFFFF || qtiles > 65535)
        return snprintf(msg, cap, "%lld chunks x %d queries are too many for one call", (long long)p.chunks, B), VS_EINVAL;
    *out = p;
    return VS_OK;
}

// the set of either call: the pointers, the dtype, the bitmap's geometry, the plan of `level` and the 2^27 rule
inline int facet_quantile_check_set(bool have_pointers, bool have_words, int64_t bit0, int64_t ld_words, int32_t B, int dtype, int64_t n_rows,
                                    int32_t n_labels, int32_t R, int level, int64_t rows_per_chunk, FacetQuantilePlan* plan, char* msg, size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    int rc = value_check_dtype(dtype, msg, cap);
    if (rc == VS_OK) rc = check_bit0(bit0, msg, cap);
    if (rc == VS_OK) rc = facet_quantile_plan(n_rows, B, n_labels, R, level, have_words && ld_words != 0, rows_per_chunk, plan, msg, cap);
    if (rc == VS_OK) rc = check_ld_words(have_words, bit0, ld_words, n_rows, msg, cap);
    if (rc == VS_OK) rc = facet_quantile_check_scratch(B, n_labels, R, msg, cap);
    return rc;
}

// what a level's counting call needs besides the set
inline int facet_quantile_check_level_args(int level, bool have_state, bool have_level0, char* msg, size_t cap) {
    const int rc = quantile_check_level(level, msg, cap);
    if (rc != VS_OK) return rc;
    if (level == 0 ? !have_level0 : !have_state)
        return snprintf(msg, cap, "NULL argument: level %d needs %s", level, level == 0 ? "missing, total and other" : "slot_prefix and n_slots"), VS_EINVAL;
    return VS_OK;
}

}  // namespace vs
