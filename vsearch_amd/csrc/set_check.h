// set_check.h -- the argument checks every aggregation over a row set repeats (facets, term counts, term sums, numeric fields): the rows and the
// batch, one set or one per query, the chunking, the geometry of a bitmap or of id lists, the stride of an output -- and the automatic-chunk rule
// of them all.  Every function writes its message into msg and returns a VS_* code.
// Plain C++ with no HIP in it, so that the stand-alone check programs build with a host compiler.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "vsearch_hip.h"

namespace vs {

constexpr int kSpanRows = 2048;                       // rows a wave loads the bitmap words of at a time: 64 lanes x 32 bits (set_walk.h)
constexpr int64_t kSetMaxRows = 0xFFFFFFFFll;         // a chunk's count fits a uint32 bin
constexpr int32_t kTermMaxCols = 65535;               // the packets hold uint16 column ids; n_cols itself is the padding id
constexpr int kAutoItems = 1024;                      // workgroups an automatic plan aims at (4 a CU)
constexpr int64_t kMinChunk = 8192;                   // rows of an automatic chunk at least, where a workgroup keeps bins per label or per value

inline int check_n_rows(int64_t n_rows, char* msg, size_t cap) {
    if (n_rows < 1 || n_rows > kSetMaxRows) return snprintf(msg, cap, "n_rows must be in 1..2^32 - 1 (got %lld)", (long long)n_rows), VS_EINVAL;
    return VS_OK;
}
inline int check_batch(int32_t B, char* msg, size_t cap) {
    if (B < 1) return snprintf(msg, cap, "B must be positive (got %d)", B), VS_EINVAL;
    return VS_OK;
}
inline int check_n_cols(int32_t n_cols, char* msg, size_t cap) {
    if (n_cols < 1 || n_cols > kTermMaxCols) return snprintf(msg, cap, "n_cols must be in 1..%d (got %d)", kTermMaxCols, n_cols), VS_EINVAL;
    return VS_OK;
}
// one set serves one query; what: how the call names its set ("bitmap" | "set")
inline int check_chunking(bool per_query, int32_t B, int64_t rows_per_chunk, const char* what, char* msg, size_t cap) {
    if (!per_query && B > 1) return snprintf(msg, cap, "one %s for all queries (ld_words = 0) takes B = 1, got B = %d", what, B), VS_EINVAL;
    if (rows_per_chunk < 0 || rows_per_chunk % 64 != 0 || rows_per_chunk > kSetMaxRows)
        return snprintf(msg, cap, "rows_per_chunk must be 0 (automatic) or a positive multiple of 64 below 2^32 (got %lld)", (long long)rows_per_chunk),
               VS_EINVAL;
    return VS_OK;
}
// the rows, the batch, the columns and the chunking of a term aggregation, in the order the calls report them
inline int check_term_set(int64_t n_rows, int32_t B, int32_t n_cols, bool per_query, int64_t rows_per_chunk, char* msg, size_t cap) {
    int rc = check_n_rows(n_rows, msg, cap);
    if (rc == VS_OK) rc = check_batch(B, msg, cap);
    if (rc == VS_OK) rc = check_n_cols(n_cols, msg, cap);
    if (rc == VS_OK) rc = check_chunking(per_query, B, rows_per_chunk, "set", msg, cap);
    return rc;
}

// The automatic chunk over `items` work items a chunk: a few workgroups per CU over the batch; a chunk is at least floor_rows rows (the term
// aggregations: one span; the others: kMinChunk, or 16 rows a bin a workgroup keeps), so zeroing and flushing a workgroup's bins stays small
// against the work of the chunk's rows; whole spans.
inline int64_t auto_chunk(int64_t n_rows, int64_t items, int64_t floor_rows = kSpanRows) {
    const int64_t want = std::max<int64_t>(1, kAutoItems / items);
    const int64_t rows = std::max<int64_t>((n_rows + want - 1) / want, floor_rows);
    return (rows + kSpanRows - 1) / kSpanRows * kSpanRows;
}

inline int check_bit0(int64_t bit0, char* msg, size_t cap) {
    if (bit0 < 0) return snprintf(msg, cap, "bit0 must be >= 0 (got %lld)", (long long)bit0), VS_EINVAL;
    return VS_OK;
}
// ld_words = 0: one bitmap for all queries
inline int check_ld_words(bool have_words, int64_t bit0, int64_t ld_words, int64_t n_rows, char* msg, size_t cap) {
    const int64_t span = (bit0 + n_rows + 31) >> 5;
    if (have_words && (ld_words < 0 || (ld_words > 0 && ld_words < span)))
        return snprintf(msg, cap, "ld_words = %lld is shorter than the %lld words a query's bitmap spans", (long long)ld_words, (long long)span), VS_EINVAL;
    return VS_OK;
}
// the stride of a [B, n_cols] output; out: its name ("counts" | "sums")
inline int check_ld_out(int64_t ld, int32_t n_cols, const char* out, char* msg, size_t cap) {
    if (ld < n_cols) return snprintf(msg, cap, "ld_%s = %lld is shorter than n_cols = %d", out, (long long)ld, n_cols), VS_EINVAL;
    return VS_OK;
}

// A bitmap-driven call over an index: the bitmap's geometry and the output's stride around the call's plan rule, plan(per_query) -> code.
template <class PlanFn>
inline int check_bitmap_call(bool have_words, int64_t bit0, int64_t ld_words, int64_t n_rows, int32_t n_cols, bool have_outputs, int64_t ld_out,
                             const char* out, PlanFn plan, char* msg, size_t cap) {
    if (!have_outputs) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    int rc = check_bit0(bit0, msg, cap);
    if (rc == VS_OK) rc = plan(have_words && ld_words != 0);
    if (rc == VS_OK) rc = check_ld_words(have_words, bit0, ld_words, n_rows, msg, cap);
    if (rc == VS_OK) rc = check_ld_out(ld_out, n_cols, out, msg, cap);
    return rc;
}

// An id-list-driven call: the lists' geometry and the output's stride around the plan rule, taken over the m entries of a query: plan() -> code.
template <class PlanFn>
inline int check_ids_call(bool have_ids, int64_t m, int64_t ld, int32_t n_cols, bool have_outputs, int64_t ld_out, const char* out, PlanFn plan,
                          char* msg, size_t cap) {
    if (!have_ids || !have_outputs) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    if (m < 1 || m > kSetMaxRows) return snprintf(msg, cap, "m must be in 1..2^32 - 1 entries a query (got %lld)", (long long)m), VS_EINVAL;
    if (ld < m) return snprintf(msg, cap, "ld = %lld is shorter than m = %lld", (long long)ld, (long long)m), VS_EINVAL;
    int rc = plan();
    if (rc == VS_OK) rc = check_ld_out(ld_out, n_cols, out, msg, cap);
    return rc;
}

// the arguments the two top-n calls of the term aggregations share
inline int check_term_topn(bool have_pointers, int32_t B, int32_t n_cols, int32_t n, char* msg, size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    int rc = check_batch(B, msg, cap);
    if (rc == VS_OK) rc = check_n_cols(n_cols, msg, cap);
    if (rc == VS_OK && (n < 1 || n > VS_TERM_MAX_TOPN)) rc = (snprintf(msg, cap, "n must be in 1..%d (got %d)", VS_TERM_MAX_TOPN, n), VS_EINVAL);
    return rc;
}

}  // namespace vs
