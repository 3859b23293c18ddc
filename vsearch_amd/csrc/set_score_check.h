// set_score_check.h -- the plan rule and the argument checks of the scores of a document set (vs_set_score_plan, vs_index_set_scores) that need
// no device, built on set_check.h.  Every function writes its message into msg and returns a VS_* code.
// Plain C++ with no HIP in it, as set_check.h.
#pragma once

#include "set_check.h"

namespace vs {

constexpr int32_t kSetScoreMaxCols = 32763;           // the widest index whose LDS query image fits (scan_image_fits of csr_scan.h; set_scores.hip asserts it)

struct SetScorePlan {
    int64_t chunks = 1, rows_per_chunk = kSpanRows;
};

// A work item is (query, chunk of rows).  A workgroup loads the query's LDS image (4 x n_cols bytes, 118 KB at most) when its query changes, so a
// chunk must be long enough that the image is a small share of what its rows stream: the floor is auto_chunk's own, one span of 2048 rows.  At 20
// packets (160 non-zeros) a row a span streams 2 MB of an fp32 index, sixteen images; the image comes out of L2 after the first workgroup has
// read it.  A longer floor would leave CUs idle on a one-query call over a million rows (8192 rows: 123 work items for 256 CUs, 1.26 ms against 0.79), and the
// every-row scan of one query is the case the call is measured on.  Above the floor a chunk is auto_chunk's n_rows / (kAutoItems / B) rounded up
// to 64 rows, NOT to whole spans: one workgroup fits a CU, so the work items run in rounds of cu_count, and whole spans cut 21 M rows into 933
// chunks -- 3.6 rounds of 256, the last one 64 % full, measured 8 % behind the one-query range scan; 1023 chunks fill four rounds.  (The walk
// starts its spans at the chunk's first row: a chunk edge inside a span costs a short last span, nothing else.)  A shared bitmap serves any B
// here -- the queries differ, not the sets -- so per_query does not enter the rule.
inline int64_t set_score_auto_chunk(int64_t n_rows, int32_t B) {
    const int64_t want = std::max<int64_t>(1, kAutoItems / B);
    return std::max<int64_t>(kSpanRows, ((n_rows + want - 1) / want + 63) / 64 * 64);
}
inline int set_score_plan(int64_t n_rows, int32_t B, int32_t n_cols, bool /*per_query*/, int64_t rows_per_chunk, SetScorePlan* out, char* msg,
                          size_t cap) {
    int rc = check_n_rows(n_rows, msg, cap);
    if (rc == VS_OK) rc = check_batch(B, msg, cap);
    if (rc == VS_OK) rc = check_n_cols(n_cols, msg, cap);
    if (rc == VS_OK) rc = check_chunking(true, B, rows_per_chunk, "bitmap", msg, cap);
    if (rc != VS_OK) return rc;
    SetScorePlan p;
    p.rows_per_chunk = rows_per_chunk ? rows_per_chunk : set_score_auto_chunk(n_rows, B);
    p.chunks = (n_rows + p.rows_per_chunk - 1) / p.rows_per_chunk;
    if (p.chunks > 0x7FFFFFFF / (int64_t)B)
        return snprintf(msg, cap, "%lld chunks x %d queries are too many work items for one call: take longer chunks", (long long)p.chunks, B), VS_EINVAL;
    *out = p;
    return VS_OK;
}

// what vs_index_set_scores checks before it looks at the index: the pointers, the query dtype (ok: VS_F32 | VS_F16), the batch, the bitmap's first
// bit and stride sign, the chunking
inline int set_score_check_call(bool have_pointers, bool q_dtype_ok, int32_t B, int64_t bit0, int64_t ld_words, int64_t rows_per_chunk, char* msg,
                                size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    if (!q_dtype_ok) return snprintf(msg, cap, "q_dtype must be VS_F32 or VS_F16"), VS_EINVAL;
    int rc = check_batch(B, msg, cap);
    if (rc == VS_OK) rc = check_bit0(bit0, msg, cap);
    if (rc == VS_OK) rc = check_chunking(true, B, rows_per_chunk, "bitmap", msg, cap);
    if (rc == VS_OK && ld_words < 0) rc = (snprintf(msg, cap, "ld_words must be >= 0 (got %lld)", (long long)ld_words), VS_EINVAL);
    return rc;
}

// ... and what it checks against the index's shape: the query's and the output's strides, the bitmap's geometry, and the plan
inline int set_score_check_shape(int64_t n_rows, int32_t n_cols, int64_t ldq, bool have_words, int64_t bit0, int64_t ld_words, int32_t B,
                                 int64_t rows_per_chunk, int64_t ld_scores, SetScorePlan* plan, char* msg, size_t cap) {
    if (ldq < n_cols) return snprintf(msg, cap, "query has %lld columns, index has %d", (long long)ldq, n_cols), VS_EINVAL;
    if (ld_scores < n_rows) return snprintf(msg, cap, "ld_scores = %lld is shorter than n_rows = %lld", (long long)ld_scores, (long long)n_rows), VS_EINVAL;
    int rc = set_score_plan(n_rows, B, n_cols, have_words && ld_words != 0, rows_per_chunk, plan, msg, cap);
    if (rc == VS_OK) rc = check_ld_words(have_words, bit0, ld_words, n_rows, msg, cap);
    return rc;
}

}  // namespace vs
