// set_score_check_main.cpp -- stand-alone driver of set_score_check.h: the plan rule of the scores of a document set and every argument check of
// vs_index_set_scores, those against an index's shape included (a machine without a GPU has no index handle to reach them through the C ABI).
// Not part of the library: tests/test_score_field_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "set_score_check.h"

using namespace vs;

static int failures = 0;

static void expect(const char* what, int got, int want, const char* msg, const char* needle) {
    const bool ok = got == want && (want == VS_OK || strstr(msg, needle) != nullptr);
    if (!ok) {
        fprintf(stderr, "FAIL %s: code %d (want %d), message \"%s\" (want \"%s\")\n", what, got, want, msg, needle);
        ++failures;
    }
}
static void expect_true(const char* what, bool ok) {
    if (!ok) {
        fprintf(stderr, "FAIL %s\n", what);
        ++failures;
    }
}

int main() {
    char msg[256] = {0};
    SetScorePlan p;
    // ---- the plan: chunks cover the rows, a multiple of 64, a given value is taken as given, a shared bitmap serves any B --------------------
    const int64_t rows[] = {1, 63, 64, 65, 2048, 2049, 4173, 1000000, 21000000, kSetMaxRows};
    for (int64_t n : rows)
        for (int32_t B : {1, 3, 8, 64, 1024, 5000})
            for (int per_query : {0, 1})
                for (int64_t rpc : {(int64_t)0, (int64_t)64, (int64_t)2048, (int64_t)4096, (int64_t)1 << 20}) {
                    const int rc = set_score_plan(n, B, 29523, per_query != 0, rpc, &p, msg, sizeof msg);
                    const int64_t given_chunks = rpc ? (n + rpc - 1) / rpc : 0;
                    if (rpc && given_chunks > 0x7FFFFFFF / B) {
                        expect("plan: too many work items", rc, VS_EINVAL, msg, "too many");
                        continue;
                    }
                    expect("plan", rc, VS_OK, msg, "");
                    expect_true("plan: covers the rows", p.chunks * p.rows_per_chunk >= n && (p.chunks - 1) * p.rows_per_chunk < n);
                    expect_true("plan: a multiple of 64", p.rows_per_chunk > 0 && p.rows_per_chunk % 64 == 0);
                    if (rpc) expect_true("plan: taken as given", p.rows_per_chunk == rpc);
                    else expect_true("plan: automatic", p.rows_per_chunk >= kSpanRows && (int64_t)B * p.chunks <= std::max<int64_t>(kAutoItems, B));
                }
    expect_true("auto: 21 M rows, one query", set_score_auto_chunk(21000000, 1) == 20544);
    expect_true("auto: 1 M rows, one query", set_score_auto_chunk(1000000, 1) == kSpanRows);
    expect_true("auto: 1 M rows, eight queries", set_score_auto_chunk(1000000, 8) == 7872);
    expect("plan: n_rows = 0", set_score_plan(0, 1, 4, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("plan: n_rows = 2^32", set_score_plan(1ll << 32, 1, 4, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("plan: B = 0", set_score_plan(10, 0, 4, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "B must be positive");
    expect("plan: n_cols = 0", set_score_plan(10, 1, 0, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "n_cols");
    expect("plan: n_cols = 65536", set_score_plan(10, 1, 65536, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "n_cols");
    expect("plan: rows_per_chunk = 100", set_score_plan(10, 1, 4, true, 100, &p, msg, sizeof msg), VS_EINVAL, msg, "rows_per_chunk");
    expect("plan: rows_per_chunk = -64", set_score_plan(10, 1, 4, true, -64, &p, msg, sizeof msg), VS_EINVAL, msg, "rows_per_chunk");
    // ---- the call, before the index is looked at ---------------------------------------------------------------------------------------------
    expect("call: good", set_score_check_call(true, true, 3, 5, 0, 0, msg, sizeof msg), VS_OK, msg, "");
    expect("call: NULL", set_score_check_call(false, true, 3, 0, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("call: q_dtype", set_score_check_call(true, false, 3, 0, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "q_dtype");
    expect("call: B = 0", set_score_check_call(true, true, 0, 0, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "B must be positive");
    expect("call: bit0 < 0", set_score_check_call(true, true, 3, -1, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "bit0");
    expect("call: ld_words < 0", set_score_check_call(true, true, 3, 0, -1, 0, msg, sizeof msg), VS_EINVAL, msg, "ld_words");
    expect("call: rows_per_chunk = 65", set_score_check_call(true, true, 3, 0, 0, 65, msg, sizeof msg), VS_EINVAL, msg, "rows_per_chunk");
    // ---- ... and against its shape: 4173 rows, 1000 columns -----------------------------------------------------------------------------------
    const int64_t n = 4173, W = (n + 31) / 32;
    expect("shape: good, per query", set_score_check_shape(n, 1000, 1000, true, 0, W, 3, 0, n, &p, msg, sizeof msg), VS_OK, msg, "");
    expect("shape: good, shared by three queries", set_score_check_shape(n, 1000, 1003, true, 37, 0, 3, 64, n + 5, &p, msg, sizeof msg), VS_OK, msg, "");
    expect("shape: good, no bitmap, three queries", set_score_check_shape(n, 1000, 1000, false, 0, 0, 3, 0, n, &p, msg, sizeof msg), VS_OK, msg, "");
    expect("shape: ldq", set_score_check_shape(n, 1000, 999, true, 0, W, 3, 0, n, &p, msg, sizeof msg), VS_EINVAL, msg, "columns");
    expect("shape: ld_scores", set_score_check_shape(n, 1000, 1000, true, 0, W, 3, 0, n - 1, &p, msg, sizeof msg), VS_EINVAL, msg, "ld_scores");
    expect("shape: ld_words", set_score_check_shape(n, 1000, 1000, true, 0, W - 1, 3, 0, n, &p, msg, sizeof msg), VS_EINVAL, msg, "ld_words");
    expect("shape: bit0 pushes the span past the stride", set_score_check_shape(n, 1000, 1000, true, 32, W, 3, 0, n, &p, msg, sizeof msg), VS_EINVAL, msg,
           "ld_words");
    expect("shape: bit0 inside the last word", set_score_check_shape(n, 1000, 1000, true, 19, W, 3, 0, n, &p, msg, sizeof msg), VS_OK, msg, "");
    expect("shape: too many work items", set_score_check_shape(kSetMaxRows, 1000, 1000, false, 0, 0, 64, 64, kSetMaxRows, &p, msg, sizeof msg), VS_EINVAL,
           msg, "too many");
    static_assert(kSetScoreMaxCols == 32763, "the widest LDS image");
    if (failures) {
        fprintf(stderr, "set_score_check: %d failure(s)\n", failures);
        return 1;
    }
    printf("set_score_check: ok\n");
    return 0;
}
