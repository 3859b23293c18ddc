// term_agg_check_main.cpp -- stand-alone driver of term_agg_check.h, the plan rule and the host-side argument checks of the term aggregations.
// Not part of the library: tests/test_term_agg_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.  The id
// lists live on the heap at their exact size [(B - 1) * ld + m], so a check that reads past one of them is reported by the sanitizer.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "term_agg_check.h"

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
    char msg[512] = {0};
    TermPlan p;
    auto plan = [&](int64_t n, int32_t B, int32_t V, bool pq, int64_t rpc) { return term_plan(n, B, V, pq, rpc, &p, msg, sizeof msg); };
    // the plan rule: the regime switches behind VS_TERM_LDS_COLS, the chunks cover the rows, an explicit chunk is taken as given
    expect("plan ok", plan(1000000, 64, 29523, true, 0), VS_OK, msg, "");
    expect_true("LDS regime at the BERT vocabulary", p.regime == 0 && p.rows_per_chunk % kTermSpanRows == 0);
    expect("plan at the switch", plan(1000, 1, VS_TERM_LDS_COLS, true, 0), VS_OK, msg, "");
    expect_true("LDS regime at VS_TERM_LDS_COLS", p.regime == 0);
    expect("plan behind the switch", plan(1000, 1, VS_TERM_LDS_COLS + 1, true, 0), VS_OK, msg, "");
    expect_true("global regime behind it", p.regime == 1);
    expect("widest", plan(1000, 1, kTermMaxCols, true, 0), VS_OK, msg, "");
    const int64_t rows[] = {1, 63, 64, 65, 2047, 2048, 2049, 1000000, 21000000, kTermMaxRows};
    const int64_t rpcs[] = {0, 64, 2048, 1 << 20};
    for (const int64_t n : rows)
        for (const int32_t B : {1, 9, 64, 4096})
            for (const int64_t rpc : rpcs) {
                if (rpc && (n + rpc - 1) / rpc > 0x7FFFFFFF / B) {                // more work items than a grid holds
                    expect("plan sweep, too many", plan(n, B, 29523, true, rpc), VS_EINVAL, msg, "too many");
                    continue;
                }
                expect("plan sweep", plan(n, B, 29523, true, rpc), VS_OK, msg, "");
                expect_true("chunks cover the rows", p.rows_per_chunk > 0 && p.rows_per_chunk % 64 == 0 && p.chunks * p.rows_per_chunk >= n &&
                                                         (p.chunks - 1) * p.rows_per_chunk < n && (rpc == 0 || p.rows_per_chunk == rpc));
            }
    expect("n_rows = 0", plan(0, 1, 8, true, 0), VS_EINVAL, msg, "n_rows must");
    expect("n_rows = 2^32", plan(kTermMaxRows + 1, 1, 8, true, 0), VS_EINVAL, msg, "n_rows must");
    expect("B = 0", plan(100, 0, 8, true, 0), VS_EINVAL, msg, "B must");
    expect("n_cols = 0", plan(100, 1, 0, true, 0), VS_EINVAL, msg, "n_cols must");
    expect("n_cols = 65536", plan(100, 1, 65536, true, 0), VS_EINVAL, msg, "n_cols must");
    expect("rows_per_chunk = 100", plan(100, 1, 8, true, 100), VS_EINVAL, msg, "multiple of 64");
    expect("rows_per_chunk = -64", plan(100, 1, 8, true, -64), VS_EINVAL, msg, "multiple of 64");
    expect("shared set, B = 2", plan(100, 2, 8, false, 0), VS_EINVAL, msg, "B = 1");
    expect("2^26 chunks", plan(kTermMaxRows, 1, 8, true, 64), VS_OK, msg, "");
    expect("2^26 chunks x 31 queries", plan(kTermMaxRows, 31, 8, true, 64), VS_OK, msg, "");      // 31 x 2^26 < 2^31
    expect("2^26 chunks x 32 queries", plan(kTermMaxRows, 32, 8, true, 64), VS_EINVAL, msg, "too many");
    // the bitmap call
    auto counts = [&](bool words, int64_t bit0, int64_t ldw, int32_t B, int64_t n, int32_t V, int64_t rpc, bool outs, int64_t ldc) {
        return term_check_counts(words, bit0, ldw, B, n, V, rpc, outs, ldc, &p, msg, sizeof msg);
    };
    expect("counts ok", counts(true, 0, 4, 3, 100, 8, 0, true, 8), VS_OK, msg, "");
    expect("counts ok, NULL words", counts(false, 0, 0, 1, 100, 8, 0, true, 11), VS_OK, msg, "");
    expect("counts ok, shared", counts(true, 33, 0, 1, 100, 8, 64, true, 8), VS_OK, msg, "");
    expect("NULL outputs", counts(true, 0, 4, 1, 100, 8, 0, false, 8), VS_EINVAL, msg, "NULL");
    expect("bit0 < 0", counts(true, -1, 4, 1, 100, 8, 0, true, 8), VS_EINVAL, msg, "bit0");
    expect("ld_words short", counts(true, 31, 4, 1, 100, 8, 0, true, 8), VS_EINVAL, msg, "ld_words");       // 131 bits span 5 words
    expect("ld_words exact", counts(true, 31, 5, 1, 100, 8, 0, true, 8), VS_OK, msg, "");
    expect("ld_words < 0", counts(true, 0, -4, 1, 100, 8, 0, true, 8), VS_EINVAL, msg, "ld_words");
    expect("NULL words, B = 2", counts(false, 0, 0, 2, 100, 8, 0, true, 8), VS_EINVAL, msg, "B = 1");
    expect("ld_counts short", counts(true, 0, 4, 1, 100, 8, 0, true, 7), VS_EINVAL, msg, "ld_counts");
    // the id-list call
    auto idsz = [&](bool ids, int32_t B, int64_t m, int64_t ld, int32_t V, bool outs, int64_t ldc) {
        return term_check_ids(ids, B, m, ld, V, outs, ldc, &p, msg, sizeof msg);
    };
    expect("ids ok", idsz(true, 2, 5, 7, 8, true, 8), VS_OK, msg, "");
    expect_true("a short list is one slice", p.chunks == 1);
    expect("ids ok, long", idsz(true, 2, 100000, 100000, 8, true, 8), VS_OK, msg, "");
    expect_true("a long list is sliced", p.chunks > 1 && p.chunks * p.rows_per_chunk >= 100000);
    expect("NULL ids", idsz(false, 2, 5, 7, 8, true, 8), VS_EINVAL, msg, "NULL");
    expect("m = 0", idsz(true, 2, 0, 7, 8, true, 8), VS_EINVAL, msg, "m must");
    expect("ld < m", idsz(true, 2, 5, 4, 8, true, 8), VS_EINVAL, msg, "shorter than m");
    expect("ids, B = 0", idsz(true, 0, 5, 5, 8, true, 8), VS_EINVAL, msg, "B must");
    expect("ids, ld_counts short", idsz(true, 2, 5, 5, 8, true, 5), VS_EINVAL, msg, "ld_counts");
    {
        const int32_t B = 3;
        const int64_t m = 4, ld = 6, n_rows = 10, off = 100;
        const size_t n_ids = (size_t)((B - 1) * ld + m);                        // the gap behind the last query's entries does not exist
        auto host = [&](const std::vector<int64_t>& v, int64_t id_offset) { return term_check_ids_host(v.data(), B, m, ld, id_offset, n_rows, msg, sizeof msg); };
        std::vector<int64_t> ids(n_ids, off + 3);
        ids[0] = off;
        ids[n_ids - 1] = off + n_rows - 1;
        ids[1] = -1;
        ids[4] = off - 50;                                                      // the gap of query 0 is not read, whatever stands there
        ids[5] = off + 999;
        expect("host list ok", host(ids, off), VS_OK, msg, "");
        for (const int64_t bad : {off - 1, off + n_rows, (int64_t)-2, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()}) {
            std::vector<int64_t> x = ids;
            x[n_ids - 1] = bad;
            expect("id outside, last entry", host(x, off), VS_EINVAL, msg, "query 2, position 3");
            x = ids;
            x[ld + 2] = bad;
            expect("id outside, query 1", host(x, off), VS_EINVAL, msg, "query 1, position 2");
        }
        std::vector<int64_t> pad(n_ids, -1);
        expect("all padding", host(pad, off), VS_OK, msg, "");
        std::vector<int64_t> z(n_ids, 0);                                       // offsets at the ends of int64 do not overflow
        expect("offset min", host(z, std::numeric_limits<int64_t>::min()), VS_EINVAL, msg, "outside");
        expect("offset max", host(z, std::numeric_limits<int64_t>::max()), VS_EINVAL, msg, "outside");
        z.assign(n_ids, -5);
        expect("a negative offset", host(z, -7), VS_OK, msg, "");
    }
    // the top-n
    auto topn = [&](bool ptrs, int32_t B, int32_t V, int64_t ldc, int32_t n, int method) { return term_check_topn(ptrs, B, V, ldc, n, method, msg, sizeof msg); };
    expect("topn ok", topn(true, 2, 8, 8, VS_TERM_MAX_TOPN, VS_TERM_JLH), VS_OK, msg, "");
    expect("topn ok, n > n_cols", topn(true, 1, 3, 9, 20, VS_TERM_LIFT), VS_OK, msg, "");
    expect("topn NULL", topn(false, 2, 8, 8, 4, VS_TERM_JLH), VS_EINVAL, msg, "NULL");
    expect("topn B = 0", topn(true, 0, 8, 8, 4, VS_TERM_JLH), VS_EINVAL, msg, "B must");
    expect("topn n_cols = 0", topn(true, 1, 0, 8, 4, VS_TERM_JLH), VS_EINVAL, msg, "n_cols must");
    expect("topn n = 0", topn(true, 1, 8, 8, 0, VS_TERM_JLH), VS_EINVAL, msg, "n must");
    expect("topn n = 1025", topn(true, 1, 8, 8, VS_TERM_MAX_TOPN + 1, VS_TERM_JLH), VS_EINVAL, msg, "n must");
    expect("topn ld_counts short", topn(true, 1, 8, 7, 4, VS_TERM_JLH), VS_EINVAL, msg, "ld_counts");
    expect("topn method = 2", topn(true, 1, 8, 8, 4, 2), VS_EINVAL, msg, "method must");
    expect("topn method = -1", topn(true, 1, 8, 8, 4, -1), VS_EINVAL, msg, "method must");
    if (failures) return 1;
    puts("term_agg_check: ok");
    return 0;
}
