// term_sum_check_main.cpp -- stand-alone driver of term_sum_check.h, the plan rule and the host-side argument checks of the term sums.
// Not part of the library: tests/test_term_sum_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.  The id
// lists live on the heap at their exact size [(B - 1) * ld + m], so a check that reads past one of them is reported by the sanitizer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "term_sum_check.h"

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
    TermSumPlan p;
    auto plan = [&](int64_t n, int32_t B, int32_t V, bool pq, int64_t rpc, int32_t tc) { return term_sum_plan(n, B, V, pq, rpc, tc, &p, msg, sizeof msg); };
    // term_fx against the contract spelled out with llrint: the edge values, then a sweep of bit patterns over every exponent
    auto spelled = [](float v) -> uint64_t {
        if (std::isnan(v)) return 0;
        const float c = std::fmin(std::fmax(v, -1048576.0f), 1048576.0f);
        return (uint64_t)(int64_t)std::llrint((double)c * 16777216.0);
    };
    const float inf = std::numeric_limits<float>::infinity();
    const float edges[] = {0x1p-25f, 0x3p-25f, -0x1p-25f, -0x3p-25f, 0x5p-25f, 0x1p-24f, 0.0f, -0.0f, std::nanf(""), 0x1p20f, -0x1p20f, 0x1p21f, -0x1p21f,
                           inf, -inf, 1.0f, -1.0f, 0x1p-149f, std::numeric_limits<float>::max(), std::nextafter(0x1p20f, 0.0f), 65504.0f, 0x1p-14f};
    const int64_t edge_fx[] = {0, 2, 0, -2, 2, 1, 0, 0, 0, (int64_t)1 << 44, -((int64_t)1 << 44), (int64_t)1 << 44, -((int64_t)1 << 44),
                               (int64_t)1 << 44, -((int64_t)1 << 44), 1 << 24, -(1 << 24), 0, (int64_t)1 << 44, ((int64_t)1 << 44) - (1 << 20),
                               (int64_t)65504 << 24, 1 << 10};
    for (size_t i = 0; i < sizeof edges / sizeof edges[0]; ++i)
        expect_true("fx edge", (int64_t)term_fx(edges[i]) == edge_fx[i] && term_fx(edges[i]) == spelled(edges[i]));
    uint32_t state = 12345u;
    for (uint32_t i = 0; i < 2000000u; ++i) {
        state = state * 1664525u + 1013904223u;
        uint32_t u = state;
        if (i & 1u) u = (u & 0x807FFFFFu) | ((90u + (i >> 1) % 64u) << 23);       // half of them next to the rounding range: 2^-37 .. 2^26
        float v;
        memcpy(&v, &u, sizeof v);
        if (term_fx(v) != spelled(v)) {
            fprintf(stderr, "FAIL fx sweep at bits %08x\n", u);
            ++failures;
            break;
        }
    }
    // automatic tiles: as few as fit VS_TERM_SUM_TILE_COLS, balanced
    const int32_t T = VS_TERM_SUM_TILE_COLS;
    const int32_t autos[][3] = {{1, 1, 1}, {T, 1, T}, {T + 1, 2, T / 2 + 1}, {29523, 2, 14762}, {2 * T, 2, T}, {2 * T + 1, 3, 12289}, {65535, 4, 16384}};
    for (const auto& c : autos) {
        expect("automatic tiles", plan(1000000, 64, c[0], true, 0, 0), VS_OK, msg, "");
        expect_true("tiles and their columns", p.tiles == c[1] && p.tile_cols == c[2]);
        expect_true("the tiles cover the columns, none is empty", (int64_t)p.tiles * p.tile_cols >= c[0] && (int64_t)(p.tiles - 1) * p.tile_cols < c[0] && p.tile_cols <= T);
    }
    // an explicit tile is taken as given
    for (const int32_t tc : {1, 7, 8, 40, 4096, T}) {
        expect("explicit tile", plan(5000, 3, 40, true, 0, tc), VS_OK, msg, "");
        expect_true("taken as given", p.tile_cols == tc && p.tiles == (40 + tc - 1) / tc);
    }
    expect("tile_cols = -1", plan(100, 1, 40, true, 0, -1), VS_EINVAL, msg, "tile_cols must");
    expect("tile_cols too wide", plan(100, 1, 40, true, 0, T + 1), VS_EINVAL, msg, "tile_cols must");
    // chunks cover the rows; an explicit chunk is taken as given; the automatic one aims at kAutoItems work items
    const int64_t rows[] = {1, 63, 64, 65, 2047, 2048, 2049, 1000000, 21000000, kTermMaxRows};
    const int64_t rpcs[] = {0, 64, 2048, 1 << 20};
    for (const int64_t n : rows)
        for (const int32_t B : {1, 9, 64, 4096})
            for (const int64_t rpc : rpcs)
                for (const int32_t tc : {0, 4096}) {
                    const int64_t tiles = tc ? (29523 + tc - 1) / tc : 2;
                    if (rpc && (n + rpc - 1) / rpc > 0x7FFFFFFF / (B * tiles)) {      // more work items than a grid holds
                        expect("plan sweep, too many", plan(n, B, 29523, true, rpc, tc), VS_EINVAL, msg, "too many");
                        continue;
                    }
                    expect("plan sweep", plan(n, B, 29523, true, rpc, tc), VS_OK, msg, "");
                    expect_true("chunks cover the rows", p.tiles == tiles && p.rows_per_chunk > 0 && p.rows_per_chunk % 64 == 0 &&
                                                             p.chunks * p.rows_per_chunk >= n && (p.chunks - 1) * p.rows_per_chunk < n &&
                                                             (rpc == 0 || p.rows_per_chunk == rpc));
                    if (rpc == 0)
                        expect_true("automatic chunks", p.rows_per_chunk % kTermSpanRows == 0 &&
                                                            p.chunks * B * tiles <= std::max<int64_t>(kAutoItems, B * tiles));
                }
    expect("n_rows = 0", plan(0, 1, 8, true, 0, 0), VS_EINVAL, msg, "n_rows must");
    expect("n_rows = 2^32", plan(kTermMaxRows + 1, 1, 8, true, 0, 0), VS_EINVAL, msg, "n_rows must");
    expect("B = 0", plan(100, 0, 8, true, 0, 0), VS_EINVAL, msg, "B must");
    expect("n_cols = 0", plan(100, 1, 0, true, 0, 0), VS_EINVAL, msg, "n_cols must");
    expect("n_cols = 65536", plan(100, 1, 65536, true, 0, 0), VS_EINVAL, msg, "n_cols must");
    expect("rows_per_chunk = 100", plan(100, 1, 8, true, 100, 0), VS_EINVAL, msg, "multiple of 64");
    expect("rows_per_chunk = -64", plan(100, 1, 8, true, -64, 0), VS_EINVAL, msg, "multiple of 64");
    expect("shared set, B = 2", plan(100, 2, 8, false, 0, 0), VS_EINVAL, msg, "B = 1");
    expect("2^26 chunks x 31 queries", plan(kTermMaxRows, 31, 8, true, 64, 0), VS_OK, msg, "");             // 31 x 2^26 < 2^31
    expect("2^26 chunks x 32 queries", plan(kTermMaxRows, 32, 8, true, 64, 0), VS_EINVAL, msg, "too many");
    expect("2^26 chunks x 16 queries x 2 tiles", plan(kTermMaxRows, 16, 8, true, 64, 4), VS_EINVAL, msg, "too many");
    expect("2^26 chunks x 15 queries x 2 tiles", plan(kTermMaxRows, 15, 8, true, 64, 4), VS_OK, msg, "");
    expect("the widest grid: no overflow in B x tiles", plan(kTermMaxRows, 0x7FFFFFFF, 65535, true, 64, 1), VS_EINVAL, msg, "too many");
    // the bitmap call
    auto sums = [&](bool words, int64_t bit0, int64_t ldw, int32_t B, int64_t n, int32_t V, int64_t rpc, int32_t tc, bool outs, int64_t lds) {
        return term_sum_check_sums(words, bit0, ldw, B, n, V, rpc, tc, outs, lds, &p, msg, sizeof msg);
    };
    expect("sums ok", sums(true, 0, 4, 3, 100, 8, 0, 0, true, 8), VS_OK, msg, "");
    expect("sums ok, NULL words", sums(false, 0, 0, 1, 100, 8, 0, 3, true, 11), VS_OK, msg, "");
    expect("sums ok, shared", sums(true, 33, 0, 1, 100, 8, 64, 0, true, 8), VS_OK, msg, "");
    expect("NULL outputs", sums(true, 0, 4, 1, 100, 8, 0, 0, false, 8), VS_EINVAL, msg, "NULL");
    expect("bit0 < 0", sums(true, -1, 4, 1, 100, 8, 0, 0, true, 8), VS_EINVAL, msg, "bit0");
    expect("ld_words short", sums(true, 31, 4, 1, 100, 8, 0, 0, true, 8), VS_EINVAL, msg, "ld_words");      // 131 bits span 5 words
    expect("ld_words exact", sums(true, 31, 5, 1, 100, 8, 0, 0, true, 8), VS_OK, msg, "");
    expect("ld_words < 0", sums(true, 0, -4, 1, 100, 8, 0, 0, true, 8), VS_EINVAL, msg, "ld_words");
    expect("NULL words, B = 2", sums(false, 0, 0, 2, 100, 8, 0, 0, true, 8), VS_EINVAL, msg, "B = 1");
    expect("ld_sums short", sums(true, 0, 4, 1, 100, 8, 0, 0, true, 7), VS_EINVAL, msg, "ld_sums");
    expect("sums, tile_cols too wide", sums(true, 0, 4, 1, 100, 8, 0, T + 1, true, 8), VS_EINVAL, msg, "tile_cols");
    // the id-list call
    auto idsz = [&](bool ids, int32_t B, int64_t m, int64_t ld, int32_t V, int32_t tc, bool outs, int64_t lds) {
        return term_sum_check_ids(ids, B, m, ld, V, tc, outs, lds, &p, msg, sizeof msg);
    };
    expect("ids ok", idsz(true, 2, 5, 7, 8, 0, true, 8), VS_OK, msg, "");
    expect_true("a short list is one slice", p.chunks == 1 && p.tiles == 1);
    expect("ids ok, long", idsz(true, 2, 100000, 100000, 8, 3, true, 8), VS_OK, msg, "");
    expect_true("a long list is sliced", p.chunks > 1 && p.chunks * p.rows_per_chunk >= 100000 && p.tiles == 3);
    expect("NULL ids", idsz(false, 2, 5, 7, 8, 0, true, 8), VS_EINVAL, msg, "NULL");
    expect("m = 0", idsz(true, 2, 0, 7, 8, 0, true, 8), VS_EINVAL, msg, "m must");
    expect("ld < m", idsz(true, 2, 5, 4, 8, 0, true, 8), VS_EINVAL, msg, "shorter than m");
    expect("ids, B = 0", idsz(true, 0, 5, 5, 8, 0, true, 8), VS_EINVAL, msg, "B must");
    expect("ids, ld_sums short", idsz(true, 2, 5, 5, 8, 0, true, 5), VS_EINVAL, msg, "ld_sums");
    expect("ids, tile_cols < 0", idsz(true, 2, 5, 5, 8, -2, true, 8), VS_EINVAL, msg, "tile_cols");
    {   // what vs_index_term_sums_ids checks in a host list before it stages it (term_check_ids_host, shared with the term counts)
        const int32_t B = 3;
        const int64_t m = 4, ld = 6, n_rows = 10, off = 100;
        const size_t n_ids = (size_t)((B - 1) * ld + m);                        // the gap behind the last query's entries does not exist
        auto host = [&](const std::vector<int64_t>& v, int64_t id_offset) { return term_check_ids_host(v.data(), B, m, ld, id_offset, n_rows, msg, sizeof msg); };
        std::vector<int64_t> ids(n_ids, off + 3);
        ids[0] = off;
        ids[n_ids - 1] = off + n_rows - 1;
        ids[1] = -1;
        ids[4] = off - 50;                                                      // the gap of query 0 is not read, whatever stands there
        expect("host list ok", host(ids, off), VS_OK, msg, "");
        for (const int64_t bad : {off - 1, off + n_rows, std::numeric_limits<int64_t>::max(), std::numeric_limits<int64_t>::min()}) {
            std::vector<int64_t> x = ids;
            x[n_ids - 1] = bad;
            expect("id outside, last entry", host(x, off), VS_EINVAL, msg, "query 2, position 3");
        }
    }
    // the top-n
    auto topn = [&](bool ptrs, bool counts, int32_t B, int32_t V, int64_t lds, int64_t ldc, int32_t n) {
        return term_sum_check_topn(ptrs, counts, B, V, lds, ldc, n, msg, sizeof msg);
    };
    expect("topn ok", topn(true, true, 2, 8, 8, 8, VS_TERM_MAX_TOPN), VS_OK, msg, "");
    expect("topn ok, n > n_cols", topn(true, false, 1, 3, 9, 0, 20), VS_OK, msg, "");
    expect("topn ok, no counts: ld_counts is not looked at", topn(true, false, 1, 8, 8, -5, 4), VS_OK, msg, "");
    expect("topn NULL", topn(false, true, 2, 8, 8, 8, 4), VS_EINVAL, msg, "NULL");
    expect("topn B = 0", topn(true, true, 0, 8, 8, 8, 4), VS_EINVAL, msg, "B must");
    expect("topn n_cols = 0", topn(true, true, 1, 0, 8, 8, 4), VS_EINVAL, msg, "n_cols must");
    expect("topn n = 0", topn(true, true, 1, 8, 8, 8, 0), VS_EINVAL, msg, "n must");
    expect("topn n = 1025", topn(true, true, 1, 8, 8, 8, VS_TERM_MAX_TOPN + 1), VS_EINVAL, msg, "n must");
    expect("topn ld_sums short", topn(true, true, 1, 8, 7, 8, 4), VS_EINVAL, msg, "ld_sums");
    expect("topn ld_counts short", topn(true, true, 1, 8, 8, 7, 4), VS_EINVAL, msg, "ld_counts");
    if (failures) return 1;
    puts("term_sum_check: ok");
    return 0;
}
