// facet_value_check_main.cpp -- stand-alone driver of facet_value_check.h: the plan rule, the limits and the host-side argument checks of the
// breakdowns.  Not part of the library: tests/test_facet_value_cpu.py builds it with the host compiler under -fsanitize=address,undefined and
// runs it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "facet_value_check.h"

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
    FacetValuePlan p;
    auto plan = [&](int64_t n, int32_t B, int32_t L, int32_t slots, bool pq, int64_t rpc) { return facet_value_plan(n, B, L, slots, pq, rpc, &p, msg, sizeof msg); };

    // ---- stats: the tile halves at 256 / 512 / 1024 labels, the global regime starts above 2048 -----------------------------------------------
    struct { int32_t L, regime, qt; } st[] = {{1, 0, 8},    {12, 0, 8},   {256, 0, 8},  {257, 0, 4},   {512, 0, 4},       {513, 0, 2},
                                              {1024, 0, 2}, {1025, 0, 1}, {2048, 0, 1}, {2049, 1, 8},  {70000, 1, 8},     {0x7FFFFFFF / 8, 1, 8}};
    for (auto& c : st) {
        expect("stats plan", plan(1 << 20, 8, c.L, 0, true, 0), VS_OK, msg, "");
        expect_true("stats plan: regime and tile", p.regime == c.regime && p.qt == c.qt);
        expect_true("stats plan: the records fit", p.regime || (int64_t)p.qt * c.L <= VS_FACET_VALUE_LDS_RECORDS);
        expect_true("stats plan: the next tile would not", p.regime || p.qt == 8 || (int64_t)2 * p.qt * c.L > VS_FACET_VALUE_LDS_RECORDS);
        expect("stats plan shared", plan(1 << 20, 1, c.L, 0, false, 0), VS_OK, msg, "");
        expect_true("stats plan shared: qt 1", p.qt == 1 && p.regime == (c.L > VS_FACET_VALUE_LDS_RECORDS ? 1 : 0));
    }
    // ---- histogram: n_labels x (n_edges + 2) bins a query against VS_FACET_LDS_BINS ----------------------------------------------------------
    struct { int32_t L, slots, regime, qt; } hs[] = {{1, 4, 0, 8},      {512, 4, 0, 8},     {513, 4, 0, 4},   {2, 1027, 0, 4},  {2, 1024, 0, 8},
                                                     {4096, 4, 0, 1},   {4097, 4, 1, 8},    {16, 1024, 0, 1}, {16, 1025, 1, 8}, {2048, 8, 0, 1},
                                                     {2049, 8, 1, 8},   {1 << 20, 4, 1, 8}, {4084, 1027, 1, 8}};
    for (auto& c : hs) {
        expect("hist plan", plan(1 << 20, 8, c.L, c.slots, true, 0), VS_OK, msg, "");
        expect_true("hist plan: regime and tile", p.regime == c.regime && p.qt == c.qt);
        expect_true("hist plan: the bins fit", p.regime || (int64_t)p.qt * c.L * c.slots <= VS_FACET_LDS_BINS);
    }
    expect("bins boundary", plan(1000, 1, VS_FACET_LDS_BINS / 4, 4, true, 0), VS_OK, msg, "");
    expect_true("bins boundary: the last LDS shape", p.regime == 0 && p.qt == 1 && p.lds_slots == VS_FACET_LDS_BINS);
    expect("cells cap", plan(1000, 1, VS_FACET_VALUE_MAX_CELLS / 4, 4, true, 0), VS_OK, msg, "");
    expect_true("cells cap: global", p.regime == 1 && p.lds_slots == 0);
    expect("cells cap + 1", plan(1000, 1, VS_FACET_VALUE_MAX_CELLS / 4 + 1, 4, true, 0), VS_EINVAL, msg, "cells");
    expect("cells cap wide", plan(1000, 1, 4085, 1027, true, 0), VS_EINVAL, msg, "cells");
    expect("stats has no cell cap", plan(1000, 1, 0x7FFFFFFF, 0, true, 0), VS_OK, msg, "");

    // ---- the automatic chunk: value_plan's rule with a floor of 16 x the LDS slots of a query ----------------------------------------------------
    expect("auto small", plan(1000, 1, 12, 0, false, 0), VS_OK, msg, "");
    expect_true("auto small: one chunk of the floor", p.chunks == 1 && p.rows_per_chunk == kMinChunk);
    expect("auto 21M", plan(21015324, 8, 12, 0, true, 0), VS_OK, msg, "");
    expect_true("auto 21M: <= 1024 chunks of whole spans",
                p.rows_per_chunk % kSpanRows == 0 && p.chunks <= 1024 && p.chunks * p.rows_per_chunk >= 21015324 && (p.chunks - 1) * p.rows_per_chunk < 21015324);
    expect("auto floor stats", plan(1 << 20, 1, 2048, 0, true, 0), VS_OK, msg, "");
    expect_true("auto floor stats: 16 rows a record", p.rows_per_chunk == 16 * 2048);
    expect("auto floor hist", plan(1 << 20, 1, 1000, 16, true, 0), VS_OK, msg, "");
    expect_true("auto floor hist: 16 rows a bin", p.rows_per_chunk == 16 * 16000 && p.rows_per_chunk % kSpanRows == 0);
    expect("auto global", plan(1 << 20, 1, 70000, 0, true, 0), VS_OK, msg, "");
    expect_true("auto global: no LDS, the plain floor", p.rows_per_chunk == kMinChunk && p.chunks == 128);
    expect("given", plan(3 * 2048 + 1, 17, 7, 0, true, 64), VS_OK, msg, "");
    expect_true("given: taken as it is", p.rows_per_chunk == 64 && p.chunks == 97 && p.qt == 8);

    // ---- every limit -------------------------------------------------------------------------------------------------------------------------------
    expect("n_rows 0", plan(0, 1, 4, 0, true, 0), VS_EINVAL, msg, "n_rows");
    expect("n_rows 2^32", plan(1ll << 32, 1, 4, 0, true, 0), VS_EINVAL, msg, "n_rows");
    expect("max rows", plan(0xFFFFFFFFll, 1, 4, 0, true, 64), VS_OK, msg, "");
    expect("B 0", plan(10, 0, 4, 0, true, 0), VS_EINVAL, msg, "B must");
    expect("n_labels 0", plan(10, 1, 0, 0, true, 0), VS_EINVAL, msg, "n_labels");
    expect("n_labels < 0", plan(10, 1, -3, 0, true, 0), VS_EINVAL, msg, "n_labels");
    expect("slots 3", plan(10, 1, 4, 3, true, 0), VS_EINVAL, msg, "n_slots");
    expect("slots 1028", plan(10, 1, 4, VS_VALUE_MAX_EDGES + 3, true, 0), VS_EINVAL, msg, "n_slots");
    expect("slots < 0", plan(10, 1, 4, -1, true, 0), VS_EINVAL, msg, "n_slots");
    expect("slots max", plan(10, 1, 4, VS_VALUE_MAX_EDGES + 2, true, 0), VS_OK, msg, "");
    expect("B x L", plan(10, 1 << 16, 1 << 15, 0, true, 0), VS_EINVAL, msg, "B x n_labels");
    expect("B x L ok", plan(10, (1 << 16) - 1, 1 << 15, 0, true, 0), VS_OK, msg, "");
    expect("shared B 2", plan(10, 2, 4, 0, false, 0), VS_EINVAL, msg, "ld_words = 0");
    expect("rpc 100", plan(10, 1, 4, 0, true, 100), VS_EINVAL, msg, "multiple of 64");
    expect("rpc < 0", plan(10, 1, 4, 0, true, -64), VS_EINVAL, msg, "multiple of 64");
    expect("too many tiles", plan(10, 65536 * 8, 1, 0, true, 0), VS_EINVAL, msg, "too many");

    // ---- the checks of the calls --------------------------------------------------------------------------------------------------------------------
    auto stats = [&](bool ptrs, bool words, int64_t bit0, int64_t ld, int32_t B, int dt, int64_t n, int32_t L, int64_t ld_out) {
        return facet_value_check_stats(ptrs, words, bit0, ld, B, dt, n, L, 0, ld_out, &p, msg, sizeof msg);
    };
    expect("stats ok", stats(true, true, 33, 4, 3, VS_VAL_F32, 64, 7, 7), VS_OK, msg, "");
    expect("stats spare", stats(true, true, 33, 4, 3, VS_VAL_I32, 64, 7, 11), VS_OK, msg, "");
    expect("stats NULL", stats(false, true, 0, 4, 3, VS_VAL_F32, 64, 7, 7), VS_EINVAL, msg, "NULL");
    expect("stats dtype", stats(true, true, 0, 4, 3, 2, 64, 7, 7), VS_EINVAL, msg, "dtype");
    expect("stats bit0", stats(true, true, -1, 4, 3, VS_VAL_I32, 64, 7, 7), VS_EINVAL, msg, "bit0");
    expect("stats ld_words short", stats(true, true, 33, 3, 3, VS_VAL_I32, 64, 7, 7), VS_EINVAL, msg, "ld_words");
    expect("stats ld_words < 0", stats(true, true, 0, -1, 1, VS_VAL_I32, 64, 7, 7), VS_EINVAL, msg, "ld_words");
    expect("stats no words B 2", stats(true, false, 0, 0, 2, VS_VAL_I32, 64, 7, 7), VS_EINVAL, msg, "ld_words = 0");
    expect("stats no words", stats(true, false, 0, 0, 1, VS_VAL_I32, 64, 7, 7), VS_OK, msg, "");
    expect("stats ld_out short", stats(true, true, 0, 4, 3, VS_VAL_I32, 64, 7, 6), VS_EINVAL, msg, "ld_out");
    expect("stats n_labels", stats(true, true, 0, 4, 3, VS_VAL_I32, 64, 0, 6), VS_EINVAL, msg, "n_labels");
    auto hist = [&](bool ptrs, int64_t ld, int32_t B, int dt, int64_t n, int32_t L, int32_t E, int64_t ldc) {
        return facet_value_check_hist(ptrs, true, 0, ld, B, dt, n, L, E, 0, ldc, &p, msg, sizeof msg);
    };
    expect("hist ok", hist(true, 4, 3, VS_VAL_F32, 64, 7, 2, 1), VS_OK, msg, "");
    expect("hist max", hist(true, 4, 3, VS_VAL_F32, 64, 2, VS_VALUE_MAX_EDGES, 1024), VS_OK, msg, "");
    expect_true("hist max: 2 x 1027 bins halve the tile twice", p.regime == 0 && p.qt == 4);
    expect("hist NULL", hist(false, 4, 3, VS_VAL_F32, 64, 7, 2, 1), VS_EINVAL, msg, "NULL");
    expect("hist 1 edge", hist(true, 4, 3, VS_VAL_F32, 64, 7, 1, 4), VS_EINVAL, msg, "n_edges");
    expect("hist 1026 edges", hist(true, 4, 3, VS_VAL_F32, 64, 7, 1026, 2000), VS_EINVAL, msg, "n_edges");
    expect("hist ld_counts short", hist(true, 4, 3, VS_VAL_F32, 64, 7, 5, 3), VS_EINVAL, msg, "ld_counts");
    expect("hist dtype", hist(true, 4, 3, 7, 64, 7, 5, 4), VS_EINVAL, msg, "dtype");
    expect("hist cells", hist(true, 4, 1, VS_VAL_F32, 64, 1 << 21, 2, 1), VS_EINVAL, msg, "cells");
    expect("hist ld_words", hist(true, 1, 3, VS_VAL_F32, 64, 7, 5, 4), VS_EINVAL, msg, "ld_words");
    {
        std::vector<uint32_t> e = {0x80000001u, 0xFFFFFFFFu, 0u, 0x7FFFFFFFu};                  // INT32_MIN + 1, -1, 0, INT32_MAX
        expect("int edges ok", value_check_edges_host(e.data(), 4, VS_VAL_I32, msg, sizeof msg), VS_OK, msg, "");
        std::vector<uint32_t> d = {5u, 5u};
        expect("int edges equal", value_check_edges_host(d.data(), 2, VS_VAL_I32, msg, sizeof msg), VS_EINVAL, msg, "ascending");
    }

    if (failures) {
        fprintf(stderr, "facet_value_check: %d failures\n", failures);
        return 1;
    }
    printf("facet_value_check: ok\n");
    return 0;
}
