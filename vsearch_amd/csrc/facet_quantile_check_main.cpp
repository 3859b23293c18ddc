// facet_quantile_check_main.cpp -- stand-alone driver of facet_quantile_check.h: the plan rule of the per-label percentiles against its stated
// rule, the limits and the argument checks.  Not part of the library: tests/test_facet_quantile_cpu.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it.  It ends with a per-label radix select over random keys and labels, composed of the headers'
// functions alone with the slot lists on the heap at their exact padded size, against a sort per label.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "facet_quantile_check.h"

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

// the rule as the header states it, written out again
static void rule(int64_t n_rows, int32_t B, int32_t L, int32_t R, int level, bool per_query, int64_t rpc, FacetQuantilePlan* w) {
    const int32_t cap = (int32_t)(128 * 1024 / ((level == 0 ? 1 : R) * (level == 2 ? 1024 : 2048) * 4));
    int64_t best = -1;
    *w = FacetQuantilePlan();
    for (int32_t qt = 1; qt <= (per_query ? 8 : 1) && qt <= cap; qt *= 2) {
        const int32_t tl = std::min(L, cap / qt);
        const int64_t lt = (L + tl - 1) / tl, passes = ((B + qt - 1) / qt) * lt;
        if (lt > VS_FACET_QUANTILE_MAX_LABEL_TILES) continue;
        if (best < 0 || passes < best) best = passes, w->qt = qt, w->tile_labels = tl, w->label_tiles = (int32_t)lt;
    }
    if (best < 0) w->regime = 1, w->qt = per_query ? 8 : 1, w->tile_labels = L, w->label_tiles = 1;
    const int64_t items = (int64_t)((B + w->qt - 1) / w->qt) * w->label_tiles;
    w->rows_per_chunk = rpc ? rpc : auto_chunk(n_rows, items, kMinChunk);
    w->chunks = (n_rows + w->rows_per_chunk - 1) / w->rows_per_chunk;
}

int main() {
    char msg[512] = {0};
    FacetQuantilePlan p, w;
    // ---- the plan against the rule: every level, labels on both sides of every tile and regime boundary ---------------------------------------------
    for (int64_t n_rows : {(int64_t)1, (int64_t)64, (int64_t)2049, (int64_t)1000000, (int64_t)21015324, (int64_t)0xFFFFFFFFll})
        for (int level = 0; level < VS_VALUE_RADIX_LEVELS; ++level)
            for (int32_t R : {1, 2, 3, 7, 8, 16})
                for (int32_t B : {1, 8, 9}) {
                    const int32_t cap = facet_quantile_lds_cells(R, level);
                    expect_true("cells", cap >= 1 && cap <= kFqMaxCells);
                    std::vector<int32_t> Ls = {1, 2, cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1};
                    for (int32_t qt : {1, 2, 4, 8})
                        for (int32_t d : {-1, 0, 1}) Ls.push_back(std::max(1, cap / qt) * VS_FACET_QUANTILE_MAX_LABEL_TILES + d);
                    for (int32_t L : Ls) {
                        if (L < 1) continue;
                        for (bool pq : {true, false}) {
                            if (!pq && B > 1) continue;
                            expect("plan ok", facet_quantile_plan(n_rows, B, L, R, level, pq, 0, &p, msg, sizeof msg), VS_OK, msg, "");
                            rule(n_rows, B, L, R, level, pq, 0, &w);
                            expect_true("plan = rule", p.regime == w.regime && p.qt == w.qt && p.tile_labels == w.tile_labels &&
                                                           p.label_tiles == w.label_tiles && p.chunks == w.chunks && p.rows_per_chunk == w.rows_per_chunk);
                            expect_true("plan: LDS", facet_quantile_lds_bytes(p, R, level) <= (size_t)kFqLdsBytes &&
                                                         (p.regime || p.qt * p.tile_labels <= kFqMaxCells));
                            expect_true("plan: tiles cover the labels", p.regime || ((int64_t)p.tile_labels * p.label_tiles >= L &&
                                                                                     (int64_t)p.tile_labels * (p.label_tiles - 1) < L));
                            expect_true("plan: chunks cover the rows", p.chunks * p.rows_per_chunk >= n_rows && (p.chunks - 1) * p.rows_per_chunk < n_rows);
                        }
                    }
                }
    expect("plan given", facet_quantile_plan(3 * 2048 + 1, 2, 40, 1, 0, true, 2048, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan given: taken as it is", p.regime == 0 && p.chunks == 4 && p.rows_per_chunk == 2048 && p.label_tiles > 1);
    expect("plan global", facet_quantile_plan(1000, 1, 16 * VS_FACET_QUANTILE_MAX_LABEL_TILES + 1, 1, 0, false, 0, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan global: one tile of all labels", p.regime == 1 && p.qt == 1 && p.label_tiles == 1);
    expect("plan lds edge", facet_quantile_plan(1000, 1, 16 * VS_FACET_QUANTILE_MAX_LABEL_TILES, 1, 0, false, 0, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan lds edge", p.regime == 0 && p.tile_labels == 16 && p.label_tiles == VS_FACET_QUANTILE_MAX_LABEL_TILES);

    // ---- the limits ----------------------------------------------------------------------------------------------------------------------------------
    expect("n 0", facet_quantile_plan(0, 1, 1, 1, 0, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("n 2^32", facet_quantile_plan(1ll << 32, 1, 1, 1, 0, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("B 0", facet_quantile_plan(10, 0, 1, 1, 0, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "B must");
    expect("L 0", facet_quantile_plan(10, 1, 0, 1, 0, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "n_labels");
    expect("B x L", facet_quantile_plan(10, 65536, 65536, 1, 0, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "2^31");
    expect("R 0", facet_quantile_plan(10, 1, 1, 0, 0, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "R must");
    expect("R 17", facet_quantile_plan(10, 1, 1, 17, 0, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "R must");
    expect("level 3", facet_quantile_plan(10, 1, 1, 1, 3, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "level");
    expect("rpc", facet_quantile_plan(10, 1, 1, 1, 0, true, 100, &p, msg, sizeof msg), VS_EINVAL, msg, "multiple of 64");
    expect("shared B 2", facet_quantile_plan(10, 2, 1, 1, 0, false, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "ld_words = 0");
    expect("scratch ok", facet_quantile_check_scratch(8, 512, 16, msg, sizeof msg), VS_OK, msg, "");
    expect("scratch big", facet_quantile_check_scratch(8, 513, 16, msg, sizeof msg), VS_EINVAL, msg, "2^27");
    expect("scratch 65536 x 1", facet_quantile_check_scratch(1, 65536, 1, msg, sizeof msg), VS_OK, msg, "");
    expect("scratch 65537 x 1", facet_quantile_check_scratch(1, 65537, 1, msg, sizeof msg), VS_EINVAL, msg, "2^27");

    // ---- the checks of a call, in the order they are reported ------------------------------------------------------------------------------------------
    expect("set ok", facet_quantile_check_set(true, true, 5, 40, 3, VS_VAL_F32, 1000, 12, 7, 1, 0, &p, msg, sizeof msg), VS_OK, msg, "");
    expect("set null", facet_quantile_check_set(false, true, 0, 40, 3, 9, 1000, 12, 7, 1, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("set dtype", facet_quantile_check_set(true, true, -1, 40, 3, 9, 1000, 12, 7, 1, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "dtype");
    expect("set bit0", facet_quantile_check_set(true, true, -1, 40, 3, VS_VAL_I32, 0, 12, 7, 1, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "bit0");
    expect("set rows", facet_quantile_check_set(true, true, 0, 1, 3, VS_VAL_I32, 0, 12, 7, 1, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("set ld", facet_quantile_check_set(true, true, 5, 31, 3, VS_VAL_I32, 1000, 12, 7, 1, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "ld_words");
    expect("set scratch", facet_quantile_check_set(true, true, 0, 40, 8, VS_VAL_I32, 1000, 513, 16, 1, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "2^27");
    expect("level 0 args", facet_quantile_check_level_args(0, false, true, msg, sizeof msg), VS_OK, msg, "");
    expect("level 0 no missing", facet_quantile_check_level_args(0, true, false, msg, sizeof msg), VS_EINVAL, msg, "missing");
    expect("level 2 args", facet_quantile_check_level_args(2, true, false, msg, sizeof msg), VS_OK, msg, "");
    expect("level 1 no state", facet_quantile_check_level_args(1, false, true, msg, sizeof msg), VS_EINVAL, msg, "slot_prefix");
    expect("level 5", facet_quantile_check_level_args(5, true, true, msg, sizeof msg), VS_EINVAL, msg, "level");

    // ---- a per-label select, composed of the headers' functions, against a sort per label -----------------------------------------------------------------
    {
        uint32_t state = 31337u;
        const int L = 5, n = 4000;
        std::vector<uint32_t> keys;
        std::vector<int32_t> labels;
        for (int i = 0; i < n; ++i) {
            state = state * 1664525u + 1013904223u;
            keys.push_back(i % 13 == 0 ? 0u : (i & 1) ? state : 0x80000000u + (state % 90u));
            state = state * 1664525u + 1013904223u;
            labels.push_back((int32_t)(state >> 8) % (L + 2) - 1);                        // -1 .. L: both ends are `other`
        }
        int64_t seen = 0, other = 0;
        for (int l = 0; l < L; ++l) {
            std::vector<uint32_t> sorted;
            int64_t missing = 0;
            for (int i = 0; i < n; ++i)
                if (labels[(size_t)i] == l) (keys[(size_t)i] ? (void)sorted.push_back(keys[(size_t)i]) : (void)++missing);
            std::sort(sorted.begin(), sorted.end());
            seen += (int64_t)sorted.size() + missing;
            for (double q : {0.0, 0.5, 0.9, 1.0}) {
                int64_t r = quantile_rank(q, (int64_t)sorted.size(), VS_QUANTILE_LOWER);
                const int64_t rank = r;
                std::vector<uint32_t> sp(16, kRadixNoSlot);                                 // one slot: the rank's prefix
                uint32_t prefix = 0u;
                bool ok = r >= 0;
                for (int level = 0; level < VS_VALUE_RADIX_LEVELS && ok; ++level) {
                    const int bins = radix_bins(level);
                    sp[0] = level ? prefix : 0u;
                    std::vector<int64_t> cum((size_t)bins + 1, 0);
                    for (int i = 0; i < n; ++i) {
                        const uint32_t k = keys[(size_t)i];
                        if (labels[(size_t)i] != l || k == 0u) continue;
                        if (level == 0 || radix_find_slot(sp.data(), radix_prefix(k, level)) == 0) ++cum[(size_t)radix_digit(k, level) + 1];
                    }
                    for (int i = 0; i < bins; ++i) cum[(size_t)i + 1] += cum[(size_t)i];
                    const int d = radix_find_bin(cum.data(), bins, r);
                    ok = d >= 0;
                    if (ok) r -= cum[(size_t)d], prefix = radix_extend(prefix, level, (uint32_t)d);
                }
                expect_true("per-label select equals the sort", ok && prefix == sorted[(size_t)rank]);
            }
        }
        for (int i = 0; i < n; ++i) other += labels[(size_t)i] < 0 || labels[(size_t)i] >= L;
        expect_true("the total identity", seen + other == n && other > 0);
    }

    if (failures) {
        fprintf(stderr, "facet_quantile_check: %d failures\n", failures);
        return 1;
    }
    printf("facet_quantile_check: ok\n");
    return 0;
}
