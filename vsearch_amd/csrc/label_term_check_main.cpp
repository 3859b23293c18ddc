// label_term_check_main.cpp -- stand-alone driver of label_term_check.h, the plan rule, the limits and the host-side argument checks of the
// per-label term aggregations.  Not part of the library: tests/test_label_term_cpu.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "label_term_check.h"

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
    LabelTermPlan p;
    auto plan = [&](int64_t n, int32_t L, int32_t V, int64_t rpi, int32_t tc) { return label_term_plan(n, L, V, rpi, tc, &p, msg, sizeof msg); };
    // automatic tiles: those of the term sums
    const int32_t T = VS_TERM_SUM_TILE_COLS;
    const int32_t autos[][3] = {{1, 1, 1}, {T, 1, T}, {T + 1, 2, T / 2 + 1}, {29523, 2, 14762}, {2 * T, 2, T}, {2 * T + 1, 3, 12289}, {65535, 4, 16384}};
    for (const auto& c : autos) {
        expect("automatic tiles", plan(1000000, 64, c[0], 0, 0), VS_OK, msg, "");
        TermSumPlan ts;
        expect("the term sums' tiles", term_sum_plan(1000000, 1, c[0], false, 0, 0, &ts, msg, sizeof msg), VS_OK, msg, "");
        expect_true("tiles and their columns", p.tiles == c[1] && p.tile_cols == c[2] && ts.tiles == p.tiles && ts.tile_cols == p.tile_cols);
    }
    for (const int32_t tc : {1, 7, 8, 40, 4096, T}) {
        expect("explicit tile", plan(5000, 3, 40, 0, tc), VS_OK, msg, "");
        expect_true("taken as given", p.tile_cols == tc && p.tiles == (40 + tc - 1) / tc);
    }
    expect("tile_cols = -1", plan(100, 1, 40, 0, -1), VS_EINVAL, msg, "tile_cols must");
    expect("tile_cols too wide", plan(100, 1, 40, 0, T + 1), VS_EINVAL, msg, "tile_cols must");
    // the item: explicit values are taken as given, the automatic one aims at kAutoItems work items over the rows; the bound holds for any
    // split of the rows over the labels (every label adds at most one short item)
    const int64_t rows[] = {1, 63, 64, 65, 2047, 2048, 2049, 1000000, 21000000, kSetMaxRows};
    for (const int64_t n : rows)
        for (const int32_t L : {1, 7, 64, 4096, VS_LABEL_TERM_MAX_LABELS})
            for (const int64_t rpi : {(int64_t)0, (int64_t)64, (int64_t)2048, (int64_t)1 << 20})
                for (const int32_t tc : {0, 4096}) {
                    const int64_t tiles = tc ? (29523 + tc - 1) / tc : 2;
                    if (rpi && (n + rpi - 1) / rpi + L > VS_LABEL_TERM_MAX_WORK_ITEMS / tiles) {
                        expect("plan sweep, too many", plan(n, L, 29523, rpi, tc), VS_EINVAL, msg, "too many");
                        continue;
                    }
                    expect("plan sweep", plan(n, L, 29523, rpi, tc), VS_OK, msg, "");
                    expect_true("the item", p.tiles == tiles && p.rows_per_item > 0 && p.rows_per_item % 64 == 0 && (rpi == 0 || p.rows_per_item == rpi) &&
                                                p.max_items == (n + p.rows_per_item - 1) / p.rows_per_item + L);
                    if (rpi == 0)
                        expect_true("automatic item", p.rows_per_item % kSpanRows == 0 &&
                                                          (p.max_items - L) * tiles <= std::max<int64_t>(kAutoItems, tiles));
                    // the worst split: every label but one holds one row
                    const int64_t ones = std::min<int64_t>(L - 1, n - 1), rest = n - ones;
                    expect_true("the bound covers the worst split", ones + (rest + p.rows_per_item - 1) / p.rows_per_item <= p.max_items);
                }
    expect("n_rows = 0", plan(0, 1, 8, 0, 0), VS_EINVAL, msg, "n_rows must");
    expect("n_rows = 2^32", plan(kSetMaxRows + 1, 1, 8, 0, 0), VS_EINVAL, msg, "n_rows must");
    expect("n_labels = 0", plan(100, 0, 8, 0, 0), VS_EINVAL, msg, "n_labels must");
    expect("n_labels = 65536", plan(100, VS_LABEL_TERM_MAX_LABELS, 8, 0, 0), VS_OK, msg, "");
    expect("n_labels = 65537", plan(100, VS_LABEL_TERM_MAX_LABELS + 1, 8, 0, 0), VS_EINVAL, msg, "n_labels must");
    expect("n_cols = 0", plan(100, 1, 0, 0, 0), VS_EINVAL, msg, "n_cols must");
    expect("n_cols = 65536", plan(100, 1, 65536, 0, 0), VS_EINVAL, msg, "n_cols must");
    expect("rows_per_item = 100", plan(100, 1, 8, 100, 0), VS_EINVAL, msg, "multiple of 64");
    expect("rows_per_item = -64", plan(100, 1, 8, -64, 0), VS_EINVAL, msg, "multiple of 64");
    // a launch of 1024-thread workgroups holds fewer than 2^32 threads: max_items x tiles <= (2^32 - 1) / 1024 = 4 194 303
    static_assert((int64_t)VS_LABEL_TERM_MAX_WORK_ITEMS * 1024 < (1ll << 32) && ((int64_t)VS_LABEL_TERM_MAX_WORK_ITEMS + 1) * 1024 >= (1ll << 32), "the bound");
    expect("4194302 + 1 items x 1 tile", plan((int64_t)4194302 * 64, 1, 8, 64, 0), VS_OK, msg, "");
    expect("4194303 + 1 items x 1 tile", plan((int64_t)4194303 * 64, 1, 8, 64, 0), VS_EINVAL, msg, "too many");
    expect("1 M rows of 64, 29 523 tiles of one column", plan(1000000, 1, 29523, 64, 1), VS_EINVAL, msg, "too many");
    expect("2097151 items x 2 tiles", plan((int64_t)2097150 * 64, 1, 8, 64, 4), VS_OK, msg, "");
    expect("2097152 items x 2 tiles", plan((int64_t)2097151 * 64, 1, 8, 64, 4), VS_EINVAL, msg, "too many");
    // the chunk of the label order: whole spans, at least kLabelOrderMinChunk, whatever the labels
    expect_true("order chunk, few labels", label_order_chunk(1000000, 64) == kLabelOrderMinChunk);
    expect_true("order chunk, many rows", label_order_chunk(21000000, 64) == (21000000 / kAutoItems / kSpanRows + 1) * kSpanRows);
    expect_true("order chunk, LDS boundary", label_order_chunk(1000000, VS_FACET_LDS_BINS) == kLabelOrderMinChunk);
    expect_true("order chunk, global regime", label_order_chunk(1000000, VS_FACET_LDS_BINS + 1) == kLabelOrderMinChunk);
    // the two calls
    auto call = [&](int64_t bit0, int64_t n, int32_t V, bool labels, int32_t L, int64_t rpi, int32_t tc, bool outs, int64_t ld) {
        return label_term_check(bit0, n, V, labels, L, rpi, tc, outs, ld, "sums", &p, msg, sizeof msg);
    };
    expect("call ok", call(0, 100, 8, true, 3, 0, 0, true, 8), VS_OK, msg, "");
    expect("call ok, spare columns", call(37, 100, 8, true, 3, 64, 3, true, 11), VS_OK, msg, "");
    expect("NULL labels", call(0, 100, 8, false, 3, 0, 0, true, 8), VS_EINVAL, msg, "NULL");
    expect("NULL outputs", call(0, 100, 8, true, 3, 0, 0, false, 8), VS_EINVAL, msg, "NULL");
    expect("bit0 < 0", call(-1, 100, 8, true, 3, 0, 0, true, 8), VS_EINVAL, msg, "bit0");
    expect("ld short", call(0, 100, 8, true, 3, 0, 0, true, 7), VS_EINVAL, msg, "ld_sums");
    expect("call, n_labels = 0", call(0, 100, 8, true, 0, 0, 0, true, 8), VS_EINVAL, msg, "n_labels must");
    expect("call, tile_cols too wide", call(0, 100, 8, true, 3, 0, T + 1, true, 8), VS_EINVAL, msg, "tile_cols");
    // 1 GiB of int64: n_labels x ld <= 2^27 -- 4546 labels at 29 523 columns, 65 536 labels at 2048
    expect("4546 x 29523", call(0, 100, 29523, true, 4546, 0, 0, true, 29523), VS_OK, msg, "");
    expect("4547 x 29523", call(0, 100, 29523, true, 4547, 0, 0, true, 29523), VS_EINVAL, msg, "1 GiB");
    expect("65536 x 2048", call(0, 100, 2048, true, VS_LABEL_TERM_MAX_LABELS, 0, 0, true, 2048), VS_OK, msg, "");
    expect("65536 x 2049 (the stride counts)", call(0, 100, 2048, true, VS_LABEL_TERM_MAX_LABELS, 0, 0, true, 2049), VS_EINVAL, msg, "1 GiB");
    // the label order
    auto order = [&](int64_t bit0, int64_t n, bool labels, int32_t L, bool outs) { return label_order_check(bit0, n, labels, L, outs, msg, sizeof msg); };
    expect("order ok", order(5, 100, true, VS_LABEL_TERM_MAX_LABELS, true), VS_OK, msg, "");
    expect("order NULL labels", order(0, 100, false, 3, true), VS_EINVAL, msg, "NULL");
    expect("order NULL outputs", order(0, 100, true, 3, false), VS_EINVAL, msg, "NULL");
    expect("order bit0 < 0", order(-3, 100, true, 3, true), VS_EINVAL, msg, "bit0");
    expect("order n_labels = 65537", order(0, 100, true, VS_LABEL_TERM_MAX_LABELS + 1, true), VS_EINVAL, msg, "n_labels must");
    if (failures) return 1;
    puts("label_term_check: ok");
    return 0;
}
