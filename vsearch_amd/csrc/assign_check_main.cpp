// assign_check_main.cpp -- stand-alone driver of assign_check.h, the plan rule and the host-side argument checks of the clustering calls.
// Not part of the library: tests/test_cluster_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.  The host
// centroids live on the heap at their exact size [(K - 1) * ldc + n_cols], so a check that reads past them is reported by the sanitizer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "assign_check.h"

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
    AssignPlan p;
    auto plan = [&](int64_t n, int32_t K, int32_t V, int64_t rpc) { return assign_plan(n, K, V, rpc, &p, msg, sizeof msg); };
    // the slice width and the slices: 1, 2 or 4 centroids a lane, slices x W >= K > (slices - 1) x W
    const int32_t ks[][3] = {{1, 64, 1}, {2, 64, 1}, {63, 64, 1}, {64, 64, 1}, {65, 128, 1}, {128, 128, 1}, {129, 256, 1}, {256, 256, 1}, {257, 256, 2},
                             {1024, 256, 4}, {4095, 256, 16}, {VS_ASSIGN_MAX_K, 256, 16}};
    for (const auto& c : ks) {
        expect("slices", plan(1000000, c[0], 29523, 0), VS_OK, msg, "");
        expect_true("slice width and slices", p.slice_w == c[1] && p.slices == c[2]);
        expect_true("the slices cover the centroids, none is empty", (int64_t)p.slices * p.slice_w >= c[0] && (int64_t)(p.slices - 1) * p.slice_w < c[0]);
        expect_true("the slab", p.slab_bytes == (int64_t)(29523 + 1) * p.slices * p.slice_w * 4);
    }
    expect("the largest slab", plan(1, VS_ASSIGN_MAX_K, kTermMaxCols, 0), VS_OK, msg, "");
    expect_true("1 GiB", p.slab_bytes == (int64_t)1 << 30);
    // chunks cover the rows; an explicit chunk is taken as given; the automatic one aims at kAssignAutoChunks workgroups
    const int64_t rows[] = {1, 63, 64, 65, 255, 256, 257, 2049, 1000000, 21000000, kTermMaxRows};
    const int64_t rpcs[] = {0, 64, 2048, 1 << 20};
    for (const int64_t n : rows)
        for (const int32_t K : {1, 64, 65, VS_ASSIGN_MAX_K})
            for (const int64_t rpc : rpcs) {
                expect("plan sweep", plan(n, K, 100, rpc), VS_OK, msg, "");
                expect_true("chunks cover the rows", p.rows_per_chunk > 0 && p.rows_per_chunk % 64 == 0 && p.chunks * p.rows_per_chunk >= n &&
                                                         (p.chunks - 1) * p.rows_per_chunk < n && (rpc == 0 || p.rows_per_chunk == rpc));
                expect_true("a 1-D grid holds the chunks", p.chunks <= 0x7FFFFFFF);
                if (rpc == 0) expect_true("automatic chunks", p.rows_per_chunk >= kAssignMinChunkRows && p.chunks <= kAssignAutoChunks);
            }
    expect("n_rows = 0", plan(0, 1, 8, 0), VS_EINVAL, msg, "n_rows must");
    expect("n_rows = 2^32", plan(kTermMaxRows + 1, 1, 8, 0), VS_EINVAL, msg, "n_rows must");
    expect("K = 0", plan(100, 0, 8, 0), VS_EINVAL, msg, "K must");
    expect("K = 4097", plan(100, VS_ASSIGN_MAX_K + 1, 8, 0), VS_EINVAL, msg, "K must");
    expect("n_cols = 0", plan(100, 1, 0, 0), VS_EINVAL, msg, "n_cols must");
    expect("n_cols = 65536", plan(100, 1, 65536, 0), VS_EINVAL, msg, "n_cols must");
    expect("rows_per_chunk = 100", plan(100, 1, 8, 100), VS_EINVAL, msg, "multiple of 64");
    expect("rows_per_chunk = -64", plan(100, 1, 8, -64), VS_EINVAL, msg, "multiple of 64");
    // the assign call
    auto call = [&](bool ptrs, int32_t K, int64_t ldc, int64_t bit0, int64_t n, int32_t V, int64_t rpc) {
        return assign_check_call(ptrs, K, ldc, bit0, n, V, rpc, &p, msg, sizeof msg);
    };
    expect("call ok", call(true, 7, 8, 0, 100, 8, 0), VS_OK, msg, "");
    expect("call ok, wide rows and a bit0", call(true, 7, 11, 37, 100, 8, 64), VS_OK, msg, "");
    expect("NULL pointers", call(false, 7, 8, 0, 100, 8, 0), VS_EINVAL, msg, "NULL");
    expect("ldc short", call(true, 7, 7, 0, 100, 8, 0), VS_EINVAL, msg, "ldc");
    expect("bit0 < 0", call(true, 7, 8, -1, 100, 8, 0), VS_EINVAL, msg, "filter_bit0");
    expect("bit0 huge", call(true, 7, 8, std::numeric_limits<int64_t>::max(), 100, 8, 0), VS_EINVAL, msg, "filter_bit0");
    expect("call, K = 0", call(true, 0, 8, 0, 100, 8, 0), VS_EINVAL, msg, "K must");
    expect("call, K too large", call(true, VS_ASSIGN_MAX_K + 1, 8, 0, 100, 8, 0), VS_EINVAL, msg, "K must");
    {   // what vs_index_assign checks in host centroids and a host bias before it stages them: exactly [(K - 1) * ldc + n_cols] floats are read
        const int32_t K = 3, V = 5;
        const int64_t ldc = 9;
        const float inf = std::numeric_limits<float>::infinity();
        std::vector<float> c((size_t)((K - 1) * ldc + V), 1.5f), bias(K, -2.0f);
        auto fin = [&](const std::vector<float>& cc, const float* b) { return assign_check_finite_host(cc.data(), K, V, ldc, b, msg, sizeof msg); };
        expect("finite", fin(c, bias.data()), VS_OK, msg, "");
        expect("finite, no bias", fin(c, nullptr), VS_OK, msg, "");
        std::vector<float> gap = c;
        gap[V] = std::nanf("");                                                 // the gap behind a row's columns is not read, whatever stands there
        gap[ldc - 1] = inf;
        expect("gaps are not looked at", fin(gap, nullptr), VS_OK, msg, "");
        for (const float bad : {inf, -inf, std::nanf("")}) {
            std::vector<float> x = c;
            x[x.size() - 1] = bad;
            expect("the last column of the last centroid", fin(x, nullptr), VS_EINVAL, msg, "centroid 2 is not finite at column 4");
            std::vector<float> b = bias;
            b[K - 1] = bad;
            expect("the last bias", fin(c, b.data()), VS_EINVAL, msg, "bias[2]");
        }
    }
    // the half norms
    auto norms = [&](bool ptrs, int32_t K, int32_t V, int64_t ldc) { return assign_check_norms(ptrs, K, V, ldc, msg, sizeof msg); };
    expect("norms ok", norms(true, VS_ASSIGN_MAX_K, 65535, 65535), VS_OK, msg, "");
    expect("norms NULL", norms(false, 1, 8, 8), VS_EINVAL, msg, "NULL");
    expect("norms K = 0", norms(true, 0, 8, 8), VS_EINVAL, msg, "K must");
    expect("norms n_cols = 0", norms(true, 1, 0, 8), VS_EINVAL, msg, "n_cols must");
    expect("norms ldc short", norms(true, 2, 8, 7), VS_EINVAL, msg, "ldc");
    // the label bitmaps
    auto maps = [&](bool ptrs, int64_t n, int32_t B, int64_t bit0, int64_t ld) { return assign_check_bitmaps(ptrs, n, B, bit0, ld, msg, sizeof msg); };
    expect("bitmaps ok", maps(true, 100, 3, 0, 4), VS_OK, msg, "");
    expect("bitmaps ok, the most values", maps(true, 100, VS_LABEL_MAX_VALUES, 31, 5), VS_OK, msg, "");      // 131 bits span 5 words
    expect("bitmaps NULL", maps(false, 100, 3, 0, 4), VS_EINVAL, msg, "NULL");
    expect("bitmaps n_rows = 0", maps(true, 0, 3, 0, 4), VS_EINVAL, msg, "n_rows must");
    expect("bitmaps B = 0", maps(true, 100, 0, 0, 4), VS_EINVAL, msg, "B must");
    expect("bitmaps B = 4097", maps(true, 100, VS_LABEL_MAX_VALUES + 1, 0, 4), VS_EINVAL, msg, "B must");
    expect("bitmaps bit0 < 0", maps(true, 100, 3, -5, 4), VS_EINVAL, msg, "bit0");
    expect("bitmaps bit0 huge", maps(true, 100, 3, std::numeric_limits<int64_t>::max(), 4), VS_EINVAL, msg, "bit0");
    expect("bitmaps ld_words short", maps(true, 100, 3, 31, 4), VS_EINVAL, msg, "ld_words");
    if (failures) return 1;
    puts("assign_check: ok");
    return 0;
}
