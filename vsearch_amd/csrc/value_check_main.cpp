// value_check_main.cpp -- stand-alone driver of value_check.h: the order keys, the bin search, the plan rule and the host-side argument checks
// of the numeric fields.  Not part of the library: tests/test_value_cpu.py builds it with the host compiler under -fsanitize=address,undefined
// and runs it.  The edge arrays live on the heap at their exact size, so a bin search that reads past one is reported by the sanitizer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "value_check.h"

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

static uint32_t f2u(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static float u2f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main() {
    char msg[512] = {0};
    // ---- keys: fp32 -------------------------------------------------------------------------------------------------------------------------
    const float inf = std::numeric_limits<float>::infinity();
    expect_true("-inf is the smallest fp32 key", value_key_f32(f2u(-inf)) == 0x007FFFFFu);
    expect_true("+0 and -0 share a key", value_key_f32(f2u(0.0f)) == value_key_f32(f2u(-0.0f)) && value_key_f32(f2u(0.0f)) == 0x80000000u);
    expect_true("+inf", value_key_f32(f2u(inf)) == 0xFF800000u);
    expect_true("unkey(0) is the sentinel", value_unkey(0u, VS_VAL_F32) == kValueNanF32 && value_unkey(0u, VS_VAL_I32) == kValueMissI32);
    uint32_t state = 12345u;
    for (uint32_t i = 0; i < 2000000u; ++i) {
        state = state * 1664525u + 1013904223u;
        const uint32_t a = state;
        state = state * 1664525u + 1013904223u;
        const uint32_t b = (i & 3u) == 0u ? (a ^ (state & 7u)) : state;            // a quarter of the pairs: neighbours
        const float fa = u2f(a), fb = u2f(b);
        const uint32_t ka = value_key_f32(a), kb = value_key_f32(b);
        if (std::isnan(fa) || std::isnan(fb)) {
            expect_true("NaN is missing", (std::isnan(fa) ? ka == 0u : ka >= 0x007FFFFFu) && (std::isnan(fb) ? kb == 0u : kb >= 0x007FFFFFu));
            continue;
        }
        expect_true("fp32 key order is the float order", (fa < fb) == (ka < kb) && (fa == fb) == (ka == kb));
        const float back = u2f(value_unkey(ka, VS_VAL_F32));
        expect_true("fp32 unkey", back == fa && (fa != 0.0f || f2u(back) == 0u));
        // int32 over the same patterns
        const int32_t ia = (int32_t)a, ib = (int32_t)b;
        expect_true("int32 key order is the integer order", (ia < ib) == (value_key_i32(a) < value_key_i32(b)));
        expect_true("int32 unkey", value_unkey(value_key_i32(a), VS_VAL_I32) == a && (value_key_i32(a) == 0u) == (ia == std::numeric_limits<int32_t>::min()));
    }
    for (uint32_t payload = 1u; payload < 0x00800000u; payload += 4099u)               // NaN patterns of both signs
        expect_true("every NaN is missing", value_key_f32(0x7F800000u | payload) == 0u && value_key_f32(0xFF800000u | payload) == 0u);
    expect_true("denormals order", value_key_f32(f2u(-0x1p-149f)) < value_key_f32(f2u(0.0f)) && value_key_f32(f2u(0.0f)) < value_key_f32(f2u(0x1p-149f)));

    // ---- the bin search against a linear scan, every edge count's shape: exact heap arrays ----------------------------------------------------
    for (int n : {1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025}) {
        std::vector<uint32_t> e((size_t)n);
        for (int i = 0; i < n; ++i) e[(size_t)i] = 0x00800000u + (uint32_t)i * 4000003u;      // ascending, never 0
        auto linear = [&](uint32_t k) { int c = 0; for (int i = 0; i < n; ++i) c += e[(size_t)i] <= k; return c; };
        for (int i = 0; i < n; ++i)
            for (uint32_t d : {0u, 1u, 0xFFFFFFFFu}) {                                       // on the edge, one above, one below
                const uint32_t k = e[(size_t)i] + d;
                expect_true("bin search on an edge", value_bin(e.data(), n, k) == linear(k));
            }
        for (uint32_t k : {0u, 1u, 0x007FFFFFu, 0x80000000u, 0xFFFFFFFFu}) expect_true("bin search at the ends", value_bin(e.data(), n, k) == linear(k));
        for (int i = 0; i < 20000; ++i) {
            state = state * 1664525u + 1013904223u;
            expect_true("bin search sweep", value_bin(e.data(), n, state) == linear(state));
        }
    }

    // ---- the plan rule ---------------------------------------------------------------------------------------------------------------------------
    ValuePlan p;
    auto plan = [&](int64_t n, int32_t B, int32_t bins, bool pq, int64_t rpc, int32_t qt) { return value_plan(n, B, bins, pq, rpc, qt, &p, msg, sizeof msg); };
    expect("plan ok", plan(21015324, 8, 1027, true, 0, 8), VS_OK, msg, "");
    expect_true("plan: one tile of 8, <= 1024 chunks of whole spans",
                p.qt == 8 && p.rows_per_chunk % 2048 == 0 && p.chunks <= 1024 && p.chunks * p.rows_per_chunk >= 21015324 &&
                    (p.chunks - 1) * p.rows_per_chunk < 21015324);
    expect("plan shared", plan(1000, 1, 0, false, 0, 8), VS_OK, msg, "");
    expect_true("plan shared: qt 1, one chunk of the floor", p.qt == 1 && p.chunks == 1 && p.rows_per_chunk == 8192);
    expect("plan given", plan(3 * 2048 + 1, 17, 4, true, 2048, 8), VS_OK, msg, "");
    expect_true("plan given: taken as it is", p.chunks == 4 && p.rows_per_chunk == 2048 && p.qt == 8);
    expect("plan topk", plan(3 * 2048 + 1, 17, 0, true, 64, 1), VS_OK, msg, "");
    expect_true("plan topk: one query a workgroup", p.qt == 1 && p.rows_per_chunk == 64 && p.chunks == 97);
    expect("plan floor", plan(1 << 20, 1, 1027, true, 0, 8), VS_OK, msg, "");
    expect_true("plan: 16 rows a bin at least", p.rows_per_chunk == 16384 + 2048 && p.rows_per_chunk >= 16 * 1027);
    expect("n_rows 0", plan(0, 1, 0, true, 0, 8), VS_EINVAL, msg, "n_rows");
    expect("n_rows 2^32", plan(1ll << 32, 1, 0, true, 0, 8), VS_EINVAL, msg, "n_rows");
    expect("B 0", plan(10, 0, 0, true, 0, 8), VS_EINVAL, msg, "B must");
    expect("bins", plan(10, 1, VS_VALUE_MAX_EDGES + 3, true, 0, 8), VS_EINVAL, msg, "n_bins");
    expect("bins < 0", plan(10, 1, -1, true, 0, 8), VS_EINVAL, msg, "n_bins");
    expect("shared B 2", plan(10, 2, 0, false, 0, 8), VS_EINVAL, msg, "ld_words = 0");
    expect("rpc 100", plan(10, 1, 0, true, 100, 8), VS_EINVAL, msg, "multiple of 64");
    expect("rpc < 0", plan(10, 1, 0, true, -64, 8), VS_EINVAL, msg, "multiple of 64");
    expect("too many tiles", plan(10, 65536 * 8, 0, true, 0, 8), VS_EINVAL, msg, "too many");
    expect("max rows", plan(0xFFFFFFFFll, 1, 0, true, 64, 8), VS_OK, msg, "");
    expect_true("max rows: 2^26 chunks", p.chunks == 1ll << 26);

    // ---- the checks of the calls --------------------------------------------------------------------------------------------------------------------
    auto set = [&](bool ptrs, bool words, int64_t bit0, int64_t ld, int32_t B, int dt, int64_t n) {
        return value_check_set(ptrs, words, bit0, ld, B, dt, n, 0, 0, 8, &p, msg, sizeof msg);
    };
    expect("set ok", set(true, true, 33, 4, 3, VS_VAL_F32, 64), VS_OK, msg, "");
    expect("set NULL", set(false, true, 0, 4, 3, VS_VAL_F32, 64), VS_EINVAL, msg, "NULL");
    expect("set dtype", set(true, true, 0, 4, 3, 2, 64), VS_EINVAL, msg, "dtype");
    expect("set bit0", set(true, true, -1, 4, 3, VS_VAL_I32, 64), VS_EINVAL, msg, "bit0");
    expect("set ld short", set(true, true, 33, 3, 3, VS_VAL_I32, 64), VS_EINVAL, msg, "ld_words");
    expect("set ld < 0", set(true, true, 0, -1, 1, VS_VAL_I32, 64), VS_EINVAL, msg, "ld_words");
    expect("set no words B 2", set(true, false, 0, 0, 2, VS_VAL_I32, 64), VS_EINVAL, msg, "ld_words = 0");
    expect("set no words", set(true, false, 0, 0, 1, VS_VAL_I32, 64), VS_OK, msg, "");
    expect("hist ok", value_check_hist(2, 1, msg, sizeof msg), VS_OK, msg, "");
    expect("hist max", value_check_hist(VS_VALUE_MAX_EDGES, 1024, msg, sizeof msg), VS_OK, msg, "");
    expect("hist 1 edge", value_check_hist(1, 4, msg, sizeof msg), VS_EINVAL, msg, "n_edges");
    expect("hist 1026 edges", value_check_hist(1026, 2000, msg, sizeof msg), VS_EINVAL, msg, "n_edges");
    expect("hist ld", value_check_hist(5, 3, msg, sizeof msg), VS_EINVAL, msg, "ld_counts");
    {
        std::vector<uint32_t> e = {f2u(-inf), f2u(-1.0f), f2u(-0.0f), f2u(0x1p-149f), f2u(inf)};
        expect("edges ok", value_check_edges_host(e.data(), 5, VS_VAL_F32, msg, sizeof msg), VS_OK, msg, "");
        std::vector<uint32_t> z = {f2u(-0.0f), f2u(0.0f)};
        expect("edges -0 +0", value_check_edges_host(z.data(), 2, VS_VAL_F32, msg, sizeof msg), VS_EINVAL, msg, "ascending");
        std::vector<uint32_t> nn = {f2u(1.0f), f2u(std::nanf(""))};
        expect("edges NaN", value_check_edges_host(nn.data(), 2, VS_VAL_F32, msg, sizeof msg), VS_EINVAL, msg, "missing");
        std::vector<uint32_t> d = {f2u(2.0f), f2u(1.0f)};
        expect("edges descending", value_check_edges_host(d.data(), 2, VS_VAL_F32, msg, sizeof msg), VS_EINVAL, msg, "ascending");
        std::vector<uint32_t> i = {0x80000001u, 0xFFFFFFFFu, 0u, 0x7FFFFFFFu};                  // INT32_MIN + 1, -1, 0, INT32_MAX
        expect("int edges ok", value_check_edges_host(i.data(), 4, VS_VAL_I32, msg, sizeof msg), VS_OK, msg, "");
        std::vector<uint32_t> m = {0x80000000u, 0u};
        expect("int edges missing", value_check_edges_host(m.data(), 2, VS_VAL_I32, msg, sizeof msg), VS_EINVAL, msg, "missing");
        std::vector<uint32_t> lo = {f2u(-inf), f2u(2.0f)}, hi = {f2u(inf), f2u(1.0f)}, bad = {f2u(1.0f), f2u(std::nanf(""))};
        expect("bounds ok", value_check_bounds_host(lo.data(), hi.data(), 2, VS_VAL_F32, msg, sizeof msg), VS_OK, msg, "");
        expect("bounds NaN", value_check_bounds_host(lo.data(), bad.data(), 2, VS_VAL_F32, msg, sizeof msg), VS_EINVAL, msg, "missing bound");
        expect("bounds INT32_MIN", value_check_bounds_host(m.data(), i.data(), 2, VS_VAL_I32, msg, sizeof msg), VS_EINVAL, msg, "missing bound");
    }
    expect("topk plan", plan(10000, 4, 0, true, 64, 1), VS_OK, msg, "");
    expect("topk ok", value_check_topk(1024, 4, p, msg, sizeof msg), VS_OK, msg, "");
    expect("topk k 0", value_check_topk(0, 4, p, msg, sizeof msg), VS_EINVAL, msg, "k must");
    expect("topk k 1025", value_check_topk(1025, 4, p, msg, sizeof msg), VS_EINVAL, msg, "k must");
    expect("topk plan big", plan(0xFFFFFFFFll, 4, 0, true, 64, 1), VS_OK, msg, "");
    expect("topk scratch", value_check_topk(1024, 4, p, msg, sizeof msg), VS_EINVAL, msg, "scratch");
    auto ranges = [&](bool ptrs, int dt, int64_t n, int32_t B, int64_t bit0, int64_t ld) { return value_check_ranges(ptrs, dt, n, B, bit0, ld, msg, sizeof msg); };
    expect("ranges ok", ranges(true, VS_VAL_I32, 100, VS_VALUE_MAX_RANGES, 33, 5), VS_OK, msg, "");
    expect("ranges NULL", ranges(false, VS_VAL_I32, 100, 1, 0, 4), VS_EINVAL, msg, "NULL");
    expect("ranges dtype", ranges(true, -1, 100, 1, 0, 4), VS_EINVAL, msg, "dtype");
    expect("ranges n", ranges(true, VS_VAL_I32, 0, 1, 0, 4), VS_EINVAL, msg, "n_rows");
    expect("ranges B", ranges(true, VS_VAL_I32, 100, VS_VALUE_MAX_RANGES + 1, 0, 4), VS_EINVAL, msg, "B must");
    expect("ranges B 0", ranges(true, VS_VAL_I32, 100, 0, 0, 4), VS_EINVAL, msg, "B must");
    expect("ranges bit0", ranges(true, VS_VAL_I32, 100, 1, -1, 4), VS_EINVAL, msg, "bit0");
    expect("ranges ld", ranges(true, VS_VAL_I32, 100, 1, 33, 4), VS_EINVAL, msg, "ld_words");

    if (failures) {
        fprintf(stderr, "value_check: %d failures\n", failures);
        return 1;
    }
    printf("value_check: ok\n");
    return 0;
}
