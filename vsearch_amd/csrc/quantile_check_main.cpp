// quantile_check_main.cpp -- stand-alone driver of quantile_check.h: the digits of the three radix levels, the quantile -> rank rule, the bin
// search of the step, the slot search of the counting kernel, the plan rule and the argument checks of the percentiles.  Not part of the
// library: tests/test_quantile_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.  The prefix sums and the
// slot lists live on the heap at their exact size, so a search that reads past one is reported by the sanitizer.  It ends with a radix select
// over random keys, composed of the header's functions alone, against a sort.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "quantile_check.h"

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

// one level of the select over sorted-or-not keys: the bins of the keys whose prefix is `prefix`, scanned, searched
static bool select_level(const std::vector<uint32_t>& keys, int level, uint32_t prefix, int64_t* r, uint32_t* next) {
    const int bins = radix_bins(level);
    std::vector<int64_t> cum((size_t)bins + 1, 0);
    for (uint32_t k : keys)
        if (k != 0u && radix_prefix(k, level) == prefix) ++cum[(size_t)radix_digit(k, level) + 1];
    for (int i = 0; i < bins; ++i) cum[(size_t)i + 1] += cum[(size_t)i];
    const int d = radix_find_bin(cum.data(), bins, *r);
    if (d < 0) return false;
    *r -= cum[(size_t)d];
    *next = radix_extend(prefix, level, (uint32_t)d);
    return true;
}

int main() {
    char msg[512] = {0};
    // ---- the digits ------------------------------------------------------------------------------------------------------------------------------
    for (uint32_t k : {1u, 0x001FFFFFu, 0x00200000u, 0x7FFFFFFFu, 0x80000000u, 0xFFE003FFu, 0xFFFFFFFFu}) {
        const uint32_t d0 = radix_digit(k, 0), d1 = radix_digit(k, 1), d2 = radix_digit(k, 2);
        expect_true("digits are in range", d0 < 2048u && d1 < 2048u && d2 < 1024u);
        expect_true("the digits spell the key", ((d0 << 21) | (d1 << 10) | d2) == k);
        expect_true("prefixes", radix_prefix(k, 0) == 0u && radix_prefix(k, 1) == d0 && radix_prefix(k, 2) == ((d0 << 11) | d1));
        expect_true("extend", radix_extend(radix_extend(radix_extend(0u, 0, d0), 1, d1), 2, d2) == k);
        expect_true("no prefix is the pad", radix_prefix(k, 1) != kRadixNoSlot && radix_prefix(k, 2) != kRadixNoSlot);
    }
    expect_true("bins", radix_bins(0) == 2048 && radix_bins(1) == 2048 && radix_bins(2) == 1024);

    // ---- quantile -> rank -------------------------------------------------------------------------------------------------------------------------
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int64_t big = 0xFFFFFFFFll;                                                    // 2^32 - 1 rows
    for (int m : {VS_QUANTILE_LOWER, VS_QUANTILE_HIGHER, VS_QUANTILE_NEAREST}) {
        expect_true("count 0", quantile_rank(0.0, 0, m) == -1 && quantile_rank(0.5, 0, m) == -1 && quantile_rank(1.0, 0, m) == -1);
        expect_true("count 1", quantile_rank(0.0, 1, m) == 0 && quantile_rank(0.37, 1, m) == 0 && quantile_rank(1.0, 1, m) == 0);
        expect_true("count 2 ends", quantile_rank(0.0, 2, m) == 0 && quantile_rank(1.0, 2, m) == 1);
        expect_true("count 2^32 - 1 ends", quantile_rank(0.0, big, m) == 0 && quantile_rank(1.0, big, m) == big - 1);
        expect_true("q outside", quantile_rank(-0.0000001, 5, m) == -1 && quantile_rank(1.0000001, 5, m) == -1 && quantile_rank(nan, 5, m) == -1);
        expect_true("q = -0.0 is 0", quantile_rank(-0.0, 5, m) == 0);
    }
    expect_true("count 2 middle", quantile_rank(0.5, 2, VS_QUANTILE_LOWER) == 0 && quantile_rank(0.5, 2, VS_QUANTILE_HIGHER) == 1 &&
                                      quantile_rank(0.5, 2, VS_QUANTILE_NEAREST) == 0);              // 0.5: half to even
    expect_true("half to even", quantile_rank(0.5, 4, VS_QUANTILE_NEAREST) == 2 && quantile_rank(0.25, 3, VS_QUANTILE_NEAREST) == 0 &&
                                    quantile_rank(0.75, 3, VS_QUANTILE_NEAREST) == 2);               // 1.5 -> 2, 0.5 -> 0, 1.5 -> 2
    expect_true("2^32 - 1 middle", quantile_rank(0.5, big, VS_QUANTILE_LOWER) == (big - 1) / 2 && quantile_rank(0.5, big, VS_QUANTILE_HIGHER) == (big - 1) / 2);
    {
        uint32_t state = 99u;
        for (int i = 0; i < 200000; ++i) {
            state = state * 1664525u + 1013904223u;
            const int64_t count = 1 + (int64_t)(state % 100000u);
            state = state * 1664525u + 1013904223u;
            const double q = (double)state / 4294967295.0;
            const int64_t lo = quantile_rank(q, count, VS_QUANTILE_LOWER), hi = quantile_rank(q, count, VS_QUANTILE_HIGHER),
                          ne = quantile_rank(q, count, VS_QUANTILE_NEAREST);
            expect_true("ranks are ordered and inside", 0 <= lo && lo <= ne && ne <= hi && hi <= count - 1 && hi - lo <= 1);
        }
    }
    expect_true("given ranks", quantile_rank_given(0, 1) == 0 && quantile_rank_given(1, 1) == -1 && quantile_rank_given(-1, 5) == -1 &&
                                   quantile_rank_given(4, 5) == 4 && quantile_rank_given(0, 0) == -1);

    // ---- the bin search of the step against a linear scan: exact heap arrays -------------------------------------------------------------------------
    {
        uint32_t state = 7u;
        for (int bins : {1024, 2048})
            for (int shape = 0; shape < 6; ++shape) {
                std::vector<int64_t> cnt((size_t)bins, 0);
                for (int i = 0; i < bins; ++i) {
                    state = state * 1664525u + 1013904223u;
                    const uint32_t x = state >> 8;
                    cnt[(size_t)i] = shape == 0 ? 1 : shape == 1 ? (x % 7u == 0u ? x % 1000u : 0) : shape == 2 ? 0 : shape == 3 ? (int64_t)x << 20 : x % 3u;
                }
                if (shape == 2) cnt[(size_t)bins - 1] = 5;                                // everything in the last bin
                if (shape == 4) std::fill(cnt.begin() + 1, cnt.end(), 0), cnt[0] = 3;     // everything in the first
                if (shape == 5) std::fill(cnt.begin(), cnt.end(), 0);                     // an empty slot
                std::vector<int64_t> cum((size_t)bins + 1, 0);
                for (int i = 0; i < bins; ++i) cum[(size_t)i + 1] = cum[(size_t)i] + cnt[(size_t)i];
                const int64_t total = cum[(size_t)bins];
                auto linear = [&](int64_t r) {
                    if (r < 0 || r >= total) return -1;
                    for (int d = 0; d < bins; ++d)
                        if (cum[(size_t)d] <= r && r < cum[(size_t)d] + cnt[(size_t)d]) return d;
                    return -2;
                };
                for (int64_t r : {(int64_t)-1, (int64_t)0, (int64_t)1, total / 2, total - 1, total, total + 1})
                    expect_true("bin search at the ends", radix_find_bin(cum.data(), bins, r) == linear(r));
                for (int i = 0; i < bins; ++i)
                    for (int64_t r : {cum[(size_t)i] - 1, cum[(size_t)i]}) expect_true("bin search on a boundary", radix_find_bin(cum.data(), bins, r) == linear(r));
            }
    }

    // ---- the slot search: 16 exact slots, every fill ---------------------------------------------------------------------------------------------------
    for (int n = 0; n <= 16; ++n) {
        std::vector<uint32_t> sp(16, kRadixNoSlot);
        for (int i = 0; i < n; ++i) sp[(size_t)i] = (uint32_t)i * 262139u;                  // ascending, 22 bits at most, 0 among them
        for (int i = 0; i < n; ++i) {
            expect_true("slot found", radix_find_slot(sp.data(), sp[(size_t)i]) == i);
            expect_true("slot next to one", radix_find_slot(sp.data(), sp[(size_t)i] + 1u) == -1);
        }
        expect_true("no slot", radix_find_slot(sp.data(), 0x3FFFFFu) == -1 && (n > 0 || radix_find_slot(sp.data(), 0u) == -1));
    }

    // ---- the plan rule ----------------------------------------------------------------------------------------------------------------------------------
    ValuePlan p;
    const int want_qt[17] = {0, 8, 8, 4, 4, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1};
    for (int R = 1; R <= 16; ++R) {
        expect("plan ok", quantile_plan(21015324, 9, R, true, 0, &p, msg, sizeof msg), VS_OK, msg, "");
        expect_true("plan qt by R", p.qt == want_qt[R] && quantile_qt(R, false) == 1);
        expect_true("plan: 128 KiB at most", quantile_lds_bytes(p.qt, R, 1) <= 128u * 1024u && quantile_lds_bytes(p.qt, R, 2) <= 64u * 1024u &&
                                                 quantile_lds_bytes(p.qt, R, 0) == (size_t)p.qt * 8192u);
        ValuePlan v;
        expect("plan chunks", value_plan(21015324, 9, 0, true, 0, p.qt, &v, msg, sizeof msg), VS_OK, msg, "");
        expect_true("plan: value_plan's chunks", v.chunks == p.chunks && v.rows_per_chunk == p.rows_per_chunk);
    }
    expect("plan shared", quantile_plan(1000, 1, 7, false, 0, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan shared: qt 1", p.qt == 1 && p.chunks == 1 && p.rows_per_chunk == 8192);
    expect("plan given", quantile_plan(3 * 2048 + 1, 17, 3, true, 2048, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan given: taken as it is", p.qt == 4 && p.chunks == 4 && p.rows_per_chunk == 2048);
    expect("plan R 0", quantile_plan(100, 1, 0, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "R must");
    expect("plan R 17", quantile_plan(100, 1, 17, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "R must");
    expect("plan n 0", quantile_plan(0, 1, 1, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("plan rpc", quantile_plan(100, 1, 1, true, 100, &p, msg, sizeof msg), VS_EINVAL, msg, "multiple of 64");
    expect("plan shared B 2", quantile_plan(100, 2, 1, false, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "ld_words = 0");

    // ---- the checks -----------------------------------------------------------------------------------------------------------------------------------------
    expect("level ok", quantile_check_level(2, msg, sizeof msg), VS_OK, msg, "");
    expect("level 3", quantile_check_level(3, msg, sizeof msg), VS_EINVAL, msg, "level");
    expect("level -1", quantile_check_level(-1, msg, sizeof msg), VS_EINVAL, msg, "level");
    expect("method ok", quantile_check_method(VS_QUANTILE_NEAREST, msg, sizeof msg), VS_OK, msg, "");
    expect("method 3", quantile_check_method(3, msg, sizeof msg), VS_EINVAL, msg, "method");
    expect("scratch ok", quantile_check_scratch(4096, 16, msg, sizeof msg), VS_OK, msg, "");
    expect("scratch big", quantile_check_scratch(4097, 16, msg, sizeof msg), VS_EINVAL, msg, "2^27");
    {
        std::vector<double> q = {0.0, 0.5, 1.0, -0.0};
        expect("q ok", quantile_check_q_host(q.data(), 4, msg, sizeof msg), VS_OK, msg, "");
        std::vector<double> b1 = {0.5, 1.0000000000000002}, b2 = {nan}, b3 = {-1e-300};
        expect("q above", quantile_check_q_host(b1.data(), 2, msg, sizeof msg), VS_EINVAL, msg, "q[1]");
        expect("q NaN", quantile_check_q_host(b2.data(), 1, msg, sizeof msg), VS_EINVAL, msg, "outside");
        expect("q below", quantile_check_q_host(b3.data(), 1, msg, sizeof msg), VS_EINVAL, msg, "outside");
        std::vector<int64_t> r = {0, 5, std::numeric_limits<int64_t>::max()}, rb = {0, -1};
        expect("ranks ok", quantile_check_ranks_host(r.data(), 3, msg, sizeof msg), VS_OK, msg, "");
        expect("ranks negative", quantile_check_ranks_host(rb.data(), 2, msg, sizeof msg), VS_EINVAL, msg, "negative");
    }

    // ---- a whole select, composed of the functions above, against a sort ---------------------------------------------------------------------------------
    {
        uint32_t state = 2024u;
        for (int shape = 0; shape < 4; ++shape) {
            std::vector<uint32_t> keys;
            for (int i = 0; i < 3000; ++i) {
                state = state * 1664525u + 1013904223u;
                const uint32_t k = shape == 0 ? state : shape == 1 ? 0x80000000u + (state % 130u) : shape == 2 ? 0xFFFFFFFFu - (state % 3u) : 1u + (state % 5000u);
                keys.push_back(i % 11 == 0 ? 0u : k);                                       // every eleventh row is missing
            }
            std::vector<uint32_t> sorted;
            for (uint32_t k : keys)
                if (k) sorted.push_back(k);
            std::sort(sorted.begin(), sorted.end());
            for (int64_t rank : {(int64_t)0, (int64_t)1, (int64_t)sorted.size() / 2, (int64_t)sorted.size() - 1}) {
                int64_t r = rank;
                uint32_t prefix = 0u;
                bool ok = true;
                for (int level = 0; level < VS_VALUE_RADIX_LEVELS && ok; ++level) ok = select_level(keys, level, prefix, &r, &prefix);
                expect_true("radix select equals the sort", ok && prefix == sorted[(size_t)rank]);
            }
            int64_t r = (int64_t)sorted.size();
            uint32_t prefix = 0u;
            expect_true("a rank at the count has no answer", !select_level(keys, 0, 0u, &r, &prefix));
        }
    }

    if (failures) {
        fprintf(stderr, "quantile_check: %d failures\n", failures);
        return 1;
    }
    printf("quantile_check: ok\n");
    return 0;
}
