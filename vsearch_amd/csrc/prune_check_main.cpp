// prune_check_main.cpp -- stand-alone driver of prune_check.h: the plan rule, every argument check, the three cell functions the kernels of
// prune.hip run, and the radix select composed of them the way the select kernel composes it (four rounds of 8 bits from the top, then the
// first cells of the tie group in stored order) against a plain sort, on heap arrays at their exact size.
// Not part of the library: tests/test_prune_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "prune_check.h"

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

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

// the select kernel's selection of one row, on the host: which eligible cells are in the top m
static std::vector<uint8_t> select_by_radix(const std::vector<uint32_t>& keys, const std::vector<uint8_t>& elig, uint32_t m) {
    const size_t n = keys.size();
    std::vector<uint8_t> top(n, 0);
    uint32_t n_elig = 0;
    for (size_t t = 0; t < n; ++t) n_elig += elig[t];
    if (m == 0 || n_elig <= m) return elig;
    uint32_t prefix = 0u, pmask = 0u, need = m;
    for (int round = 3; round >= 0; --round) {
        std::vector<uint32_t> hist((size_t)kPruneBins, 0u);
        for (size_t t = 0; t < n; ++t)
            if (elig[t] && (keys[t] & pmask) == prefix) ++hist[prune_digit(keys[t], round)];
        uint32_t acc = 0u, digit = 0u;
        for (int d = kPruneBins - 1; d >= 0; --d) {
            if (acc < need && need <= acc + hist[(size_t)d]) {
                digit = (uint32_t)d;
                break;
            }
            acc += hist[(size_t)d];
        }
        need -= acc;
        prefix |= digit << (8 * round);
        pmask |= 0xFFu << (8 * round);
    }
    int64_t seen = 0;                                          // cells of the tie group before this packet
    for (size_t p0 = 0; p0 < n; p0 += 8) {
        uint32_t gt = 0u, eq = 0u;
        const size_t cells = std::min<size_t>(8, n - p0);
        for (size_t t = 0; t < cells; ++t) {
            if (!elig[p0 + t]) continue;
            gt |= (keys[p0 + t] > prefix ? 1u : 0u) << t;
            eq |= (keys[p0 + t] == prefix ? 1u : 0u) << t;
        }
        const int64_t left = (int64_t)need - seen;
        const uint32_t kb = gt | prune_first_bits(eq, left < 0 ? 0 : (left > 8 ? 8 : (int)left));
        for (size_t t = 0; t < cells; ++t) top[p0 + t] = (uint8_t)((kb >> t) & 1u);
        seen += __builtin_popcount(eq);
    }
    return top;
}

static std::vector<uint8_t> select_by_sort(const std::vector<uint32_t>& keys, const std::vector<uint8_t>& elig, uint32_t m) {
    std::vector<size_t> order;
    for (size_t t = 0; t < keys.size(); ++t)
        if (elig[t]) order.push_back(t);
    if (m == 0 || order.size() <= m) return elig;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return keys[a] > keys[b]; });
    std::vector<uint8_t> top(keys.size(), 0);
    for (size_t i = 0; i < m; ++i) top[order[i]] = 1;
    return top;
}

int main() {
    char msg[512] = {0};
    // ---- the order key the selection ranks by (value_check.h) --------------------------------------------------------------------------------------
    {
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        const float asc[] = {-inf, -3.5f, -1e-30f, 0.0f, 1e-30f, 2.0f, inf};
        for (int i = 0; i + 1 < 7; ++i) expect_true("keys ascend with the values", value_key_f32(bits_of(asc[i])) < value_key_f32(bits_of(asc[i + 1])));
        expect_true("-0.0 ties +0.0", value_key_f32(bits_of(-0.0f)) == value_key_f32(bits_of(0.0f)));
        expect_true("a NaN of either sign ranks last", value_key_f32(bits_of(nan)) == 0u && value_key_f32(bits_of(-nan)) == 0u &&
                                                          value_key_f32(bits_of(-inf)) > 0u);
        expect_true("min_value: a NaN is never >=", !prune_value_ok(nan, true, -inf) && prune_value_ok(nan, false, 0.f) && prune_value_ok(1.f, true, 1.f) &&
                                                        !prune_value_ok(0.5f, true, 1.f) && prune_value_ok(-0.0f, true, 0.0f));
    }
    // ---- digits and tie bits -------------------------------------------------------------------------------------------------------------------------
    expect_true("digits", prune_digit(0xA1B2C3D4u, 3) == 0xA1u && prune_digit(0xA1B2C3D4u, 2) == 0xB2u && prune_digit(0xA1B2C3D4u, 1) == 0xC3u &&
                              prune_digit(0xA1B2C3D4u, 0) == 0xD4u);
    expect_true("first bits", prune_first_bits(0xB6u, 0) == 0u && prune_first_bits(0xB6u, -3) == 0u && prune_first_bits(0xB6u, 1) == 0x02u &&
                                  prune_first_bits(0xB6u, 3) == 0x16u && prune_first_bits(0xB6u, 5) == 0xB6u && prune_first_bits(0xB6u, 8) == 0xB6u &&
                                  prune_first_bits(0u, 8) == 0u);
    // ---- the radix select against a sort -------------------------------------------------------------------------------------------------------------
    {
        uint32_t state = 7u;
        auto next = [&]() { return state = state * 1664525u + 1013904223u; };
        for (int law = 0; law < 5; ++law)
            for (size_t n : {(size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)63, (size_t)513, (size_t)1025, (size_t)2051}) {
                std::vector<uint32_t> keys(n);
                std::vector<uint8_t> elig(n);
                for (size_t t = 0; t < n; ++t) {
                    const uint32_t x = next() >> 4;
                    keys[t] = law == 0 ? x : law == 1 ? 0x80000000u + (x & 3u) : law == 2 ? 0xC0FFEE00u : law == 3 ? (x & 0xFF00FF00u) : (x % 5u == 0u ? 0u : x << 4);
                    elig[t] = law == 2 ? 1 : (uint8_t)((next() >> 9) % 4u != 0u);
                }
                for (uint32_t m : {1u, 2u, 7u, 8u, 9u, (uint32_t)(n / 2), (uint32_t)n - 1u, (uint32_t)n, (uint32_t)n + 1u, 65535u, 0u})
                    expect_true("the radix select equals the sort", select_by_radix(keys, elig, m) == select_by_sort(keys, elig, m));
            }
    }
    // ---- the plan rule ----------------------------------------------------------------------------------------------------------------------------------
    PrunePlan p;
    expect("plan headline", prune_plan(21015324, 21015324ll * 96, 29523, VS_F32, 256, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan headline: 1024 register cells, 44 KB of LDS, 2 GB of keep bytes",
                p.reg_cells == 1024 && p.reg_cells >= 768 && p.lds_bytes == 4 * (923 + 1024 + 4 * 923) && p.scan_blocks == 5131 &&
                    p.scratch_bytes == 21015324ll * 96 + 4 * 21015324ll + 8 * 5132 + 8);
    expect("plan no protect", prune_plan(1000, 5000, 300, VS_F16, 0, false, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan no protect: col_keep and the histograms", p.lds_bytes == 4 * (10 + 1024) && p.scan_blocks == 1 && p.scratch_bytes == 5000 + 4000 + 16 + 8);
    expect("plan binary col_keep", prune_plan(10, 10, 65535, VS_NONE, 0, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan widest: 8 KB of col_keep, 32 KB of protect bitmaps", p.lds_bytes == 4 * (2048 + 1024 + 4 * 2048));
    expect("plan empty", prune_plan(0, 0, 5, VS_F32, 3, false, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan empty: one scan block", p.scan_blocks == 1);
    expect("plan rows", prune_plan(-1, 0, 5, VS_F32, 3, false, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("plan rows 2^32 - 1", prune_plan(0xFFFFFFFFll, 0, 5, VS_F32, 3, false, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("plan packets", prune_plan(1, 1ll << 32, 5, VS_F32, 3, false, &p, msg, sizeof msg), VS_EINVAL, msg, "n_packets");
    expect("plan cols 0", prune_plan(1, 1, 0, VS_F32, 3, false, &p, msg, sizeof msg), VS_EINVAL, msg, "n_cols");
    expect("plan cols 65536", prune_plan(1, 1, 65536, VS_F32, 3, false, &p, msg, sizeof msg), VS_EUNSUPPORTED, msg, "uint16");
    expect("plan topk -1", prune_plan(1, 1, 5, VS_F32, -1, false, &p, msg, sizeof msg), VS_EINVAL, msg, "topk must");
    expect("plan topk 65536", prune_plan(1, 1, 5, VS_F32, 65536, false, &p, msg, sizeof msg), VS_EINVAL, msg, "topk must");
    expect("plan binary topk", prune_plan(1, 1, 5, VS_NONE, 3, false, &p, msg, sizeof msg), VS_EINVAL, msg, "binary");
    expect("plan store", prune_plan(1, 1, 5, VS_I64, 3, false, &p, msg, sizeof msg), VS_EINVAL, msg, "store_dtype");
    // ---- the checks ----------------------------------------------------------------------------------------------------------------------------------------
    expect("rules ok", prune_check_rules(65535, true, VS_F16, msg, sizeof msg), VS_OK, msg, "");
    expect("rules binary col_keep", prune_check_rules(0, false, VS_NONE, msg, sizeof msg), VS_OK, msg, "");
    expect("rules binary min", prune_check_rules(0, true, VS_NONE, msg, sizeof msg), VS_EINVAL, msg, "binary");
    expect("rules binary topk", prune_check_rules(1, false, VS_NONE, msg, sizeof msg), VS_EINVAL, msg, "binary");
    PruneShape src, prot;
    src.n_rows = prot.n_rows = 100;
    src.n_cols = prot.n_cols = 300;
    prot.store_dtype = VS_NONE;
    expect("source ok", prune_check_source(src, msg, sizeof msg), VS_OK, msg, "");
    expect("protect ok", prune_check_protect(src, prot, msg, sizeof msg), VS_OK, msg, "");
    {
        PruneShape d = src;
        d.kind = VS_KIND_DENSE;
        expect("source dense", prune_check_source(d, msg, sizeof msg), VS_EUNSUPPORTED, msg, "dense");
        expect("protect dense", prune_check_protect(src, d, msg, sizeof msg), VS_EINVAL, msg, "CSR");
        PruneShape q = prot;
        q.n_rows = 99;
        expect("protect rows", prune_check_protect(src, q, msg, sizeof msg), VS_EINVAL, msg, "99 x 300");
        q = prot;
        q.n_cols = 301;
        expect("protect cols", prune_check_protect(src, q, msg, sizeof msg), VS_EINVAL, msg, "100 x 301");
        q = prot;
        q.device = 1;
        expect("protect device", prune_check_protect(src, q, msg, sizeof msg), VS_EINVAL, msg, "device 1");
    }
    expect("pointers host", prune_check_pointers(true, false, true, false, msg, sizeof msg), VS_OK, msg, "");
    expect("pointers device", prune_check_pointers(true, true, true, true, msg, sizeof msg), VS_OK, msg, "");
    expect("pointers one", prune_check_pointers(true, true, false, false, msg, sizeof msg), VS_OK, msg, "");
    expect("pointers mixed", prune_check_pointers(true, true, true, false, msg, sizeof msg), VS_EINVAL, msg, "both");
    expect("pointers mixed 2", prune_check_pointers(true, false, true, true, msg, sizeof msg), VS_EINVAL, msg, "both");
    expect("extra ok", new_index_check_extra(0, 5, msg, sizeof msg), VS_OK, msg, "");
    expect("extra rows", new_index_check_extra(-1, 0, msg, sizeof msg), VS_EINVAL, msg, ">= 0");
    expect("extra packets", new_index_check_extra(0, -1, msg, sizeof msg), VS_EINVAL, msg, ">= 0");
    expect("capacity ok", new_index_check_capacity("pruned", 100, 1000, 5, 7, msg, sizeof msg), VS_OK, msg, "");
    expect("capacity rows", new_index_check_capacity("pruned", 0xFFFFFFF0ll, 10, 0xF, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect("capacity packets", new_index_check_capacity("pruned", 10, 0xFFFFFFF0ll, 0, 0x10, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect("capacity huge extra", new_index_check_capacity("pruned", 10, 10, 0x7FFFFFFFFFFFFFFFll, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");

    if (failures) {
        fprintf(stderr, "prune_check: %d failures\n", failures);
        return 1;
    }
    printf("prune_check: ok\n");
    return 0;
}
