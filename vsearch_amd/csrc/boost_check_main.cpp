// boost_check_main.cpp -- stand-alone driver of boost_check.h: the pinned arithmetic of boosted search (boost_apply) and the host-side argument
// checks of vs_index_search_boosted.  Not part of the library: tests/test_boost_cpu.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it.
//   boost_check                 the argument checks and a few hand-made tuples
//   boost_check IN OUT          IN: int32 n, then n records {double S; float w[4]; uint32 raw[4]; int32 dtype[4]; int32 F; int32 mode} (64 bytes);
//                               OUT: n records {uint32 ok; uint32 bits of the boosted score} -- the test holds them against numpy's bits.
// The weights, values and dtypes of a record are copied to heap arrays of exactly F entries, so a read past F is reported by the sanitizer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "boost_check.h"

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

struct Record {
    double S;
    float w[4];
    uint32_t raw[4];
    int32_t dtype[4];
    int32_t F;
    int32_t mode;
};
static_assert(sizeof(Record) == 64, "the record layout the test writes");

static bool apply(const Record& r, float* out) {
    const size_t F = (size_t)r.F;
    std::vector<float> w(r.w, r.w + F);
    std::vector<uint32_t> raw(r.raw, r.raw + F);
    std::vector<int32_t> dt(r.dtype, r.dtype + F);
    return boost_apply(r.S, w.data(), raw.data(), dt.data(), r.F, r.mode, out);
}

static int run_file(const char* in, const char* out) {
    FILE* fi = fopen(in, "rb");
    if (!fi) return fprintf(stderr, "cannot open %s\n", in), 2;
    int32_t n = 0;
    if (fread(&n, 4, 1, fi) != 1 || n < 0) return fclose(fi), fprintf(stderr, "bad header\n"), 2;
    std::vector<Record> recs((size_t)n);
    if (n && fread(recs.data(), sizeof(Record), (size_t)n, fi) != (size_t)n) return fclose(fi), fprintf(stderr, "short file\n"), 2;
    fclose(fi);
    std::vector<uint32_t> res((size_t)n * 2);
    for (int32_t i = 0; i < n; ++i) {
        const Record& r = recs[(size_t)i];
        if (r.F < 1 || r.F > VS_BOOST_MAX_FIELDS) return fprintf(stderr, "record %d: F = %d\n", i, r.F), 2;
        float x = 0.f;
        const bool ok = apply(r, &x);
        res[2 * (size_t)i] = ok ? 1u : 0u;
        res[2 * (size_t)i + 1] = ok ? f2u(x) : 0u;
    }
    FILE* fo = fopen(out, "wb");
    if (!fo) return fprintf(stderr, "cannot open %s\n", out), 2;
    const bool wrote = n == 0 || fwrite(res.data(), 8, (size_t)n, fo) == (size_t)n;
    fclose(fo);
    if (!wrote) return fprintf(stderr, "short write\n"), 2;
    printf("boost_check: %d records\n", n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3) return run_file(argv[1], argv[2]);
    char msg[256] = {0};
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // ---- hand-made tuples ---------------------------------------------------------------------------------------------------------------------
    auto one = [&](double S, float w, uint32_t raw, int dt, int mode, float* out) {
        Record r{};
        r.S = S; r.w[0] = w; r.raw[0] = raw; r.dtype[0] = dt; r.F = 1; r.mode = mode;
        return apply(r, out);
    };
    float x = -1.f;
    expect_true("weight 0 over +inf: the sum as it is", one(1.5, 0.f, f2u(inf), VS_VAL_F32, VS_BOOST_ADD, &x) && x == 1.5f);
    expect_true("weight 0 over +inf, mul", one(1.5, 0.f, f2u(inf), VS_VAL_F32, VS_BOOST_MUL, &x) && x == 1.5f);
    expect_true("missing fp32 is neutral", one(2.0, 3.f, f2u(nan), VS_VAL_F32, VS_BOOST_ADD, &x) && x == 2.0f);
    expect_true("missing int32 is neutral, mul", one(2.0, 3.f, 0x80000000u, VS_VAL_I32, VS_BOOST_MUL, &x) && x == 2.0f);
    expect_true("add", one(1.0, 0.5f, f2u(3.0f), VS_VAL_F32, VS_BOOST_ADD, &x) && x == 2.5f);
    expect_true("mul", one(2.0, 0.5f, 3u, VS_VAL_I32, VS_BOOST_MUL, &x) && x == 5.0f);
    expect_true("int32 extremes", one(0.0, 1.f, 0x7FFFFFFFu, VS_VAL_I32, VS_BOOST_ADD, &x) && x == 2147483648.0f);
    expect_true("int32 minimum + 1", one(0.0, 1.f, 0x80000001u, VS_VAL_I32, VS_BOOST_ADD, &x) && x == -2147483648.0f);
    expect_true("inf - inf matches nothing", !one((double)inf, 1.f, f2u(-inf), VS_VAL_F32, VS_BOOST_ADD, &x));
    expect_true("0 * inf matches nothing", !one(0.0, 1.f, f2u(inf), VS_VAL_F32, VS_BOOST_MUL, &x));
    expect_true("a NaN weight matches nothing, value or not", !one(1.0, nan, f2u(1.0f), VS_VAL_F32, VS_BOOST_ADD, &x) &&
                                                                  !one(1.0, nan, f2u(nan), VS_VAL_F32, VS_BOOST_ADD, &x));
    expect_true("-0.0 comes out as +0.0", one(0.0, -1.f, f2u(0.0f), VS_VAL_F32, VS_BOOST_ADD, &x) && f2u(x) == 0u);
    expect_true("-0.0 product, mul", one(-1.0, -1.f, f2u(1.0f), VS_VAL_F32, VS_BOOST_MUL, &x) && f2u(x) == 0u);
    expect_true("an inf weight goes through", one(1.0, inf, f2u(2.0f), VS_VAL_F32, VS_BOOST_ADD, &x) && x == inf);
    {
        // field order is pinned: S one fp64 ulp above an fp32 tie, t = +half an ulp and -one ulp.  (S + h) - u rounds up to even and stays above
        // the tie; (S - u) + h lands on the tie and stays there: the fp32 results differ in the last bit
        Record r{};
        r.S = 1.0 + 0x1p-24 + 0x1p-52; r.F = 2; r.mode = VS_BOOST_ADD;
        r.w[0] = r.w[1] = 1.f;
        r.dtype[0] = r.dtype[1] = VS_VAL_F32;
        r.raw[0] = f2u(0x1p-53f); r.raw[1] = f2u(-0x1p-52f);
        float a = 0.f, b = 0.f;
        expect_true("(S + h) - u", apply(r, &a) && a == 1.0f + 0x1p-23f);
        r.raw[0] = f2u(-0x1p-52f); r.raw[1] = f2u(0x1p-53f);
        expect_true("(S - u) + h", apply(r, &b) && b == 1.0f);
    }
    // ---- the argument checks --------------------------------------------------------------------------------------------------------------------
    const uint32_t col[4] = {0u, 0u, 0u, 0u};
    const float w8[8] = {0.f, 1.f, -1.f, 0.5f, 1e30f, -1e30f, 0x1p-149f, 2.f};
    const void* f4[4] = {col, col, col, col};
    const void* fnull[4] = {col, nullptr, col, col};
    const int32_t d4[4] = {VS_VAL_F32, VS_VAL_I32, VS_VAL_F32, VS_VAL_I32};
    const int32_t dbad[4] = {VS_VAL_F32, 2, VS_VAL_F32, VS_VAL_I32};
    expect("fields ok", boost_check_fields(f4, d4, 4, VS_BOOST_MUL, w8, msg, sizeof msg), VS_OK, msg, "");
    expect("F 0", boost_check_fields(f4, d4, 0, VS_BOOST_ADD, w8, msg, sizeof msg), VS_EINVAL, msg, "n_fields");
    expect("F 5", boost_check_fields(f4, d4, 5, VS_BOOST_ADD, w8, msg, sizeof msg), VS_EINVAL, msg, "n_fields");
    expect("mode", boost_check_fields(f4, d4, 1, 2, w8, msg, sizeof msg), VS_EINVAL, msg, "mode");
    expect("mode < 0", boost_check_fields(f4, d4, 1, -1, w8, msg, sizeof msg), VS_EINVAL, msg, "mode");
    expect("NULL table", boost_check_fields(nullptr, d4, 1, VS_BOOST_ADD, w8, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("NULL dtypes", boost_check_fields(f4, nullptr, 1, VS_BOOST_ADD, w8, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("NULL weights", boost_check_fields(f4, d4, 1, VS_BOOST_ADD, nullptr, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("NULL field", boost_check_fields(fnull, d4, 2, VS_BOOST_ADD, w8, msg, sizeof msg), VS_EINVAL, msg, "fields[1] is NULL");
    expect("NULL field past F", boost_check_fields(fnull, d4, 1, VS_BOOST_ADD, w8, msg, sizeof msg), VS_OK, msg, "");
    expect("dtype", boost_check_fields(f4, dbad, 2, VS_BOOST_ADD, w8, msg, sizeof msg), VS_EINVAL, msg, "field_dtypes[1]");
    {
        std::vector<float> w(w8, w8 + 8);                                                       // exact size on the heap
        expect("weights ok", boost_check_weights_host(w.data(), 2, 4, msg, sizeof msg), VS_OK, msg, "");
        w[5] = nan;
        expect("weights NaN", boost_check_weights_host(w.data(), 2, 4, msg, sizeof msg), VS_EINVAL, msg, "weights[1, 1]");
        w[5] = -inf;
        expect("weights inf", boost_check_weights_host(w.data(), 4, 2, msg, sizeof msg), VS_EINVAL, msg, "weights[2, 1]");
    }
    if (failures) {
        fprintf(stderr, "boost_check: %d failures\n", failures);
        return 1;
    }
    printf("boost_check: ok\n");
    return 0;
}
