// fuse_check_main.cpp -- stand-alone driver of fuse_check.h, the host-side argument checks of vs_fuse_topk.  Not part of the library:
// tests/test_fuse_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.  The arrays live on the heap at
// their exact sizes -- ids [(L - 1) * list_stride + (B - 1) * ld + kk], weights [L] or [(B - 1) * ldw + L], fill [(B - 1) * ldf + L] --, so a
// check that reads past one of them is reported by the sanitizer.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "fuse_check.h"

using namespace vs;

static int failures = 0;

static void expect(const char* what, int got, int want, const char* msg, const char* needle) {
    const bool ok = got == want && (want == VS_OK || strstr(msg, needle) != nullptr);
    if (!ok) {
        fprintf(stderr, "FAIL %s: code %d (want %d), message \"%s\" (want \"%s\")\n", what, got, want, msg, needle);
        ++failures;
    }
}

int main() {
    char msg[512] = {0};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    auto sizes = [&](int32_t L, int32_t B, int32_t kk, int64_t ld, int64_t stride, bool w, int64_t ldw, bool f, int64_t ldf, int mode, float c, int32_t k) {
        return fuse_check_sizes(L, B, kk, ld, stride, w, ldw, f, ldf, mode, c, k, msg, sizeof msg);
    };
    // sizes: the limits themselves pass, one step beyond each fails
    expect("sizes ok, 4 x 1024", sizes(4, 3, 1024, 1024, 3 * 1024, false, 0, false, 0, VS_FUSE_RRF, 60.f, 1024), VS_OK, msg, "");
    expect("sizes ok, 8 x 512", sizes(8, 2, 512, 600, 2 * 600, true, 9, true, 8, VS_FUSE_RAW, 0.f, 1), VS_OK, msg, "");
    expect("sizes ok, one list", sizes(1, 2, 1, 1, 0, true, 0, false, 0, VS_FUSE_MNZ, 60.f, 5), VS_OK, msg, "");
    expect("B = 0", sizes(2, 0, 4, 4, 4, false, 0, false, 0, VS_FUSE_RRF, 60.f, 2), VS_EINVAL, msg, "B must");
    expect("L = 0", sizes(0, 1, 4, 4, 4, false, 0, false, 0, VS_FUSE_RRF, 60.f, 2), VS_EINVAL, msg, "L must");
    expect("L = 9", sizes(9, 1, 4, 4, 4, false, 0, false, 0, VS_FUSE_RRF, 60.f, 2), VS_EINVAL, msg, "L must");
    expect("kk = 0", sizes(2, 1, 0, 4, 4, false, 0, false, 0, VS_FUSE_RRF, 60.f, 2), VS_EINVAL, msg, "kk must");
    expect("kk = 1025", sizes(2, 1, 1025, 1025, 1025, false, 0, false, 0, VS_FUSE_RRF, 60.f, 2), VS_EINVAL, msg, "kk must");
    expect("L * kk = 4102", sizes(7, 1, 586, 586, 586, false, 0, false, 0, VS_FUSE_RRF, 60.f, 2), VS_EINVAL, msg, "at most 4096");
    expect("L * kk = 5120", sizes(5, 1, 1024, 1024, 1024, false, 0, false, 0, VS_FUSE_RRF, 60.f, 2), VS_EINVAL, msg, "at most 4096");
    expect("k = 0", sizes(2, 1, 4, 4, 4, false, 0, false, 0, VS_FUSE_RRF, 60.f, 0), VS_EINVAL, msg, "k must");
    expect("k = 1025", sizes(2, 1, 4, 4, 4, false, 0, false, 0, VS_FUSE_RRF, 60.f, 1025), VS_EINVAL, msg, "k must");
    expect("ld < kk", sizes(2, 1, 4, 3, 4, false, 0, false, 0, VS_FUSE_RRF, 60.f, 2), VS_EINVAL, msg, "shorter than kk");
    expect("list_stride short", sizes(2, 3, 4, 6, 15, false, 0, false, 0, VS_FUSE_RRF, 60.f, 2), VS_EINVAL, msg, "list_stride");
    expect("list_stride exact", sizes(2, 3, 4, 6, 16, false, 0, false, 0, VS_FUSE_RRF, 60.f, 2), VS_OK, msg, "");
    expect("mode = 4", sizes(2, 1, 4, 4, 4, false, 0, false, 0, 4, 60.f, 2), VS_EINVAL, msg, "mode must");
    expect("mode = -1", sizes(2, 1, 4, 4, 4, false, 0, false, 0, -1, 60.f, 2), VS_EINVAL, msg, "mode must");
    expect("rrf_c < 0", sizes(2, 1, 4, 4, 4, false, 0, false, 0, VS_FUSE_RRF, -1.f, 2), VS_EINVAL, msg, "rrf_c");
    expect("rrf_c inf", sizes(2, 1, 4, 4, 4, false, 0, false, 0, VS_FUSE_RRF, inf, 2), VS_EINVAL, msg, "rrf_c");
    expect("rrf_c NaN", sizes(2, 1, 4, 4, 4, false, 0, false, 0, VS_FUSE_RRF, nan, 2), VS_EINVAL, msg, "rrf_c");
    expect("ldw short", sizes(3, 2, 4, 4, 8, true, 2, false, 0, VS_FUSE_RRF, 60.f, 2), VS_EINVAL, msg, "ldw");
    expect("ldw ignored without weights", sizes(3, 2, 4, 4, 8, false, 2, false, 0, VS_FUSE_RRF, 60.f, 2), VS_OK, msg, "");
    expect("ldf short", sizes(3, 2, 4, 4, 8, false, 0, true, 2, VS_FUSE_RAW, 60.f, 2), VS_EINVAL, msg, "ldf");

    // host arrays: L = 2, B = 2, kk = 3, ld = 4, list_stride = 9 -> ids [9 + 4 + 3]
    const int32_t L = 2, B = 2, kk = 3;
    const int64_t ld = 4, stride = 9, top = 0xFFFFFFFEll;
    const size_t n_ids = (size_t)((L - 1) * stride + (B - 1) * ld + kk);
    auto host = [&](const std::vector<int64_t>& ids, const float* w, int64_t ldw, const float* f, int64_t ldf) {
        return fuse_check_host(ids.data(), L, B, kk, ld, stride, w, ldw, f, ldf, msg, sizeof msg);
    };
    std::vector<int64_t> ids(n_ids, 5);
    ids[0] = 0;
    ids[n_ids - 1] = top;                                                       // the last entry of the last list: the scan reaches it and stops
    expect("host ok", host(ids, nullptr, 0, nullptr, 0), VS_OK, msg, "");
    for (const int64_t bad : {top + 1, (int64_t)-2, (int64_t)1 << 40}) {
        std::vector<int64_t> x = ids;
        x[n_ids - 1] = bad;
        expect("id outside, last entry", host(x, nullptr, 0, nullptr, 0), VS_EINVAL, msg, "outside [-1");
        x = ids;
        x[stride + 1] = bad;
        expect("id outside, list 1", host(x, nullptr, 0, nullptr, 0), VS_EINVAL, msg, "list 1, query 0, position 1");
    }
    {
        std::vector<int64_t> x = ids;                                           // behind a list's first -1 nothing is read, whatever stands there
        x[ld + 0] = -1;
        x[ld + 1] = top + 1;
        x[ld + 2] = -7;
        expect("behind the padding", host(x, nullptr, 0, nullptr, 0), VS_OK, msg, "");
        std::fill(x.begin(), x.end(), (int64_t)-1);
        expect("all padding", host(x, nullptr, 0, nullptr, 0), VS_OK, msg, "");
    }
    {
        const std::vector<float> w = {1.f, 0.f};                                // [L] for the batch
        expect("batch weights", host(ids, w.data(), 0, nullptr, 0), VS_OK, msg, "");
        for (const float bad : {inf, -inf, nan}) {
            const std::vector<float> x = {0.5f, bad};
            expect("batch weight not finite", host(ids, x.data(), 0, nullptr, 0), VS_EINVAL, msg, "query 0, list 1");
        }
        std::vector<float> wq = {1.f, 2.f, nan, 3.f, 4.f};                      // [B, ldw = 3]: exactly (B - 1) * 3 + L values, the gap is not read
        expect("query weights", host(ids, wq.data(), 3, nullptr, 0), VS_OK, msg, "");
        wq[4] = inf;
        expect("query weight not finite", host(ids, wq.data(), 3, nullptr, 0), VS_EINVAL, msg, "query 1, list 1");
        std::vector<float> f = {0.f, -1.f, inf, 2.f, 0.25f};                    // [B, ldf = 3]
        expect("fill", host(ids, nullptr, 0, f.data(), 3), VS_OK, msg, "");
        f[3] = nan;
        expect("fill not finite", host(ids, nullptr, 0, f.data(), 3), VS_EINVAL, msg, "fill");
    }
    if (failures) return 1;
    puts("fuse_check: ok");
    return 0;
}
