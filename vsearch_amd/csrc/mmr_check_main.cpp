// mmr_check_main.cpp -- stand-alone driver of mmr_check.h, the host-side argument checks of vs_mmr_select_csr.  Not part of the library:
// tests/test_mmr_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.  The arrays live on the heap at
// their exact sizes, so a check that reads past rowptr [B * kk + 1], cols [rowptr[B * kk]] or lam [B] is reported by the sanitizer.
#include <cstdio>
#include <cstring>
#include <vector>

#include "mmr_check.h"

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
    const int32_t V = 29523;
    // sizes
    expect("sizes ok", mmr_check_sizes(3, 1024, 1024, 32768, 1024, VS_MMR_DOT, msg, sizeof msg), VS_OK, msg, "");
    expect("B = 0", mmr_check_sizes(0, 4, 4, V, 2, VS_MMR_COSINE, msg, sizeof msg), VS_EINVAL, msg, "B must");
    expect("kk = 0", mmr_check_sizes(1, 0, 4, V, 2, VS_MMR_COSINE, msg, sizeof msg), VS_EINVAL, msg, "kk must");
    expect("kk = 1025", mmr_check_sizes(1, 1025, 1025, V, 2, VS_MMR_COSINE, msg, sizeof msg), VS_EINVAL, msg, "kk must");
    expect("k = 0", mmr_check_sizes(1, 4, 4, V, 0, VS_MMR_COSINE, msg, sizeof msg), VS_EINVAL, msg, "k must");
    expect("k = 1025", mmr_check_sizes(1, 4, 4, V, 1025, VS_MMR_COSINE, msg, sizeof msg), VS_EINVAL, msg, "k must");
    expect("ld < kk", mmr_check_sizes(1, 4, 3, V, 2, VS_MMR_COSINE, msg, sizeof msg), VS_EINVAL, msg, "shorter");
    expect("mode", mmr_check_sizes(1, 4, 4, V, 2, 7, msg, sizeof msg), VS_EINVAL, msg, "mode");
    expect("n_cols = 0", mmr_check_sizes(1, 4, 4, 0, 2, VS_MMR_COSINE, msg, sizeof msg), VS_EINVAL, msg, "n_cols");
    expect("n_cols = 32769", mmr_check_sizes(1, 4, 4, 32769, 2, VS_MMR_COSINE, msg, sizeof msg), VS_EUNSUPPORTED, msg, "wider");
    // host arrays: B = 2, kk = 3, rows of 2, 0, 3 | 1, 0, 2 cells
    const int32_t B = 2, kk = 3;
    const std::vector<int64_t> rowptr = {0, 2, 2, 5, 6, 6, 8};
    const std::vector<int32_t> cols = {0, 7, 1, 2, V - 1, 5, 0, V - 1};
    const std::vector<float> lam = {0.f, 1.f};
    expect("host ok", mmr_check_host(rowptr.data(), cols.data(), lam.data(), B, kk, V, msg, sizeof msg), VS_OK, msg, "");
    {
        std::vector<int64_t> rp = rowptr;
        rp[4] = 4;                                                              // falls below rowptr[3] = 5
        expect("non-monotone rowptr", mmr_check_host(rp.data(), cols.data(), lam.data(), B, kk, V, msg, sizeof msg), VS_EINVAL, msg, "monotone");
        rp = rowptr;
        rp[0] = -1;
        expect("negative rowptr[0]", mmr_check_host(rp.data(), cols.data(), lam.data(), B, kk, V, msg, sizeof msg), VS_EINVAL, msg, "negative");
    }
    for (const int32_t bad : {V, -1, 1 << 30}) {
        std::vector<int32_t> c = cols;
        c.back() = bad;                                                         // the last cell: the scan must reach it and stop there
        expect("column outside", mmr_check_host(rowptr.data(), c.data(), lam.data(), B, kk, V, msg, sizeof msg), VS_EINVAL, msg, "outside [0");
    }
    for (const float bad : {-0.25f, 1.5f, NAN}) {
        const std::vector<float> l = {0.5f, bad};
        expect("lam outside", mmr_check_host(rowptr.data(), cols.data(), l.data(), B, kk, V, msg, sizeof msg), VS_EINVAL, msg, "lam[1]");
    }
    {
        const std::vector<int64_t> rp(B * kk + 1, 0);                           // no cells at all: cols is never read
        expect("empty rows", mmr_check_host(rp.data(), nullptr, lam.data(), B, kk, V, msg, sizeof msg), VS_OK, msg, "");
    }
    if (failures) return 1;
    puts("mmr_check: ok");
    return 0;
}
