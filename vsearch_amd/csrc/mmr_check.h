// mmr_check.h -- the argument checks of vs_mmr_select_csr that need no device: sizes, and the host CSR arrays before they are staged.  Plain
// C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_mmr_cpu.py builds one).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "vsearch_hip.h"

namespace vs {

constexpr int kMmrMaxKK = VS_MMR_MAX_DEPTH;   // candidates of a list
constexpr int kMmrMaxK = VS_MMR_MAX_DEPTH;    // picks asked for (picks beyond the candidates are padding)
constexpr int kMmrMaxCols = 32768;            // cells of the LDS image (128 KiB of the CU's 160 KiB; the vs_index_queries_from_rows limit)

// -> VS_OK, or the code of the first violated limit with its message in msg
inline int mmr_check_sizes(int32_t B, int32_t kk, int64_t ld, int32_t n_cols, int32_t k, int mode, char* msg, size_t cap) {
    if (B <= 0) return snprintf(msg, cap, "B must be positive (got %d)", B), VS_EINVAL;
    if (kk < 1 || kk > kMmrMaxKK) return snprintf(msg, cap, "the candidate depth kk must be in 1..%d (got %d)", kMmrMaxKK, kk), VS_EINVAL;
    if (k < 1 || k > kMmrMaxK) return snprintf(msg, cap, "k must be in 1..%d (got %d)", kMmrMaxK, k), VS_EINVAL;
    if (ld < kk) return snprintf(msg, cap, "ld = %lld is shorter than kk = %d", (long long)ld, kk), VS_EINVAL;
    if (mode != VS_MMR_COSINE && mode != VS_MMR_DOT) return snprintf(msg, cap, "mode must be VS_MMR_COSINE or VS_MMR_DOT (got %d)", mode), VS_EINVAL;
    if (n_cols < 1) return snprintf(msg, cap, "n_cols must be positive (got %d)", n_cols), VS_EINVAL;
    if (n_cols > kMmrMaxCols)
        return snprintf(msg, cap, "n_cols = %d is wider than the %d-cell LDS image of the selection kernel (column tiles are not built)", n_cols,
                        kMmrMaxCols), VS_EUNSUPPORTED;
    return VS_OK;
}

// host arrays: rowptr [B * kk + 1] starts at >= 0 and never falls, every column lies in [0, n_cols), every lam in [0, 1]
inline int mmr_check_host(const int64_t* rowptr, const int32_t* cols, const float* lam, int32_t B, int32_t kk, int32_t n_cols, char* msg, size_t cap) {
    const size_t rows = (size_t)B * (size_t)kk;
    if (rowptr[0] < 0) return snprintf(msg, cap, "rowptr[0] = %lld is negative", (long long)rowptr[0]), VS_EINVAL;
    for (size_t r = 0; r < rows; ++r)
        if (rowptr[r + 1] < rowptr[r])
            return snprintf(msg, cap, "rowptr is not monotone: rowptr[%zu] = %lld > rowptr[%zu] = %lld", r, (long long)rowptr[r], r + 1,
                            (long long)rowptr[r + 1]), VS_EINVAL;
    for (int64_t e = rowptr[0]; e < rowptr[rows]; ++e)
        if (cols[e] < 0 || cols[e] >= n_cols)
            return snprintf(msg, cap, "column %d (entry %lld) is outside [0, %d)", cols[e], (long long)e, n_cols), VS_EINVAL;
    for (int32_t b = 0; b < B; ++b)
        if (!(lam[b] >= 0.f && lam[b] <= 1.f)) return snprintf(msg, cap, "lam[%d] = %g is outside [0, 1]", b, (double)lam[b]), VS_EINVAL;
    return VS_OK;
}

}  // namespace vs
