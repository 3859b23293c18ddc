// fuse_check.h -- the argument checks of vs_fuse_topk that need no device: sizes and strides, and the host arrays before they are staged.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_fuse_cpu.py builds one).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "vsearch_hip.h"

namespace vs {

constexpr int kFuseMaxLists = VS_FUSE_MAX_LISTS;       // the list number takes 3 bits of a sort key
constexpr int kFuseMaxKK = VS_FUSE_MAX_DEPTH;          // the position takes 10
constexpr int kFuseMaxEntries = VS_FUSE_MAX_ENTRIES;   // L * kk: the keys of a query live in LDS twice over
constexpr int kFuseMaxK = VS_FUSE_MAX_DEPTH;
constexpr int64_t kFuseIdEnd = 0xFFFFFFFFll;           // ids lie in [-1, 2^32 - 1): the keys hold 32-bit ids

// -> VS_OK, or VS_EINVAL for the first violated limit with its message in msg
inline int fuse_check_sizes(int32_t L, int32_t B, int32_t kk, int64_t ld, int64_t list_stride, bool weights, int64_t ldw, bool fill, int64_t ldf,
                            int mode, float rrf_c, int32_t k, char* msg, size_t cap) {
    if (B <= 0) return snprintf(msg, cap, "B must be positive (got %d)", B), VS_EINVAL;
    if (L < 1 || L > kFuseMaxLists) return snprintf(msg, cap, "the number of lists L must be in 1..%d (got %d)", kFuseMaxLists, L), VS_EINVAL;
    if (kk < 1 || kk > kFuseMaxKK) return snprintf(msg, cap, "the list depth kk must be in 1..%d (got %d)", kFuseMaxKK, kk), VS_EINVAL;
    if ((int64_t)L * kk > kFuseMaxEntries)
        return snprintf(msg, cap, "L * kk = %lld entries a query, at most %d fit", (long long)L * kk, kFuseMaxEntries), VS_EINVAL;
    if (k < 1 || k > kFuseMaxK) return snprintf(msg, cap, "k must be in 1..%d (got %d)", kFuseMaxK, k), VS_EINVAL;
    if (ld < kk) return snprintf(msg, cap, "ld = %lld is shorter than kk = %d", (long long)ld, kk), VS_EINVAL;
    if (L > 1 && list_stride < (int64_t)(B - 1) * ld + kk)
        return snprintf(msg, cap, "list_stride = %lld is shorter than a list of %d queries ((B - 1) * ld + kk = %lld)", (long long)list_stride, B,
                        (long long)(B - 1) * ld + kk), VS_EINVAL;
    if (mode != VS_FUSE_RRF && mode != VS_FUSE_SUM && mode != VS_FUSE_MNZ && mode != VS_FUSE_RAW)
        return snprintf(msg, cap, "mode must be VS_FUSE_RRF, VS_FUSE_SUM, VS_FUSE_MNZ or VS_FUSE_RAW (got %d)", mode), VS_EINVAL;
    if (!(rrf_c >= 0.f) || std::isinf(rrf_c)) return snprintf(msg, cap, "rrf_c must be finite and >= 0 (got %g)", (double)rrf_c), VS_EINVAL;
    if (weights && ldw != 0 && ldw < L) return snprintf(msg, cap, "ldw = %lld is neither 0 nor at least L = %d", (long long)ldw, L), VS_EINVAL;
    if (fill && ldf < L) return snprintf(msg, cap, "ldf = %lld is shorter than L = %d", (long long)ldf, L), VS_EINVAL;
    return VS_OK;
}

// host arrays: every id in front of a list's first -1 lies in [0, 2^32 - 1) (what stands behind the -1 is not read), every weight and every
// fill value a call reads is finite.  weights / fill may be NULL.
inline int fuse_check_host(const int64_t* ids, int32_t L, int32_t B, int32_t kk, int64_t ld, int64_t list_stride, const float* weights,
                           int64_t ldw, const float* fill, int64_t ldf, char* msg, size_t cap) {
    for (int32_t l = 0; l < L; ++l)
        for (int32_t b = 0; b < B; ++b) {
            const int64_t* row = ids + (size_t)l * (size_t)list_stride + (size_t)b * (size_t)ld;
            for (int32_t j = 0; j < kk && row[j] != -1; ++j)
                if (row[j] < 0 || row[j] >= kFuseIdEnd)
                    return snprintf(msg, cap, "id %lld (list %d, query %d, position %d) is outside [-1, 2^32 - 1)", (long long)row[j], l, b, j), VS_EINVAL;
        }
    if (weights)
        for (int32_t b = 0; b < (ldw ? B : 1); ++b)
            for (int32_t l = 0; l < L; ++l)
                if (!std::isfinite(weights[(size_t)b * (size_t)ldw + l]))
                    return snprintf(msg, cap, "weight %g (query %d, list %d) is not finite", (double)weights[(size_t)b * (size_t)ldw + l], b, l), VS_EINVAL;
    if (fill)
        for (int32_t b = 0; b < B; ++b)
            for (int32_t l = 0; l < L; ++l)
                if (!std::isfinite(fill[(size_t)b * (size_t)ldf + l]))
                    return snprintf(msg, cap, "fill %g (query %d, list %d) is not finite", (double)fill[(size_t)b * (size_t)ldf + l], b, l), VS_EINVAL;
    return VS_OK;
}

}  // namespace vs
