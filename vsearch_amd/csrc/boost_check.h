// boost_check.h -- the pinned arithmetic of boosted search (vs_index_search_boosted) and the argument checks of the call that need no device.
// boost_apply is what every range kernel runs with BO = 1 (range.hip, csr_scan_mq.h), __host__ __device__, so that the stand-alone check
// exercises the very code and numpy reproduces every bit:
//     t_j = +0.0                                  if w[j] == 0 or the row has no value in field j (NaN / INT32_MIN)
//         = fp64(w[j]) * fp64(value_j)            otherwise -- two 32-bit quantities: the product is EXACT in fp64
//     VS_BOOST_ADD:  x = (((S + t_0) + t_1) + ...)                       fp64 additions in field order
//     VS_BOOST_MUL:  u = (((1.0 + t_0) + t_1) + ...),  x = S * u
//     boosted = canon_zero(fl32(x));  x != x: the row matches nothing (an infinity met its opposite, or 0 * inf).  A NaN weight: no match.
// Every fp64 operation rounds once and the products are exact, so an fma contraction of `S + w * v` could not change a bit; contraction is
// switched off all the same, so that host and device run the same operations.
// Plain C++ with no HIP in it, so that a stand-alone program can run it under a host sanitizer (tests/test_boost_cpu.py builds one).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "vsearch_hip.h"

namespace vs {

#if defined(__HIPCC__)
#define VS_BOOST_HD __host__ __device__
#else
#define VS_BOOST_HD
#endif

// what a boosted scan carries behind its range arguments (device pointers; w belongs to the first query of the launch)
struct BoostArgs {
    const uint32_t* field[VS_BOOST_MAX_FIELDS];      // [n_rows] raw 32-bit values
    int32_t dtype[VS_BOOST_MAX_FIELDS];               // VS_VAL_F32 | VS_VAL_I32
    const float* w;                                   // [B, F]
    int32_t F;
    int32_t mode;                                     // VS_BOOST_ADD | VS_BOOST_MUL
};

VS_BOOST_HD inline bool boost_missing(uint32_t raw, int dtype) {
    return dtype == VS_VAL_F32 ? (raw & 0x7FFFFFFFu) > 0x7F800000u : raw == 0x80000000u;
}
VS_BOOST_HD inline double boost_value(uint32_t raw, int dtype) {
    if (dtype == VS_VAL_F32) {
        float f;
        memcpy(&f, &raw, 4);
        return (double)f;
    }
    return (double)(int32_t)raw;
}

// S: the fp64 row sum before its rounding; w [F]: the query's weights; raw [F] / dtype [F]: the row's values.  -> false: the row matches
// nothing for this query; true: *out is the boosted score (never NaN, never -0.0).
VS_BOOST_HD inline bool boost_apply(double S, const float* w, const uint32_t* raw, const int32_t* dtype, int F, int mode, float* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double u = mode == VS_BOOST_MUL ? 1.0 : S;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < VS_BOOST_MAX_FIELDS; ++j) {
        if (j >= F) break;
        const float wj = w[j];
        double t = 0.0;
        if (wj != 0.0f) {                                           // (a NaN weight comes here)
            if (wj != wj) return false;
            if (!boost_missing(raw[j], dtype[j])) t = (double)wj * boost_value(raw[j], dtype[j]);
        }
        u = u + t;
    }
    const double x = mode == VS_BOOST_MUL ? S * u : u;
    if (x != x) return false;
    const float f = (float)x;
    *out = f == 0.0f ? 0.0f : f;                                    // canon_zero
    return true;
}

// ---- the argument checks: pure host ---------------------------------------------------------------------------------------------------------
inline int boost_check_shape(int32_t F, int mode, char* msg, size_t cap) {
    if (F < 1 || F > VS_BOOST_MAX_FIELDS) return snprintf(msg, cap, "n_fields must be in 1..%d (got %d)", VS_BOOST_MAX_FIELDS, F), VS_EINVAL;
    if (mode != VS_BOOST_ADD && mode != VS_BOOST_MUL)
        return snprintf(msg, cap, "mode must be VS_BOOST_ADD (0) or VS_BOOST_MUL (1), got %d", mode), VS_EINVAL;
    return VS_OK;
}
// the host tables of a call: F field pointers and F dtypes
inline int boost_check_fields(const void* const* fields, const int32_t* dtypes, int32_t F, int mode, const void* weights, char* msg, size_t cap) {
    const int rc = boost_check_shape(F, mode, msg, cap);
    if (rc != VS_OK) return rc;
    if (!fields || !dtypes || !weights) return snprintf(msg, cap, "NULL argument (fields / field_dtypes / weights)"), VS_EINVAL;
    for (int32_t j = 0; j < F; ++j) {
        if (!fields[j]) return snprintf(msg, cap, "fields[%d] is NULL", j), VS_EINVAL;
        if (dtypes[j] != VS_VAL_F32 && dtypes[j] != VS_VAL_I32)
            return snprintf(msg, cap, "field_dtypes[%d] must be VS_VAL_F32 (0) or VS_VAL_I32 (1), got %d", j, dtypes[j]), VS_EINVAL;
    }
    return VS_OK;
}
// host weights [B, F]: finite
inline int boost_check_weights_host(const float* w, int32_t B, int32_t F, char* msg, size_t cap) {
    for (int64_t i = 0; i < (int64_t)B * F; ++i) {
        uint32_t u;
        memcpy(&u, &w[i], 4);
        if ((u & 0x7F800000u) == 0x7F800000u)
            return snprintf(msg, cap, "weights[%lld, %lld] is not finite", (long long)(i / F), (long long)(i % F)), VS_EINVAL;
    }
    return VS_OK;
}

}  // namespace vs
