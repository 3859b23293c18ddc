// value_set.h -- what the translation units of the numeric fields (values.hip, quantiles.hip) share: the set arguments of a call, the walk of a
// workgroup's waves over the packed bitmaps of a tile of queries (2048-row spans, all-zero spans left at once, a row's value loaded once for the
// tile), and the host side of staging a set.  Moved out of values.hip as it was.
#pragma once
#include "common.h"
#include "bitmap_span.h"
#include "staging.h"
#include "value_check.h"

namespace vs {

constexpr int kValThreads = 256;
constexpr int kValWaves = kValThreads / 64;

inline int plan_or_fail(int rc, const char* msg) { return rc == VS_OK ? VS_OK : fail(rc, "%s", msg); }

inline int device_in_range(int device) {
    VS_TRY(need_device());
    int ndev = 0;
    VS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VS_EINVAL, "device %d out of range", device);
    return VS_OK;
}

struct SetArgs {
    const uint32_t* words;            // [B, ld_words] or null (every row set)
    int64_t bit0, ld_words;
    const uint32_t* and_words;        // shared by the queries, or null
    int64_t and_bit0;
    const uint32_t* values;           // [n_rows] raw
    int dtype;
    int64_t n_rows;
    int32_t B;
    int64_t rows_per_chunk;
};

// One wave's walk over its spans of the chunk: body(row0, raw, key, sp, s, sh, live) is called for every 64-row step with a set row -- raw /
// key: this lane's row's value and its key where some query has the row (else 0); query q's rows of the step are window64(sp[q], s, sh) & live.
template <int QT, class Body>
__device__ __forceinline__ void walk_set(const SetArgs& a, int q0, int nq, int64_t r0, int64_t r1, int w, int lane, Body body) {
    const int64_t n_w = (a.bit0 + a.n_rows + 31) >> 5, n_aw = (a.and_bit0 + a.n_rows + 31) >> 5;
    for (int64_t rb = r0 + (int64_t)w * kValueSpanRows; rb < r1; rb += (int64_t)kValWaves * kValueSpanRows) {
        const int nsub = (int)((min(r1, rb + kValueSpanRows) - rb + 63) >> 6);
        Span an{~0u, ~0u};
        int sha = 0;
        if (a.and_words) {
            const int64_t p = a.and_bit0 + rb;
            an = load_span(a.and_words, p >> 5, n_aw, lane);
            sha = (int)(p & 31);
            if (__builtin_amdgcn_ballot_w64((an.lo | an.hi) != 0u) == 0ull) continue;
        }
        Span sp[QT];
        Span u{~0u, ~0u};
        int sh = 0;
        if (a.words) {
            const int64_t p = a.bit0 + rb;
            sh = (int)(p & 31);
            u.lo = u.hi = 0u;
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                sp[q] = Span{0u, 0u};
                if (q < nq) sp[q] = load_span(a.words + (size_t)(q0 + q) * (size_t)a.ld_words, p >> 5, n_w, lane);
                u.lo |= sp[q].lo;
                u.hi |= sp[q].hi;
            }
            if (__builtin_amdgcn_ballot_w64((u.lo | u.hi) != 0u) == 0ull) continue;      // no value of the span is touched
        } else {
#pragma unroll
            for (int q = 0; q < QT; ++q) sp[q] = u;
        }
        for (int s = 0; s < nsub; ++s) {
            const int64_t row0 = rb + (int64_t)s * 64;
            const int64_t nvalid = r1 - row0;                                        // >= 1
            const uint64_t vm = nvalid >= 64 ? ~0ull : ((1ull << nvalid) - 1ull);    // bits at or past the last row are ignored
            const uint64_t live = window64(an, s, sha) & vm;
            const uint64_t many = window64(u, s, sh) & live;
            if (many == 0ull) continue;                                              // (uniform)
            uint32_t raw = 0u, key = 0u;
            if ((many >> lane) & 1ull) {                                             // once for the tile
                raw = a.values[row0 + lane];
                key = value_key(raw, a.dtype);
            }
            body(row0, raw, key, sp, s, sh, live);
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------
// the staged inputs of a set: bitmap words, a caller's and-bitmap, the values
struct SetStage {
    Staged w, a, v;
    int in(const uint32_t* words, int64_t bit0, int64_t ld_words, const uint32_t* and_user, const uint32_t* and_dev, int32_t B, const void* values,
           int dtype, int64_t n_rows, const ValuePlan& plan, bool dev, hipStream_t s, SetArgs* out) {
        const int64_t span = (bit0 + n_rows + 31) >> 5;
        uint32_t *d_w, *d_a, *d_v;
        VS_TRY(w.in(words, (size_t)((B - 1) * ld_words + span), dev, true, s, &d_w));
        VS_TRY(a.in(and_user, (size_t)span, dev, true, s, &d_a));
        VS_TRY(v.in(static_cast<const uint32_t*>(values), (size_t)n_rows, dev, true, s, &d_v));
        out->words = d_w;
        out->bit0 = bit0;
        out->ld_words = words ? ld_words : 0;
        out->and_words = and_user ? d_a : and_dev;
        out->and_bit0 = and_user ? bit0 : 0;
        out->values = d_v;
        out->dtype = dtype;
        out->n_rows = n_rows;
        out->B = B;
        out->rows_per_chunk = plan.rows_per_chunk;
        return VS_OK;
    }
};

inline int finish_call(bool dev, void* stream, hipStream_t s) {
    if (!stream || !dev) VS_HIP(hipStreamSynchronize(s));
    if (Profiler::get().on) Profiler::get().drain();
    return VS_OK;
}

inline const uint32_t* live_words(vs_index* idx) { return idx->has_tomb ? idx->live.as<uint32_t>() : nullptr; }

}  // namespace vs
