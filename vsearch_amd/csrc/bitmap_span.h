// bitmap_span.h -- how a wave reads a packed row bitmap (the layout of vs_index_search_filtered) in spans of 2048 rows, whatever bit the rows
// start at: the two primitives under the walks of set_walk.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vs {

// lane l holds words w0 + l and w0 + l + 1 of a bitmap (0 past its last word)
struct Span {
    uint32_t lo, hi;
};
__device__ __forceinline__ Span load_span(const uint32_t* w, int64_t w0, int64_t n_words, int lane) {
    const int64_t i = w0 + lane;
    Span s;
    s.lo = i < n_words ? w[i] : 0u;
    s.hi = i + 1 < n_words ? w[i + 1] : 0u;
    return s;
}
// bits [64 s + sh, 64 s + sh + 64) of the span (s uniform, sh in 0..31): words 2 s, 2 s + 1 and 2 s + 2
__device__ __forceinline__ uint64_t window64(const Span& sp, int s, int sh) {
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)sp.lo, 2 * s);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)sp.hi, 2 * s);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)sp.hi, 2 * s + 1);
    uint64_t v = (((uint64_t)b << 32) | a) >> sh;
    if (sh) v |= (uint64_t)c << (64 - sh);
    return v;
}

}  // namespace vs
