// topn_stream.h -- the streaming top-n of a workgroup: 64-bit keys (larger = better, 0 = no candidate, all distinct) are
// ballot-pushed into an LDS buffer of kTopCap keys; whenever more than kTopKeep are in, the buffer is sorted, cut to its K best, and the K-th key
// becomes the threshold that later keys must beat.  What vs_facet_topn, vs_term_topn, vs_term_sum_topn and vs_value_topk share.
#pragma once
#include "topk_keys.h"

namespace vs {

constexpr int kTopCap = 4096;                         // keys of the candidate buffer
constexpr int kTopKeep = 2048;                        // sorted and cut when more are in

// push the lanes' keys that pass into the buffer (cnt_sh: its fill); the caller guarantees the room
__device__ __forceinline__ void top_push(uint64_t* cand, int* cnt_sh, bool pass, uint64_t key, int lane) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
    if (m == 0ull) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(cnt_sh, __popcll(m));
    base = __shfl(base, 0, 64);
    if (pass) cand[base + __popcll(m & ((1ull << lane) - 1ull))] = key;
}

// after a barrier: sort the buffer when it is more than half full (or at the end) and cut it to K -> the new threshold.  Only the power of two
// that holds the keys (and the K slots the caller reads) is sorted: a sparse set's last sort is a few hundred keys, not 4096.
template <int THREADS>
__device__ __forceinline__ uint64_t top_cut(uint64_t* cand, int* cnt_sh, int K, bool last, uint64_t tau, int tid) {
    const int cnt = *cnt_sh;                                     // (uniform: read after the caller's barrier)
    if (last || cnt > kTopKeep) {
        int n = 2;
        while (n < cnt || n < K) n <<= 1;                        // <= kTopCap: cnt <= kTopCap, K <= 1024
        for (int i = cnt + tid; i < n; i += THREADS) cand[i] = 0ull;
        wg_sort_desc<THREADS>(cand, n, tid);
        if (!last && cnt > K) {
            tau = cand[K - 1];
            __syncthreads();
            if (tid == 0) *cnt_sh = K;
        }
    }
    __syncthreads();
    return tau;
}

// One workgroup of THREADS threads streams the keys key_of(i), i in [0, n_items), n_items >= 1, through cand [kTopCap] and leaves the K best sorted at the
// front of cand, zeros behind them.  key_of is called by thread i % THREADS.
template <int THREADS, class KeyOf>
__device__ __forceinline__ void stream_topn(int64_t n_items, int K, KeyOf key_of, uint64_t* cand, int* cnt_sh) {
    constexpr int SB = (kTopCap - kTopKeep) / THREADS;           // steps between cuts
    static_assert(SB >= 1, "a step adds up to THREADS candidates");
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) *cnt_sh = 0;
    __syncthreads();
    uint64_t tau = 0ull;
    const int64_t iters = (n_items + THREADS - 1) / THREADS;
    for (int64_t it0 = 0; it0 < iters; it0 += SB) {
        const int64_t it1 = min(iters, it0 + SB);
        for (int64_t it = it0; it < it1; ++it) {
            const int64_t i = it * THREADS + tid;
            const uint64_t key = i < n_items ? key_of(i) : 0ull;
            top_push(cand, cnt_sh, key > tau, key, lane);
        }
        __syncthreads();
        tau = top_cut<THREADS>(cand, cnt_sh, K, it1 >= iters, tau, tid);
    }
}

}  // namespace vs
