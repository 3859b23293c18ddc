// set_list_check.h -- the hash, the window arithmetic, the plan rule and the argument checks of the set egress (vs_set_list_plan, vs_set_count,
// vs_set_ids, vs_set_sample, vs_set_from_ids) that need no device.  The hash and the window functions are what the kernels of set_list.hip run,
// __host__ __device__, so that the stand-alone check exercises the very code.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_set_list_cpu.py builds one).
#pragma once

#include "set_check.h"

namespace vs {

#if defined(__HIPCC__)
#define VS_SET_HD __host__ __device__
#else
#define VS_SET_HD
#endif

constexpr int kSetThreads = 256;                      // threads of the workgroups of set_list.hip
constexpr int kSetWaves = kSetThreads / 64;
constexpr int64_t kSetMaxOutIds = 1ll << 27;          // ids of one vs_set_ids call (1 GiB)
constexpr int64_t kSetMaxScratchKeys = 1ll << 27;     // keys of vs_set_sample's per-chunk lists (1 GiB): the rule of vs_value_topk
constexpr int64_t kSetMaxSpanCounts = 1ll << 27;      // (query, span) counts of one call

// ---- the sample hash: pinned, all arithmetic modulo 2^64 ------------------------------------------------------------------------------------
constexpr uint64_t kSetGolden = 0x9E3779B97F4A7C15ull;
// the splitmix64 finaliser
VS_SET_HD inline uint64_t set_mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// a query's key: the seed through the mix first, so that consecutive seeds share no structure
VS_SET_HD inline uint64_t set_sample_seed_key(uint64_t seed) { return set_mix64(seed + kSetGolden); }
// the hash of a global id under a query's key (id >= -1 + 1: id + 1 wraps like everything else)
VS_SET_HD inline uint32_t set_sample_hash_keyed(uint64_t k, uint64_t id) { return (uint32_t)(set_mix64(k ^ (kSetGolden * (id + 1ull))) >> 32); }
VS_SET_HD inline uint32_t set_sample_hash(uint64_t seed, uint64_t id) { return set_sample_hash_keyed(set_sample_seed_key(seed), id); }
// The key a row goes through the top-n stream with (larger = better): smallest hash first, then smallest row; never 0 since row <= 2^32 - 2.
VS_SET_HD inline uint64_t set_sample_key(uint32_t h, uint32_t row) { return ((uint64_t)(uint32_t)~h << 32) | (uint32_t)~row; }
VS_SET_HD inline uint32_t set_sample_key_hash(uint64_t key) { return ~(uint32_t)(key >> 32); }
VS_SET_HD inline uint32_t set_sample_key_row(uint64_t key) { return ~(uint32_t)key; }

// ---- the window of vs_set_ids: ranks [off, off + limit) of a list ----------------------------------------------------------------------------
// a negative offset on the device reads as 0 (a host one is VS_EINVAL)
VS_SET_HD inline int64_t set_window_offset(int64_t off) { return off < 0 ? 0 : off; }
// does rank (>= 0) fall into the window?  Written without off + limit, which may pass 2^63.
VS_SET_HD inline bool set_rank_in_window(int64_t rank, int64_t off, int64_t limit) { return rank >= off && rank - off < limit; }
// a span holding ranks [base, base + cnt) has nothing for the window: it is left without reading the bitmap
VS_SET_HD inline bool set_span_misses(int64_t base, int64_t cnt, int64_t off, int64_t limit) {
    return cnt == 0 || limit == 0 || base + cnt <= off || (base >= off && base - off >= limit);
}
// slot j of the window lies behind the last member of a list of `count` ranks: it holds -1
VS_SET_HD inline bool set_slot_is_tail(int64_t j, int64_t off, int64_t count) { return off >= count || j >= count - off; }

// ---- the plan rule: pure host arithmetic ----------------------------------------------------------------------------------------------------
struct SetListPlan {
    int64_t chunks = 1, rows_per_chunk = kSpanRows, spans = 1;
};

// A work item is (query, chunk of rows).  rows_per_chunk = 0: auto_chunk over the batch, kMinChunk rows at least (a span a wave); any other
// value is a positive multiple of 64, rounded up to whole spans (a wave counts and lists span by span).
inline int set_list_plan(int64_t n_rows, int32_t B, bool per_query, int64_t rows_per_chunk, SetListPlan* out, char* msg, size_t cap) {
    int rc = check_n_rows(n_rows, msg, cap);
    if (rc == VS_OK) rc = check_batch(B, msg, cap);
    if (rc == VS_OK) rc = check_chunking(per_query, B, rows_per_chunk, "bitmap", msg, cap);
    if (rc != VS_OK) return rc;
    SetListPlan p;
    p.rows_per_chunk = rows_per_chunk == 0 ? auto_chunk(n_rows, B, kMinChunk) : (rows_per_chunk + kSpanRows - 1) / kSpanRows * kSpanRows;
    p.chunks = (n_rows + p.rows_per_chunk - 1) / p.rows_per_chunk;
    p.spans = (n_rows + kSpanRows - 1) / kSpanRows;
    if (B > 65535 || p.spans > kSetMaxSpanCounts / B)
        return snprintf(msg, cap, "%lld spans x %d queries are too many for one call", (long long)p.spans, B), VS_EINVAL;
    *out = p;
    return VS_OK;
}

// the set of a count / ids / sample call: the bitmap's geometry, and the plan
inline int set_list_check_set(bool have_pointers, bool have_words, int64_t bit0, int64_t ld_words, int32_t B, int64_t n_rows, int64_t rows_per_chunk,
                              SetListPlan* plan, char* msg, size_t cap) {
    if (!have_pointers) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    int rc = check_bit0(bit0, msg, cap);
    if (rc == VS_OK) rc = set_list_plan(n_rows, B, have_words && ld_words != 0, rows_per_chunk, plan, msg, cap);
    if (rc == VS_OK) rc = check_ld_words(have_words, bit0, ld_words, n_rows, msg, cap);
    return rc;
}

// vs_set_ids: the window's length and the size of the output
inline int set_list_check_ids(int64_t limit, int32_t B, bool have_out_ids, char* msg, size_t cap) {
    if (limit < 0) return snprintf(msg, cap, "limit must be >= 0 (got %lld)", (long long)limit), VS_EINVAL;
    if (limit > kSetMaxOutIds / B) return snprintf(msg, cap, "B x limit = %d x %lld is more than 2^27 ids: page through the list", B, (long long)limit), VS_EINVAL;
    if (limit > 0 && !have_out_ids) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    return VS_OK;
}
// a host offsets array: none negative
inline int set_list_check_offsets_host(const int64_t* offsets, int32_t B, char* msg, size_t cap) {
    for (int32_t b = 0; b < B; ++b)
        if (offsets[b] < 0) return snprintf(msg, cap, "offsets[%d] = %lld is negative", b, (long long)offsets[b]), VS_EINVAL;
    return VS_OK;
}

// vs_set_sample: n and the scratch the per-chunk lists take
inline int set_list_check_sample(int32_t n, int32_t B, const SetListPlan& plan, char* msg, size_t cap) {
    if (n < 1 || n > VS_SET_MAX_SAMPLE) return snprintf(msg, cap, "n must be in 1..%d (got %d)", VS_SET_MAX_SAMPLE, n), VS_EINVAL;
    if (plan.chunks > kSetMaxScratchKeys / ((int64_t)B * n))
        return snprintf(msg, cap, "%lld chunks x %d queries x n = %d are more than 2^27 scratch keys: take longer chunks", (long long)plan.chunks, B, n),
               VS_EINVAL;
    return VS_OK;
}

// vs_set_from_ids: the lists' and the bitmaps' geometry
inline int set_list_check_from_ids(bool have_ids, bool have_out, int32_t B, int64_t m, int64_t ld_ids, int64_t n_rows, int64_t bit0, int64_t ld_words,
                                   char* msg, size_t cap) {
    if (!have_out || (m > 0 && !have_ids)) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    int rc = check_n_rows(n_rows, msg, cap);
    if (rc != VS_OK) return rc;
    if (B < 1 || B > 65535) return snprintf(msg, cap, "B must be in 1..65535 (got %d)", B), VS_EINVAL;
    if (m < 0 || m > kSetMaxRows) return snprintf(msg, cap, "m must be in 0..2^32 - 1 entries a query (got %lld)", (long long)m), VS_EINVAL;
    if (ld_ids < m) return snprintf(msg, cap, "ld_ids = %lld is shorter than m = %lld", (long long)ld_ids, (long long)m), VS_EINVAL;
    if (bit0 < 0 || bit0 > (1ll << 32)) return snprintf(msg, cap, "bit0 must be in 0..2^32 (got %lld)", (long long)bit0), VS_EINVAL;
    const int64_t span = (bit0 + n_rows + 31) >> 5;
    if (ld_words < span)
        return snprintf(msg, cap, "ld_words = %lld is shorter than the %lld words a bitmap spans", (long long)ld_words, (long long)span), VS_EINVAL;
    return VS_OK;
}
// host id lists: an id at or above n_rows names no row (ids below 0 are padding)
inline int set_list_check_id_lists_host(const int64_t* ids, int32_t B, int64_t m, int64_t ld_ids, int64_t n_rows, char* msg, size_t cap) {
    for (int32_t b = 0; b < B; ++b)
        for (int64_t j = 0; j < m; ++j) {
            const int64_t id = ids[(size_t)b * (size_t)ld_ids + (size_t)j];
            if (id >= n_rows) return snprintf(msg, cap, "ids[%d, %lld] = %lld is out of range for %lld rows", b, (long long)j, (long long)id, (long long)n_rows), VS_EINVAL;
        }
    return VS_OK;
}
// what the invert pass keeps of word w of a bitmap whose rows are bits [bit0, bit0 + n_rows): the bits of the rows
VS_SET_HD inline uint32_t set_row_bits_of_word(int64_t w, int64_t bit0, int64_t n_rows) {
    const int64_t lo = w * 32, end = bit0 + n_rows;
    uint32_t keep = 0xFFFFFFFFu;
    if (bit0 > lo) keep &= bit0 - lo >= 32 ? 0u : 0xFFFFFFFFu << (bit0 - lo);
    if (end < lo + 32) keep &= end <= lo ? 0u : 0xFFFFFFFFu >> (lo + 32 - end);
    return keep;
}

}  // namespace vs
