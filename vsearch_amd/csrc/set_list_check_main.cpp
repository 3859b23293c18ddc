// set_list_check_main.cpp -- stand-alone driver of set_list_check.h: the pinned hash against its known answers, the sample key, the window
// arithmetic of vs_set_ids against a plain list on heap arrays at their exact size, the invert mask, the plan rule and every argument check.
// Not part of the library: tests/test_set_list_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.  With
// arguments "hash SEED ID ..." it prints the hash of every (seed, id) pair instead, one a line: the test reads the known answers from it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "set_list_check.h"

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

// vs_set_ids over one query, composed of the header's functions alone as the kernels compose them: span counts, exclusive bases, the skip rule,
// the window, the tail.  out has exactly `limit` slots.
static void list_by_spans(const std::vector<uint8_t>& in_set, int64_t off, int64_t limit, int64_t id_offset, int64_t span_rows, std::vector<int64_t>* out,
                          int64_t* count, int* spans_read) {
    const int64_t n = (int64_t)in_set.size(), spans = (n + span_rows - 1) / span_rows;
    std::vector<int64_t> cnt((size_t)spans, 0), base((size_t)spans, 0);
    for (int64_t r = 0; r < n; ++r) cnt[(size_t)(r / span_rows)] += in_set[(size_t)r];
    int64_t total = 0;
    for (int64_t s = 0; s < spans; ++s) {
        base[(size_t)s] = total;
        total += cnt[(size_t)s];
    }
    *count = total;
    *spans_read = 0;
    out->assign((size_t)limit, 12345);                                                // every slot must be written
    off = set_window_offset(off);
    for (int64_t s = 0; s < spans; ++s) {
        if (set_span_misses(base[(size_t)s], cnt[(size_t)s], off, limit)) continue;
        ++*spans_read;
        int64_t rank = base[(size_t)s];
        for (int64_t r = s * span_rows; r < std::min(n, (s + 1) * span_rows); ++r) {
            if (!in_set[(size_t)r]) continue;
            if (set_rank_in_window(rank, off, limit)) (*out)[(size_t)(rank - off)] = r + id_offset;
            ++rank;
        }
    }
    for (int64_t j = 0; j < limit; ++j)
        if (set_slot_is_tail(j, off, total)) (*out)[(size_t)j] = -1;
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "hash") == 0) {
        for (int i = 2; i + 1 < argc; i += 2)
            printf("0x%08x\n", set_sample_hash(strtoull(argv[i], nullptr, 0), (uint64_t)strtoll(argv[i + 1], nullptr, 0)));
        return 0;
    }
    char msg[512] = {0};
    // ---- the hash: its known answers ----------------------------------------------------------------------------------------------------------
    expect_true("hash (0, 0)", set_sample_hash(0ull, 0ull) == 0x0397ab29u);
    expect_true("hash (0, 1)", set_sample_hash(0ull, 1ull) == 0xc0737b7cu);
    expect_true("hash (1, 0)", set_sample_hash(1ull, 0ull) == 0xddc1ed05u);
    expect_true("hash (12345, 21015323)", set_sample_hash(12345ull, 21015323ull) == 0xfa680e94u);
    expect_true("hash (2^64 - 1, 2^32 - 2)", set_sample_hash(~0ull, 0xFFFFFFFEull) == 0x29fc86afu);
    expect_true("the keyed form is the same function", set_sample_hash_keyed(set_sample_seed_key(77ull), 5ull) == set_sample_hash(77ull, 5ull));
    expect_true("id -1 wraps to the multiplier 0", set_sample_hash(3ull, ~0ull) == (uint32_t)(set_mix64(set_sample_seed_key(3ull)) >> 32));
    // ---- the sample key: order, round trip, never 0 ---------------------------------------------------------------------------------------------
    {
        const uint32_t hs[4] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu}, rows[4] = {0u, 1u, 0x7FFFFFFFu, 0xFFFFFFFEu};
        for (uint32_t h : hs)
            for (uint32_t r : rows) {
                const uint64_t k = set_sample_key(h, r);
                expect_true("key round trip", k != 0ull && set_sample_key_hash(k) == h && set_sample_key_row(k) == r);
                for (uint32_t h2 : hs)
                    for (uint32_t r2 : rows) {
                        const bool first = h < h2 || (h == h2 && r < r2);           // (h, row) ascending is key descending
                        expect_true("key order", first == (k > set_sample_key(h2, r2)));
                    }
            }
    }
    // ---- the window arithmetic against a plain list: exact heap arrays -----------------------------------------------------------------------
    {
        uint32_t state = 11u;
        for (int shape = 0; shape < 6; ++shape)
            for (int64_t n : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)200, (int64_t)517}) {
                std::vector<uint8_t> in((size_t)n, 0);
                for (int64_t r = 0; r < n; ++r) {
                    state = state * 1664525u + 1013904223u;
                    const uint32_t x = state >> 8;
                    in[(size_t)r] = shape == 0 ? 0 : shape == 1 ? 1 : shape == 2 ? (r == 0) : shape == 3 ? (r == n - 1) : shape == 4 ? (x % 100u == 0u) : (x & 1u);
                }
                std::vector<int64_t> all;
                for (int64_t r = 0; r < n; ++r)
                    if (in[(size_t)r]) all.push_back(r + 1000);
                const int64_t total = (int64_t)all.size();
                for (int64_t off : {(int64_t)-3, (int64_t)0, (int64_t)1, total / 2, total - 1, total, total + 1, (int64_t)0x7FFFFFFFFFFFFFFFll})
                    for (int64_t limit : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)64, total, total + 5}) {
                        std::vector<int64_t> got;
                        int64_t count = -1;
                        int read = 0;
                        list_by_spans(in, off, limit, 1000, 64, &got, &count, &read);
                        const int64_t o = off < 0 ? 0 : off;
                        bool ok = count == total && (int64_t)got.size() == limit;
                        for (int64_t j = 0; j < limit && ok; ++j) {
                            const bool have = o < total && j < total - o;
                            ok = got[(size_t)j] == (have ? all[(size_t)(o + j)] : -1);
                        }
                        expect_true("the window equals the plain list's", ok);
                        // no span outside the window is read: at most the spans the window's rows touch
                        int64_t want_read = 0;
                        if (limit > 0 && o < total) {
                            const int64_t last = std::min(total, o > total - limit ? total : o + limit) - 1;
                            want_read = (all[(size_t)last] - 1000) / 64 - (all[(size_t)o] - 1000) / 64 + 1;
                        }
                        expect_true("spans outside the window are not read", read <= want_read);
                    }
            }
    }
    // ---- the invert mask ---------------------------------------------------------------------------------------------------------------------------
    for (int64_t bit0 : {(int64_t)0, (int64_t)1, (int64_t)31, (int64_t)32, (int64_t)37, (int64_t)101})
        for (int64_t n : {(int64_t)1, (int64_t)31, (int64_t)32, (int64_t)33, (int64_t)64, (int64_t)100}) {
            const int64_t words = (bit0 + n + 31) >> 5;
            for (int64_t w = 0; w < words; ++w) {
                uint32_t want = 0u;
                for (int64_t bit = w * 32; bit < w * 32 + 32; ++bit)
                    if (bit >= bit0 && bit < bit0 + n) want |= 1u << (bit & 31);
                expect_true("row bits of a word", set_row_bits_of_word(w, bit0, n) == want);
            }
        }
    // ---- the plan rule ----------------------------------------------------------------------------------------------------------------------------------
    SetListPlan p;
    expect("plan auto", set_list_plan(21015324, 8, true, 0, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan auto: 128 chunks a query, whole spans", p.rows_per_chunk == 165888 && p.chunks == 127 && p.spans == 10262);
    expect("plan small", set_list_plan(1000, 1, false, 0, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan small: one chunk of 8192", p.rows_per_chunk == 8192 && p.chunks == 1 && p.spans == 1);
    expect("plan 64", set_list_plan(4097, 3, true, 64, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan 64: rounded up to a span", p.rows_per_chunk == 2048 && p.chunks == 3 && p.spans == 3);
    expect("plan 6144", set_list_plan(6144, 1, true, 6144, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan 6144: taken as it is", p.rows_per_chunk == 6144 && p.chunks == 1 && p.spans == 3);
    expect("plan 2^32 - 1", set_list_plan(0xFFFFFFFFll, 1, true, 0, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan 2^32 - 1: spans", p.spans == 2097152 && p.chunks * p.rows_per_chunk >= 0xFFFFFFFFll);
    expect("plan n 0", set_list_plan(0, 1, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("plan n 2^32", set_list_plan(1ll << 32, 1, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("plan B 0", set_list_plan(100, 0, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "B must");
    expect("plan rpc", set_list_plan(100, 1, true, 100, &p, msg, sizeof msg), VS_EINVAL, msg, "multiple of 64");
    expect("plan shared B 2", set_list_plan(100, 2, false, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "ld_words = 0");
    expect("plan too many spans", set_list_plan(0xFFFFFFFFll, 65, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "too many");
    expect("plan B 65536", set_list_plan(100, 65536, true, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "too many");

    // ---- the checks -----------------------------------------------------------------------------------------------------------------------------------------
    expect("set ok", set_list_check_set(true, true, 37, 5, 3, 100, 0, &p, msg, sizeof msg), VS_OK, msg, "");
    expect("set NULL", set_list_check_set(false, true, 0, 5, 3, 100, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("set bit0", set_list_check_set(true, true, -1, 5, 3, 100, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "bit0");
    expect("set ld", set_list_check_set(true, true, 64, 5, 3, 100, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "ld_words");
    expect("set every row", set_list_check_set(true, false, 0, 0, 1, 100, 0, &p, msg, sizeof msg), VS_OK, msg, "");
    expect("set every row B 2", set_list_check_set(true, false, 0, 0, 2, 100, 0, &p, msg, sizeof msg), VS_EINVAL, msg, "B = 1");
    expect("ids ok", set_list_check_ids(1ll << 27, 1, true, msg, sizeof msg), VS_OK, msg, "");
    expect("ids count only", set_list_check_ids(0, 9, false, msg, sizeof msg), VS_OK, msg, "");
    expect("ids negative", set_list_check_ids(-1, 1, true, msg, sizeof msg), VS_EINVAL, msg, "limit");
    expect("ids big", set_list_check_ids((1ll << 26) + 1, 2, true, msg, sizeof msg), VS_EINVAL, msg, "2^27");
    expect("ids NULL", set_list_check_ids(5, 2, false, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    {
        std::vector<int64_t> ok = {0, 5, 0x7FFFFFFFFFFFFFFFll}, bad = {0, -1, 2};
        expect("offsets ok", set_list_check_offsets_host(ok.data(), 3, msg, sizeof msg), VS_OK, msg, "");
        expect("offsets negative", set_list_check_offsets_host(bad.data(), 3, msg, sizeof msg), VS_EINVAL, msg, "offsets[1]");
    }
    (void)set_list_plan(21015324, 8, true, 0, &p, msg, sizeof msg);
    expect("sample ok", set_list_check_sample(1024, 8, p, msg, sizeof msg), VS_OK, msg, "");
    expect("sample n 0", set_list_check_sample(0, 8, p, msg, sizeof msg), VS_EINVAL, msg, "n must");
    expect("sample n 1025", set_list_check_sample(1025, 8, p, msg, sizeof msg), VS_EINVAL, msg, "n must");
    (void)set_list_plan(0xFFFFFFFFll, 1, true, 2048, &p, msg, sizeof msg);
    expect("sample scratch", set_list_check_sample(1024, 1, p, msg, sizeof msg), VS_EINVAL, msg, "2^27");
    expect("from ids ok", set_list_check_from_ids(true, true, 3, 7, 7, 100, 37, 5, msg, sizeof msg), VS_OK, msg, "");
    expect("from ids m 0", set_list_check_from_ids(false, true, 1, 0, 0, 100, 0, 4, msg, sizeof msg), VS_OK, msg, "");
    expect("from ids NULL", set_list_check_from_ids(false, true, 1, 2, 2, 100, 0, 4, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("from ids NULL out", set_list_check_from_ids(true, false, 1, 2, 2, 100, 0, 4, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("from ids ld_ids", set_list_check_from_ids(true, true, 2, 7, 6, 100, 0, 4, msg, sizeof msg), VS_EINVAL, msg, "ld_ids");
    expect("from ids ld_words", set_list_check_from_ids(true, true, 2, 7, 7, 100, 37, 4, msg, sizeof msg), VS_EINVAL, msg, "ld_words");
    expect("from ids bit0", set_list_check_from_ids(true, true, 2, 7, 7, 100, -1, 4, msg, sizeof msg), VS_EINVAL, msg, "bit0");
    expect("from ids B", set_list_check_from_ids(true, true, 0, 7, 7, 100, 0, 4, msg, sizeof msg), VS_EINVAL, msg, "B must");
    expect("from ids m", set_list_check_from_ids(true, true, 1, -1, 7, 100, 0, 4, msg, sizeof msg), VS_EINVAL, msg, "m must");
    {
        std::vector<int64_t> ids = {0, 99, -1, -7, 5, 5, 98, 3};                            // [2, 4], exact
        expect("id lists ok", set_list_check_id_lists_host(ids.data(), 2, 4, 4, 100, msg, sizeof msg), VS_OK, msg, "");
        expect("id lists past the rows", set_list_check_id_lists_host(ids.data(), 2, 4, 4, 99, msg, sizeof msg), VS_EINVAL, msg, "ids[0, 1]");
        expect("id lists with a stride", set_list_check_id_lists_host(ids.data(), 2, 3, 5, 100, msg, sizeof msg), VS_OK, msg, "");
    }

    if (failures) {
        fprintf(stderr, "set_list_check: %d failures\n", failures);
        return 1;
    }
    printf("set_list_check: ok\n");
    return 0;
}
