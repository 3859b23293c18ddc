// select_check_main.cpp -- stand-alone driver of select_check.h: the plan rule, every argument check and the per-shard split rule of a
// row-sharded selection, the latter against a plain recount on heap arrays at their exact size.
// Not part of the library: tests/test_select_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "select_check.h"

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

static int split(const std::vector<int64_t>& ids, const std::vector<int64_t>& cuts, std::vector<int64_t>& begin, char* msg, size_t cap) {
    begin.assign(cuts.size(), -7);
    return select_split_by_shard(ids.data(), (int64_t)ids.size(), cuts.data(), (int32_t)cuts.size() - 1, begin.data(), msg, cap);
}

int main() {
    char msg[512] = {0};
    // ---- the plan rule ----------------------------------------------------------------------------------------------------------------------------------
    SelectPlan p;
    expect("plan one", select_plan(1, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan one: one scan block", p.scan_blocks == 1 && p.scratch_bytes == 8 + 16 + 32);
    expect("plan 4096", select_plan(4096, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan 4096: still one block", p.scan_blocks == 1);
    expect("plan 4097", select_plan(4097, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan 4097: two blocks", p.scan_blocks == 2 && p.scratch_bytes == 8 * 4097 + 24 + 32);
    expect("plan headline", select_plan(21015324, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan headline: 5131 blocks, 168 MB of staged ids", p.scan_blocks == 5131 && p.scratch_bytes == 8 * 21015324ll + 8 * 5132 + 32);
    expect("plan largest", select_plan(0xFFFFFFFEll, &p, msg, sizeof msg), VS_OK, msg, "");
    expect("plan empty", select_plan(0, &p, msg, sizeof msg), VS_EINVAL, msg, "empty selection");
    expect("plan negative", select_plan(-1, &p, msg, sizeof msg), VS_EINVAL, msg, "n must be");
    expect("plan 2^32 - 1", select_plan(0xFFFFFFFFll, &p, msg, sizeof msg), VS_EINVAL, msg, "n must be");
    // ---- the checks ----------------------------------------------------------------------------------------------------------------------------------------
    expect("args ok", select_check_args(true, true, true, 5, 0, 7, msg, sizeof msg), VS_OK, msg, "");
    expect("args src", select_check_args(false, true, true, 5, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("args out", select_check_args(true, true, false, 5, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("args ids", select_check_args(true, false, true, 5, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "ids is NULL");
    expect("args empty", select_check_args(true, true, true, 0, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "empty selection");
    expect("args empty without ids", select_check_args(true, false, true, 0, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "empty selection");
    expect("args negative n", select_check_args(true, true, true, -3, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "n must be");
    expect("args rows_extra", select_check_args(true, true, true, 5, -1, 0, msg, sizeof msg), VS_EINVAL, msg, ">= 0");
    expect("args packets_extra", select_check_args(true, true, true, 5, 0, -1, msg, sizeof msg), VS_EINVAL, msg, ">= 0");
    {
        const std::vector<int64_t> ids = {3, 0, 9, 9, 0};
        expect("host ids ok", select_check_host_ids(ids.data(), 5, 0, 10, msg, sizeof msg), VS_OK, msg, "");
        expect("host ids n_rows", select_check_host_ids(ids.data(), 5, 0, 9, msg, sizeof msg), VS_EINVAL, msg, "id 9 (position 2");
        expect("host ids offset", select_check_host_ids(ids.data(), 5, 1, 10, msg, sizeof msg), VS_EINVAL, msg, "id 0 (position 1");
        const std::vector<int64_t> shifted = {100, 109};
        expect("host ids shifted", select_check_host_ids(shifted.data(), 2, 100, 10, msg, sizeof msg), VS_OK, msg, "");
        const std::vector<int64_t> minus = {4, -1};
        expect("host ids -1", select_check_host_ids(minus.data(), 2, 0, 10, msg, sizeof msg), VS_EINVAL, msg, "id -1 (position 1");
        const std::vector<int64_t> far = {0x7FFFFFFFFFFFFFFFll, (int64_t)0x8000000000000000ull};
        expect("host ids int64 max", select_check_host_ids(far.data(), 1, -5, 10, msg, sizeof msg), VS_EINVAL, msg, "outside");
        expect("host ids int64 min", select_check_host_ids(far.data() + 1, 1, 5, 10, msg, sizeof msg), VS_EINVAL, msg, "outside");
        expect("host ids empty source", select_check_host_ids(ids.data(), 1, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "outside");
    }
    SelectShape csr, dense;
    dense.kind = VS_KIND_DENSE;
    dense.device = 1;
    expect("dense: csr is free", select_check_dense(csr, 5, 7, 3, msg, sizeof msg), VS_OK, msg, "");
    expect("dense ok", select_check_dense(dense, 0, 0, 1, msg, sizeof msg), VS_OK, msg, "");
    expect("dense rows_extra", select_check_dense(dense, 1, 0, 1, msg, sizeof msg), VS_EINVAL, msg, "no append");
    expect("dense packets_extra", select_check_dense(dense, 0, 1, 1, msg, sizeof msg), VS_EINVAL, msg, "no append");
    expect("dense device", select_check_dense(dense, 0, 0, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "own device");
    for (const char* noun : {"selected", "compacted"}) {                    // (vs_index_compact has no check header of its own: its noun is covered here)
        char text[96];
        snprintf(text, sizeof text, "the %s index with its spare capacity exceeds 2^32 rows or packets", noun);
        expect("capacity ok", new_index_check_capacity(noun, 100, 1000, 5, 7, msg, sizeof msg), VS_OK, msg, "");
        expect("capacity rows", new_index_check_capacity(noun, 0xFFFFFFF0ll, 10, 0xF, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
        expect("capacity packets", new_index_check_capacity(noun, 10, 0xFFFFFFF0ll, 0, 0x10, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
        expect("capacity repeats past 2^32", new_index_check_capacity(noun, 1ll << 20, 1ll << 33, 0, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
        expect("capacity huge extra", new_index_check_capacity(noun, 10, 10, 0x7FFFFFFFFFFFFFFFll, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
        expect_true("capacity: the whole sentence with the call's noun", strcmp(msg, text) == 0);
    }
    expect_true("new_index_bytes", new_index_bytes(10, 100, 32) == 100 * 48 + 44 && new_index_bytes(0, 0, 0) == 4 && value_bytes(VS_F16) == 16);
    // ---- the split rule -------------------------------------------------------------------------------------------------------------------------------------
    std::vector<int64_t> begin;
    const std::vector<int64_t> cuts = {0, 10, 10, 25, 40};                    // four shards, the second one empty
    expect("split ascending", split({0, 3, 9, 10, 24, 25, 39}, cuts, begin, msg, sizeof msg), VS_OK, msg, "");
    expect_true("split ascending: begins", begin == std::vector<int64_t>({0, 3, 3, 5, 7}));
    expect("split inside a shard any order", split({9, 0, 9, 24, 10, 10, 39}, cuts, begin, msg, sizeof msg), VS_OK, msg, "");
    expect_true("split any order: begins", begin == std::vector<int64_t>({0, 3, 3, 6, 7}));
    expect("split skips shards", split({30, 26}, cuts, begin, msg, sizeof msg), VS_OK, msg, "");
    expect_true("split skips: begins", begin == std::vector<int64_t>({0, 0, 0, 0, 2}));
    expect("split first shard only", split({1}, cuts, begin, msg, sizeof msg), VS_OK, msg, "");
    expect_true("split first only: begins", begin == std::vector<int64_t>({0, 1, 1, 1, 1}));
    expect("split nothing", split({}, cuts, begin, msg, sizeof msg), VS_OK, msg, "");
    expect_true("split nothing: begins", begin == std::vector<int64_t>({0, 0, 0, 0, 0}));
    expect("split back", split({3, 12, 9}, cuts, begin, msg, sizeof msg), VS_EINVAL, msg, "id 9 (position 2");
    expect("split back names the rule", split({30, 24}, cuts, begin, msg, sizeof msg), VS_EINVAL, msg, "across shards");
    expect("split id n_rows", split({3, 40}, cuts, begin, msg, sizeof msg), VS_EINVAL, msg, "outside [0, 40)");
    expect("split id -1", split({-1}, cuts, begin, msg, sizeof msg), VS_EINVAL, msg, "outside [0, 40)");
    expect("split cuts start", split({1}, {1, 5}, begin, msg, sizeof msg), VS_EINVAL, msg, "row 0");
    expect("split cuts descend", split({1}, {0, 5, 4}, begin, msg, sizeof msg), VS_EINVAL, msg, "ascend");
    {
        const int64_t one = 1, c[2] = {0, 5};
        int64_t b[2];
        expect("split no shards", select_split_by_shard(&one, 1, c, 0, b, msg, sizeof msg), VS_EINVAL, msg, "n_shards");
        expect("split NULL", select_split_by_shard(nullptr, 1, c, 1, b, msg, sizeof msg), VS_EINVAL, msg, "NULL");
        expect("split NULL begin", select_split_by_shard(&one, 1, c, 1, nullptr, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    }
    {   // a long non-decreasing list against a recount
        uint32_t state = 5u;
        auto next = [&]() { return state = state * 1664525u + 1013904223u; };
        const std::vector<int64_t> c7 = {0, 1, 1, 500, 501, 4096, 4097, 9000};
        std::vector<int64_t> ids;
        for (size_t s = 0; s + 1 < c7.size(); ++s)
            for (int t = 0, m = (int)(next() % 300u); t < m && c7[s + 1] > c7[s]; ++t) ids.push_back(c7[s] + (int64_t)(next() % (uint32_t)(c7[s + 1] - c7[s])));
        expect("split long", split(ids, c7, begin, msg, sizeof msg), VS_OK, msg, "");
        bool ok = begin.front() == 0 && begin.back() == (int64_t)ids.size();
        for (size_t s = 0; s + 1 < c7.size() && ok; ++s)
            for (int64_t i = begin[s]; i < begin[s + 1]; ++i) ok = ok && ids[(size_t)i] >= c7[s] && ids[(size_t)i] < c7[s + 1];
        expect_true("split long: every id lies in its shard", ok);
    }

    if (failures) {
        fprintf(stderr, "select_check: %d failures\n", failures);
        return 1;
    }
    printf("select_check: ok\n");
    return 0;
}
