// concat_check_main.cpp -- stand-alone driver of concat_check.h: the plan rule, every argument check, the table's bases and the source search of
// the kernels, the latter against a plain scan on heap arrays at their exact size.
// Not part of the library: tests/test_concat_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "concat_check.h"

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

static int plan(const std::vector<int64_t>& rows, const std::vector<int64_t>& packets, int32_t n_cols, const std::vector<int>& dtypes, int out_dtype, ConcatPlan* p,
                char* msg, size_t cap) {
    return concat_plan((int32_t)rows.size(), rows.data(), packets.data(), n_cols, dtypes.data(), out_dtype, p, msg, cap);
}

int main() {
    char msg[512] = {0};
    // ---- the plan rule ----------------------------------------------------------------------------------------------------------------------------------
    ConcatPlan p;
    expect("plan one", plan({5}, {7}, 100, {VS_F32}, VS_F32, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan one: totals, a 48-byte entry and the counters", p.rows == 5 && p.packets == 7 && p.scratch_bytes == 48 + 16 && !p.all_binary);
    expect_true("plan one: the LDS of the table", p.lds_bytes == 6152 && p.lds_bytes >= kConcatMapLds && p.lds_bytes >= kConcatCopyLds);
    expect("plan mixed", plan({3, 0, 9}, {4, 0, 0}, 100, {VS_F32, VS_F16, VS_NONE}, VS_F16, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan mixed: totals", p.rows == 12 && p.packets == 4 && p.scratch_bytes == 3 * 48 + 16);
    expect("plan binary", plan({3, 2}, {4, 1}, 100, {VS_NONE, VS_NONE}, VS_NONE, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan binary: all binary", p.all_binary);
    expect("plan binary to fp16", plan({3, 2}, {4, 1}, 100, {VS_NONE, VS_NONE}, VS_F16, &p, msg, sizeof msg), VS_OK, msg, "");
    expect("plan binarising", plan({3, 2}, {4, 1}, 100, {VS_NONE, VS_F16}, VS_NONE, &p, msg, sizeof msg), VS_EINVAL, msg, "binarising is not covered");
    expect("plan out_dtype", plan({3}, {4}, 100, {VS_F32}, 7, &p, msg, sizeof msg), VS_EINVAL, msg, "out_dtype must be");
    expect("plan store dtype", plan({3, 2}, {4, 1}, 100, {VS_F32, 5}, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "source 1: bad store_dtype");
    expect("plan empty", plan({0, 0}, {0, 0}, 100, {VS_F32, VS_F32}, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "empty join");
    expect("plan negative rows", plan({3, -1}, {4, 1}, 100, {VS_F32, VS_F32}, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "source 1: n_rows");
    expect("plan negative packets", plan({3, 1}, {-4, 1}, 100, {VS_F32, VS_F32}, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "source 0: n_packets");
    expect("plan n_cols 0", plan({3}, {4}, 0, {VS_F32}, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "n_cols must be positive");
    expect("plan n_cols 65536", plan({3}, {4}, 65536, {VS_F32}, VS_F32, &p, msg, sizeof msg), VS_EUNSUPPORTED, msg, "uint16");
    expect("plan n_cols 65535", plan({3}, {4}, 65535, {VS_F32}, VS_F32, &p, msg, sizeof msg), VS_OK, msg, "");
    expect("plan rows 2^32 - 2", plan({0x7FFFFFFFll, 0x7FFFFFFFll}, {1, 1}, 10, {VS_F32, VS_F32}, VS_F32, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan rows 2^32 - 2: the largest join", p.rows == 0xFFFFFFFEll);
    expect("plan rows 2^32 - 1", plan({0x7FFFFFFFll, 0x80000000ll}, {1, 1}, 10, {VS_F32, VS_F32}, VS_F32, &p, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect("plan packets 2^32", plan({5, 5}, {0x80000000ll, 0x80000000ll}, 10, {VS_F32, VS_F32}, VS_F32, &p, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect("plan packets 2^32 - 1", plan({5, 5}, {0x80000000ll, 0x7FFFFFFFll}, 10, {VS_F32, VS_F32}, VS_F32, &p, msg, sizeof msg), VS_OK, msg, "");
    {
        std::vector<int64_t> r256(256, 1000), k256(256, 12000), r257(257, 1);
        std::vector<int> d256(256, VS_F16), d257(257, VS_F16);
        expect("plan 256 sources", plan(r256, k256, 30000, d256, VS_F16, &p, msg, sizeof msg), VS_OK, msg, "");
        expect_true("plan 256 sources: totals and the table", p.rows == 256000 && p.packets == 3072000 && p.scratch_bytes == 256 * 48 + 16);
        expect("plan 257 sources", plan(r257, r257, 30000, d257, VS_F16, &p, msg, sizeof msg), VS_EINVAL, msg, "n_src must be in 1..256");
        const int64_t one = 1;
        const int dt = VS_F32;
        expect("plan no sources", concat_plan(0, &one, &one, 10, &dt, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "n_src must be");
        expect("plan NULL rows", concat_plan(1, nullptr, &one, 10, &dt, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "NULL");
        expect("plan NULL packets", concat_plan(1, &one, nullptr, 10, &dt, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "NULL");
        expect("plan NULL dtypes", concat_plan(1, &one, &one, 10, nullptr, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    }
    // ---- the checks ----------------------------------------------------------------------------------------------------------------------------------------
    expect("args ok", concat_check_args(true, true, 3, 0, 7, msg, sizeof msg), VS_OK, msg, "");
    expect("args srcs", concat_check_args(false, true, 3, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("args out", concat_check_args(true, false, 3, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("args n_src 0", concat_check_args(true, true, 0, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "n_src must be");
    expect("args n_src 257", concat_check_args(true, true, 257, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "n_src must be");
    expect("args n_src negative", concat_check_args(true, true, -1, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "n_src must be");
    expect("args rows_extra", concat_check_args(true, true, 3, -1, 0, msg, sizeof msg), VS_EINVAL, msg, ">= 0");
    expect("args packets_extra", concat_check_args(true, true, 3, 0, -1, msg, sizeof msg), VS_EINVAL, msg, ">= 0");
    ConcatShape a, b;
    a.n_cols = b.n_cols = 100;
    expect("source ok", concat_check_source(a, b, 1, msg, sizeof msg), VS_OK, msg, "");
    b.n_cols = 101;
    expect("source width", concat_check_source(a, b, 2, msg, sizeof msg), VS_EINVAL, msg, "source 2 has 101 columns");
    b.n_cols = 100;
    b.device = 1;
    expect("source device", concat_check_source(a, b, 1, msg, sizeof msg), VS_EINVAL, msg, "device 1");
    b.kind = VS_KIND_DENSE;
    expect("source dense", concat_check_source(a, b, 3, msg, sizeof msg), VS_EUNSUPPORTED, msg, "source 3 is a dense (matrix) index");
    expect("source 0 dense", concat_check_source(b, b, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "source 0 is a dense");
    expect("out_dtype fp32", concat_check_out_dtype(VS_F32, true, msg, sizeof msg), VS_OK, msg, "");
    expect("out_dtype none", concat_check_out_dtype(VS_NONE, true, msg, sizeof msg), VS_OK, msg, "");
    expect("out_dtype none valued", concat_check_out_dtype(VS_NONE, false, msg, sizeof msg), VS_EINVAL, msg, "binarising");
    expect("capacity ok", new_index_check_capacity("joined", 100, 1000, 5, 7, msg, sizeof msg), VS_OK, msg, "");
    expect("capacity rows", new_index_check_capacity("joined", 0xFFFFFFF0ll, 10, 0xF, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect("capacity packets", new_index_check_capacity("joined", 10, 0xFFFFFFF0ll, 0, 0x10, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect("capacity huge extra", new_index_check_capacity("joined", 10, 10, 0x7FFFFFFFFFFFFFFFll, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect_true("grid map: one more thread for the last pointer", concat_map_grid(255) == 1 && concat_map_grid(256) == 2 && concat_map_grid(1) == 1);
    expect_true("grid copy", concat_copy_grid(1, 256) == 1 && concat_copy_grid(1024, 256) == 1 && concat_copy_grid(1025, 256) == 2 &&
                                 concat_copy_grid(1ll << 31, 256) == 256 * 32);
    // ---- the table's bases and the search -----------------------------------------------------------------------------------------------------------------
    {
        uint32_t state = 11u;
        auto next = [&]() { return state = state * 1664525u + 1013904223u; };
        for (int n_src : {1, 2, 3, 17, 255, 256}) {
            std::vector<ConcatShape> shapes((size_t)n_src);
            for (auto& s : shapes) {
                s.n_rows = next() % 4u == 0u ? 0 : (int64_t)(next() % 70u);             // empty sources in every place
                s.n_packets = s.n_rows == 0 || next() % 5u == 0u ? 0 : (int64_t)(next() % 300u);
                s.store_dtype = (int)(next() % 3u) - 1;
            }
            std::vector<ConcatEntry> table((size_t)n_src);
            concat_fill_bases(shapes.data(), n_src, table.data());
            std::vector<uint32_t> row_base((size_t)kConcatMaxSources, kConcatNoBase), pk_base((size_t)kConcatMaxSources, kConcatNoBase);
            int64_t rows = 0, packets = 0;
            bool ok = true;
            for (int s = 0; s < n_src; ++s) {
                ok = ok && table[(size_t)s].row_base == (uint32_t)rows && table[(size_t)s].pk_base == (uint32_t)packets && table[(size_t)s].store_dtype == shapes[(size_t)s].store_dtype;
                row_base[(size_t)s] = table[(size_t)s].row_base;
                pk_base[(size_t)s] = table[(size_t)s].pk_base;
                rows += shapes[(size_t)s].n_rows;
                packets += shapes[(size_t)s].n_packets;
            }
            expect_true("bases are the running sums", ok);
            // every row and every packet is found in the source that holds it
            int64_t r = 0, q = 0;
            for (int s = 0; s < n_src && ok; ++s) {
                for (int64_t i = 0; i < shapes[(size_t)s].n_rows; ++i, ++r) ok = ok && concat_find(row_base.data(), (uint32_t)r) == s;
                for (int64_t i = 0; i < shapes[(size_t)s].n_packets; ++i, ++q) ok = ok && concat_find(pk_base.data(), (uint32_t)q) == s;
            }
            expect_true("search: every row and packet lies in its source", ok && r == rows && q == packets);
        }
        // the largest bases: a row and a packet just below 2^32 behind 255 sources that end there
        std::vector<uint32_t> base((size_t)kConcatMaxSources, 0xFFFFFFFDu);
        base[0] = 0u;
        expect_true("search: the last source at the top of the range", concat_find(base.data(), 0xFFFFFFFDu) == 255 && concat_find(base.data(), 0xFFFFFFFCu) == 0);
    }

    if (failures) {
        fprintf(stderr, "concat_check: %d failures\n", failures);
        return 1;
    }
    printf("concat_check: ok\n");
    return 0;
}
