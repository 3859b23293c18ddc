// combine_check_main.cpp -- stand-alone driver of combine_check.h: the plan rule at the widths the tests use, every argument check of
// vs_index_combine, the flags of the count step, the capacity rule and the grids.
// Not part of the library: tests/test_combine_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstring>

#include "combine_check.h"

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

int main() {
    char msg[512] = {0};
    CombinePlan p;
    // ---- the plan rule ----------------------------------------------------------------------------------------------------------------------------------
    expect("plan 1 column", combine_plan(10, 10, 10, 1, VS_F32, VS_NONE, VS_F32, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan 1 column: one word a bitmap", p.count_lds_bytes == 4 * 2 * 4 && p.wave_lds_bytes == 4 * (3 + 2048) * 4 && p.group_slots == 8 &&
                                                        p.group_lds_bytes == (3 + 8) * 4 + 128);
    expect("plan 300 columns", combine_plan(10, 10, 10, 300, VS_F16, VS_F16, VS_F16, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan 300 columns", p.wave_cells == 2048 && p.group_cells == 32768 && p.count_lds_bytes == 4 * 2 * 10 * 4 && p.wave_lds_bytes == 4 * (30 + 2048) * 4 &&
                                        p.group_slots == 304 && p.group_lds_bytes == (30 + 304) * 4 + 128);
    expect("plan V", combine_plan(21015324, 21015324ll * 96, 21015324ll * 11, 29523, VS_F32, VS_NONE, VS_F32, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan V: 923 words a bitmap, 19 268 bytes a wave", p.wave_lds_bytes == 4 * (3 * 923 + 2048) * 4 && p.group_slots == 29528 &&
                                                                       p.group_lds_bytes == (3 * 923 + 29528) * 4 + 128 && p.scan_blocks == (21015324 + 4095) / 4096);
    expect_true("plan V: the long rows are bounded by the packets", p.long_rows_cap == (21015324ll * 107) / 256 + 1);
    expect_true("plan V: scratch", p.scratch_bytes == 4 * 21015324ll + 4 * p.long_rows_cap + 8 * (p.scan_blocks + 1) + 64);
    expect("plan 65535", combine_plan(10, 10, 10, 65535, VS_NONE, VS_F32, VS_F16, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan 65535: both routes fit the LDS", p.wave_lds_bytes == 4 * (3 * 2048 + 2048) * 4 && p.wave_lds_bytes <= kCombineLdsMax &&
                                                           p.group_slots == 32768 && p.group_lds_bytes == (3 * 2048 + 32768) * 4 + 128 && p.group_lds_bytes <= kCombineLdsMax);
    expect_true("plan 65535: the long rows are bounded by the rows", p.long_rows_cap == 1);
    expect("plan no rows", combine_plan(0, 0, 0, 300, VS_F32, VS_F32, VS_F32, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan no rows", p.long_rows_cap == 0 && p.scan_blocks == 1 && p.scratch_bytes == 16 + 64);
    expect("plan 65536 columns", combine_plan(10, 10, 10, 65536, VS_F32, VS_F32, VS_F32, &p, msg, sizeof msg), VS_EUNSUPPORTED, msg, "uint16");
    expect("plan 0 columns", combine_plan(10, 10, 10, 0, VS_F32, VS_F32, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "n_cols must be positive");
    expect("plan negative rows", combine_plan(-1, 10, 10, 5, VS_F32, VS_F32, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("plan 2^32 - 1 rows", combine_plan(0xFFFFFFFFll, 10, 10, 5, VS_F32, VS_F32, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("plan negative packets a", combine_plan(1, -1, 1, 5, VS_F32, VS_F32, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "n_packets");
    expect("plan 2^32 packets b", combine_plan(1, 1, 1ll << 32, 5, VS_F32, VS_F32, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "n_packets");
    expect("plan bad dtype a", combine_plan(1, 1, 1, 5, VS_I32, VS_F32, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "source store_dtype");
    expect("plan bad dtype b", combine_plan(1, 1, 1, 5, VS_F32, VS_U8, VS_F32, &p, msg, sizeof msg), VS_EINVAL, msg, "source store_dtype");
    expect("plan binarising", combine_plan(1, 1, 1, 5, VS_F32, VS_F32, VS_NONE, &p, msg, sizeof msg), VS_EINVAL, msg, "binarising");
    expect("plan bad out dtype", combine_plan(1, 1, 1, 5, VS_F32, VS_F32, VS_I32, &p, msg, sizeof msg), VS_EINVAL, msg, "out_dtype must be");
    // ---- the grids ------------------------------------------------------------------------------------------------------------------------------------------
    expect_true("count grid", combine_count_grid(0, 256) == 1 && combine_count_grid(4, 256) == 1 && combine_count_grid(5, 256) == 2 &&
                                  combine_count_grid(1000000, 256) == 2048 && combine_count_grid(1000000, 0) == 8);
    expect_true("wave grid", combine_wave_grid(0, 256) == 1 && combine_wave_grid(9, 256) == 3 && combine_wave_grid(1000000, 256) == 1024);
    expect_true("group grid", combine_group_grid(0, 256) == 1 && combine_group_grid(3, 256) == 3 && combine_group_grid(100000, 256) == 512);
    expect_true("long rows cap", combine_long_rows_cap(5, 0, 0) == 1 && combine_long_rows_cap(0, 0, 0) == 0 && combine_long_rows_cap(1000, 255, 256) == 2 &&
                                     combine_long_rows_cap(1000, 256, 256) == 3);
    // ---- the argument checks ----------------------------------------------------------------------------------------------------------------------------------
    expect("args ok", combine_check_args(true, true, true, VS_F16, 0, 7, msg, sizeof msg), VS_OK, msg, "");
    expect("args a", combine_check_args(false, true, true, VS_F32, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("args b", combine_check_args(true, false, true, VS_F32, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("args out", combine_check_args(true, true, false, VS_F32, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("args binarising", combine_check_args(true, true, true, VS_NONE, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "binarising");
    expect("args dtype", combine_check_args(true, true, true, VS_I64, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "out_dtype must be");
    expect("args rows_extra", combine_check_args(true, true, true, VS_F32, -1, 0, msg, sizeof msg), VS_EINVAL, msg, ">= 0");
    expect("args packets_extra", combine_check_args(true, true, true, VS_F32, 0, -1, msg, sizeof msg), VS_EINVAL, msg, ">= 0");
    CombineShape a, b, dense;
    a.n_rows = b.n_rows = dense.n_rows = 10;
    a.n_cols = b.n_cols = dense.n_cols = 300;
    dense.kind = VS_KIND_DENSE;
    expect("sources ok", combine_check_sources(a, b, msg, sizeof msg), VS_OK, msg, "");
    expect("sources the same", combine_check_sources(a, a, msg, sizeof msg), VS_OK, msg, "");
    expect("sources dense a", combine_check_sources(dense, b, msg, sizeof msg), VS_EUNSUPPORTED, msg, "no stored cells to combine");
    expect("sources dense b", combine_check_sources(a, dense, msg, sizeof msg), VS_EUNSUPPORTED, msg, "no stored cells to combine");
    b.n_rows = 11;
    expect("sources rows", combine_check_sources(a, b, msg, sizeof msg), VS_EINVAL, msg, "index a is 10 x 300, index b 11 x 300");
    b.n_rows = 10;
    b.n_cols = 301;
    expect("sources cols", combine_check_sources(a, b, msg, sizeof msg), VS_EINVAL, msg, "index b 10 x 301");
    b.n_cols = 300;
    b.device = 1;
    expect("sources devices", combine_check_sources(a, b, msg, sizeof msg), VS_EINVAL, msg, "index a lives on device 0, index b on device 1");
    // ---- the flags of the count step ---------------------------------------------------------------------------------------------------------------------------
    expect("flags none", combine_check_flags(kCombineNoRow, kCombineNoRow, kCombineNoRow, msg, sizeof msg), VS_OK, msg, "");
    expect("flags a", combine_check_flags(7, kCombineNoRow, kCombineNoRow, msg, sizeof msg), VS_EINVAL, msg, "row 7 of index a stores a column twice");
    expect("flags b", combine_check_flags(kCombineNoRow, 0, kCombineNoRow, msg, sizeof msg), VS_EINVAL, msg, "row 0 of index b stores a column twice");
    expect("flags both, b lower", combine_check_flags(9, 3, kCombineNoRow, msg, sizeof msg), VS_EINVAL, msg, "row 3 of index b");
    expect("flags both, same row", combine_check_flags(4, 4, kCombineNoRow, msg, sizeof msg), VS_EINVAL, msg, "row 4 of index a");
    expect("flags a repeat before a wide row", combine_check_flags(9, kCombineNoRow, 2, msg, sizeof msg), VS_EINVAL, msg, "row 9 of index a");
    expect("flags too wide", combine_check_flags(kCombineNoRow, kCombineNoRow, 5, msg, sizeof msg), VS_EUNSUPPORTED, msg, "row 5 has a union of more than 32768 cells");
    // ---- the capacity rule ---------------------------------------------------------------------------------------------------------------------------------------
    expect("capacity ok", new_index_check_capacity("combined", 100, 1000, 5, 7, msg, sizeof msg), VS_OK, msg, "");
    expect("capacity nothing", new_index_check_capacity("combined", 0, 0, 0, 0, msg, sizeof msg), VS_OK, msg, "");
    expect("capacity rows", new_index_check_capacity("combined", 0xFFFFFFF0ll, 10, 0xF, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect("capacity packets", new_index_check_capacity("combined", 10, 0xFFFFFFF0ll, 0, 0x10, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect("capacity huge extra", new_index_check_capacity("combined", 10, 10, 0x7FFFFFFFFFFFFFFFll, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");

    if (failures) {
        fprintf(stderr, "combine_check: %d failures\n", failures);
        return 1;
    }
    printf("combine_check: ok\n");
    return 0;
}
