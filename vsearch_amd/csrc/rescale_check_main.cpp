// rescale_check_main.cpp -- stand-alone driver of rescale_check.h: the plan rule at the widths where the column-scale route changes, every
// argument check of vs_index_rescale and vs_index_row_stats, the capacity rule and the grids.
// Not part of the library: tests/test_rescale_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstring>

#include "rescale_check.h"

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

static int plan(int64_t rows, int64_t packets, int32_t cols, int sd, int od, bool rs, bool cs, RescalePlan* p, char* msg, size_t cap) {
    return rescale_plan(rows, packets, cols, sd, od, rs, cs, p, msg, cap);
}

int main() {
    char msg[512] = {0};
    RescalePlan p;
    // ---- the plan rule: the route of the column scales by width -----------------------------------------------------------------------------------------
    expect("plan 1 column", plan(10, 10, 1, VS_F32, VS_F32, false, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan 1 column: a 16-byte image", p.col_route == kColScaleLds && p.lds_bytes == 16 && p.threads == kRescaleImgThreads);
    expect("plan 300 columns", plan(10, 10, 300, VS_F32, VS_F16, true, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan 300 columns: 1200 bytes, staged scales", p.col_route == kColScaleLds && p.lds_bytes == 1200 && p.scratch_bytes == 4 * 10 + 4 * 300);
    expect("plan V", plan(21015324, 21015324ll * 96, 29523, VS_F32, VS_F32, true, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan V: the image is 118 096 bytes", p.col_route == kColScaleLds && p.lds_bytes == 118096 && p.runs == (21015324 + 63) / 64);
    expect_true("plan V: staged scales", p.scratch_bytes == 4 * 21015324ll + 4 * 29523);
    expect("plan image limit", plan(10, 10, kRescaleImgMaxCols, VS_F16, VS_F32, false, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan image limit: 40 960 columns fill the LDS", kRescaleImgMaxCols == 40960 && p.col_route == kColScaleLds && p.lds_bytes == 160 * 1024);
    expect("plan one past", plan(10, 10, kRescaleImgMaxCols + 1, VS_F16, VS_F32, false, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan one past: from memory, no LDS", p.col_route == kColScaleMemory && p.lds_bytes == 0 && p.threads == kRescaleThreads);
    expect("plan 65535", plan(10, 10, 65535, VS_NONE, VS_F32, false, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan 65535: from memory", p.col_route == kColScaleMemory && p.lds_bytes == 0);
    expect("plan no column scales", plan(10, 10, 65535, VS_F32, VS_F32, true, false, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan no column scales: no route, no LDS", p.col_route == kColScaleNone && p.lds_bytes == 0 && p.scratch_bytes == 40);
    expect("plan no scale", plan(10, 10, 300, VS_F32, VS_F32, false, false, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan no scale: no scratch", p.col_route == kColScaleNone && p.scratch_bytes == 0 && p.threads == kRescaleThreads);
    expect("plan no packets", plan(5, 0, 300, VS_F32, VS_F32, true, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan no packets: one run", p.runs == 1);
    expect("plan no rows", plan(0, 0, 300, VS_F32, VS_F32, true, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("plan no rows: no run, a grid of one", p.runs == 0 && rescale_grid(p, 256) == 1);
    expect("plan 65536 columns", plan(10, 10, 65536, VS_F32, VS_F32, false, true, &p, msg, sizeof msg), VS_EUNSUPPORTED, msg, "uint16");
    expect("plan 0 columns", plan(10, 10, 0, VS_F32, VS_F32, false, true, &p, msg, sizeof msg), VS_EINVAL, msg, "n_cols must be positive");
    expect("plan negative rows", plan(-1, 10, 5, VS_F32, VS_F32, false, true, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("plan 2^32 - 1 rows", plan(0xFFFFFFFFll, 10, 5, VS_F32, VS_F32, false, true, &p, msg, sizeof msg), VS_EINVAL, msg, "n_rows");
    expect("plan negative packets", plan(1, -1, 5, VS_F32, VS_F32, false, true, &p, msg, sizeof msg), VS_EINVAL, msg, "n_packets");
    expect("plan 2^32 packets", plan(1, 1ll << 32, 5, VS_F32, VS_F32, false, true, &p, msg, sizeof msg), VS_EINVAL, msg, "n_packets");
    expect("plan bad source dtype", plan(1, 1, 5, VS_I32, VS_F32, false, true, &p, msg, sizeof msg), VS_EINVAL, msg, "source store_dtype");
    expect("plan binarising", plan(1, 1, 5, VS_F32, VS_NONE, false, true, &p, msg, sizeof msg), VS_EINVAL, msg, "binarising");
    expect("plan bad out dtype", plan(1, 1, 5, VS_F32, VS_I32, false, true, &p, msg, sizeof msg), VS_EINVAL, msg, "out_dtype must be");
    // ---- the grids ------------------------------------------------------------------------------------------------------------------------------------------
    expect("grid plan", plan(64 * 16 * 1000, 10, 300, VS_F32, VS_F32, false, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("grid image: two persistent workgroups a CU", rescale_grid(p, 256) == 512 && rescale_grid(p, 0) == 2);
    expect("grid plan few", plan(65, 10, 300, VS_F32, VS_F32, false, true, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("grid image: two runs, one workgroup", p.runs == 2 && rescale_grid(p, 256) == 1);
    expect("grid plan plain", plan(64 * 4 * 10 + 1, 10, 300, VS_F32, VS_F32, true, false, &p, msg, sizeof msg), VS_OK, msg, "");
    expect_true("grid plain: four runs a workgroup", rescale_grid(p, 256) == 11);
    expect_true("stats grid", stats_grid(0) == 1 && stats_grid(1) == 1 && stats_grid(256) == 1 && stats_grid(257) == 2 && stats_grid(21015324) == 82092);
    // ---- the argument checks ----------------------------------------------------------------------------------------------------------------------------------
    expect("args ok", rescale_check_args(true, true, VS_F16, 0, 7, msg, sizeof msg), VS_OK, msg, "");
    expect("args src", rescale_check_args(false, true, VS_F32, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("args out", rescale_check_args(true, false, VS_F32, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("args binarising", rescale_check_args(true, true, VS_NONE, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "binarising");
    expect("args dtype", rescale_check_args(true, true, VS_I64, 0, 0, msg, sizeof msg), VS_EINVAL, msg, "out_dtype must be");
    expect("args rows_extra", rescale_check_args(true, true, VS_F32, -1, 0, msg, sizeof msg), VS_EINVAL, msg, ">= 0");
    expect("args packets_extra", rescale_check_args(true, true, VS_F32, 0, -1, msg, sizeof msg), VS_EINVAL, msg, ">= 0");
    RescaleShape csr, dense;
    dense.kind = VS_KIND_DENSE;
    expect("source csr", rescale_check_source(csr, "rescale", msg, sizeof msg), VS_OK, msg, "");
    expect("source dense", rescale_check_source(dense, "rescale", msg, sizeof msg), VS_EUNSUPPORTED, msg, "no stored cells to rescale");
    expect("stats none", stats_check_outputs(true, 0u, 0u, msg, sizeof msg), VS_OK, msg, "");
    expect("stats all host", stats_check_outputs(true, 31u, 0u, msg, sizeof msg), VS_OK, msg, "");
    expect("stats all device", stats_check_outputs(true, 31u, 31u, msg, sizeof msg), VS_OK, msg, "");
    expect("stats some, device", stats_check_outputs(true, 5u, 5u, msg, sizeof msg), VS_OK, msg, "");
    expect("stats a stale device bit of a NULL output", stats_check_outputs(true, 5u, 7u, msg, sizeof msg), VS_OK, msg, "");
    expect("stats mixed", stats_check_outputs(true, 31u, 4u, msg, sizeof msg), VS_EINVAL, msg, "mix host and device");
    expect("stats mixed two", stats_check_outputs(true, 3u, 1u, msg, sizeof msg), VS_EINVAL, msg, "mix host and device");
    expect("stats src", stats_check_outputs(false, 31u, 0u, msg, sizeof msg), VS_EINVAL, msg, "NULL");
    expect("capacity ok", new_index_check_capacity("rescaled", 100, 1000, 5, 7, msg, sizeof msg), VS_OK, msg, "");
    expect("capacity nothing", new_index_check_capacity("rescaled", 0, 0, 0, 0, msg, sizeof msg), VS_OK, msg, "");
    expect("capacity rows", new_index_check_capacity("rescaled", 0xFFFFFFF0ll, 10, 0xF, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect("capacity packets", new_index_check_capacity("rescaled", 10, 0xFFFFFFF0ll, 0, 0x10, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect("capacity huge extra", new_index_check_capacity("rescaled", 10, 10, 0x7FFFFFFFFFFFFFFFll, 0, msg, sizeof msg), VS_EUNSUPPORTED, msg, "2^32");
    expect_true("image bytes", rescale_img_bytes(1) == 16 && rescale_img_bytes(4) == 16 && rescale_img_bytes(5) == 32 && rescale_img_bytes(29523) == 118096);

    if (failures) {
        fprintf(stderr, "rescale_check: %d failures\n", failures);
        return 1;
    }
    printf("rescale_check: ok\n");
    return 0;
}
