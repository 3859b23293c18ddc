// combine_check.h -- the constants, the plan rule, the argument checks and the grids of the combined index (vs_combine_plan, vs_index_combine)
// that need no device.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_combine_cpu.py builds one).
#pragma once

#include "new_index_check.h"

namespace vs {

constexpr int kCombineThreads = 256;                  // threads of a count workgroup and of a wave-route fill workgroup
constexpr int kCombineWaves = kCombineThreads / 64;   // a wave takes a row
constexpr int kCombineWaveCells = 2048;               // wave route: rows with cells_a + cells_b <= this; one fp32 slot a union cell, 8 KB a wave
constexpr int kCombineRegPackets = 2;                 // packets of a source row a lane of the wave route holds in registers: lane l holds packets l and l + 64
constexpr int kCombineRegCells = 64 * 8 * kCombineRegPackets;   // cells a side of the longest row read once and held (1024); a longer row is re-read by every pass
static_assert(kCombineRegCells >= 768, "the 96 packets of a 768-cell row are held in registers");
constexpr int kCombineGroupThreads = 1024;            // workgroup route: one workgroup a longer row
constexpr int kCombineGroupCells = 32768;             // workgroup route: the largest union a row may have (128 KB of slots beside the bitmaps)
constexpr int64_t kCombineLdsMax = 160 * 1024;        // LDS of a CU
constexpr int kCombineScanScratch = 16 * 8;           // workgroup route: the wave sums of block_excl_scan<16>

struct CombinePlan {
    int32_t wave_cells = kCombineWaveCells;           // the wave route's limit on cells_a + cells_b
    int32_t group_cells = kCombineGroupCells;         // the workgroup route's limit on the union
    int32_t count_lds_bytes = 0;                      // of a count workgroup: two bitmaps a wave
    int32_t wave_lds_bytes = 0;                       // of a wave-route fill workgroup: two bitmaps, the prefix and the slots, a wave
    int32_t group_lds_bytes = 0;                      // of a workgroup-route fill workgroup: two bitmaps, the prefix, the slots, the scan's sums
    int32_t group_slots = 0;                          // slots of the workgroup route at this width: min(group_cells, n_cols rounded up to 8)
    int64_t long_rows_cap = 0;                        // entries of the list of rows the workgroup route takes
    int64_t scan_blocks = 1;                          // blocks of 4096 rows of the two-level scan
    int64_t scratch_bytes = 0;                        // union counts + the list of long rows + block sums + the totals
};

constexpr int kCombineTotalsBytes = 64;               // the device words the host reads after the scan (CombineTotals of combine.hip)

inline int64_t combine_words(int32_t n_cols) { return ((int64_t)n_cols + 31) >> 5; }

inline int combine_check_out_dtype(int out_dtype, char* msg, size_t cap) {
    if (out_dtype == VS_NONE) return snprintf(msg, cap, "out_dtype VS_NONE: binarising an index is not covered (VS_F32 or VS_F16)"), VS_EINVAL;
    if (!valued_dtype_ok(out_dtype)) return snprintf(msg, cap, "out_dtype must be VS_F32 or VS_F16 (got %d)", out_dtype), VS_EINVAL;
    return VS_OK;
}

// a row with more than wave_cells stored cells on both sides together spans more than wave_cells / 8 packets: at most this many rows are long
inline int64_t combine_long_rows_cap(int64_t n_rows, int64_t packets_a, int64_t packets_b) {
    return std::min<int64_t>(n_rows, (packets_a + packets_b) / (kCombineWaveCells / 8) + 1);
}

inline int combine_plan(int64_t n_rows, int64_t packets_a, int64_t packets_b, int32_t n_cols, int dtype_a, int dtype_b, int out_dtype, CombinePlan* out,
                        char* msg, size_t cap) {
    if (n_rows < 0 || n_rows >= 0xFFFFFFFFll) return snprintf(msg, cap, "n_rows must be in 0..2^32 - 2 (got %lld)", (long long)n_rows), VS_EINVAL;
    if (packets_a < 0 || packets_a >= (1ll << 32) || packets_b < 0 || packets_b >= (1ll << 32))
        return snprintf(msg, cap, "n_packets must be in 0..2^32 - 1 (got %lld and %lld)", (long long)packets_a, (long long)packets_b), VS_EINVAL;
    if (n_cols < 1) return snprintf(msg, cap, "n_cols must be positive (got %d)", n_cols), VS_EINVAL;
    if (n_cols > kTermMaxCols) return snprintf(msg, cap, "n_cols = %d > %d: column ids are stored as uint16", n_cols, kTermMaxCols), VS_EUNSUPPORTED;
    if (!store_dtype_ok(dtype_a) || !store_dtype_ok(dtype_b)) return snprintf(msg, cap, "bad source store_dtype %d / %d", dtype_a, dtype_b), VS_EINVAL;
    const int rc = combine_check_out_dtype(out_dtype, msg, cap);
    if (rc != VS_OK) return rc;
    CombinePlan p;
    const int64_t words = combine_words(n_cols);
    p.group_slots = (int32_t)std::min<int64_t>(kCombineGroupCells, ((int64_t)n_cols + 7) & ~(int64_t)7);
    p.count_lds_bytes = (int32_t)(kCombineWaves * 2 * words * 4);
    p.wave_lds_bytes = (int32_t)(kCombineWaves * (3 * words + kCombineWaveCells) * 4);
    p.group_lds_bytes = (int32_t)((3 * words + p.group_slots) * 4 + kCombineScanScratch);
    p.long_rows_cap = combine_long_rows_cap(n_rows, packets_a, packets_b);
    p.scan_blocks = std::max<int64_t>(1, (n_rows + 4095) / 4096);
    p.scratch_bytes = 4 * n_rows + 4 * p.long_rows_cap + 8 * (p.scan_blocks + 1) + kCombineTotalsBytes;
    *out = p;
    return VS_OK;
}
static_assert(kCombineWaves * (3 * 2048 + kCombineWaveCells) * 4 <= kCombineLdsMax, "the wave route fits the LDS at 65 535 columns");
static_assert((3 * 2048 + kCombineGroupCells) * 4 + kCombineScanScratch <= kCombineLdsMax, "the workgroup route fits the LDS at 65 535 columns");

// what the checks read of an index handle
struct CombineShape {
    int kind = VS_KIND_CSR, store_dtype = VS_F32, device = 0;
    int64_t n_rows = 0, n_packets = 0;
    int32_t n_cols = 0;
};

// the arguments of vs_index_combine that need neither a handle nor a device
inline int combine_check_args(bool have_a, bool have_b, bool have_out, int out_dtype, int64_t rows_extra, int64_t packets_extra, char* msg, size_t cap) {
    if (new_index_check_extra(rows_extra, packets_extra, msg, cap) != VS_OK) return VS_EINVAL;
    const int rc = combine_check_out_dtype(out_dtype, msg, cap);
    if (rc != VS_OK) return rc;
    if (!have_a || !have_b || !have_out) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    return VS_OK;
}

inline int combine_check_sources(const CombineShape& a, const CombineShape& b, char* msg, size_t cap) {
    if (a.kind != VS_KIND_CSR || b.kind != VS_KIND_CSR)
        return snprintf(msg, cap, "a dense (matrix) index has no stored cells to combine (build it as CSR packets)"), VS_EUNSUPPORTED;
    if (a.n_rows != b.n_rows || a.n_cols != b.n_cols)
        return snprintf(msg, cap, "index a is %lld x %d, index b %lld x %d: row r is combined with row r, column by column", (long long)a.n_rows, a.n_cols,
                        (long long)b.n_rows, b.n_cols), VS_EINVAL;
    if (a.device != b.device) return snprintf(msg, cap, "index a lives on device %d, index b on device %d", a.device, b.device), VS_EINVAL;
    return VS_OK;
}

// what the count step found, read back with the totals: the lowest row with a repeated column in a / in b, the lowest row whose union
// exceeds the workgroup route's slots (none: kCombineNoRow)
constexpr uint32_t kCombineNoRow = 0xFFFFFFFFu;
inline int combine_check_flags(uint32_t repeat_a, uint32_t repeat_b, uint32_t too_wide, char* msg, size_t cap) {
    if (repeat_a != kCombineNoRow || repeat_b != kCombineNoRow) {
        const bool in_a = repeat_a <= repeat_b;               // (both: the lower row, a first)
        return snprintf(msg, cap, "row %u of index %s stores a column twice: the sum of a repeated column depends on the order (make the columns of a row unique)",
                        in_a ? repeat_a : repeat_b, in_a ? "a" : "b"), VS_EINVAL;
    }
    if (too_wide != kCombineNoRow)
        return snprintf(msg, cap, "row %u has a union of more than %d cells: a combined row is staged in LDS", too_wide, kCombineGroupCells), VS_EUNSUPPORTED;
    return VS_OK;
}

// the grids: persistent workgroups of four waves stride over the rows (count: 8 a CU; fill, whose LDS holds two workgroups a CU at most: 4);
// the workgroup route takes a workgroup a long row
inline int64_t combine_count_grid(int64_t n_rows, int cu_count) {
    return std::max<int64_t>(1, std::min<int64_t>((n_rows + kCombineWaves - 1) / kCombineWaves, (int64_t)std::max(cu_count, 1) * 8));
}
inline int64_t combine_wave_grid(int64_t n_rows, int cu_count) {
    return std::max<int64_t>(1, std::min<int64_t>((n_rows + kCombineWaves - 1) / kCombineWaves, (int64_t)std::max(cu_count, 1) * 4));
}
inline int64_t combine_group_grid(int64_t n_long, int cu_count) { return std::max<int64_t>(1, std::min<int64_t>(n_long, (int64_t)std::max(cu_count, 1) * 2)); }

}  // namespace vs
