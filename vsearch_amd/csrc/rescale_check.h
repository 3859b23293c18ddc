// rescale_check.h -- the constants, the plan rule and the argument checks of the reweighted index (vs_rescale_plan, vs_index_rescale,
// vs_index_row_stats) that need no device.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_rescale_cpu.py builds one).
#pragma once

#include "new_index_check.h"

namespace vs {

constexpr int kRescaleRun = 64;                       // rows a wave of the rescale takes: their packets are one contiguous range, shared with the source
constexpr int kRescaleSteps = 4;                      // 64-packet steps of a run whose loads are all issued before the first store
constexpr int kRescaleThreads = 256;                  // threads of a workgroup without an LDS image (no column scales, or read from memory)
constexpr int kRescaleImgThreads = 1024;              // threads of a workgroup that holds the column scales as an LDS image: the image may fill the
                                                      // CU's LDS, so the one workgroup a CU then holds brings all 16 waves itself
constexpr int64_t kRescaleLdsMax = 160 * 1024;        // LDS of a CU: the image is the whole of a workgroup's LDS
constexpr int kStatsThreads = 256;                    // threads of a row-stats workgroup
constexpr int kStatsRowsPerWave = 64;                 // rows a wave of the row stats takes, one after the other: lane i keeps row i's results
constexpr int kStatsRowsPerBlock = kStatsRowsPerWave * (kStatsThreads / 64);   // a workgroup's contiguous row range (256)

enum : int { kColScaleNone = 0, kColScaleLds = 1, kColScaleMemory = 2 };       // vs_rescale_plan's out_col_route

// the image of the column scales: n_cols floats, whole 16-byte quads (no scale applies to a padding cell: there is no entry for id n_cols)
inline int64_t rescale_img_bytes(int32_t n_cols) { return ((int64_t)n_cols * 4 + 15) & ~(int64_t)15; }
// the widest index whose column scales are held in LDS (40 960 columns)
constexpr int32_t kRescaleImgMaxCols = (int32_t)(kRescaleLdsMax / 4);

struct RescalePlan {
    int32_t col_route = kColScaleNone;                // where the kernel reads a cell's column scale
    int32_t lds_bytes = 0;                            // of a rescale workgroup: the image, or nothing
    int32_t threads = kRescaleThreads;                // of a rescale workgroup
    int64_t runs = 0;                                 // 64-row runs: what the waves of the grid share out
    int64_t scratch_bytes = 0;                        // host scales staged on the device: 4 bytes a row and 4 a column, for the scales given
};

inline int rescale_plan(int64_t n_rows, int64_t n_packets, int32_t n_cols, int src_dtype, int out_dtype, bool has_row_scale, bool has_col_scale,
                        RescalePlan* out, char* msg, size_t cap) {
    if (n_rows < 0 || n_rows >= 0xFFFFFFFFll) return snprintf(msg, cap, "n_rows must be in 0..2^32 - 2 (got %lld)", (long long)n_rows), VS_EINVAL;
    if (n_packets < 0 || n_packets >= (1ll << 32)) return snprintf(msg, cap, "n_packets must be in 0..2^32 - 1 (got %lld)", (long long)n_packets), VS_EINVAL;
    if (n_cols < 1) return snprintf(msg, cap, "n_cols must be positive (got %d)", n_cols), VS_EINVAL;
    if (n_cols > kTermMaxCols) return snprintf(msg, cap, "n_cols = %d > %d: column ids are stored as uint16", n_cols, kTermMaxCols), VS_EUNSUPPORTED;
    if (!store_dtype_ok(src_dtype)) return snprintf(msg, cap, "bad source store_dtype %d", src_dtype), VS_EINVAL;
    if (out_dtype == VS_NONE) return snprintf(msg, cap, "out_dtype VS_NONE: binarising an index is not covered (VS_F32 or VS_F16)"), VS_EINVAL;
    if (!valued_dtype_ok(out_dtype)) return snprintf(msg, cap, "out_dtype must be VS_F32 or VS_F16 (got %d)", out_dtype), VS_EINVAL;
    RescalePlan p;
    if (has_col_scale) {
        const bool fits = n_cols <= kRescaleImgMaxCols;
        p.col_route = fits ? kColScaleLds : kColScaleMemory;
        p.lds_bytes = fits ? (int32_t)rescale_img_bytes(n_cols) : 0;
        p.threads = fits ? kRescaleImgThreads : kRescaleThreads;
    }
    p.runs = (n_rows + kRescaleRun - 1) / kRescaleRun;
    p.scratch_bytes = (has_row_scale ? 4 * n_rows : 0) + (has_col_scale ? 4 * (int64_t)n_cols : 0);
    *out = p;
    return VS_OK;
}

// what the checks read of an index handle
struct RescaleShape {
    int kind = VS_KIND_CSR, store_dtype = VS_F32, device = 0;
    int64_t n_rows = 0, n_packets = 0;
    int32_t n_cols = 0;
};

// the arguments of vs_index_rescale that need neither the handle nor a device
inline int rescale_check_args(bool have_src, bool have_out, int out_dtype, int64_t rows_extra, int64_t packets_extra, char* msg, size_t cap) {
    if (new_index_check_extra(rows_extra, packets_extra, msg, cap) != VS_OK) return VS_EINVAL;
    if (out_dtype == VS_NONE) return snprintf(msg, cap, "out_dtype VS_NONE: binarising an index is not covered (VS_F32 or VS_F16)"), VS_EINVAL;
    if (!valued_dtype_ok(out_dtype)) return snprintf(msg, cap, "out_dtype must be VS_F32 or VS_F16 (got %d)", out_dtype), VS_EINVAL;
    if (!have_src || !have_out) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    return VS_OK;
}

inline int rescale_check_source(const RescaleShape& src, const char* what, char* msg, size_t cap) {
    if (src.kind != VS_KIND_CSR)
        return snprintf(msg, cap, "a dense (matrix) index has no stored cells to %s (build it as CSR packets)", what), VS_EUNSUPPORTED;
    return VS_OK;
}

// (the scales are each on the host or on the device, independently; a scale on the device belongs to the source's GPU: checked with the device)
// the outputs of vs_index_row_stats: the non-NULL ones all on the host or all on the device.  on_device: bit i = output i is a device pointer,
// have: bit i = output i is given
inline int stats_check_outputs(bool have_src, uint32_t have, uint32_t on_device, char* msg, size_t cap) {
    if (!have_src) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    on_device &= have;
    if (on_device != 0u && on_device != have)
        return snprintf(msg, cap, "the outputs mix host and device pointers: pass all of them on the host or all on the device"), VS_EINVAL;
    return VS_OK;
}

// the grid of the rescale: a wave a run; an image workgroup is persistent (it loads the image once), at most two a CU
inline int64_t rescale_grid(const RescalePlan& p, int cu_count) {
    const int64_t waves = p.threads / 64;
    const int64_t want = std::max<int64_t>(1, (p.runs + waves - 1) / waves);
    const int64_t most = (int64_t)std::max(cu_count, 1) * (p.col_route == kColScaleLds ? 2 : 32);
    return std::min(want, most);
}

// the grid of the row stats: a workgroup a block of 256 rows
inline int64_t stats_grid(int64_t n_rows) { return std::max<int64_t>(1, (n_rows + kStatsRowsPerBlock - 1) / kStatsRowsPerBlock); }

}  // namespace vs
