// select_check.h -- the constants, the plan rule and the argument checks of the sub-index (vs_select_plan, vs_index_select_rows) that need no
// device, and the per-shard split rule a row-sharded selection follows (vs_select_split).
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_select_cpu.py builds one).
#pragma once

#include "new_index_check.h"

namespace vs {

constexpr int kSelectThreads = 256;                   // threads of the workgroups of select.hip
constexpr int kSelectRun = 64;                        // new rows a wave of the gather takes: their packets are one contiguous range of the new index
constexpr int kSelectSteps = 4;                       // 64-packet steps of a run whose loads are all issued before the first store
constexpr int64_t kSelectScanRows = 4096;             // ids of a scan block (block_scan.h: kScanRows)
constexpr int64_t kSelectMaxIds = 0xFFFFFFFEll;       // the new index's rows: n + rows_extra < 2^32 - 1, as in vs_index_compact

struct SelectPlan {
    int64_t scan_blocks = 1;                          // blocks of 4096 ids of the two-level scan
    int64_t scratch_bytes = 0;                        // the ids staged on the device (host ids) + block sums + totals, flag and counts
};

inline int select_plan(int64_t n_ids, SelectPlan* out, char* msg, size_t cap) {
    if (n_ids == 0) return snprintf(msg, cap, "empty selection: n must be positive"), VS_EINVAL;
    if (n_ids < 0 || n_ids > kSelectMaxIds) return snprintf(msg, cap, "n must be in 1..2^32 - 2 (got %lld)", (long long)n_ids), VS_EINVAL;
    SelectPlan p;
    p.scan_blocks = (n_ids + kSelectScanRows - 1) / kSelectScanRows;
    p.scratch_bytes = 8 * n_ids + 8 * (p.scan_blocks + 1) + 32;
    *out = p;
    return VS_OK;
}

// what the checks read of an index handle
struct SelectShape {
    int kind = VS_KIND_CSR, device = 0;
    int64_t n_rows = 0;
};

// the arguments that need neither the handle nor a device
inline int select_check_args(bool have_src, bool have_ids, bool have_out, int64_t n, int64_t rows_extra, int64_t packets_extra, char* msg, size_t cap) {
    if (new_index_check_extra(rows_extra, packets_extra, msg, cap) != VS_OK) return VS_EINVAL;
    if (!have_src || !have_out) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    if (n == 0) return snprintf(msg, cap, "empty selection: n must be positive"), VS_EINVAL;
    if (n < 0 || n > kSelectMaxIds) return snprintf(msg, cap, "n must be in 1..2^32 - 2 (got %lld)", (long long)n), VS_EINVAL;
    if (!have_ids) return snprintf(msg, cap, "ids is NULL"), VS_EINVAL;
    return VS_OK;
}

// host ids: every one names a stored row (-1 is not accepted: a selected row has to exist)
inline int select_check_host_ids(const int64_t* ids, int64_t n, int64_t id_offset, int64_t n_rows, char* msg, size_t cap) {
    for (int64_t i = 0; i < n; ++i) {
        // (the difference of two int64 in this order always fits a uint64)
        if (ids[i] < id_offset || (uint64_t)ids[i] - (uint64_t)id_offset >= (uint64_t)n_rows)
            return snprintf(msg, cap, "document id %lld (position %lld of the selection) is outside [%lld, %lld)", (long long)ids[i], (long long)i,
                            (long long)id_offset, (long long)(id_offset + n_rows)), VS_EINVAL;
    }
    return VS_OK;
}

// the dense matrix kind: a row gather of the padded matrix, as in vs_index_compact
inline int select_check_dense(const SelectShape& src, int64_t rows_extra, int64_t packets_extra, int device, char* msg, size_t cap) {
    if (src.kind == VS_KIND_CSR) return VS_OK;
    if (rows_extra || packets_extra) return snprintf(msg, cap, "a dense (matrix) index has no append: rows_extra and packets_extra must be 0"), VS_EINVAL;
    if (device != src.device) return snprintf(msg, cap, "a dense (matrix) index is selected from on its own device"), VS_EUNSUPPORTED;
    return VS_OK;
}

// ---- the split of a selection over the shards of a row-sharded index ------------------------------------------------------------------------------
// Shard s holds the global rows [cuts[s], cuts[s + 1]); cuts [n_shards + 1] ascends from 0.  The ids are dealt to the shards IN THE ORDER GIVEN:
// begin[s] .. begin[s + 1] are the positions of the ids of shard s.  That is the unsharded selection exactly when the shard of ids[i] never
// decreases along i; a list that goes back to an earlier shard would move a row across shards and is VS_EINVAL.  An id outside every shard is
// VS_EINVAL.  begin: [n_shards + 1].
inline int select_split_by_shard(const int64_t* ids, int64_t n, const int64_t* cuts, int32_t n_shards, int64_t* begin, char* msg, size_t cap) {
    if (n_shards < 1) return snprintf(msg, cap, "n_shards must be positive (got %d)", n_shards), VS_EINVAL;
    if (n < 0) return snprintf(msg, cap, "n must be >= 0"), VS_EINVAL;
    if (!cuts || !begin || (!ids && n > 0)) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    if (cuts[0] != 0) return snprintf(msg, cap, "cuts must start at row 0"), VS_EINVAL;
    for (int32_t s = 0; s < n_shards; ++s)
        if (cuts[s + 1] < cuts[s]) return snprintf(msg, cap, "cuts must ascend (shard %d ends at row %lld, before it starts)", s, (long long)cuts[s + 1]), VS_EINVAL;
    int32_t s = 0;
    begin[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids[i];
        if (id < 0 || id >= cuts[n_shards])
            return snprintf(msg, cap, "document id %lld (position %lld of the selection) is outside [0, %lld)", (long long)id, (long long)i, (long long)cuts[n_shards]), VS_EINVAL;
        if (id < cuts[s])
            return snprintf(msg, cap, "document id %lld (position %lld of the selection) goes back to an earlier shard than shard %d: a selection cannot move rows across shards", (long long)id,
                            (long long)i, s), VS_EINVAL;
        while (id >= cuts[s + 1]) begin[++s] = i;     // (id < cuts[n_shards]: s stays below n_shards)
    }
    while (s < n_shards) begin[++s] = n;
    return VS_OK;
}

}  // namespace vs
