// concat_check.h -- the constants, the plan rule, the argument checks, the source table and the grids of the joined index (vs_concat_plan,
// vs_index_concat) that need no device.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_concat_cpu.py builds one).
#pragma once

#include "new_index_check.h"

namespace vs {

constexpr int kConcatMaxSources = 256;                // sources of one join: the table of a workgroup is this many slots
constexpr int kConcatThreads = 256;                   // threads of the workgroups of concat.hip
constexpr int kConcatWaves = kConcatThreads / 64;
constexpr int kConcatSteps = 4;                       // 64-packet steps of a round whose loads are all issued before the first store
constexpr int kConcatRound = 64 * kConcatSteps;       // result packets a wave takes at a time
constexpr uint32_t kConcatNoBase = 0xFFFFFFFFu;       // the base of a table slot behind the last source: above every row and every packet
constexpr int64_t kConcatMaxRows = 0xFFFFFFFEll;      // the new index's rows: total + rows_extra < 2^32 - 1, as in vs_index_compact

// a source as the kernels read it: one entry of the device table, in the order of the sources.  Rows and packets below 2^32: the bases fit 32 bits
struct ConcatEntry {
    uint32_t row_base = 0, pk_base = 0;               // R_s and P_s: the rows and the packets of the sources before this one
    const void* pk = nullptr;                         // uint32 [n_rows + 1]
    const void* cols = nullptr;                       // packets of 8 uint16 column ids
    const void* vals = nullptr;                       // 8 values a packet (fp32 | fp16), absent for a binary source
    const void* live = nullptr;                       // the source's live words, or NULL: no row of it is deleted
    int32_t store_dtype = VS_F32;
    int32_t pad = 0;
};
static_assert(sizeof(ConcatEntry) == 48, "the plan counts these bytes");

constexpr int kConcatCounterBytes = 16;               // the device words the host reads after the map step: the dead rows
// the LDS of a workgroup: the part of the table a kernel searches and reads, kConcatMaxSources slots whatever n_src is (a search of fixed depth).
// map: two bases (the row bases with one slot more) and two pointers a slot; copy: one base (one slot more), two pointers and the dtype a slot;
// either rounded up to whole 8 bytes
constexpr int32_t kConcatMapLds = ((kConcatMaxSources + 1) * 4 + kConcatMaxSources * (4 + 8 + 8) + 7) & ~7;
constexpr int32_t kConcatCopyLds = ((kConcatMaxSources + 1) * 4 + kConcatMaxSources * (8 + 8 + 4) + 7) & ~7;

struct ConcatPlan {
    int64_t rows = 0, packets = 0;                    // the totals
    int64_t scratch_bytes = 0;                        // the source table + the counters
    int32_t lds_bytes = 0;                            // of a workgroup (the larger of the two kernels')
    bool all_binary = true;
};

inline int concat_check_n_src(int32_t n_src, char* msg, size_t cap) {
    if (n_src < 1 || n_src > kConcatMaxSources) return snprintf(msg, cap, "n_src must be in 1..%d (got %d)", kConcatMaxSources, n_src), VS_EINVAL;
    return VS_OK;
}

// out_dtype against the sources' stores: VS_F32 / VS_F16 always, VS_NONE only when every source is binary
inline int concat_check_out_dtype(int out_dtype, bool all_binary, char* msg, size_t cap) {
    if (out_dtype == VS_NONE) {
        if (!all_binary) return snprintf(msg, cap, "out_dtype VS_NONE with a valued source: binarising is not covered (VS_F32 or VS_F16)"), VS_EINVAL;
        return VS_OK;
    }
    if (out_dtype != VS_F32 && out_dtype != VS_F16) return snprintf(msg, cap, "out_dtype must be VS_F32, VS_F16 or VS_NONE (got %d)", out_dtype), VS_EINVAL;
    return VS_OK;
}

inline int concat_plan(int32_t n_src, const int64_t* rows, const int64_t* packets, int32_t n_cols, const int* dtypes, int out_dtype, ConcatPlan* out, char* msg,
                       size_t cap) {
    int rc = concat_check_n_src(n_src, msg, cap);
    if (rc != VS_OK) return rc;
    if (!rows || !packets || !dtypes) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    if (n_cols < 1) return snprintf(msg, cap, "n_cols must be positive (got %d)", n_cols), VS_EINVAL;
    if (n_cols > kTermMaxCols) return snprintf(msg, cap, "n_cols = %d > %d: column ids are stored as uint16", n_cols, kTermMaxCols), VS_EUNSUPPORTED;
    ConcatPlan p;
    for (int32_t s = 0; s < n_src; ++s) {
        if (rows[s] < 0 || rows[s] >= 0xFFFFFFFFll) return snprintf(msg, cap, "source %d: n_rows must be in 0..2^32 - 2 (got %lld)", s, (long long)rows[s]), VS_EINVAL;
        if (packets[s] < 0 || packets[s] >= (1ll << 32))
            return snprintf(msg, cap, "source %d: n_packets must be in 0..2^32 - 1 (got %lld)", s, (long long)packets[s]), VS_EINVAL;
        if (!store_dtype_ok(dtypes[s])) return snprintf(msg, cap, "source %d: bad store_dtype %d", s, dtypes[s]), VS_EINVAL;
        p.rows += rows[s];                             // (256 terms below 2^32 each: no overflow)
        p.packets += packets[s];
        p.all_binary = p.all_binary && dtypes[s] == VS_NONE;
    }
    rc = concat_check_out_dtype(out_dtype, p.all_binary, msg, cap);
    if (rc != VS_OK) return rc;
    if (p.rows == 0) return snprintf(msg, cap, "empty join: the sources hold no row"), VS_EINVAL;
    rc = new_index_check_capacity("joined", p.rows, p.packets, 0, 0, msg, cap);
    if (rc != VS_OK) return rc;
    p.scratch_bytes = (int64_t)n_src * (int64_t)sizeof(ConcatEntry) + kConcatCounterBytes;
    p.lds_bytes = std::max(kConcatMapLds, kConcatCopyLds);
    *out = p;
    return VS_OK;
}

// the arguments of vs_index_concat that need neither a handle nor a device
inline int concat_check_args(bool have_srcs, bool have_out, int32_t n_src, int64_t rows_extra, int64_t packets_extra, char* msg, size_t cap) {
    if (new_index_check_extra(rows_extra, packets_extra, msg, cap) != VS_OK) return VS_EINVAL;
    const int rc = concat_check_n_src(n_src, msg, cap);
    if (rc != VS_OK) return rc;
    if (!have_srcs || !have_out) return snprintf(msg, cap, "NULL argument"), VS_EINVAL;
    return VS_OK;
}

// what the checks read of an index handle
struct ConcatShape {
    int kind = VS_KIND_CSR, store_dtype = VS_F32, device = 0;
    int64_t n_rows = 0, n_packets = 0;
    int32_t n_cols = 0;
};

// source s against source 0
inline int concat_check_source(const ConcatShape& first, const ConcatShape& s, int32_t at, char* msg, size_t cap) {
    if (s.kind != VS_KIND_CSR) return snprintf(msg, cap, "source %d is a dense (matrix) index: it has no packets to join (build it as CSR packets)", at), VS_EUNSUPPORTED;
    if (s.n_cols != first.n_cols) return snprintf(msg, cap, "source %d has %d columns, source 0 has %d: joined rows share one vocabulary", at, s.n_cols, first.n_cols), VS_EINVAL;
    if (s.device != first.device) return snprintf(msg, cap, "source %d lives on device %d, source 0 on device %d", at, s.device, first.device), VS_EINVAL;
    return VS_OK;
}

// the bases of the table: entry s starts at the rows and packets of the sources before it.  rows / packets: the shapes of the n_src sources
inline void concat_fill_bases(const ConcatShape* shapes, int32_t n_src, ConcatEntry* table) {
    int64_t r = 0, p = 0;
    for (int32_t s = 0; s < n_src; ++s) {
        table[s].row_base = (uint32_t)r;
        table[s].pk_base = (uint32_t)p;
        table[s].store_dtype = shapes[s].store_dtype;
        r += shapes[s].n_rows;
        p += shapes[s].n_packets;
    }
}

// the search of the kernels, on the host: the LAST slot whose base is <= x among kConcatMaxSources slots (slots behind the last source hold
// kConcatNoBase).  Of sources that start at the same place -- every one but the last of them is empty -- the last is found: the one that holds x
inline int concat_find(const uint32_t* base, uint32_t x) {
    int i = 0;
    for (int step = kConcatMaxSources / 2; step > 0; step >>= 1)
        if (base[i + step] <= x) i += step;
    return i;
}

// the grids: map takes a thread a result row and one more for the last pointer; copy persistent workgroups of four waves over rounds of 256 packets
inline int64_t concat_map_grid(int64_t rows) { return (rows + 1 + kConcatThreads - 1) / kConcatThreads; }
inline int64_t concat_copy_grid(int64_t packets, int cu_count) {
    const int64_t rounds = (packets + kConcatRound - 1) / kConcatRound;
    return std::max<int64_t>(1, std::min<int64_t>((rounds + kConcatWaves - 1) / kConcatWaves, (int64_t)std::max(cu_count, 1) * 32));
}

}  // namespace vs
