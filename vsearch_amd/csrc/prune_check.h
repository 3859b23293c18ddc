// prune_check.h -- the constants, the plan rule and the argument checks of index pruning (vs_prune_plan, vs_index_prune) that need no device,
// and the three small functions the select and pack kernels of prune.hip run on a cell or a packet -- the eligibility test, the digit of a
// key, the first cells of a tie group -- __host__ __device__, so that the stand-alone check exercises the very code.
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (tests/test_prune_cpu.py builds one).
#pragma once

#include "new_index_check.h"
#include "value_check.h"

namespace vs {

constexpr int kPruneThreads = 256;                    // threads of the workgroups of prune.hip
constexpr int kPruneWaves = kPruneThreads / 64;       // a wave takes a row
constexpr int kPruneRegPackets = 2;                   // packets of a row a lane holds in registers: lane l holds packets l and l + 64
constexpr int kPruneRegCells = 64 * 8 * kPruneRegPackets;   // cells of the longest row selected from registers (1024); a longer row is re-read
constexpr int32_t kPruneMaxTopk = 65535;              // a row has no more distinct columns
constexpr int kPruneBins = 256;                       // bins of a wave's histogram: 8 bits of the key a round, 4 rounds
static_assert(kPruneRegCells >= 768, "the 96 packets of a 768-cell row are selected from registers");

struct PrunePlan {
    int32_t reg_cells = kPruneRegCells;
    int32_t lds_bytes = 0;                            // of a select workgroup: col_keep once, a histogram and (with a protect index) a bitmap a wave
    int64_t scan_blocks = 1;                          // blocks of 4096 rows of the two-level scan
    int64_t scratch_bytes = 0;                        // keep bytes (one a source packet) + kept counts + block sums + the non-zero count
};

// the rules against the store: a binary index holds 1 everywhere, so a cut by value is a mistake of the caller's
inline int prune_check_rules(int32_t topk, bool has_min, int store_dtype, char* msg, size_t cap) {
    if (topk < 0 || topk > kPruneMaxTopk) return snprintf(msg, cap, "topk must be in 0..%d (0: no cut; got %d)", kPruneMaxTopk, topk), VS_EINVAL;
    if (!store_dtype_ok(store_dtype)) return snprintf(msg, cap, "bad store_dtype %d", store_dtype), VS_EINVAL;
    if (store_dtype == VS_NONE && (topk > 0 || has_min))
        return snprintf(msg, cap, "topk and min_value need stored values: every value of a binary index is 1 (col_keep alone is allowed)"), VS_EINVAL;
    return VS_OK;
}

inline int64_t prune_keep_words(int32_t n_cols) { return ((int64_t)n_cols + 31) >> 5; }

inline int prune_plan(int64_t n_rows, int64_t n_packets, int32_t n_cols, int store_dtype, int32_t topk, bool has_protect, PrunePlan* out, char* msg,
                      size_t cap) {
    if (n_rows < 0 || n_rows >= 0xFFFFFFFFll) return snprintf(msg, cap, "n_rows must be in 0..2^32 - 2 (got %lld)", (long long)n_rows), VS_EINVAL;
    if (n_packets < 0 || n_packets >= (1ll << 32)) return snprintf(msg, cap, "n_packets must be in 0..2^32 - 1 (got %lld)", (long long)n_packets), VS_EINVAL;
    if (n_cols < 1) return snprintf(msg, cap, "n_cols must be positive (got %d)", n_cols), VS_EINVAL;
    if (n_cols > kTermMaxCols) return snprintf(msg, cap, "n_cols = %d > %d: column ids are stored as uint16", n_cols, kTermMaxCols), VS_EUNSUPPORTED;
    const int rc = prune_check_rules(topk, false, store_dtype, msg, cap);
    if (rc != VS_OK) return rc;
    PrunePlan p;
    const int64_t words = prune_keep_words(n_cols);
    p.lds_bytes = (int32_t)(4 * (words + (int64_t)kPruneWaves * kPruneBins + (has_protect ? (int64_t)kPruneWaves * words : 0)));
    p.scan_blocks = std::max<int64_t>(1, (n_rows + 4095) / 4096);
    p.scratch_bytes = n_packets + 4 * n_rows + 8 * (p.scan_blocks + 1) + 8;
    *out = p;
    return VS_OK;
}

// what the checks read of an index handle
struct PruneShape {
    int kind = VS_KIND_CSR, store_dtype = VS_F32, device = 0;
    int64_t n_rows = 0;
    int32_t n_cols = 0;
};

inline int prune_check_source(const PruneShape& src, char* msg, size_t cap) {
    if (src.kind != VS_KIND_CSR)
        return snprintf(msg, cap, "a dense (matrix) index stores every element: it has no cells to prune (build it as CSR packets)"), VS_EUNSUPPORTED;
    return VS_OK;
}

inline int prune_check_protect(const PruneShape& src, const PruneShape& prot, char* msg, size_t cap) {
    if (prot.kind != VS_KIND_CSR) return snprintf(msg, cap, "the protect index must be a CSR index (binary or valued)"), VS_EINVAL;
    if (prot.n_rows != src.n_rows || prot.n_cols != src.n_cols)
        return snprintf(msg, cap, "the protect index is %lld x %d, the source %lld x %d: row r protects cells of row r", (long long)prot.n_rows, prot.n_cols,
                        (long long)src.n_rows, src.n_cols), VS_EINVAL;
    if (prot.device != src.device) return snprintf(msg, cap, "the protect index lives on device %d, the source on device %d", prot.device, src.device), VS_EINVAL;
    return VS_OK;
}

// col_keep and out_kept: both on the host or both on the device, like the arrays of every other call
inline int prune_check_pointers(bool have_keep, bool keep_on_device, bool have_kept, bool kept_on_device, char* msg, size_t cap) {
    if (have_keep && have_kept && keep_on_device != kept_on_device)
        return snprintf(msg, cap, "col_keep is a %s pointer and out_kept a %s pointer: pass both on the host or both on the device", keep_on_device ? "device" : "host",
                        kept_on_device ? "device" : "host"), VS_EINVAL;
    return VS_OK;
}

// ---- what the kernels run on a cell or a packet ---------------------------------------------------------------------------------------------
// eligible under min_value: the fp32-widened stored value compared as a float; a NaN on either side is never >=
VS_VALUE_HD inline bool prune_value_ok(float v, bool has_min, float min_value) { return !has_min || v >= min_value; }
// the 8 bits of `key` that round `round` (3 = the most significant, first) of the radix select ranks by
VS_VALUE_HD inline uint32_t prune_digit(uint32_t key, int round) { return (key >> (8 * round)) & 0xFFu; }
// the first `take` set bits of an 8-bit cell mask (stored order inside a packet is bit order); take <= 0: none
VS_VALUE_HD inline uint32_t prune_first_bits(uint32_t bits, int take) {
    uint32_t out = 0u;
    for (int t = 0; t < 8; ++t) {
        const uint32_t b = (bits >> t) & 1u;
        if (b && take > 0) {
            out |= 1u << t;
            --take;
        }
    }
    return out;
}

}  // namespace vs
