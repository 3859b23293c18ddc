// new_index.h -- what the calls that take stored indexes and return a NEW one share (vs_index_compact, vs_index_prune, vs_index_select_rows,
// vs_index_rescale, vs_index_combine, vs_index_concat): the small helpers of an entry point, the opening of a call, the new
// handle with its capacity and its out-of-memory sentence, its shape, its tombstones, the hand-over to the caller's GPU -- and the device code
// more than one of them runs.  An entry point is its own checks and plan, open_sources, its own kernels, set_csr_shape, hand_over.  The host
// rules are new_index_check.h.
#pragma once
#include "common.h"
#include "new_index_check.h"

#include <algorithm>

namespace vs {

// ---- the small helpers of an entry point ------------------------------------------------------------------------------------------------------
int need_device();                                                // VS_ENODEVICE without a visible GPU: the library has no CPU fallback
int device_in_range(int device);                                  // need_device, and "device %d out of range (have %d)"
inline int64_t bit_words(int64_t rows) { return (rows + 31) >> 5; }
inline unsigned grid_for(int64_t items, int per_block, int64_t cap) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, cap));
}
// a device pointer of the caller's belongs to the index's GPU (on_device: what is_device_ptr said of it)
int ptr_on(const void* p, bool on_device, int device, const char* what);
// a handle that is destroyed unless it is handed over
struct IndexGuard {
    vs_index* p;
    ~IndexGuard() { if (p) vs_index_destroy(p); }
};

// ---- the scaffold of a call ---------------------------------------------------------------------------------------------------------------------
// Makes the sources' GPU current and waits for it: deletions, ids and scales may still be enqueued on a caller's stream, and everything a call
// does below runs on the null stream.
int open_sources(int device_of_sources);
// A CSR handle with room for rows + rows_extra rows and packets + packets_extra packets on `device`, owned by *guard.  Out of memory is
// VS_ENOMEM "<verb> needs <bytes> bytes of HBM for the new index next to the <hint>": the hint names what the index stands next to and what
// the caller can drop.
int new_csr_index(const char* verb, const char* hint, int64_t rows, int64_t packets, int64_t rows_extra, int64_t packets_extra, int32_t n_cols, int dtype,
                  int device, IndexGuard* guard);
// The dense (matrix) kind: a handle of `rows` padded rows of src's shape on src's GPU, owned by *guard, its rows gathered from src: row j is
// src's row ids[j] - id_offset (device ids).
int new_dense_rows(const char* verb, const vs_index* src, const int64_t* ids, int64_t id_offset, int64_t rows, IndexGuard* guard);
void set_csr_shape(vs_index* idx, int64_t rows, int64_t packets, int64_t nnz, bool logical_dense);   // with lanes_per_row (pick_lanes)
int pick_lanes(int64_t n_packets, int64_t n_rows);                // lanes_per_row of a CSR index of that shape (csr_index.hip's rule)
int move_csr(const vs_index* a, int device, vs_index** out);      // a CSR index with its capacity, copied whole to another GPU (no tombstones)

// Tombstones a call's map kernel writes itself (live_words_from_ballot): the bitmap of the new handle with every row it can ever hold live
// (the layout of mutable.hip: whole 16-byte quads over max(rows_cap, rows) rows), and afterwards the dead count the kernel found at *d_dead --
// none: the bitmap is released, the handle is one without tombstones.
int alloc_live(vs_index* idx, int64_t rows);
int settle_dead(vs_index* idx, const unsigned long long* d_dead);

// where the tombstones of the handle a call hands over come from
struct TombFrom {
    enum Kind { kNone, kOwnBits, kSourceBits, kHostWords } kind;
    const vs_index* src;                                          // kSourceBits: rows are 1:1 with this source's
    const uint32_t* words;                                        // kHostWords: (rows + 31) / 32 live words
    static TombFrom none() { return TombFrom{kNone, nullptr, nullptr}; }
    static TombFrom own_bits() { return TombFrom{kOwnBits, nullptr, nullptr}; }                       // written into the new handle by the call
    static TombFrom source_bits(const vs_index* src) { return TombFrom{kSourceBits, src, nullptr}; }
    static TombFrom host_words(const uint32_t* words) { return TombFrom{words ? kHostWords : kNone, nullptr, words}; }
};
// The tail of a call: waits for the GPU; a result that belongs on another GPU moves there (move_csr) and the copy on the sources' GPU is
// dropped; the tombstones follow -- the handle's own bits with the move, a source's bits or host words after it --; *out takes the handle.
int hand_over(IndexGuard& guard, int src_device, int device, const TombFrom& tomb, vs_index** out);

// ---- kernels more than one call runs (new_index.hip; all on the null stream) ------------------------------------------------------------------------
// *d_nnz += the non-zeros of rows [0, rows) of idx's packets (pads sit at the tail of a row's last packet only)
int launch_nnz_recount(const vs_index* idx, int64_t rows, unsigned long long* d_nnz);
// Row pointers from per-row cell counts (prune: kept cells, combine: union cells; bit 31 of a count is the caller's own flag and is not
// counted).  cells_scan: the block sums (d_sums: [scan_blocks + 1] pairs), *d_nnz += the cells, *packets = the new packets; cells_row_pointers:
// new_pk[r] = packets of the rows before r, new_pk[n_rows] = packets.
int cells_scan(const int32_t* d_cells, int64_t n_rows, int64_t scan_blocks, uint2* d_sums, unsigned long long* d_nnz, int64_t* packets);
int cells_row_pointers(const int32_t* d_cells, int64_t n_rows, int64_t scan_blocks, const uint2* d_sums, int64_t packets, uint32_t* new_pk);
// select.hip: the packet gather (four 64-packet steps in flight): new row j takes the packets of src's row ids[j] - id_offset (device ids);
// new_pk: the new row pointers.  vs_index_select_rows over the caller's ids, vs_index_compact over the live rows
int launch_packet_gather(const vs_index* src, const int64_t* d_ids, int64_t id_offset, const uint32_t* new_pk, int64_t n_new, uint4* dst_cols, uint4* dst_vals);

// ---- device code --------------------------------------------------------------------------------------------------------------------------------
// The live words of 64 new rows from a wave: lane l speaks for new row `pos` (pos - l is a multiple of 64).  Two whole words of the new bitmap,
// written from a ballot with plain stores -- bits past the last new row n stay set: rows still to be appended are live --; *dead counts the
// cleared ones.
__device__ __forceinline__ void live_words_from_ballot(bool is_dead, int64_t pos, int64_t n, uint32_t* new_live, unsigned long long* dead) {
    const int lane = threadIdx.x & 63;
    const unsigned long long dead_bits = __ballot(is_dead);
    const int64_t w0 = pos - lane;
    if (lane == 0 && w0 < n) new_live[w0 >> 5] = ~(uint32_t)dead_bits;
    if (lane == 32 && w0 + 32 < n) new_live[(w0 >> 5) + 1] = ~(uint32_t)(dead_bits >> 32);
    if (lane == 0 && dead_bits) atomicAdd(dead, (unsigned long long)__popcll(dead_bits));
}

}  // namespace vs
