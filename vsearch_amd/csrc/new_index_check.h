// new_index_check.h -- the host rules every call that returns a NEW index shares (vs_index_compact, vs_index_prune, vs_index_select_rows,
// vs_index_rescale, vs_index_combine, vs_index_concat): the spare capacity asked for, the 2^32 limits of the new index, the dtype predicates
// and the bytes a new index takes.  The call gives its noun ("compacted", "pruned", "selected", "rescaled", "combined", "joined").
// Plain C++ with no HIP in it, so that a stand-alone program can run them under a host sanitizer (the *_check_main.cpp programs do).
#pragma once

#include "set_check.h"

namespace vs {

inline bool store_dtype_ok(int dt) { return dt == VS_F32 || dt == VS_F16 || dt == VS_NONE; }     // what a CSR index can store
inline bool valued_dtype_ok(int dt) { return dt == VS_F32 || dt == VS_F16; }                     // what a call that computes values can write

inline int new_index_check_extra(int64_t rows_extra, int64_t packets_extra, char* msg, size_t cap) {
    if (rows_extra < 0 || packets_extra < 0) return snprintf(msg, cap, "rows_extra and packets_extra must be >= 0"), VS_EINVAL;
    return VS_OK;
}

// row and packet counts with their spare capacity fit 32 bits (the row pointers are uint32, and row 2^32 - 1 is no row).  `packets` is a 64-bit
// sum: a selection with repeats or a join can hold more packets than any source stores.  The extras are bounded first, so that no sum overflows
inline int new_index_check_capacity(const char* noun, int64_t rows, int64_t packets, int64_t rows_extra, int64_t packets_extra, char* msg, size_t cap) {
    if (rows_extra > (1ll << 32) || packets_extra > (1ll << 32) || packets < 0 || packets >= (1ll << 32) || rows + rows_extra >= (1ll << 32) - 1 ||
        packets + packets_extra >= (1ll << 32))
        return snprintf(msg, cap, "the %s index with its spare capacity exceeds 2^32 rows or packets", noun), VS_EUNSUPPORTED;
    return VS_OK;
}

// HBM of a CSR index of that capacity: 16 bytes of column ids and vb bytes of values a packet, a row pointer a row and one more
inline size_t new_index_bytes(int64_t rows, int64_t packets, size_t vb) { return (size_t)packets * (16 + vb) + (size_t)(rows + 1) * 4; }
inline size_t value_bytes(int store_dtype) { return store_dtype == VS_F32 ? 32 : (store_dtype == VS_F16 ? 16 : 0); }

}  // namespace vs
