"""ctypes binding of ``libvsearch_hip.so`` (C ABI: ``include/vsearch_hip.h``).

The product path has no CPU fallback: if the shared library is missing, or no HIP device is
visible, every compute entry point raises -- loudly -- instead of routing elsewhere.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvsearch_hip.so")
CSRC = os.path.join(_HERE, "csrc")

# error codes / dtypes (mirror include/vsearch_hip.h)
VS_OK, VS_EINVAL, VS_ERANGE, VS_ENOMEM, VS_EHIP, VS_EUNSUPPORTED, VS_ENODEVICE = 0, -1, -2, -3, -4, -5, -6
VS_F32, VS_F16, VS_I32, VS_I64, VS_U16, VS_U8, VS_NONE = 0, 1, 2, 3, 4, 5, -1
VS_KIND_DENSE, VS_KIND_CSR = 0, 1
# term filters (VS_TERM_FILTER_*): distinct terms a pass of the scan serves, terms a call takes, entries of a must / must_not / should list
TERM_FILTER_SLOTS, TERM_FILTER_TERMS, TERM_FILTER_LIST = 255, 4096, 64
# diversified search (VS_MMR_*): similarity modes, the deepest candidate list / most picks, the widest vocabulary of vs_mmr_select_csr
MMR_COSINE, MMR_DOT, MMR_MAX_DEPTH, MMR_MAX_COLS = 0, 1, 1024, 32768
# fused search (VS_FUSE_*): fusion modes, the most lists, the deepest list / most results, the most entries (L * kk) of vs_fuse_topk
FUSE_RRF, FUSE_SUM, FUSE_MNZ, FUSE_RAW, FUSE_MAX_LISTS, FUSE_MAX_DEPTH, FUSE_MAX_ENTRIES = 0, 1, 2, 3, 8, 1024, 4096
# range search (VS_RANGE_MAX_HITS): the most hits vs_index_search_range lists per query
RANGE_MAX_HITS = 2048
# boosted search (VS_BOOST_*): the modes, the most numeric fields of one vs_index_search_boosted call
BOOST_ADD, BOOST_MUL, BOOST_MAX_FIELDS = 0, 1, 4
# facet counts (VS_FACET_LDS_BINS, VS_FACET_MAX_TOPN): uint32 bins of a workgroup's LDS histograms, the most labels vs_facet_topn lists
FACET_LDS_BINS, FACET_MAX_TOPN = 16384, 1024
# term aggregations (VS_TERM_*): columns of a workgroup's LDS histogram, the most columns vs_term_topn lists, its scoring methods
TERM_LDS_COLS, TERM_MAX_TOPN, TERM_LIFT, TERM_JLH = 36864, 1024, 0, 1
# term sums (VS_TERM_FX_*, VS_TERM_SUM_TILE_COLS): a cell adds its value clamped to +-2^20 times 2^24; the columns of a workgroup's tile of 64-bit bins
TERM_FX_SHIFT, TERM_FX_CLAMP_LOG2, TERM_SUM_TILE_COLS = 24, 20, 18432
# clustering (VS_ASSIGN_MAX_K, VS_LABEL_MAX_VALUES): the most centroids of vs_index_assign, the most bitmaps of vs_label_bitmaps
ASSIGN_MAX_K, LABEL_MAX_VALUES = 4096, 4096
# per-label term aggregations (VS_LABEL_TERM_MAX_*): the most labels, the most cells (n_labels x ld), the most work items (max_items x tiles) of one call
LABEL_TERM_MAX_LABELS, LABEL_TERM_MAX_CELLS, LABEL_TERM_MAX_WORK_ITEMS = 65536, 1 << 27, 4194303
# numeric fields (VS_VAL_*, VS_VALUE_MAX_*): the value types, the most ranges of vs_value_range_bitmaps, edges of a histogram, rows of vs_value_topk
VAL_F32, VAL_I32, VALUE_MAX_RANGES, VALUE_MAX_EDGES, VALUE_MAX_TOPK = 0, 1, 4096, 1025, 1024
# percentiles (VS_VALUE_RADIX_*, VS_VALUE_MAX_RANKS, VS_QUANTILE_*): bins of a radix level, the levels, the most ranks of a call, the rank rules
VALUE_RADIX_BINS, VALUE_RADIX_LEVELS, VALUE_MAX_RANKS = 2048, 3, 16
QUANTILE_LOWER, QUANTILE_HIGHER, QUANTILE_NEAREST = 0, 1, 2
# breakdowns (VS_FACET_VALUE_*): (query, label) records of a workgroup's LDS in the stats kernel, n_labels x (n_edges + 2) cells a query at most
FACET_VALUE_LDS_RECORDS, FACET_VALUE_MAX_CELLS = 2048, 1 << 22
# per-label percentiles (VS_FACET_QUANTILE_MAX_LABEL_TILES): label tiles the LDS regime of the counting kernel takes at most
FACET_QUANTILE_MAX_LABEL_TILES = 16
# set egress (VS_SET_MAX_*): the most rows vs_set_sample lists per query, the most ids (B x limit) of one vs_set_ids call
SET_MAX_SAMPLE, SET_MAX_OUT_IDS = 1024, 1 << 27


class VsearchNativeError(RuntimeError):
    pass


class IndexInfo(C.Structure):
    _fields_ = [("kind", C.c_int32), ("store_dtype", C.c_int32), ("n_rows", C.c_int64), ("n_cols", C.c_int32),
                ("device", C.c_int32), ("nnz", C.c_int64), ("n_packets", C.c_int64), ("device_bytes", C.c_int64),
                ("bytes_per_pass", C.c_int64), ("lanes_per_row", C.c_int32), ("queries_per_pass", C.c_int32),
                ("last_scan_bytes", C.c_int64), ("aux_bytes", C.c_int64), ("last_path", C.c_int32), ("last_fallbacks", C.c_int32),
                ("last_walk_postings", C.c_int64), ("head_columns", C.c_int32), ("postings_state", C.c_int32),
                ("postings_walk", C.c_int32), ("last_packed_tiles", C.c_int32), ("n_live", C.c_int64)]


_vp, _i32, _i64, _int = C.c_void_p, C.c_int32, C.c_int64, C.c_int
_SIGNATURES = {
    "vs_version": ([], _int),
    "vs_last_error": ([], C.c_char_p),
    "vs_device_count": ([C.POINTER(_i32)], _int),
    "vs_index_create_csr": ([_vp, _int, _vp, _int, _vp, _int, _int, _i64, _i32, _int, C.POINTER(_vp)], _int),
    "vs_index_create_reserved": ([_i64, _i64, _i32, _int, _int, C.POINTER(_vp)], _int),
    "vs_index_append_csr": ([_vp, _vp, _int, _vp, _int, _vp, _int, _i64], _int),
    "vs_index_slice_rows": ([_vp, _i64, _i64, _int, C.POINTER(_vp)], _int),
    "vs_npz_inspect": ([C.c_char_p, _i32, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_index_append_npz": ([_vp, C.c_char_p, _i32], _int),
    "vs_index_save_npz": ([_vp, C.c_char_p, _int], _int),
    "vs_index_save_native": ([_vp, C.c_char_p], _int),
    "vs_index_load_native": ([C.c_char_p, _int, C.POINTER(_vp)], _int),
    "vs_index_create_dense": ([_vp, _int, _int, _i64, _i32, _i64, _int, C.POINTER(_vp)], _int),
    "vs_index_create_dense_auto": ([_vp, _int, _int, _i64, _i32, _i64, C.c_double, _int, C.POINTER(_vp)], _int),
    "vs_index_create_synthetic": ([C.c_uint64, _i64, _i64, _i32, _i32, _int, _int, _int, _int, C.POINTER(_vp)], _int),
    "vs_index_search": ([_vp, _vp, _int, _i64, _i32, _i32, _i64, _vp, _vp, _vp], _int),
    "vs_index_search_filtered": ([_vp, _vp, _int, _i64, _i32, _i32, _vp, _i64, _i64, _i64, _vp, _vp, _vp], _int),
    "vs_index_search_range": ([_vp, _vp, _int, _i64, _i32, _vp, _i32, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp], _int),
    "vs_index_last_range_plan": ([_vp, C.POINTER(_i32), C.POINTER(_i64)], _int),
    "vs_index_search_boosted": ([_vp, _vp, _int, _i64, _i32, _vp, _i32, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, C.POINTER(_vp),
                                 C.POINTER(_i32), _i32, _vp, _int, _vp], _int),
    "vs_facet_plan": ([_i64, _i32, _i32, _int, _i64, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_facet_counts": ([_vp, _i64, _i64, _vp, _i32, _vp, _i64, _i32, _i64, _vp, _i64, _vp, _vp, _int, _vp], _int),
    "vs_index_facet_counts": ([_vp, _vp, _i64, _i64, _i32, _vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp], _int),
    "vs_facet_topn": ([_vp, _i64, _i32, _i32, _i32, _i64, _vp, _vp, _int, _vp], _int),
    "vs_term_plan": ([_i64, _i32, _i32, _int, _i64, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_index_term_counts": ([_vp, _vp, _i64, _i64, _i32, _i64, _vp, _i64, _vp, _vp], _int),
    "vs_index_term_counts_ids": ([_vp, _vp, _i32, _i64, _i64, _i64, _int, _vp, _i64, _vp, _vp], _int),
    "vs_term_topn": ([_vp, _i64, _vp, _i32, _i32, _vp, _i64, _int, _i32, _i64, _vp, _vp, _vp, _vp, _int, _vp], _int),
    "vs_term_sum_plan": ([_i64, _i32, _i32, _int, _i64, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_index_term_sums": ([_vp, _vp, _i64, _i64, _i32, _i64, _i32, _vp, _i64, _vp, _vp], _int),
    "vs_index_term_sums_ids": ([_vp, _vp, _i32, _i64, _i64, _i64, _int, _i32, _vp, _i64, _vp, _vp], _int),
    "vs_term_sum_topn": ([_vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i64, _vp, _vp, _vp, _int, _vp], _int),
    "vs_assign_plan": ([_i64, _i32, _i32, _i64, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_centroid_half_norms": ([_vp, _i64, _i32, _i32, _int, _vp, _int, _vp], _int),
    "vs_index_assign": ([_vp, _vp, _i64, _i32, _vp, _vp, _i64, _i64, _vp, _vp, _vp], _int),
    "vs_label_bitmaps": ([_vp, _i64, _vp, _i32, _i64, _vp, _i64, _int, _vp], _int),
    "vs_label_term_plan": ([_i64, _i32, _i32, _i64, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_label_order": ([_vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp], _int),
    "vs_index_label_term_sums": ([_vp, _vp, _i64, _vp, _i32, _i64, _i32, _vp, _i64, _vp, _vp, _vp], _int),
    "vs_index_label_term_counts": ([_vp, _vp, _i64, _vp, _i32, _i64, _i32, _vp, _i64, _vp, _vp, _vp], _int),
    "vs_value_range_bitmaps": ([_vp, _int, _i64, _vp, _vp, _i32, _i64, _vp, _i64, _int, _vp], _int),
    "vs_value_plan": ([_i64, _i32, _i32, _int, _i64, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_value_stats": ([_vp, _i64, _i64, _vp, _i32, _vp, _int, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _int, _vp], _int),
    "vs_index_value_stats": ([_vp, _vp, _i64, _i64, _i32, _vp, _int, _i64, _vp, _vp, _vp, _vp, _vp, _vp], _int),
    "vs_value_histogram": ([_vp, _i64, _i64, _vp, _i32, _vp, _int, _i64, _vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp, _int, _vp], _int),
    "vs_index_value_histogram": ([_vp, _vp, _i64, _i64, _i32, _vp, _int, _vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp, _vp], _int),
    "vs_value_topk": ([_vp, _i64, _i64, _vp, _i32, _vp, _int, _i64, _i32, _int, _i64, _i64, _vp, _vp, _int, _vp], _int),
    "vs_index_value_topk": ([_vp, _vp, _i64, _i64, _i32, _vp, _int, _i32, _int, _i64, _i64, _vp, _vp, _vp], _int),
    "vs_value_quantile_plan": ([_i64, _i32, _i32, _int, _i64, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_value_quantiles": ([_vp, _i64, _i64, _vp, _i32, _vp, _int, _i64, _vp, _int, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _int, _vp], _int),
    "vs_index_value_quantiles": ([_vp, _vp, _i64, _i64, _i32, _vp, _int, _vp, _int, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp], _int),
    "vs_value_radix_counts": ([_vp, _i64, _i64, _vp, _i32, _vp, _int, _i64, _int, _i32, _vp, _vp, _i64, _vp, _vp, _int, _vp], _int),
    "vs_index_value_radix_counts": ([_vp, _vp, _i64, _i64, _i32, _vp, _int, _int, _i32, _vp, _vp, _i64, _vp, _vp, _vp], _int),
    "vs_value_radix_step": ([_int, _vp, _i32, _i32, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp], _int),
    "vs_facet_value_plan": ([_i64, _i32, _i32, _i32, _int, _i64, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_facet_value_stats": ([_vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _int, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _int, _vp], _int),
    "vs_index_facet_value_stats": ([_vp, _vp, _i64, _i64, _i32, _vp, _i32, _vp, _int, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp], _int),
    "vs_facet_value_histogram": ([_vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _int, _i64, _vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _int,
                                  _vp], _int),
    "vs_facet_value_quantile_plan": ([_i64, _i32, _i32, _i32, _int, _int, _i64, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32),
                                      C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_facet_value_quantiles": ([_vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _int, _i64, _vp, _int, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _int,
                                  _vp], _int),
    "vs_index_facet_value_quantiles": ([_vp, _vp, _i64, _i64, _i32, _vp, _i32, _vp, _int, _vp, _int, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
                                       _int),
    "vs_facet_value_radix_counts": ([_vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _int, _i64, _int, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _int, _vp],
                                    _int),
    "vs_index_facet_value_radix_counts": ([_vp, _vp, _i64, _i64, _i32, _vp, _i32, _vp, _int, _int, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp], _int),
    "vs_index_facet_value_histogram": ([_vp, _vp, _i64, _i64, _i32, _vp, _i32, _vp, _int, _vp, _i32, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
                                       _int),
    "vs_set_score_plan": ([_i64, _i32, _i32, _int, _i64, C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_index_set_scores": ([_vp, _vp, _int, _i64, _i32, _vp, _i64, _i64, _i64, _vp, _i64, _vp], _int),
    "vs_set_sample_hash": ([C.c_uint64, _i64], C.c_uint32),
    "vs_set_list_plan": ([_i64, _i32, _int, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)], _int),
    "vs_set_count": ([_vp, _i64, _i64, _vp, _i32, _i64, _i64, _vp, _int, _vp], _int),
    "vs_index_set_count": ([_vp, _vp, _i64, _i64, _i32, _i64, _vp, _vp], _int),
    "vs_set_ids": ([_vp, _i64, _i64, _vp, _i32, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _int, _vp], _int),
    "vs_index_set_ids": ([_vp, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _i64, _vp, _vp, _vp], _int),
    "vs_set_sample": ([_vp, _i64, _i64, _vp, _i32, _i64, _vp, _i32, _i64, _i64, _vp, _vp, _vp, _int, _vp], _int),
    "vs_index_set_sample": ([_vp, _vp, _i64, _i64, _i32, _vp, _i32, _i64, _i64, _vp, _vp, _vp, _vp], _int),
    "vs_set_from_ids": ([_vp, _i32, _i64, _i64, _i64, _i64, _int, _vp, _i64, _int, _vp], _int),
    "vs_filter_pack": ([_vp, _i32, _i64, _i64, _vp, _i64, _int, _vp], _int),
    "vs_index_scores": ([_vp, _vp, _int, _i64, _i32, _vp, _vp], _int),
    "vs_index_explain": ([_vp, _vp, _int, _i64, _i32, _vp, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp], _int),
    "vs_index_get_rows": ([_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp], _int),
    "vs_index_queries_from_rows": ([_vp, _vp, _i32, _i32, _i64, _vp, _i64, _vp, _int, _i64, C.c_float, _vp, _i64, _vp], _int),
    "vs_index_delete_rows": ([_vp, _vp, _i64, _i64, _vp], _int),
    "vs_index_restore_rows": ([_vp, _vp, _i64, _i64, _vp], _int),
    "vs_index_live_rows": ([_vp, C.POINTER(_i64)], _int),
    "vs_index_live_bitmap": ([_vp, _vp, _i64], _int),
    "vs_index_compact": ([_vp, _i64, _i64, _int, C.POINTER(_vp), _vp], _int),
    "vs_prune_plan": ([_i64, _i64, _i32, _int, _i32, _int, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i32)], _int),
    "vs_index_prune": ([_vp, _i32, C.c_float, _vp, _vp, _i64, _i64, _int, C.POINTER(_vp), _vp], _int),
    "vs_select_plan": ([_i64, C.POINTER(_i64)], _int),
    "vs_select_split": ([_vp, _i64, _vp, _i32, _vp], _int),
    "vs_index_select_rows": ([_vp, _vp, _i64, _i64, _i64, _i64, _int, C.POINTER(_vp)], _int),
    "vs_index_row_stats": ([_vp, _vp, _vp, _vp, _vp, _vp], _int),
    "vs_rescale_plan": ([_i64, _i64, _i32, _int, _int, _int, _int, C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i32)], _int),
    "vs_index_rescale": ([_vp, _vp, _vp, _int, _i64, _i64, _int, C.POINTER(_vp)], _int),
    "vs_combine_plan": ([_i64, _i64, _i64, _i32, _int, _int, _int, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i64)], _int),
    "vs_index_combine": ([_vp, _vp, C.c_float, C.c_float, _int, _i64, _i64, _int, C.POINTER(_vp)], _int),
    "vs_concat_plan": ([_i32, _vp, _vp, _i32, _vp, _int, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i32)], _int),
    "vs_index_concat": ([_vp, _i32, _int, _i64, _i64, _int, C.POINTER(_vp)], _int),
    "vs_index_term_bitmaps": ([_vp, _vp, _vp, _i32, _vp, _i64, _vp, _int, _vp], _int),
    "vs_term_filter_combine": ([_vp, _i64, _i64, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i64, _int, _vp], _int),
    "vs_index_prepare": ([_vp, _vp], _int),
    "vs_index_info": ([_vp, C.POINTER(IndexInfo)], _int),
    "vs_index_set_option": ([_vp, C.c_char_p, _int], _int),
    "vs_index_set_queries_per_pass": ([_vp, _int], _int),
    "vs_index_export_csr": ([_vp, _vp, _vp, _vp, _int], _int),
    "vs_index_export_dense": ([_vp, _vp, _int, _i64], _int),
    "vs_index_destroy": ([_vp], None),
    "vs_shard_group_create": ([C.POINTER(_vp), _i32, C.POINTER(_vp)], _int),
    "vs_shard_group_search": ([_vp, _vp, _int, _i64, _i32, _i32, _vp, _vp], _int),
    "vs_shard_group_search_filtered": ([_vp, _vp, _int, _i64, _i32, _i32, _vp, _i64, _vp, _vp], _int),
    "vs_shard_group_explain": ([_vp, _vp, _int, _i64, _i32, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp], _int),
    "vs_shard_group_get_rows": ([_vp, _vp, _i64, _vp, _vp, _vp], _int),
    "vs_shard_group_queries_from_rows": ([_vp, _vp, _i32, _i32, _i64, _vp, _i64, _vp, _int, _i64, C.c_float, _vp, _i64], _int),
    "vs_shard_group_delete_rows": ([_vp, _vp, _i64], _int),
    "vs_shard_group_restore_rows": ([_vp, _vp, _i64], _int),
    "vs_shard_group_term_bitmaps": ([_vp, _vp, _vp, _i32, _vp, _i64, _vp, _int], _int),
    "vs_shard_group_destroy": ([_vp], None),
    "vs_merge_topk": ([_vp, _vp, _i32, _i64, _i32, _vp, _vp, _int, _vp], _int),
    "vs_topk_exclude": ([_vp, _vp, _i32, _i32, _i64, _vp, _i32, _i64, _i32, _vp, _vp, _int, _vp], _int),
    "vs_topk_collapse": ([_vp, _vp, _i32, _i32, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _vp], _int),
    "vs_group_filter": ([_vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _int, _vp], _int),
    "vs_mmr_select_csr": ([_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i64, _i32, _vp, _i32, _int, _vp, _vp, _vp, _vp, _vp, _int, _vp], _int),
    "vs_fuse_topk": ([_vp, _vp, _i32, _i32, _i32, _i64, _i64, _vp, _i64, _vp, _i64, _int, C.c_float, _i32, _vp, _vp, _vp, _vp, _vp, _int, _vp], _int),
    "vs_topk_mask": ([_vp, _i32, _i32, _i64, _i32, _vp, _int, _vp], _int),
    "vs_bow_mask": ([_vp, _i32, _i32, _i32, _i32, _int, _vp, _int, _vp], _int),
    "vs_embed_mask": ([_vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _int, _int, _int, _vp], _int),
    "vs_dense_to_csr": ([_vp, _i32, _i32, _i64, _vp, _vp, _vp, _i64, _int, _vp], _int),
    "vs_embed_mask_to_csr": ([_vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _int, _vp, _vp, _vp, _i64, _int, _vp], _int),
    "vs_head_pool": ([_vp, _i32, _i32, _i32, _vp, _int, _vp], _int),
    "vs_head_project_pool": ([_vp, _vp, _i32, _i32, _i32, _i32, _vp, _int, _vp], _int),
    "vs_elu1p": ([_vp, _i64, _vp, _int, _vp], _int),
    "vs_head_pool_mean_topk": ([_vp, _i32, _i32, _i32, _i32, _vp, _int, _vp], _int),
    "vs_rerank_scores": ([_vp, _int, _i64, _i64, _i64, _vp, _i64, _i32, _i32, _i32, _vp, _int, _vp], _int),
    "vs_rerank_topk": ([_vp, _vp, _i32, _i32, _vp, _vp, _int, _vp], _int),
    "vs_bot_build": ([_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp], _int),
    "vs_profile_enable": ([_int], _int),
    "vs_profile_reset": ([], _int),
    "vs_profile_read": ([C.c_char_p, C.POINTER(C.c_double), C.POINTER(_i64)], _int),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def build(force: bool = False) -> str:
    """Compile libvsearch_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VsearchNativeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(or `make -C {CSRC}`). vsearch_amd has no CPU fallback.")
        # PyTorch-ROCm ships its own HIP/HSA runtime (torch/lib/libamdhip64.so, same SONAME as
        # /opt/rocm's).  Two runtimes in one process leave the second without devices, so torch's
        # must be loaded first; libvsearch_hip's DT_NEEDED libamdhip64.so.7 then binds to it.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        handle = C.CDLL(LIB_PATH)
        for name, (argtypes, restype) in _SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError if the ABI and the header drift apart
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = handle
    return _lib


def last_error() -> str:
    return lib().vs_last_error().decode("utf-8", "replace")


def check(rc: int):
    """Map VS_E* codes to the exception types the reference raises at the same points."""
    if rc == VS_OK:
        return
    msg = last_error()
    if rc == VS_ERANGE:
        raise RuntimeError(msg)                      # torch.topk: "selected index k out of range"
    if rc == VS_EINVAL:
        raise ValueError(msg)
    if rc == VS_ENOMEM:
        raise MemoryError(msg)
    if rc == VS_EUNSUPPORTED:
        raise NotImplementedError(msg)
    raise VsearchNativeError(f"libvsearch_hip error {rc}: {msg}")


def device_count() -> int:
    n = _i32(0)
    check(lib().vs_device_count(C.byref(n)))
    return n.value


def require_device():
    if device_count() <= 0:
        raise VsearchNativeError("no HIP device visible: vsearch_amd computes on MI355X only (no CPU fallback)")
