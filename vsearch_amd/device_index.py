"""Thin object wrapper over the ``vs_index`` handle of libvsearch_hip.so.

numpy arrays are passed as host pointers, torch CUDA tensors as device pointers (the library
detects which); results come back in the same kind as the query (numpy in -> numpy out, torch
in -> torch tensors on the index device, on torch's current stream).
"""
from __future__ import annotations

import ctypes as C
from typing import Any, NamedTuple

import numpy as np

from . import _native as nat

_NP2VS = {np.dtype(np.float32): nat.VS_F32, np.dtype(np.float16): nat.VS_F16,
          np.dtype(np.int32): nat.VS_I32, np.dtype(np.int64): nat.VS_I64}


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _torch_vs_dtype(t):
    import torch
    return {torch.float32: nat.VS_F32, torch.float16: nat.VS_F16, torch.int32: nat.VS_I32, torch.int64: nat.VS_I64}[t.dtype]


def as_arg(x, allowed=None):
    """-> (pointer, vs dtype, keep-alive object). Accepts numpy arrays and torch tensors (CPU or CUDA)."""
    if x is None:
        return None, nat.VS_NONE, None
    if _is_torch(x):
        t = x.detach()
        if not t.is_contiguous():
            t = t.contiguous()
        dt = _torch_vs_dtype(t)
        if allowed and dt not in allowed:
            raise TypeError(f"unsupported dtype {t.dtype}")
        return C.c_void_p(t.data_ptr()), dt, t
    a = np.ascontiguousarray(x)
    if a.dtype not in _NP2VS:
        raise TypeError(f"unsupported dtype {a.dtype}")
    dt = _NP2VS[a.dtype]
    if allowed and dt not in allowed:
        raise TypeError(f"unsupported dtype {a.dtype}")
    return C.c_void_p(a.ctypes.data), dt, a


def current_stream(device: int):
    """hipStream_t of torch's current stream on `device` (None when torch has no CUDA/HIP device)."""
    try:
        import torch
        if torch.cuda.is_available():
            # the null stream is passed as hipStreamLegacy ((hipStream_t)1): same stream, but not "no stream given" (which blocks)
            return C.c_void_p(torch.cuda.current_stream(device).cuda_stream or 1)
    except Exception:
        pass
    return None


def npz_inspect(path: str, shift: int = 0):
    """(n_rows, n_cols after the shift, nnz after the shift, 8-nnz packets) of a scipy.sparse.save_npz CSR shard; no GPU needed."""
    n_rows, n_cols, nnz, packets = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_npz_inspect(str(path).encode(), int(shift), C.byref(n_rows), C.byref(n_cols), C.byref(nnz), C.byref(packets)))
    return n_rows.value, n_cols.value, nnz.value, packets.value


class Explanation(NamedTuple):
    """Per (query, document) pair: the top contributing columns, their contributions q[c] * v (largest first, then column ascending;
    -1 / 0 in unused slots), the pair's score and its number of matched terms (-1: the id is not a row of this index)."""
    cols: Any          # int32 [B, k, topn]
    contrib: Any       # float32 [B, k, topn]
    scores: Any        # float32 [B, k]
    n_matched: Any     # int32 [B, k]


MAX_EXPLAIN_TOPN = 1024


def _explain_args(q, ids, topn):
    """Argument checks of explain() that need no device -> (B, k, topn, on_device)"""
    if isinstance(topn, bool) or not isinstance(topn, (int, np.integer)):
        raise TypeError(f"topn must be an int, got {type(topn).__name__}")
    topn = int(topn)
    if not 0 <= topn <= MAX_EXPLAIN_TOPN:
        raise ValueError(f"topn must be in 0..{MAX_EXPLAIN_TOPN}, got {topn}")
    if not hasattr(ids, "ndim") or ids.ndim != 2:
        raise ValueError("ids must be a [B, k] array of document ids")
    if _is_torch(ids):
        import torch
        if ids.dtype != torch.int64:
            raise TypeError(f"ids must be int64, got {ids.dtype}")
    elif np.asarray(ids).dtype != np.int64:
        raise TypeError(f"ids must be int64, got {np.asarray(ids).dtype}")
    ids_dev = _is_torch(ids) and ids.is_cuda
    if q is not None:
        if q.ndim != 2:
            raise ValueError("queries must be [B, V]")
        if int(q.shape[0]) != int(ids.shape[0]):
            raise ValueError(f"{int(q.shape[0])} queries but ids has {int(ids.shape[0])} rows")
        q_dev = _is_torch(q) and q.is_cuda
        if q_dev != ids_dev or (q_dev and q.device != ids.device):
            raise ValueError("queries and ids must live on the same device (both host, or both on the index's GPU)")
    return int(ids.shape[0]), int(ids.shape[1]), topn, ids_dev


def _explain_outputs(B, k, topn, device):
    """(numpy | torch on `device`) output arrays of explain() and their pointers"""
    if device is not None:
        import torch
        dev = torch.device("cuda", device)
        out = (torch.full((B, k, topn), -1, dtype=torch.int32, device=dev), torch.zeros((B, k, topn), dtype=torch.float32, device=dev),
               torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int32, device=dev))
        ptrs = [C.c_void_p(t.data_ptr()) if t.numel() else None for t in out]
    else:
        out = (np.full((B, k, topn), -1, dtype=np.int32), np.zeros((B, k, topn), dtype=np.float32),
               np.empty((B, k), dtype=np.float32), np.empty((B, k), dtype=np.int32))
        ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in out]
    return out, ptrs


def _int64_ids(ids, ndim, name="ids"):
    """checks of an id array: int64, `ndim` dimensions -> on_device"""
    if not hasattr(ids, "ndim") or ids.ndim != ndim:
        raise ValueError(f"{name} must be a {'[n]' if ndim == 1 else '[B, m]'} array of document ids")
    if _is_torch(ids):
        import torch
        if ids.dtype != torch.int64:
            raise TypeError(f"{name} must be int64, got {ids.dtype}")
    elif np.asarray(ids).dtype != np.int64:
        raise TypeError(f"{name} must be int64, got {np.asarray(ids).dtype}")
    return _is_torch(ids) and ids.is_cuda


def _row_ids(ids, name="ids"):
    """An id list of delete_rows / restore_rows -> (int64 1-D numpy array | CUDA tensor, on_device).  Lists, tuples and integer arrays of any
    width are taken; anything that is not integer is a TypeError, more than one dimension a ValueError (checked before the library is reached)."""
    if _is_torch(ids):
        import torch
        if ids.dtype in (torch.bool,) or ids.is_floating_point() or ids.is_complex():
            raise TypeError(f"{name} must be integer document ids, got {ids.dtype}")
        if ids.ndim != 1:
            raise ValueError(f"{name} must be a 1-D list of document ids, got {ids.ndim} dimensions")
        if ids.is_cuda:
            return ids.to(torch.int64).contiguous(), True
        ids = ids.numpy()
    a = np.asarray(ids)
    if a.size == 0 and a.ndim == 1:
        return np.zeros(0, dtype=np.int64), False
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name} must be integer document ids, got {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"{name} must be a 1-D list of document ids, got {a.ndim} dimensions")
    return np.ascontiguousarray(a, dtype=np.int64), False


def _compact_args(rows_extra, packets_extra):
    for name, v in (("rows_extra", rows_extra), ("packets_extra", packets_extra)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
        if v < 0:
            raise ValueError(f"{name} must be >= 0, got {v}")
    return int(rows_extra), int(packets_extra)


def _new_index_call(fn, args, sources):
    """One call of the library that returns a new index next to its sources (compact, prune, select_rows, rescale, combine, concat).  If HBM
    cannot hold them all, the postings copy of every distinct source that has one is dropped (prepare() rebuilds it) and the call retried
    once; with no copy to drop the MemoryError stands."""
    try:
        nat.check(fn(*args))
    except MemoryError:
        holders = [x for x in {id(x): x for x in sources}.values() if x.info().aux_bytes]
        if not holders:
            raise
        for x in holders:
            x.set_option("blocked_postings", 0)                # releases the copy; back to auto for the next prepare()
            x.set_option("blocked_postings", -1)
        nat.check(fn(*args))


def _prune_args(topk, min_value):
    """The cut rules of prune() -> (topk for the library: 0 = no cut, min_value: NaN = none); checked before the library is reached."""
    if topk is None:
        topk = 0
    if isinstance(topk, bool) or not isinstance(topk, (int, np.integer)):
        raise TypeError(f"topk must be an int or None, got {type(topk).__name__}")
    if topk < 0 or topk > 65535:
        raise ValueError(f"topk must be in 0..65535 (0 / None: no cut), got {topk}")
    if min_value is None:
        return int(topk), float("nan")
    if isinstance(min_value, bool) or not isinstance(min_value, (int, float, np.integer, np.floating)):
        raise TypeError(f"min_value must be a number or None, got {type(min_value).__name__}")
    if np.isnan(min_value):
        raise ValueError("min_value must not be NaN (None: no threshold)")
    return int(topk), float(np.float32(min_value))


def _col_mask(cols, n_cols, name):
    """column ids (integers, 1-D) or a bool mask [n_cols] -> bool numpy [n_cols]"""
    if _is_torch(cols):
        cols = cols.detach().cpu().numpy()
    a = np.asarray(cols)
    if a.dtype == np.bool_:
        if a.shape != (n_cols,):
            raise ValueError(f"a bool {name} mask must have shape ({n_cols},), got {a.shape}")
        return a.copy()
    if a.size == 0:
        return np.zeros(n_cols, dtype=bool)
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name} must be integer column ids or a bool mask, got {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"{name} must be a 1-D list of column ids, got {a.ndim} dimensions")
    if a.min() < 0 or a.max() >= n_cols:
        raise ValueError(f"{name} holds a column outside [0, {n_cols})")
    m = np.zeros(n_cols, dtype=bool)
    m[a] = True
    return m


def _col_keep_words(n_cols, keep_cols=None, drop_cols=None):
    """col_keep of vs_index_prune: uint32 words, bit c = column c may stay (keep_cols minus drop_cols) -- None when every column stays"""
    if keep_cols is None and drop_cols is None:
        return None
    m = np.ones(n_cols, dtype=bool) if keep_cols is None else _col_mask(keep_cols, n_cols, "keep_cols")
    if drop_cols is not None:
        m &= ~_col_mask(drop_cols, n_cols, "drop_cols")
    bits = np.zeros(((n_cols + 31) // 32) * 32, dtype=np.uint8)
    bits[:n_cols] = m
    return np.ascontiguousarray(np.packbits(bits, bitorder="little").view(np.uint32))


def prune_plan(n_rows, n_packets, n_cols, store_dtype, topk=0, has_protect=False):
    """vs_prune_plan (pure host arithmetic) -> (reg_cells, scratch_bytes, lds_bytes)"""
    reg, scratch, lds = C.c_int32(0), C.c_int64(0), C.c_int32(0)
    nat.check(nat.lib().vs_prune_plan(int(n_rows), int(n_packets), int(n_cols), int(store_dtype), int(topk), 1 if has_protect else 0, C.byref(reg),
                                      C.byref(scratch), C.byref(lds)))
    return reg.value, scratch.value, lds.value


def select_plan(n):
    """vs_select_plan (pure host arithmetic) -> scratch_bytes: what select_rows() of n ids allocates next to both indexes"""
    scratch = C.c_int64(0)
    nat.check(nat.lib().vs_select_plan(int(n), C.byref(scratch)))
    return scratch.value


class RowStats(NamedTuple):
    """row_stats(): per stored row -- cells int32 (stored cells), nonzero int32 (cells with a non-zero value), l1 float64 (sum of |w|), sumsq
    float64 (sum of w * w, each product exact), max float32 (largest value; NaN = no value).  The sums are fp64 sums in the pinned order of
    the exact scores; no square root is taken."""
    cells: Any
    nonzero: Any
    l1: Any
    sumsq: Any
    max: Any


_STORE_DTYPES = {"fp32": nat.VS_F32, "float32": nat.VS_F32, "fp16": nat.VS_F16, "float16": nat.VS_F16, nat.VS_F32: nat.VS_F32, nat.VS_F16: nat.VS_F16}
COL_SCALE_ROUTES = ("none", "lds", "memory")         # vs_rescale_plan's out_col_route


def _rescale_dtype(dtype, src_dtype):
    """out_dtype of rescale(): None keeps a valued source's dtype; a binary source then has none to keep (ValueError)"""
    if dtype is None:
        if src_dtype == nat.VS_NONE:
            raise ValueError("a binary index has no value dtype to keep: pass dtype='fp32' or 'fp16'")
        return int(src_dtype)
    if isinstance(dtype, (type, np.dtype)):
        dtype = np.dtype(dtype).name
    elif str(dtype) in ("torch.float32", "torch.float16"):
        dtype = str(dtype)[6:]
    if isinstance(dtype, bool) or dtype not in _STORE_DTYPES:
        raise ValueError(f"dtype must be 'fp32' or 'fp16' (binarising an index is not covered), got {dtype!r}")
    return _STORE_DTYPES[dtype]


def _scale_arg(x, n, name, device):
    """A scale of rescale() -> (float32 contiguous numpy array | CUDA tensor on `device`, pointer) or (None, None); the length is checked before
    the library is reached"""
    if x is None:
        return None, None
    if _is_torch(x):
        import torch
        if x.dtype == torch.bool or x.is_complex():
            raise TypeError(f"{name} must be numbers, got {x.dtype}")
        if x.ndim != 1 or int(x.shape[0]) != n:
            raise ValueError(f"{name} must have shape ({n},), got {tuple(x.shape)}")
        if x.is_cuda:
            x = x.detach().to(device=f"cuda:{device}", dtype=torch.float32).contiguous()
            return x, C.c_void_p(x.data_ptr()) if n else None
        x = x.detach().numpy()
    a = np.asarray(x)
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise TypeError(f"{name} must be numbers, got {a.dtype}")
    if a.shape != (n,):
        raise ValueError(f"{name} must have shape ({n},), got {a.shape}")
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, C.c_void_p(a.ctypes.data) if n else None


def rescale_plan(n_rows, n_packets, n_cols, src_dtype, out_dtype, has_row_scale=False, has_col_scale=False):
    """vs_rescale_plan (pure host arithmetic) -> (scratch_bytes, lds_bytes, col_route: "none" | "lds" | "memory")"""
    scratch, lds, route = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    nat.check(nat.lib().vs_rescale_plan(int(n_rows), int(n_packets), int(n_cols), int(src_dtype), int(out_dtype), 1 if has_row_scale else 0,
                                        1 if has_col_scale else 0, C.byref(scratch), C.byref(lds), C.byref(route)))
    return scratch.value, lds.value, COL_SCALE_ROUTES[route.value]


class CombinePlan(NamedTuple):
    """combine_plan(): wave_cells -- rows whose stored cells on both sides together are at most this many are filled a wave a row --,
    group_cells -- the largest union a longer row, filled by a workgroup, may have --, the LDS bytes of a fill workgroup of either route, and
    the scratch bytes the call allocates next to the three indexes."""
    wave_cells: int
    group_cells: int
    wave_lds_bytes: int
    group_lds_bytes: int
    scratch_bytes: int


def combine_plan(n_rows, packets_a, packets_b, n_cols, dtype_a, dtype_b, out_dtype):
    """vs_combine_plan (pure host arithmetic) -> CombinePlan"""
    wc, gc, wl, gl, scratch = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
    nat.check(nat.lib().vs_combine_plan(int(n_rows), int(packets_a), int(packets_b), int(n_cols), int(dtype_a), int(dtype_b), int(out_dtype),
                                        C.byref(wc), C.byref(gc), C.byref(wl), C.byref(gl), C.byref(scratch)))
    return CombinePlan(wc.value, gc.value, wl.value, gl.value, scratch.value)


def _combine_dtype(dtype, dtype_a, dtype_b):
    """out_dtype of combine(): None gives fp32, unless both sources are fp16"""
    if dtype is None:
        return nat.VS_F16 if dtype_a == nat.VS_F16 and dtype_b == nat.VS_F16 else nat.VS_F32
    return _rescale_dtype(dtype, nat.VS_F32)


def _combine_weight(w, name):
    """A weight of combine() -> float (rounded to float32 by the call); anything that is not a real number is a TypeError"""
    if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)):
        raise TypeError(f"{name} must be a number, got {type(w).__name__}")
    with np.errstate(over="ignore"):
        return float(np.float32(w))


class ConcatPlan(NamedTuple):
    """concat_plan(): the rows and the packets of the joined index, the scratch bytes the call allocates next to the indexes (the source
    table and the counters) and the LDS bytes of a workgroup (the table's image)."""
    rows: int
    packets: int
    scratch_bytes: int
    lds_bytes: int


CONCAT_MAX_SOURCES = 256                             # kConcatMaxSources


def concat_plan(rows, packets, n_cols, dtypes, out_dtype) -> ConcatPlan:
    """vs_concat_plan (pure host arithmetic) -> ConcatPlan.  rows, packets, dtypes: one entry a source (dtypes: VS_F32 | VS_F16 | VS_NONE);
    out_dtype: VS_F32 | VS_F16, or VS_NONE when every source is binary."""
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    packets = np.ascontiguousarray(packets, dtype=np.int64)
    dtypes = np.ascontiguousarray(dtypes, dtype=np.int32)
    if rows.ndim != 1 or packets.shape != rows.shape or dtypes.shape != rows.shape:
        raise ValueError("rows, packets and dtypes must be 1-D with one entry a source")
    r, k, scratch, lds = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
    nat.check(nat.lib().vs_concat_plan(int(rows.size), ptr(rows), ptr(packets), int(n_cols), ptr(dtypes), int(out_dtype), C.byref(r), C.byref(k),
                                       C.byref(scratch), C.byref(lds)))
    return ConcatPlan(r.value, k.value, scratch.value, lds.value)


def _concat_dtype(dtype, src_dtypes):
    """out_dtype of concat(): None gives binary if every source is binary, fp16 if every valued source stores fp16, else fp32"""
    if dtype is None:
        valued = [d for d in src_dtypes if d != nat.VS_NONE]
        if not valued:
            return nat.VS_NONE
        return nat.VS_F16 if all(d == nat.VS_F16 for d in valued) else nat.VS_F32
    if dtype in ("binary", nat.VS_NONE) and not isinstance(dtype, bool):
        if any(d != nat.VS_NONE for d in src_dtypes):
            raise ValueError("dtype 'binary' with a valued source: binarising an index is not covered ('fp32' or 'fp16')")
        return nat.VS_NONE
    return _rescale_dtype(dtype, nat.VS_F32)


def _concat_sources(first, others, cls):
    """[first] + others as a list of `cls`; others: one index or a sequence of them.  More than CONCAT_MAX_SOURCES raise ValueError"""
    others = [others] if isinstance(others, cls) else list(others)
    for o in others:
        if not isinstance(o, cls):
            raise TypeError(f"others must be {cls.__name__}s, got {type(o).__name__}")
    if 1 + len(others) > CONCAT_MAX_SOURCES:
        raise ValueError(f"a join takes at most {CONCAT_MAX_SOURCES} sources, got {1 + len(others)} (join in stages)")
    return [first] + others


def _select_ids(ids):
    """The id list of select_rows() -> (int64 1-D numpy array | CUDA tensor, on_device); an empty list is a ValueError (checked before the
    library is reached)."""
    ids, on_dev = _row_ids(ids)
    if int(ids.shape[0]) == 0:
        raise ValueError("empty selection: select_rows() needs at least one id")
    return ids, on_dev


def split_by_shard(ids, cuts):
    """vs_select_split (pure host arithmetic): global ids dealt to the shards whose rows are [cuts[s], cuts[s + 1]), IN THE ORDER GIVEN ->
    begin int64 [n_shards + 1]: ids[begin[s]:begin[s + 1]] are shard s's.  A list that goes back to an earlier shard raises ValueError."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    cuts = np.ascontiguousarray(cuts, dtype=np.int64)
    if ids.ndim != 1 or cuts.ndim != 1 or cuts.size < 2:
        raise ValueError("ids must be 1-D, cuts 1-D with one entry more than there are shards")
    begin = np.zeros(cuts.size, dtype=np.int64)
    nat.check(nat.lib().vs_select_split(C.c_void_p(ids.ctypes.data) if ids.size else None, int(ids.size), C.c_void_p(cuts.ctypes.data), int(cuts.size) - 1,
                                        C.c_void_p(begin.ctypes.data)))
    return begin


def _split_on_device(ids, cuts):
    """split_by_shard for ids that live on a GPU: the same rule with torch on that GPU -- only the per-shard counts come to the host"""
    import torch
    edges = torch.tensor(cuts, dtype=torch.int64, device=ids.device)
    if int(ids.min()) < 0 or int(ids.max()) >= int(cuts[-1]):
        raise ValueError(f"the selection holds a document id outside [0, {int(cuts[-1])})")
    shard = torch.bucketize(ids, edges[1:], right=True)           # the shard of every id: the first whose end lies beyond it
    if bool((shard[1:] < shard[:-1]).any()):
        raise ValueError("the selection goes back to an earlier shard: a selection cannot move rows across shards")
    counts = torch.bincount(shard, minlength=len(cuts) - 1).cpu().numpy()
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _by_example_args(ids, weights=None, q=None, k=None, a=None):
    """Argument checks of queries_from_rows() / search_by_example() that need no device -> (B, m, on_device)"""
    on_dev = _int64_ids(ids, 2)
    B, m = int(ids.shape[0]), int(ids.shape[1])
    if m < 1:
        raise ValueError("ids must hold at least one example id per query (m >= 1)")
    for name, x in (("weights", weights), ("q", q)):
        if x is None:
            continue
        if not hasattr(x, "ndim") or x.ndim != 2:
            raise ValueError(f"{name} must be a 2-D array")
        if int(x.shape[0]) != B or (name == "weights" and int(x.shape[1]) != m):
            raise ValueError(f"{name} has shape {tuple(x.shape)}, ids {tuple(ids.shape)}")
        x_dev = _is_torch(x) and x.is_cuda
        if x_dev != on_dev or (x_dev and x.device != ids.device):
            raise ValueError(f"{name} and ids must live on the same device (both host, or both on the index's GPU)")
    _k_a_args(k, a)
    return B, m, on_dev


def _k_a_args(k=None, a=None):
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"k must be an int, got {type(k).__name__}")
        if k < 1:
            raise ValueError(f"k must be >= 1, got {k}")
    if a is not None:
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)):
            raise TypeError(f"a must be an int, got {type(a).__name__}")
        if a < 1:
            raise ValueError(f"a must be in 1..V, got {a}")


def _check_a(a, V):
    if a is not None and not 1 <= int(a) <= V:
        raise ValueError(f"a must be in 1..{V}, got {a}")


def resparsify(q, a: int, device: int):
    """Keep the `a` largest entries of every row of fp32 queries q [B, V] (vs_topk_mask: ties at the a-th value go to the lower column,
    as build_topk_mask), zeros elsewhere.  numpy in -> numpy out; torch CUDA in -> a new tensor on torch's current stream."""
    B, V = int(q.shape[0]), int(q.shape[1])
    _check_a(a, V)
    if _is_torch(q) and q.is_cuda:
        import torch
        x = q.contiguous()
        mask = torch.empty((B, V), dtype=torch.uint8, device=x.device)
        nat.check(nat.lib().vs_topk_mask(C.c_void_p(x.data_ptr()), B, V, V, int(a), C.c_void_p(mask.data_ptr()), int(device),
                                         current_stream(int(device))))
        return x.masked_fill(mask == 0, 0.0)
    x = np.ascontiguousarray(q, dtype=np.float32)
    mask = np.empty((B, V), dtype=np.uint8)
    nat.check(nat.lib().vs_topk_mask(C.c_void_p(x.ctypes.data), B, V, V, int(a), C.c_void_p(mask.ctypes.data), int(device), None))
    return np.where(mask != 0, x, np.float32(0))


def topk_exclude(ids, scores, excl, k: int, device: int = 0):
    """Per query b: the top list ids / scores [B, kk] (canonical order) without the ids excl[b] ([B, m]; -1 is no id) -> the first k
    survivors [B, k], padded with id -1 / score -inf (vs_topk_exclude).  numpy in -> numpy out; torch CUDA in -> torch's current stream."""
    nat.require_device()
    B, kk, m = int(ids.shape[0]), int(ids.shape[1]), int(excl.shape[1])
    p_i, _, k1 = as_arg(ids, (nat.VS_I64,))
    p_s, _, k2 = as_arg(scores, (nat.VS_F32,))
    p_e, _, k3 = as_arg(excl, (nat.VS_I64,))
    if _is_torch(ids) and ids.is_cuda:
        import torch
        out_i = torch.empty((B, k), dtype=torch.int64, device=ids.device)
        out_s = torch.empty((B, k), dtype=torch.float32, device=ids.device)
        nat.check(nat.lib().vs_topk_exclude(p_i, p_s, B, kk, kk, p_e, m, m, int(k), C.c_void_p(out_i.data_ptr()), C.c_void_p(out_s.data_ptr()),
                                            int(device), current_stream(int(device))))
        return out_i, out_s
    out_i = np.empty((B, k), dtype=np.int64)
    out_s = np.empty((B, k), dtype=np.float32)
    nat.check(nat.lib().vs_topk_exclude(p_i, p_s, B, kk, kk, p_e, m, m, int(k), C.c_void_p(out_i.ctypes.data), C.c_void_p(out_s.ctypes.data),
                                        int(device), None))
    if _is_torch(ids):
        import torch
        return torch.from_numpy(out_i), torch.from_numpy(out_s)
    return out_i, out_s


def _search_by_example(obj, ids, k, weights, q, alpha, a, exclude, filter):
    """queries_from_rows -> optional top-`a` re-sparsify -> search of k + m (or k) -> exclusion of the example ids"""
    B, m, on_dev = _by_example_args(ids, weights, q, k, a)
    nat.require_device()
    device = obj.device
    qq = obj.queries_from_rows(ids, weights=weights, q=q, alpha=alpha)
    if a is not None:
        qq = resparsify(qq, a, device)
    k = int(k)
    if not exclude:
        return obj.search(qq, k, filter=filter)
    n = obj.n_rows
    kk = min(k + m, n) if k <= n else k                                 # (k > n: the search raises as it does for any query)
    out_ids, out_sc = obj.search(qq, kk, filter=filter)
    if _is_torch(ids) and not on_dev:
        ids = ids.numpy()
    return topk_exclude(out_ids, out_sc, ids, k, device)


class GroupedResults(NamedTuple):
    """Per query: the top k groups in the order of their best rows (-1 in unused slots), and each group's best `per_group` rows in rank
    order with their scores (id -1 / score -inf in unused slots)."""
    groups: Any        # int32 [B, k]
    ids: Any           # int64 [B, k, per_group]
    scores: Any        # float32 [B, k, per_group]


MAX_GROUPS_K, MAX_PER_GROUP, MAX_GROUP_ROWS, MAX_COLLAPSE_KK = 1024, 64, 8192, 16384


def _grouped_args(k, per_group, depth=None):
    """Argument checks of search_grouped() that need no device -> (k, per_group, depth or None)"""
    for name, v in (("k", k), ("per_group", per_group)) + ((("depth", depth),) if depth is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
        if v < 1:
            raise ValueError(f"{name} must be >= 1, got {v}")
    k, m = int(k), int(per_group)
    if k > MAX_GROUPS_K:
        raise ValueError(f"k must be at most {MAX_GROUPS_K} groups, got {k}")
    if m > MAX_PER_GROUP:
        raise ValueError(f"per_group must be at most {MAX_PER_GROUP}, got {m}")
    if k * m > MAX_GROUP_ROWS:
        raise ValueError(f"k * per_group must be at most {MAX_GROUP_ROWS}, got {k} x {m}")
    return k, m, (None if depth is None else int(depth))


class GroupState:
    """The state of a grouped walk for B queries (what vs_topk_collapse keeps in its output buffers) as numpy arrays or as torch tensors on
    GPU `device`: group [B, k], count [B, k], ids [B, k, m], scores [B, k, m], status [B], incomplete [1]."""

    def __init__(self, B, k, m, device=None):
        self.B, self.k, self.m, self.device = int(B), int(k), int(m), device
        if device is not None:
            import torch
            dev = torch.device("cuda", device)
            self.group = torch.empty((B, k), dtype=torch.int32, device=dev)
            self.count = torch.empty((B, k), dtype=torch.int32, device=dev)
            self.ids = torch.empty((B, k, m), dtype=torch.int64, device=dev)
            self.scores = torch.empty((B, k, m), dtype=torch.float32, device=dev)
            self.status = torch.zeros(B, dtype=torch.int32, device=dev)
            self.incomplete = torch.zeros(1, dtype=torch.int32, device=dev)
        else:
            self.group = np.full((B, k), -1, dtype=np.int32)
            self.count = np.zeros((B, k), dtype=np.int32)
            self.ids = np.full((B, k, m), -1, dtype=np.int64)
            self.scores = np.full((B, k, m), -np.inf, dtype=np.float32)
            self.status = np.zeros(B, dtype=np.int32)
            self.incomplete = np.zeros(1, dtype=np.int32)


def _ptr(x, offset_bytes=0):
    if x is None:
        return None
    return C.c_void_p((x.data_ptr() if _is_torch(x) else x.ctypes.data) + offset_bytes)


def topk_collapse(state: GroupState, ids, scores, groups, qmap=None, init=False, exhausted_hint=False, device: int = 0):
    """Continue the grouped walk of query qmap[i] (None: query i) over list i of ids / scores [B', kk] (canonical order; vs_topk_collapse)
    -> None; the state is updated in place and state.incomplete[0] holds the listed queries left incomplete.  Lists longer than 16 384
    entries are walked in column blocks.  All numpy, or all torch CUDA tensors on `device` (enqueued on torch's current stream)."""
    nat.require_device()
    Bp, kk = int(ids.shape[0]), int(ids.shape[1])
    on_dev = state.device is not None
    ids = ids.contiguous() if _is_torch(ids) else np.ascontiguousarray(ids, dtype=np.int64)
    scores = scores.contiguous() if _is_torch(scores) else np.ascontiguousarray(scores, dtype=np.float32)
    stream = current_stream(int(device)) if on_dev else None
    for c0 in range(0, kk, MAX_COLLAPSE_KK):
        c = min(MAX_COLLAPSE_KK, kk - c0)
        nat.check(nat.lib().vs_topk_collapse(_ptr(ids, c0 * 8), _ptr(scores, c0 * 4), Bp, c, kk, _ptr(qmap), _ptr(groups), int(groups.shape[0]),
                                             state.B, state.k, state.m, _ptr(state.group), _ptr(state.count), _ptr(state.ids),
                                             _ptr(state.scores), _ptr(state.status), _ptr(state.incomplete), 1 if (init and c0 == 0) else 0,
                                             1 if (exhausted_hint and c0 + c == kk) else 0, int(device), stream))


def group_filter(state: GroupState, groups, qmap, filter_words=None, filter_ld: int = 0, out=None, device: int = 0):
    """The rows the next round of the listed queries still has to rank (vs_group_filter) -> int32 words [B', W], W = ceil(n_rows / 32): the
    caller's filter (filter_words: [W] with filter_ld = 0, or [B, filter_ld]) AND group not full AND (group open OR fewer than k open) AND
    not kept.  All numpy, or all torch CUDA tensors on `device`."""
    nat.require_device()
    n = int(groups.shape[0])
    W = (n + 31) // 32
    Bp = int(qmap.shape[0]) if qmap is not None else state.B
    on_dev = state.device is not None
    if out is None:
        if on_dev:
            import torch
            try:
                out = torch.empty((Bp, W), dtype=torch.int32, device=torch.device("cuda", state.device))
            except torch.cuda.OutOfMemoryError:
                raise MemoryError(f"the per-query bitmaps of {Bp} unfinished queries over {n} rows take {Bp * W * 4} bytes of device memory: "
                                  f"search fewer queries a call, or start deeper (depth=)") from None
        else:
            out = np.zeros((Bp, W), dtype=np.uint32)
    nat.check(nat.lib().vs_group_filter(_ptr(groups), n, Bp, _ptr(qmap), state.B, state.k, state.m, _ptr(state.group), _ptr(state.count),
                                        _ptr(state.ids), _ptr(filter_words), int(filter_ld), _ptr(out), int(out.shape[1]), int(device),
                                        current_stream(int(device)) if on_dev else None))
    return out


def _search_grouped(obj, q, k, per_group, groups, filter, depth, rounds_out=None, left_out=None):
    """The rounds of a grouped search: search of depth kk under F_t -> vs_topk_collapse -> (for the queries left
    incomplete) vs_group_filter, kk doubled; ends when the device counter of incomplete queries reads 0.  obj: a DeviceIndex or a ShardGroup
    (its search(filter=) runs every round); groups: int32 [n_rows], on obj.device when it is a CUDA tensor.  rounds_out / left_out: lists
    that receive the number of rounds / the incomplete queries after each round (tests, tools/probe_grouped.py)."""
    import torch
    from .doc_filter import DocFilter, as_doc_filter
    k, m, depth = _grouped_args(k, per_group, depth)
    if q.ndim != 2:
        raise ValueError("queries must be [B, V]")
    n = int(obj.n_rows)
    if not hasattr(groups, "shape") or groups.ndim != 1 or int(groups.shape[0]) != n:
        raise ValueError(f"groups must hold one entry per row ({n}), got shape {tuple(getattr(groups, 'shape', ()))}")
    nat.require_device()
    device = int(obj.device)
    dev = torch.device("cuda", device)
    as_numpy = not _is_torch(q)
    qd = (torch.from_numpy(np.ascontiguousarray(q)) if as_numpy else q).to(dev)
    g = groups if _is_torch(groups) else torch.from_numpy(np.ascontiguousarray(groups))
    if g.dtype != torch.int32:
        if g.is_floating_point() or g.dtype == torch.bool:
            raise TypeError(f"groups must be integer group ids, got {g.dtype}")
        g = g.to(torch.int32)
    g = g.to(dev).contiguous()
    B = int(qd.shape[0])
    f = as_doc_filter(filter, n, device=device, batch=B) if filter is not None else None
    st = GroupState(B, k, m, device)
    kk = min(n, 2 * k * m if depth is None else depth)
    qa, fa, qmap, t = qd, f, None, 0
    while True:
        if isinstance(obj, ShardGroup):
            torch.cuda.current_stream(device).synchronize()              # (the group runs on its own streams)
        ids, sc = obj.search(qa, kk, filter=fa)
        topk_collapse(st, ids, sc, g, qmap=qmap, init=t == 0, exhausted_hint=kk >= n, device=device)
        t += 1
        left = int(st.incomplete.item())                                 # the one synchronisation of a round
        if left_out is not None:
            left_out.append(left)
        if left == 0:
            break
        qmap = (st.status == 0).nonzero().flatten().to(torch.int32)
        qa = qd.index_select(0, qmap.to(torch.int64))
        words = group_filter(st, g, qmap, None if f is None else f.words, 0 if f is None else f.ld, device=device)
        fa = DocFilter(words, n)
        kk = min(n, 2 * kk)
    if rounds_out is not None:
        rounds_out.append(t)
    if as_numpy:
        torch.cuda.current_stream(device).synchronize()
        return GroupedResults(st.group.cpu().numpy(), st.ids.cpu().numpy(), st.scores.cpu().numpy())
    return GroupedResults(st.group, st.ids, st.scores)


class DiverseResults(NamedTuple):
    """Per query: the k hits Maximal Marginal Relevance picked from the candidate list, in pick order -- their ids, the search's own scores,
    their positions in the candidate list and the MMR value each was picked at (id -1 / score -inf / pos -1 / mmr -inf in unused slots)."""
    ids: Any           # int64 [B, k]
    scores: Any        # float32 [B, k]
    pos: Any           # int32 [B, k]
    mmr: Any           # float32 [B, k]


MAX_MMR_DEPTH = nat.MMR_MAX_DEPTH
DEFAULT_MMR_ROW_BYTES = 1 << 30          # candidate rows held at a time by search_diverse / diversify: a starting point, not a measured optimum
_MMR_MODES = {"cosine": nat.MMR_COSINE, "dot": nat.MMR_DOT}


def _lam_array(lam, B):
    """lam of search_diverse / mmr_select: one number or one per query -> float32 numpy [B], every value in [0, 1]"""
    if _is_torch(lam):
        lam = lam.detach().cpu().numpy()
    a = np.asarray(lam)
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise TypeError(f"lam must be a number or one number per query, got {a.dtype}")
    if a.ndim == 0:
        a = np.full(B, a, dtype=np.float32)
    elif a.shape != (B,):
        raise ValueError(f"lam must be one number or one per query ({B}), got shape {a.shape}")
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not bool(((a >= 0) & (a <= 1)).all()):
        raise ValueError("lam must lie in [0, 1]")
    return a


def _diverse_args(k, depth=None, sim="cosine"):
    """Argument checks of search_diverse() / diversify() that need no device -> (k, depth or None, mode)"""
    for name, v in (("k", k),) + ((("depth", depth),) if depth is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
        if v < 1:
            raise ValueError(f"{name} must be >= 1, got {v}")
    if sim not in _MMR_MODES:
        raise ValueError(f"sim must be one of {sorted(_MMR_MODES)}, got {sim!r}")
    if depth is not None:
        if depth < k:
            raise ValueError(f"depth = {depth} is smaller than k = {k}: the picks come out of the depth candidates")
        if depth > MAX_MMR_DEPTH:
            raise ValueError(f"depth must be at most {MAX_MMR_DEPTH} candidates, got {depth}")
    return int(k), (None if depth is None else int(depth)), _MMR_MODES[sim]


def mmr_select(indptr, indices, values, ids, scores, k: int, lam, mode: str, n_cols: int, device: int = 0, out=None):
    """Maximal Marginal Relevance over hit lists (vs_mmr_select_csr): per query b pick k of the candidates ids / scores [B, kk] (the
    entries before the first id -1), whose stored rows are rows b * kk + j of the compact CSR indptr / indices / values (what get_rows
    returns for ids.reshape(-1)).  lam: one number or one per query; mode: "cosine" | "dot"; n_cols: the rows' column count (<= 32 768).
    -> (ids int64, scores float32, pos int32, mmr float32, pen float32), all [B, k]; out: five such arrays to write instead.  All numpy,
    or all torch CUDA tensors on `device` (enqueued on torch's current stream)."""
    nat.require_device()
    if mode not in _MMR_MODES:
        raise ValueError(f"mode must be one of {sorted(_MMR_MODES)}, got {mode!r}")
    if not hasattr(ids, "ndim") or ids.ndim != 2 or tuple(scores.shape) != tuple(ids.shape):
        raise ValueError("ids and scores must be [B, kk] arrays of one shape")
    B, kk, k = int(ids.shape[0]), int(ids.shape[1]), int(k)
    if int(indptr.shape[0]) != B * kk + 1:
        raise ValueError(f"indptr must hold {B * kk + 1} entries (one row per candidate), got {int(indptr.shape[0])}")
    lam_h = _lam_array(lam, B)
    on_dev = _is_torch(ids) and ids.is_cuda
    if on_dev:
        import torch
        tens = [x.contiguous() for x in (indptr, indices, values, ids, scores)]
        for t, dt, name in zip(tens, (torch.int64, torch.int32, torch.float32, torch.int64, torch.float32), ("indptr", "indices", "values", "ids", "scores")):
            if t.dtype != dt:
                raise TypeError(f"{name} must be {dt}, got {t.dtype}")
        lam_a = torch.from_numpy(lam_h).to(ids.device)
        if out is None:
            out = tuple(torch.empty((B, max(k, 0)), dtype=dt, device=ids.device)
                        for dt in (torch.int64, torch.float32, torch.int32, torch.float32, torch.float32))
        stream = current_stream(int(device))
    else:
        tens = [np.ascontiguousarray(_host(x), dtype=dt) for x, dt in zip((indptr, indices, values, ids, scores),
                                                                           (np.int64, np.int32, np.float32, np.int64, np.float32))]
        lam_a = lam_h
        if out is None:
            out = tuple(np.empty((B, max(k, 0)), dtype=dt) for dt in (np.int64, np.float32, np.int32, np.float32, np.float32))
        stream = None
    nat.check(nat.lib().vs_mmr_select_csr(*[_ptr(t) if _numel(t) else None for t in tens[:3]], _ptr(tens[3]), _ptr(tens[4]), B, kk, kk,
                                          int(n_cols), _ptr(lam_a), k, _MMR_MODES[mode], *[_ptr(o) for o in out], int(device), stream))
    return tuple(out)


class FusedResults(NamedTuple):
    """Per query: the k documents with the largest fused value over L hit lists (fused descending, then id ascending) -- their ids, the fused
    values, and per list the document's 0-based position (-1: not in it) and the list's own score (-inf: not in it); n is the size of the
    union of the lists, whatever k is.  Unused slots hold id -1 / fused -inf / ranks -1 / scores -inf."""
    ids: Any           # int64 [B, k]
    fused: Any         # float32 [B, k]
    ranks: Any         # int32 [B, k, L]
    scores: Any        # float32 [B, k, L]
    n: Any             # int32 [B]


MAX_FUSE_LISTS, MAX_FUSE_DEPTH, MAX_FUSE_ENTRIES = nat.FUSE_MAX_LISTS, nat.FUSE_MAX_DEPTH, nat.FUSE_MAX_ENTRIES
_FUSE_MODES = {"rrf": nat.FUSE_RRF, "sum": nat.FUSE_SUM, "mnz": nat.FUSE_MNZ, "raw": nat.FUSE_RAW}


def _fuse_args(k, mode="rrf", c=60.0, depth=None, L=None):
    """Argument checks of fuse_topk() / search_fused() that need no device -> (k, mode code, c, depth or None)"""
    for name, v in (("k", k),) + ((("depth", depth),) if depth is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
        if not 1 <= v <= MAX_FUSE_DEPTH:
            raise ValueError(f"{name} must be in 1..{MAX_FUSE_DEPTH}, got {v}")
    if mode not in _FUSE_MODES:
        raise ValueError(f"the fusion method must be one of {sorted(_FUSE_MODES)}, got {mode!r}")
    c = float(c)
    if not (c >= 0 and c != float("inf")):
        raise ValueError(f"c must be finite and >= 0, got {c}")
    if L is not None:
        if not 1 <= L <= MAX_FUSE_LISTS:
            raise ValueError(f"1..{MAX_FUSE_LISTS} lists can be fused, got {L}")
        if depth is not None and L * depth > MAX_FUSE_ENTRIES:
            raise ValueError(f"{L} lists of depth {depth} hold more than {MAX_FUSE_ENTRIES} entries a query")
    return int(k), _FUSE_MODES[mode], c, (None if depth is None else int(depth))


def _fuse_rows(x, B, L, name):
    """weights / fill of fuse_topk: None | [L] (the batch's) | [B, >= L] (one row a query) -> (float32 numpy array or None, its row stride)"""
    if x is None:
        return None, 0
    if _is_torch(x):
        x = x.detach().cpu().numpy()
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim == 1 and a.shape[0] == L:
        return a, 0
    if a.ndim == 2 and a.shape[0] == B and a.shape[1] >= L:
        return a, int(a.shape[1])
    raise ValueError(f"{name} must be [L = {L}] for the batch or [B = {B}, >= L] per query, got shape {a.shape}")


def _stack_lists(lists):
    """A sequence of L (ids [B, kk_l], scores [B, kk_l]) pairs -> ids int64 / scores float32 [L, B, max kk_l], the shorter lists padded with
    id -1 / score -inf.  On the device when the first pair is; numpy otherwise."""
    lists = [tuple(p) for p in lists]
    if not lists or any(len(p) != 2 for p in lists):
        raise ValueError("the lists must be a non-empty sequence of (ids, scores) pairs")
    for i, s in lists:
        if not hasattr(i, "ndim") or i.ndim != 2 or tuple(s.shape) != tuple(i.shape) or int(i.shape[0]) != int(lists[0][0].shape[0]):
            raise ValueError("every list must be a pair of [B, kk] arrays of one shape, with one B for all lists")
    L, B, kk = len(lists), int(lists[0][0].shape[0]), max(int(i.shape[1]) for i, _ in lists)
    first = lists[0][0]
    if _is_torch(first) and first.is_cuda:
        import torch
        ids = torch.full((L, B, kk), -1, dtype=torch.int64, device=first.device)
        sc = torch.full((L, B, kk), float("-inf"), dtype=torch.float32, device=first.device)
        as_t = lambda x: x if _is_torch(x) else torch.from_numpy(np.ascontiguousarray(x))
        for l, (i, s) in enumerate(lists):
            ids[l, :, :i.shape[1]] = as_t(i).to(first.device)
            sc[l, :, :i.shape[1]] = as_t(s).to(first.device)
        return ids, sc
    ids = np.full((L, B, kk), -1, dtype=np.int64)
    sc = np.full((L, B, kk), -np.inf, dtype=np.float32)
    as_n = lambda x: x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x)
    for l, (i, s) in enumerate(lists):
        ids[l, :, :i.shape[1]] = as_n(i)
        sc[l, :, :i.shape[1]] = as_n(s)
    return ids, sc


def fuse_topk(ids, scores, k: int, mode: str = "rrf", weights=None, c: float = 60.0, fill=None, device: int = 0, out=None) -> FusedResults:
    """Rank / score fusion of L hit lists per query (vs_fuse_topk; the exact numerics: include/vsearch_hip.h): the union of the lists' ids,
    each given a fused value, the top k by (fused descending, id ascending).  ids int64 / scores float32 [L, B, kk]; or ids a sequence of L
    (ids [B, kk_l], scores) pairs and scores None: shorter lists are padded with id -1 / score -inf.  A list ends at its first id -1.
    mode: "rrf" (sum of w_l / (c + rank), ranks from 1; scores are not read) | "sum" (weighted sum of min-max normalised scores) | "mnz"
    ("sum" times the number of lists holding the document) | "raw" (weighted sum of the raw scores; a list that lacks the document adds
    w_l * fill).  weights / fill: None, [L] for the batch or [B, >= L] per query.  L <= 8, kk and k <= 1024, L * kk <= 4096.  All numpy,
    or all torch CUDA tensors on `device` (enqueued on torch's current stream); out: the five arrays of a FusedResults to write instead."""
    nat.require_device()
    if scores is None:
        ids, scores = _stack_lists(ids)
    if not hasattr(ids, "ndim") or ids.ndim != 3 or tuple(scores.shape) != tuple(ids.shape):
        raise ValueError("ids and scores must be [L, B, kk] arrays of one shape")
    L, B, kk = (int(x) for x in ids.shape)
    k, mode_code, c, _ = _fuse_args(k, mode, c)
    w, ldw = _fuse_rows(weights, B, L, "weights")
    f, ldf = _fuse_rows(fill, B, L, "fill")
    if f is not None and ldf == 0:
        f, ldf = np.ascontiguousarray(np.broadcast_to(f, (B, L))), L
    on_dev = _is_torch(ids) and ids.is_cuda
    if on_dev:
        import torch
        ids, scores = ids.contiguous(), scores.contiguous()
        if ids.dtype != torch.int64 or scores.dtype != torch.float32:
            raise TypeError(f"ids must be int64 and scores float32, got {ids.dtype} and {scores.dtype}")
        w, f = (None if x is None else torch.from_numpy(x).to(ids.device) for x in (w, f))
        if out is None:
            out = tuple(torch.empty(shape, dtype=dt, device=ids.device) for shape, dt in
                        (((B, k), torch.int64), ((B, k), torch.float32), ((B, k, L), torch.int32), ((B, k, L), torch.float32), ((B,), torch.int32)))
        stream = current_stream(int(device))
    else:
        ids, scores = np.ascontiguousarray(_host(ids), dtype=np.int64), np.ascontiguousarray(_host(scores), dtype=np.float32)
        if out is None:
            out = tuple(np.empty(shape, dtype=dt) for shape, dt in
                        (((B, k), np.int64), ((B, k), np.float32), ((B, k, L), np.int32), ((B, k, L), np.float32), ((B,), np.int32)))
        stream = None
    nat.check(nat.lib().vs_fuse_topk(_ptr(ids), _ptr(scores), L, B, kk, kk, B * kk, _ptr(w), ldw, _ptr(f), ldf, mode_code, c, k,
                                     *[_ptr(o) for o in out], int(device), stream))
    return FusedResults(*out)


def _search_fused(obj, qs, k, mode="rrf", weights=None, c=60.0, depth=None, filter=None):
    """search(q_l, depth, filter=) for each of the L query batches -> fuse_topk of the L lists.  depth defaults to min(n_rows, 1024,
    4096 / L, max(4 k, k + 16)): a starting point, not a measured optimum.  Deleted rows and the filter act through the searches.
    obj: a DeviceIndex or a ShardGroup."""
    import torch
    qs = list(qs) if isinstance(qs, (list, tuple)) else [qs[l] for l in range(int(qs.shape[0]))] if getattr(qs, "ndim", 0) == 3 else None
    if not qs or any(getattr(q, "ndim", 0) != 2 or int(q.shape[0]) != int(qs[0].shape[0]) for q in qs):
        raise ValueError("the queries must be [L, B, V] or a non-empty list of L batches [B, V] of one B")
    L = len(qs)
    k, _, c, depth = _fuse_args(k, mode, c, depth, L)
    if depth is None:
        depth = max(1, min(int(obj.n_rows), MAX_FUSE_DEPTH, MAX_FUSE_ENTRIES // L, max(4 * k, k + 16)))
    nat.require_device()
    device = int(obj.device)
    as_numpy = not _is_torch(qs[0])
    on_host = as_numpy or not qs[0].is_cuda
    dev = torch.device("cuda", device)
    lists = []
    for q in qs:
        qd = (torch.from_numpy(np.ascontiguousarray(q)) if not _is_torch(q) else q).to(dev)
        if isinstance(obj, ShardGroup):
            torch.cuda.current_stream(device).synchronize()                   # (the group runs on its own streams)
        lists.append(obj.search(qd, depth, filter=filter))
    res = fuse_topk(lists, None, k, mode, weights, c, None, device)
    if on_host:
        torch.cuda.current_stream(device).synchronize()
        res = FusedResults(*(t.cpu().numpy() if as_numpy else t.cpu() for t in res))
    return res


class RangeResults(NamedTuple):
    """search_range: per query the number of matching documents (exact, whatever max_hits is) and the first max_hits of them in the
    canonical order (score descending, id ascending): all of them when counts[b] <= max_hits, else the top max_hits; id -1 / score
    -inf behind the matches."""
    ids: Any           # int64 [B, max_hits]
    scores: Any        # float32 [B, max_hits]
    counts: Any        # int64 [B]


MAX_RANGE_HITS = nat.RANGE_MAX_HITS


def _range_args(q, min_score, max_hits):
    """Argument checks of a range search that need no device -> (B, thresholds float32 ndarray [B], max_hits)"""
    if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)):
        raise TypeError(f"max_hits must be an int, got {type(max_hits).__name__}")
    max_hits = int(max_hits)
    if not 0 <= max_hits <= MAX_RANGE_HITS:
        raise ValueError(f"max_hits must be in 0..{MAX_RANGE_HITS}, got {max_hits}")
    if not hasattr(q, "ndim") or q.ndim != 2:
        raise ValueError("queries must be [B, V]")
    B = int(q.shape[0])
    if _is_torch(min_score):
        min_score = min_score.detach().cpu().numpy()
    thr = np.asarray(min_score, dtype=np.float32)
    if thr.ndim == 0:
        thr = np.full(B, thr, dtype=np.float32)
    if thr.ndim != 1 or thr.shape[0] != B:
        raise ValueError(f"min_score: one number, or one per query ({B}); got shape {tuple(thr.shape)}")
    if np.isnan(thr).any():
        raise ValueError("min_score is NaN")
    return B, np.ascontiguousarray(thr), max_hits


BOOST_MODES = {"add": nat.BOOST_ADD, "mul": nat.BOOST_MUL}
MAX_BOOST_FIELDS = nat.BOOST_MAX_FIELDS


def _boost_args(q, boosts, weights, mode, min_score, max_hits, n_rows=None):
    """Argument checks of a boosted search that need no device -> (B, thresholds float32 ndarray [B], max_hits, (fields, dtypes, weights
    [B, F], mode code)).  boosts: 1..4 value columns [n_rows], float32 or int32 (value_column() converts), numpy or torch.  weights: one per
    field (shared by the queries) or [B, F]; host weights must be finite, a CUDA tensor is passed as it is (a NaN there makes its query
    match nothing).  min_score None: no floor (-inf)."""
    if mode not in BOOST_MODES:
        raise ValueError(f"mode must be one of {sorted(BOOST_MODES)}, got {mode!r}")
    B, thr, K = _range_args(q, -np.inf if min_score is None else min_score, max_hits)
    if hasattr(boosts, "ndim") or not isinstance(boosts, (list, tuple)):
        raise TypeError("boosts must be a list of value columns (one array per field)")
    F = len(boosts)
    if not 1 <= F <= MAX_BOOST_FIELDS:
        raise ValueError(f"a boosted search takes 1..{MAX_BOOST_FIELDS} fields, got {F}")
    dtypes = []
    for j, f in enumerate(boosts):
        if f is None or not hasattr(f, "shape"):
            raise TypeError(f"boosts[{j}] is not an array of values")
        dtypes.append(_value_dtype(f))
        if len(f.shape) != 1 or (n_rows is not None and int(f.shape[0]) != int(n_rows)):
            raise ValueError(f"boosts[{j}] must hold one entry per row{'' if n_rows is None else f' ({int(n_rows)})'}, got shape {tuple(f.shape)}")
    if _is_torch(weights) and weights.is_cuda:
        w = weights
        if w.dim() == 1:
            w = w.unsqueeze(0).expand(B, -1)
        if tuple(w.shape) != (B, F):
            raise ValueError(f"weights: one per field ({F}), or [B, F] = [{B}, {F}]; got shape {tuple(weights.shape)}")
        w = w.float().contiguous()
    else:
        w = np.asarray(weights.detach().numpy() if _is_torch(weights) else weights, dtype=np.float32)
        if w.ndim == 1:
            w = np.broadcast_to(w[None, :], (B, w.shape[0]))
        if w.ndim != 2 or w.shape != (B, F):
            raise ValueError(f"weights: one per field ({F}), or [B, F] = [{B}, {F}]; got shape {tuple(np.shape(weights))}")
        if not np.isfinite(w).all():
            raise ValueError("weights must be finite")
        w = np.ascontiguousarray(w, dtype=np.float32)
    return B, thr, K, (list(boosts), dtypes, w, BOOST_MODES[mode])


def _boost_c_args(boost, device):
    """(fields, dtypes, weights, mode) -> (the trailing arguments of vs_index_search_boosted, what they point into).  device: a torch device --
    columns and weights are moved there -- or None: host arrays."""
    fields, dtypes, w, mode = boost
    if device is not None:
        import torch
        fs = [(f if _is_torch(f) else torch.from_numpy(np.ascontiguousarray(f))).to(device).contiguous() for f in fields]
        wt = (w if _is_torch(w) else torch.from_numpy(w)).to(device).contiguous()
        ptrs, wp = [f.data_ptr() for f in fs], wt.data_ptr()
    else:
        fs = [np.ascontiguousarray(f.numpy() if _is_torch(f) else f) for f in fields]
        wt = w
        ptrs, wp = [f.ctypes.data for f in fs], wt.ctypes.data
    F = len(fs)
    return ((C.c_void_p * F)(*ptrs), (C.c_int32 * F)(*dtypes), F, C.c_void_p(wp), mode), (fs, wt)


def _boost_on_device(boost):
    return boost is not None and (any(_is_torch(f) and f.is_cuda for f in boost[0]) or (_is_torch(boost[2]) and boost[2].is_cuda))


def _words_to_int32(words_i64):
    """uint32 values held in int64 -> the int32 words of a DocFilter"""
    import torch
    return (words_i64 - ((words_i64 >> 31) << 32)).to(torch.int32)


def _range_shards(group, q, min_score, max_hits, filter, want_words, boost=None):
    """Range search of a ShardGroup: every shard with its id_offset (and its bit range of the filter); lists merged with vs_merge_topk on
    the first shard's GPU, counts summed, bitmaps placed at their bit offsets -> (ids, scores, counts, words | None) on that GPU.
    boost (a boosted search: _boost_args' tuple over the group's rows): every shard gets its row slice of every field."""
    import torch
    B, thr, K = _range_args(q, min_score, max_hits)
    nat.require_device()
    dev0 = torch.device("cuda", group.device)
    qt = q if _is_torch(q) else torch.from_numpy(np.ascontiguousarray(q))
    n_total = group.n_rows
    f = None
    if filter is not None:
        from .doc_filter import as_doc_filter
        f = as_doc_filter(filter, n_total, device=dev0, batch=B)
    W = (n_total + 31) // 32
    words = torch.zeros((B, W + 1), dtype=torch.int64, device=dev0) if want_words else None
    counts = torch.zeros(B, dtype=torch.int64, device=dev0)
    lists, row0 = [], 0
    for sh in group._shards:
        dev = torch.device("cuda", sh.device)
        n = int(sh.info().n_rows)
        fs = f.to(dev) if f is not None else None
        bs = None if boost is None else ([f[row0:row0 + n] for f in boost[0]],) + tuple(boost[1:])
        ids, sc, cnt, w = sh._range_call(qt.to(dev), thr, K, fs, row0, want_words, filter_bit0=row0, boost=bs)
        counts += cnt.to(dev0)
        if K:
            lists.append((ids.to(dev0), sc.to(dev0)))
        if want_words:
            w = w.to(dev0).to(torch.int64) & 0xFFFFFFFF
            w0, sft, wn = row0 >> 5, row0 & 31, int(w.shape[1])
            words[:, w0:w0 + wn] |= (w << sft) & 0xFFFFFFFF
            if sft:
                words[:, w0 + 1:w0 + 1 + wn] |= w >> (32 - sft)
        row0 += n
    if K:
        ids, sc = merge_topk(torch.cat([l[0] for l in lists], dim=1).contiguous(), torch.cat([l[1] for l in lists], dim=1).contiguous(), K,
                             device=group.device)
    else:
        ids = torch.empty((B, 0), dtype=torch.int64, device=dev0)
        sc = torch.empty((B, 0), dtype=torch.float32, device=dev0)
    if want_words:
        words = _words_to_int32(words[:, :W]).contiguous()
    return ids, sc, counts, words


def _range_out(q, *tensors):
    """results in the kind of the query: torch CUDA in -> as they are, torch CPU in -> CPU tensors, numpy in -> ndarrays"""
    if _is_torch(q) and q.is_cuda:
        return tensors
    if _is_torch(q):
        return tuple(t.cpu() for t in tensors)
    return tuple(t.cpu().numpy() for t in tensors)


# ---- facet counts: how a document set spreads over per-row labels (vs_facet_counts, vs_index_facet_counts, vs_facet_topn) ----------------
class FacetCounts(NamedTuple):
    """facet_counts: per query the documents of the set per label (counts [B, n_labels]), the size of the set (total [B]) and its documents
    whose label is outside [0, n_labels) -- -1 = "no label" -- (other [B]); counts.sum(1) + other == total.  All int64."""
    counts: Any
    total: Any
    other: Any


class TopFacets(NamedTuple):
    """top_facets: per query the `topn` labels with the most documents of the set, count descending then label ascending (labels int32
    [B, topn], counts int64 [B, topn]; unused slots label -1 / count 0), with the set's total and other as in FacetCounts."""
    labels: Any
    counts: Any
    total: Any
    other: Any


MAX_FACET_TOPN = nat.FACET_MAX_TOPN


def facet_plan(n_rows: int, B: int, n_labels: int, per_query: bool, rows_per_chunk: int = 0):
    """The launch vs_facet_counts takes for these arguments (vs_facet_plan; pure host arithmetic, no GPU needed) -> (regime, qt, chunks,
    rows_per_chunk): regime 0 = LDS histograms, 1 = global atomics; qt = queries a workgroup serves."""
    regime, qt, chunks, rpc = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_facet_plan(int(n_rows), int(B), int(n_labels), 1 if per_query else 0, int(rows_per_chunk), C.byref(regime), C.byref(qt),
                                      C.byref(chunks), C.byref(rpc)))
    return regime.value, qt.value, chunks.value, rpc.value


def _facet_args(labels, n_labels, n_rows, rows_per_chunk=0):
    """Argument checks of a facet count that need no device -> (n_labels, rows_per_chunk)"""
    for name, v in (("n_labels", n_labels), ("rows_per_chunk", rows_per_chunk)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
    n_labels, rows_per_chunk = int(n_labels), int(rows_per_chunk)
    if not 1 <= n_labels <= 0x7FFFFFFF:
        raise ValueError(f"n_labels must be in 1..2^31 - 1, got {n_labels}")
    if rows_per_chunk < 0 or rows_per_chunk % 64:
        raise ValueError(f"rows_per_chunk must be 0 (automatic) or a positive multiple of 64, got {rows_per_chunk}")
    if not hasattr(labels, "shape") or labels.ndim != 1 or int(labels.shape[0]) != int(n_rows):
        raise ValueError(f"labels must hold one entry per row ({int(n_rows)}), got shape {tuple(getattr(labels, 'shape', ()))}")
    dt = str(labels.dtype)
    if "float" in dt or "bool" in dt or "complex" in dt:
        raise TypeError(f"labels must be integer codes, got {labels.dtype}")
    return n_labels, rows_per_chunk


def _topn_args(topn, min_count):
    for name, v in (("topn", topn), ("min_count", min_count)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
    if not 1 <= int(topn) <= MAX_FACET_TOPN:
        raise ValueError(f"topn must be in 1..{MAX_FACET_TOPN}, got {int(topn)}")
    return int(topn), int(min_count)


def _labels_on(labels, device: int):
    """labels (numpy / torch, any integer dtype) -> contiguous int32 tensor on GPU `device` (the tensor itself when it is one already)"""
    import torch
    t = labels if _is_torch(labels) else torch.from_numpy(np.ascontiguousarray(labels))
    if t.dtype != torch.int32:
        t = t.clamp(-1, 0x7FFFFFFF).to(torch.int32)              # (anything negative is "no label"; too large stays outside n_labels)
    return t.to(torch.device("cuda", device)).contiguous()


def facet_topn(counts, topn: int, min_count: int = 1, device: int = 0):
    """Per query the `topn` labels with the largest counts [B, n_labels] (vs_facet_topn) -> (labels int32 [B, topn], counts int64 [B, topn]):
    count descending, then label ascending; only labels with count >= max(min_count, 1); unused slots label -1 / count 0.  numpy in ->
    numpy out; torch CUDA in -> tensors on `device`, enqueued on torch's current stream."""
    topn, min_count = _topn_args(topn, min_count)
    if not hasattr(counts, "shape") or counts.ndim != 2:
        raise ValueError("counts must be [B, n_labels]")
    B, L = int(counts.shape[0]), int(counts.shape[1])
    nat.require_device()
    if _is_torch(counts) and counts.is_cuda:
        import torch
        c = counts.to(torch.int64).contiguous()
        labels = torch.empty((B, topn), dtype=torch.int32, device=c.device)
        out = torch.empty((B, topn), dtype=torch.int64, device=c.device)
        nat.check(nat.lib().vs_facet_topn(_ptr(c), L, B, L, topn, min_count, _ptr(labels), _ptr(out), int(device), current_stream(int(device))))
        return labels, out
    c = np.ascontiguousarray(_host(counts), dtype=np.int64)
    labels = np.empty((B, topn), dtype=np.int32)
    out = np.empty((B, topn), dtype=np.int64)
    nat.check(nat.lib().vs_facet_topn(_ptr(c), L, B, L, topn, min_count, _ptr(labels), _ptr(out), int(device), None))
    return labels, out


def _facet_out(labels, *tensors):
    """results in the kind of the labels: torch in -> CUDA tensors as they are, numpy in -> ndarrays"""
    return tensors if _is_torch(labels) else tuple(t.cpu().numpy() for t in tensors)


# ---- term aggregations: what a document set is about (vs_index_term_counts, vs_index_term_counts_ids, vs_term_topn) -------------------------
class TermCounts(NamedTuple):
    """term_counts: per query the documents of the set that have each vocabulary column (counts [B, n_cols]) and the size of the set
    (total [B]).  All int64."""
    counts: Any
    total: Any


class TopTerms(NamedTuple):
    """top_terms / significant_terms: per query the `topn` most significant columns of the set (cols int32 [B, topn], scores float32
    [B, topn]), with the documents of the set that have the column (df int64 [B, topn]), the documents of the background that have it
    (bg int64 [B, topn]) and the size of the set (total int64 [B]).  Unused slots: col -1 / score -inf / df 0 / bg 0."""
    cols: Any
    scores: Any
    df: Any
    bg: Any
    total: Any


MAX_TERM_TOPN = nat.TERM_MAX_TOPN
_TERM_METHODS = {"lift": nat.TERM_LIFT, "jlh": nat.TERM_JLH}


def term_plan(n_rows: int, B: int, n_cols: int, per_query: bool, rows_per_chunk: int = 0):
    """The launch vs_index_term_counts takes for these arguments (vs_term_plan; pure host arithmetic, no GPU needed) -> (regime, chunks,
    rows_per_chunk): regime 0 = one LDS histogram of all columns per workgroup, 1 = global atomics."""
    regime, chunks, rpc = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_term_plan(int(n_rows), int(B), int(n_cols), 1 if per_query else 0, int(rows_per_chunk), C.byref(regime),
                                     C.byref(chunks), C.byref(rpc)))
    return regime.value, chunks.value, rpc.value


def _term_topn_args(topn, method, min_count):
    """Argument checks of a term top-n that need no device -> (topn, method name, min_count); "count" orders by the raw count"""
    for name, v in (("topn", topn), ("min_count", min_count)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
    if not 1 <= int(topn) <= MAX_TERM_TOPN:
        raise ValueError(f"topn must be in 1..{MAX_TERM_TOPN}, got {int(topn)}")
    if method not in _TERM_METHODS and method != "count":
        raise ValueError(f'method must be "jlh", "lift" or "count", got {method!r}')
    return int(topn), method, int(min_count)


def term_topn(counts, total, bg, bg_total: int, topn: int = 20, method: str = "jlh", min_count: int = 1, device: int = 0):
    """Per query the `topn` most significant columns of counts [B, n_cols] / total [B] against the background bg [n_cols] / bg_total
    (vs_term_topn) -> (cols int32, scores float32, fg int64, bg int64), all [B, topn].  With fgp = fg / total and bgp = bg / bg_total in
    fp64: "lift" scores fgp / bgp; "jlh" (fgp - bgp) * (fgp / bgp) and lists only columns with fgp > bgp.  A candidate has fg >=
    max(min_count, 1) and bg > 0.  Score (rounded to fp32) descending, then column ascending; unused slots -1 / -inf / 0 / 0.  numpy in ->
    numpy out; torch CUDA in -> tensors on `device`, enqueued on torch's current stream."""
    topn, method, min_count = _term_topn_args(topn, method, min_count)
    if method == "count":
        raise ValueError('method "count" orders by the exact integers: use facet_topn(counts, topn, min_count)')
    if not hasattr(counts, "shape") or counts.ndim != 2:
        raise ValueError("counts must be [B, n_cols]")
    B, V = int(counts.shape[0]), int(counts.shape[1])
    if tuple(total.shape) != (B,) or tuple(bg.shape) != (V,):
        raise ValueError(f"total must be [{B}] and bg [{V}], got {tuple(total.shape)} and {tuple(bg.shape)}")
    nat.require_device()
    code = _TERM_METHODS[method]
    if _is_torch(counts) and counts.is_cuda:
        import torch
        dev = counts.device
        c, t, g = (x.to(dev).to(torch.int64).contiguous() for x in (counts, total, bg))
        outs = (torch.empty((B, topn), dtype=torch.int32, device=dev), torch.empty((B, topn), dtype=torch.float32, device=dev),
                torch.empty((B, topn), dtype=torch.int64, device=dev), torch.empty((B, topn), dtype=torch.int64, device=dev))
        nat.check(nat.lib().vs_term_topn(_ptr(c), V, _ptr(t), B, V, _ptr(g), int(bg_total), code, topn, min_count, *(_ptr(o) for o in outs),
                                         int(device), current_stream(int(device))))
        return outs
    c, t, g = (np.ascontiguousarray(_host(x), dtype=np.int64) for x in (counts, total, bg))
    outs = (np.empty((B, topn), dtype=np.int32), np.empty((B, topn), dtype=np.float32), np.empty((B, topn), dtype=np.int64),
            np.empty((B, topn), dtype=np.int64))
    nat.check(nat.lib().vs_term_topn(_ptr(c), V, _ptr(t), B, V, _ptr(g), int(bg_total), code, topn, min_count, *(_ptr(o) for o in outs),
                                     int(device), None))
    return outs


def _term_ids(ids):
    """ids of a term count -> int64 [B, m] (a 1-D list is one query), numpy or tensor as given"""
    if isinstance(ids, (list, tuple)):
        ids = np.asarray(ids, dtype=np.int64)
    if not hasattr(ids, "shape") or ids.ndim not in (1, 2):
        raise ValueError("ids must be int64 [B, m] (or [m]: one query)")
    if "int64" not in str(ids.dtype):
        raise TypeError(f"ids must be int64, got {ids.dtype}")
    if ids.ndim == 1:
        ids = ids[None, :]
    if int(ids.shape[1]) < 1:
        raise ValueError("ids must hold at least one entry a query (pad with -1)")
    return ids


def _background_arg(background):
    if background is not None and (not isinstance(background, tuple) or len(background) != 2):
        raise TypeError("background must be a TermCounts (what term_counts() returns)")


def _top_terms(obj, filter, ids, topn, method, min_count, background):
    """term_counts of the set, the background (given, or every live document: one more pass), then the top-n on the object's first GPU"""
    topn, method, min_count = _term_topn_args(topn, method, min_count)
    _background_arg(background)
    return _top_terms_of(obj, obj.term_counts(filter=filter, ids=ids), topn, method, min_count, background)


def _top_terms_of(obj, fg, topn, method, min_count, background):
    """the top-n of counts already taken: fg = (counts [B, V], total [B]) on obj's GPU, one row a query -- or a label (_label_top_terms)"""
    import torch
    dev = fg.counts.device
    if background is None and method != "count":
        background = obj.term_counts()
    bgc = bgt = None
    if background is not None:
        bgc = torch.as_tensor(background.counts).to(dev).to(torch.int64).reshape(-1)
        bgt = int(torch.as_tensor(background.total).reshape(-1)[0])
        if int(bgc.shape[0]) != int(fg.counts.shape[1]):
            raise ValueError(f"background.counts holds {int(bgc.shape[0])} columns, the index {int(fg.counts.shape[1])}")
    if method == "count":                                          # the exact integers: vs_facet_topn over the counts
        cols, df = facet_topn(fg.counts, topn, min_count, device=obj.device)
        bg = torch.zeros_like(df) if bgc is None else torch.where(cols >= 0, bgc[cols.clamp(min=0).long()], torch.zeros_like(df))
        scores = torch.where(cols >= 0, df.to(torch.float32), torch.full_like(df, float("-inf"), dtype=torch.float32))
        return TopTerms(cols, scores, df, bg, fg.total)
    cols, scores, df, bg = term_topn(fg.counts, fg.total, bgc, bgt, topn, method, min_count, device=obj.device)
    return TopTerms(cols, scores, df, bg, fg.total)


# ---- term sums: how much weight a document set puts on each column (vs_index_term_sums, vs_index_term_sums_ids, vs_term_sum_topn) ---------------
TERM_FX_ONE = 1 << nat.TERM_FX_SHIFT                   # the fixed-point image of the value 1.0
MAX_TERM_TILE_COLS = nat.TERM_SUM_TILE_COLS


class TermSums(NamedTuple):
    """term_sums: per query the fixed-point weight the set puts on each vocabulary column (sums int64 [B, n_cols]: every stored cell adds its
    value, clamped to +-2^20, times 2^24, rounded to nearest even) and the size of the set (total int64 [B]).  Integers: the result does
    not depend on the order of the additions, shards add exactly."""
    sums: Any
    total: Any

    def values(self):
        """the sums as float64 [B, n_cols]: sums * 2^-24"""
        if _is_torch(self.sums):
            import torch
            return self.sums.to(torch.float64) * (1.0 / TERM_FX_ONE)
        return np.asarray(self.sums).astype(np.float64) * (1.0 / TERM_FX_ONE)

    def mean(self):
        """the set's centroid, float32 [B, n_cols]: (double(sums) * 2^-24) / double(total) rounded once to fp32 -- the chain of the top-n's
        score; a query whose set is empty (total = 0) gets an all-zero row"""
        if _is_torch(self.sums):
            import torch
            t = self.total.to(torch.float64).reshape(-1, 1)
            m = (self.values() / torch.where(t > 0, t, torch.ones_like(t))).to(torch.float32)
            return torch.where(t > 0, m, torch.zeros_like(m))
        t = np.asarray(self.total).astype(np.float64).reshape(-1, 1)
        m = (self.values() / np.where(t > 0, t, 1.0)).astype(np.float32)
        return np.where(t > 0, m, np.float32(0))


class TopWeights(NamedTuple):
    """top_weight_terms / centroid_terms: per query the `topn` columns with the largest mean weight over the set (cols int32 [B, topn],
    scores float32 [B, topn] = the mean weight), their fixed-point sums (sums int64 [B, topn]) and the size of the set (total int64
    [B]).  Unused slots: col -1 / score -inf / sum 0."""
    cols: Any
    scores: Any
    sums: Any
    total: Any


def term_sum_plan(n_rows: int, B: int, n_cols: int, per_query: bool, rows_per_chunk: int = 0, tile_cols: int = 0):
    """The launch vs_index_term_sums takes for these arguments (vs_term_sum_plan; pure host arithmetic, no GPU needed) -> (tiles, tile_cols,
    chunks, rows_per_chunk): the columns are cut into `tiles` tiles of `tile_cols`, a workgroup owns one tile of one query's chunk."""
    tiles, tc, chunks, rpc = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_term_sum_plan(int(n_rows), int(B), int(n_cols), 1 if per_query else 0, int(rows_per_chunk), int(tile_cols),
                                         C.byref(tiles), C.byref(tc), C.byref(chunks), C.byref(rpc)))
    return tiles.value, tc.value, chunks.value, rpc.value


def _rows_per_chunk_arg(rows_per_chunk) -> int:
    """The tuning knob of the chunked walks: 0 (automatic) or a positive multiple of 64"""
    if isinstance(rows_per_chunk, bool) or not isinstance(rows_per_chunk, (int, np.integer)) or rows_per_chunk < 0 or rows_per_chunk % 64:
        raise ValueError(f"rows_per_chunk must be 0 (automatic) or a positive multiple of 64, got {rows_per_chunk!r}")
    return int(rows_per_chunk)


class _TermAgg(NamedTuple):
    """A term aggregation over a document set: its two entry points (bitmap driven, id-list driven) and its result tuple"""
    bitmap: str
    ids: str
    result: Any


_TERM_COUNTS = _TermAgg("vs_index_term_counts", "vs_index_term_counts_ids", TermCounts)
_TERM_SUMS = _TermAgg("vs_index_term_sums", "vs_index_term_sums_ids", TermSums)


def _term_sum_args(rows_per_chunk, tile_cols):
    """Argument checks of a term sum's tuning knobs that need no device -> (rows_per_chunk, tile_cols)"""
    rows_per_chunk = _rows_per_chunk_arg(rows_per_chunk)
    if isinstance(tile_cols, bool) or not isinstance(tile_cols, (int, np.integer)) or not 0 <= tile_cols <= MAX_TERM_TILE_COLS:
        raise ValueError(f"tile_cols must be 0 (automatic) or in 1..{MAX_TERM_TILE_COLS}, got {tile_cols!r}")
    return rows_per_chunk, int(tile_cols)


def _weight_topn_args(topn, min_count):
    """Argument checks of a weight top-n that need no device -> (topn, min_count)"""
    for name, v in (("topn", topn), ("min_count", min_count)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
    if not 1 <= int(topn) <= MAX_TERM_TOPN:
        raise ValueError(f"topn must be in 1..{MAX_TERM_TOPN}, got {int(topn)}")
    return int(topn), int(min_count)


def term_sum_topn(sums, total, topn: int = 20, counts=None, min_count: int = 0, device: int = 0):
    """Per query the `topn` columns with the largest mean weight, from sums [B, n_cols] / total [B] (vs_term_sum_topn) -> (cols int32, scores
    float32, sums int64), all [B, topn].  A candidate has sum > 0 and, when `counts` [B, n_cols] (``term_counts`` of the same set) is
    given, counts >= min_count.  score = float32((double(sum) * 2^-24) / double(total)); score descending, then column ascending; unused
    slots -1 / -inf / 0.  numpy in -> numpy out; torch CUDA in -> tensors on `device`, enqueued on torch's current stream."""
    topn, min_count = _weight_topn_args(topn, min_count)
    if not hasattr(sums, "shape") or sums.ndim != 2:
        raise ValueError("sums must be [B, n_cols]")
    B, V = int(sums.shape[0]), int(sums.shape[1])
    if tuple(total.shape) != (B,):
        raise ValueError(f"total must be [{B}], got {tuple(total.shape)}")
    if counts is not None and tuple(counts.shape) != (B, V):
        raise ValueError(f"counts must be [{B}, {V}] as sums, got {tuple(counts.shape)}")
    nat.require_device()
    if _is_torch(sums) and sums.is_cuda:
        import torch
        dev = sums.device
        s, t = (x.to(dev).to(torch.int64).contiguous() for x in (sums, total))
        c = counts.to(dev).to(torch.int64).contiguous() if counts is not None else None
        outs = (torch.empty((B, topn), dtype=torch.int32, device=dev), torch.empty((B, topn), dtype=torch.float32, device=dev),
                torch.empty((B, topn), dtype=torch.int64, device=dev))
        nat.check(nat.lib().vs_term_sum_topn(_ptr(s), V, _ptr(t), _ptr(c) if c is not None else None, V, B, V, topn, min_count,
                                             *(_ptr(o) for o in outs), int(device), current_stream(int(device))))
        return outs
    s, t = (np.ascontiguousarray(_host(x), dtype=np.int64) for x in (sums, total))
    c = np.ascontiguousarray(_host(counts), dtype=np.int64) if counts is not None else None
    outs = (np.empty((B, topn), dtype=np.int32), np.empty((B, topn), dtype=np.float32), np.empty((B, topn), dtype=np.int64))
    nat.check(nat.lib().vs_term_sum_topn(_ptr(s), V, _ptr(t), _ptr(c) if c is not None else None, V, B, V, topn, min_count,
                                         *(_ptr(o) for o in outs), int(device), None))
    return outs


def _top_weights(obj, filter, ids, topn, min_count):
    """term_sums of the set (and its term_counts when min_count asks for them), then the top-n on the object's first GPU"""
    topn, min_count = _weight_topn_args(topn, min_count)
    res = obj.term_sums(filter=filter, ids=ids)
    counts = obj.term_counts(filter=filter, ids=ids).counts if min_count > 0 else None
    cols, scores, sums = term_sum_topn(res.sums, res.total, topn, counts=counts, min_count=min_count, device=obj.device)
    return TopWeights(cols, scores, sums, res.total)


# ---- per-label term aggregations: the term sums / counts of every label's rows in one pass (vs_label_term_plan, vs_label_order, ------------------
# vs_index_label_term_sums, vs_index_label_term_counts)
MAX_LABEL_TERM_LABELS = nat.LABEL_TERM_MAX_LABELS
MAX_LABEL_TERM_CELLS = nat.LABEL_TERM_MAX_CELLS


class LabelTermSums(NamedTuple):
    """label_term_sums: per label the fixed-point weight the set's documents with that label put on each vocabulary column (sums int64
    [n_labels, n_cols], ``TermSums``'s fixed point), the set's documents of each label (total int64 [n_labels]) and its documents whose
    label is outside [0, n_labels) (other int64 [1]): total.sum() + other is the size of the set.  Row l is, bit for bit, ``term_sums`` of
    the set ``from_labels(labels, [l]) & filter``."""
    sums: Any
    total: Any
    other: Any

    def values(self):
        """the sums as float64 [n_labels, n_cols]: sums * 2^-24"""
        return TermSums(self.sums, self.total).values()

    def mean(self):
        """every label's centroid, float32 [n_labels, n_cols]: ``TermSums.mean``'s chain; a label without documents gets an all-zero row"""
        return TermSums(self.sums, self.total).mean()


class LabelTermCounts(NamedTuple):
    """label_term_counts: per label the set's documents with that label that have each vocabulary column (counts int64 [n_labels, n_cols]),
    with total [n_labels] and other [1] as in ``LabelTermSums``."""
    counts: Any
    total: Any
    other: Any


class LabelOrder(NamedTuple):
    """label_order: the set's documents grouped by label -- rows int64 [n_set], of which rows[ptr[l]:ptr[l + 1]] are the documents of label
    l in no specified order; ptr int64 [n_labels + 1]; other int64 [1], the set's documents whose label is outside [0, n_labels)."""
    ptr: Any
    rows: Any
    other: Any


def label_term_plan(n_rows: int, n_labels: int, n_cols: int, rows_per_item: int = 0, tile_cols: int = 0):
    """The launch vs_index_label_term_sums / _counts take for these arguments (vs_label_term_plan; pure host arithmetic, no GPU needed) ->
    (tiles, tile_cols, rows_per_item, max_items): a workgroup owns one column tile of one item, at most rows_per_item rows of one label;
    the grid holds max_items = ceil(n_rows / rows_per_item) + n_labels items a tile."""
    tiles, tc, rpi, items = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_label_term_plan(int(n_rows), int(n_labels), int(n_cols), int(rows_per_item), int(tile_cols), C.byref(tiles),
                                           C.byref(tc), C.byref(rpi), C.byref(items)))
    return tiles.value, tc.value, rpi.value, items.value


def label_term_slices(n_labels: int, n_cols: int):
    """The labels [0, n_labels) cut into slices (l0, n) that one label_term_sums / label_term_counts call takes: n <= 65 536 and n x n_cols <=
    2^27.  A caller with more cells than one call holds -- a k-means of K = 4096 clusters over 65 535 columns -- takes a slice a call with
    ``labels - l0`` as the labels (a label outside the slice falls outside [0, n): it contributes nowhere); the integers are those of one call."""
    step = max(1, min(MAX_LABEL_TERM_LABELS, MAX_LABEL_TERM_CELLS // max(int(n_cols), 1)))
    return [(l0, min(step, int(n_labels) - l0)) for l0 in range(0, int(n_labels), step)]


def _label_term_args(labels, n_labels, n_rows, n_cols=None, rows_per_item=0, tile_cols=0):
    """Argument checks of a per-label term aggregation that need no device -> (n_labels, rows_per_item, tile_cols)"""
    n_labels, _ = _facet_args(labels, n_labels, n_rows)
    if n_labels > MAX_LABEL_TERM_LABELS:
        raise ValueError(f"n_labels must be in 1..{MAX_LABEL_TERM_LABELS}, got {n_labels}")
    if n_cols is not None and n_labels * int(n_cols) > MAX_LABEL_TERM_CELLS:
        raise ValueError(f"n_labels x n_cols = {n_labels * int(n_cols)} is more than {MAX_LABEL_TERM_CELLS} cells (1 GiB of int64)")
    if isinstance(rows_per_item, bool) or not isinstance(rows_per_item, (int, np.integer)) or rows_per_item < 0 or rows_per_item % 64:
        raise ValueError(f"rows_per_item must be 0 (automatic) or a positive multiple of 64, got {rows_per_item!r}")
    _, tile_cols = _term_sum_args(0, tile_cols)
    return n_labels, int(rows_per_item), tile_cols


# ---- clustering: the nearest of K centroids for every row (vs_assign_plan, vs_index_assign, vs_centroid_half_norms, vs_label_bitmaps) -----------
MAX_ASSIGN_K = nat.ASSIGN_MAX_K
MAX_LABEL_VALUES = nat.LABEL_MAX_VALUES


class Assignment(NamedTuple):
    """assign: per row the centroid with the largest value (labels int32 [N]; the lowest index among equals) and that value (values
    float32 [N]).  A row that is deleted or not allowed by the filter has label -1 / value -inf."""
    labels: Any
    values: Any


def assign_plan(n_rows: int, K: int, n_cols: int, rows_per_chunk: int = 0):
    """The launch vs_index_assign takes for these arguments (vs_assign_plan; pure host arithmetic, no GPU needed) -> (slice_w, slices, chunks,
    rows_per_chunk, slab_bytes): a lane owns slice_w / 64 centroids of each of the `slices` slices, a workgroup a chunk of rows; the
    transposed centroids take slab_bytes of device scratch."""
    w, s, chunks, rpc, slab = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_assign_plan(int(n_rows), int(K), int(n_cols), int(rows_per_chunk), C.byref(w), C.byref(s), C.byref(chunks),
                                       C.byref(rpc), C.byref(slab)))
    return w.value, s.value, chunks.value, rpc.value, slab.value


def _assign_args(centroids, bias, n_cols, rows_per_chunk=0):
    """Argument checks of an assignment that need no device -> (centroids float32 [K, V] tensor, bias float32 [K] tensor | None,
    rows_per_chunk).  A tensor on a GPU is not read here: the finiteness of device centroids is the caller's."""
    import torch
    rows_per_chunk = _rows_per_chunk_arg(rows_per_chunk)
    c = centroids if _is_torch(centroids) else torch.from_numpy(np.ascontiguousarray(np.asarray(centroids)))
    c = c.detach()
    if c.dim() != 2:
        raise ValueError(f"centroids must be [K, n_cols], got {c.dim()} dimensions")
    if not c.is_floating_point():
        raise TypeError(f"centroids must be floating point, got {c.dtype}")
    K, V = int(c.shape[0]), int(c.shape[1])
    if not 1 <= K <= MAX_ASSIGN_K:
        raise ValueError(f"the number of centroids must be in 1..{MAX_ASSIGN_K}, got {K}")
    if V != int(n_cols):
        raise ValueError(f"centroids have {V} columns, the index has {int(n_cols)}")
    c = c.to(torch.float32)
    if not c.is_cuda and not bool(torch.isfinite(c).all()):
        raise ValueError("centroids must be finite")
    b = None
    if bias is not None:
        b = bias if _is_torch(bias) else torch.from_numpy(np.ascontiguousarray(np.asarray(bias)))
        b = b.detach()
        if tuple(b.shape) != (K,):
            raise ValueError(f"bias must be [{K}], got {tuple(b.shape)}")
        if not b.is_floating_point():
            raise TypeError(f"bias must be floating point, got {b.dtype}")
        b = b.to(torch.float32)
        if not b.is_cuda and not bool(torch.isfinite(b).all()):
            raise ValueError("bias must be finite")
    return c, b, int(rows_per_chunk)


def centroid_half_norms(centroids, round_f16: bool = False, device: int = 0):
    """hn[j] = float32(0.5 * ||c'_j||^2) in the fixed order of vs_centroid_half_norms (256 strided fp64 partial sums of the fp32 squares, then a
    halving tree); round_f16: the centroids are rounded to fp16 first, as an fp16 index rounds them.  With bias = -hn, ``assign`` picks the
    nearest centroid in the Euclidean sense.  numpy in -> numpy out; torch CUDA in -> a tensor on `device`, on torch's current stream."""
    if not hasattr(centroids, "shape") or len(centroids.shape) != 2:
        raise ValueError("centroids must be [K, n_cols]")
    K, V = int(centroids.shape[0]), int(centroids.shape[1])
    if not 1 <= K <= MAX_ASSIGN_K:
        raise ValueError(f"the number of centroids must be in 1..{MAX_ASSIGN_K}, got {K}")
    nat.require_device()
    if _is_torch(centroids) and centroids.is_cuda:
        import torch
        c = centroids.detach().to(torch.float32).contiguous()
        out = torch.empty(K, dtype=torch.float32, device=c.device)
        nat.check(nat.lib().vs_centroid_half_norms(_ptr(c), V, K, V, 1 if round_f16 else 0, _ptr(out), int(device), current_stream(int(device))))
        return out
    c = np.ascontiguousarray(_host(centroids), dtype=np.float32)
    out = np.empty(K, dtype=np.float32)
    nat.check(nat.lib().vs_centroid_half_norms(_ptr(c), V, K, V, 1 if round_f16 else 0, _ptr(out), int(device), None))
    return out


def _label_values(values):
    """values of a label-bitmap call -> (int32 ndarray [B], scalar?)"""
    scalar = isinstance(values, (int, np.integer)) and not isinstance(values, bool)
    v = np.atleast_1d(np.asarray(_host(values.detach().cpu()) if _is_torch(values) else values))
    if v.ndim != 1:
        raise TypeError("values: an int, or a 1-D sequence of ints")
    if not 1 <= v.shape[0] <= MAX_LABEL_VALUES:
        raise ValueError(f"the number of values must be in 1..{MAX_LABEL_VALUES}, got {v.shape[0]}")
    if v.dtype == np.bool_ or not np.issubdtype(v.dtype, np.integer):
        raise TypeError("values: an int, or a 1-D sequence of ints")
    if v.size and (int(v.min()) < -0x80000000 or int(v.max()) > 0x7FFFFFFF):
        raise ValueError("a value does not fit an int32 label")
    return np.ascontiguousarray(v, dtype=np.int32), scalar


def label_bitmaps(labels, values, bit0: int = 0, ld_words=None, device: int = 0):
    """Per value the bitmap of the rows that carry it (vs_label_bitmaps) -> words int32 [B, ld_words]: bit bit0 + r of row b is set iff
    labels[r] == values[b]; ld_words defaults to the (bit0 + n_rows + 31) // 32 words a bitmap spans.  labels: int32 [n_rows]; numpy in ->
    numpy out (words behind the span are zero), torch CUDA in -> a tensor on `device`, on torch's current stream."""
    vals, _ = _label_values(values)
    if not hasattr(labels, "shape") or len(labels.shape) != 1 or int(labels.shape[0]) < 1:
        raise ValueError("labels must be a non-empty 1-D array")
    n, B = int(labels.shape[0]), int(vals.shape[0])
    if isinstance(bit0, bool) or not isinstance(bit0, (int, np.integer)) or bit0 < 0:
        raise ValueError(f"bit0 must be an int >= 0, got {bit0!r}")
    span = (int(bit0) + n + 31) // 32
    ld = span if ld_words is None else int(ld_words)
    if ld < span:
        raise ValueError(f"ld_words = {ld} is shorter than the {span} words a bitmap spans")
    nat.require_device()
    if _is_torch(labels) and labels.is_cuda:
        import torch
        l = labels.detach().to(torch.int32).contiguous()
        v = torch.from_numpy(vals).to(l.device)
        out = torch.zeros((B, ld), dtype=torch.int32, device=l.device) if ld > span else torch.empty((B, ld), dtype=torch.int32, device=l.device)
        nat.check(nat.lib().vs_label_bitmaps(_ptr(l), n, _ptr(v), B, int(bit0), _ptr(out), ld, int(device), current_stream(int(device))))
        return out
    l = np.ascontiguousarray(_host(labels), dtype=np.int32)
    out = np.zeros((B, ld), dtype=np.int32)
    nat.check(nat.lib().vs_label_bitmaps(_ptr(l), n, _ptr(vals), B, int(bit0), _ptr(out), ld, int(device), None))
    return out


# ---- numeric fields: range filters, stats, histograms and sort by value (vs_value_range_bitmaps, vs_value_stats, vs_value_histogram, vs_value_topk)
MAX_VALUE_RANGES, MAX_VALUE_EDGES, MAX_VALUE_TOPK = nat.VALUE_MAX_RANGES, nat.VALUE_MAX_EDGES, nat.VALUE_MAX_TOPK
INT32_MISSING = -0x80000000                              # the missing sentinel of an int32 field (a float field's is NaN)


class ValueStats(NamedTuple):
    """value_stats: per query, count = the documents of the set that have a value, missing = those without one (count + missing = the size
    of the set); min / max in the field's type (the missing sentinel -- NaN / INT32_MIN -- when count is 0); sum int64: the exact sum of an
    int32 field, the sum of round(clamp(v, +-2^20) * 2^24) of a float field (the fixed point of the term sums), modulo 2^64."""
    count: Any
    missing: Any
    min: Any
    max: Any
    sum: Any

    def mean(self):
        """the mean value per query in fp64 (NaN for a set without values)"""
        is_t = _is_torch(self.sum)
        s, c = (self.sum.cpu().numpy(), self.count.cpu().numpy()) if is_t else (np.asarray(self.sum), np.asarray(self.count))
        mn = self.min.cpu().numpy() if is_t else np.asarray(self.min)
        scale = 2.0 ** -nat.TERM_FX_SHIFT if mn.dtype.kind == "f" else 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.where(c > 0, s.astype(np.float64) * scale / c.astype(np.float64), np.nan)
        if is_t:
            import torch
            return torch.from_numpy(m).to(self.sum.device)
        return m


class ValueHistogram(NamedTuple):
    """histogram: counts int64 [B, E - 1] -- bin i holds edges[i] <= v < edges[i + 1]; below: v < edges[0]; above: v >= edges[E - 1]; missing:
    documents of the set without a value; total = counts.sum(1) + below + above + missing, the size of the set."""
    counts: Any
    below: Any
    above: Any
    missing: Any
    total: Any


class SortedResults(NamedTuple):
    """top_by_value / value_topk: per query the k documents of the set with the largest (descending) or smallest values, ties by id
    ascending: ids int64 [B, k], values [B, k] in the field's type; id -1 / the missing sentinel behind the last."""
    ids: Any
    values: Any


def value_plan(n_rows: int, B: int, n_bins: int, per_query: bool, rows_per_chunk: int = 0):
    """The launch vs_value_stats / vs_value_histogram take for these arguments (vs_value_plan; pure host arithmetic, no GPU needed) ->
    (qt, chunks, rows_per_chunk): qt = queries a workgroup serves; n_bins = n_edges + 2 for a histogram, 0 for stats."""
    qt, chunks, rpc = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_value_plan(int(n_rows), int(B), int(n_bins), 1 if per_query else 0, int(rows_per_chunk), C.byref(qt), C.byref(chunks),
                                      C.byref(rpc)))
    return qt.value, chunks.value, rpc.value


def value_column(values, missing=None, what="values"):
    """The values of a numeric field -> a contiguous 1-D ndarray, int32 or float32, with the missing sentinel written in.  Integer input
    becomes int32: a value outside [-2^31 + 1, 2^31 - 1] raises (INT32_MIN is the sentinel: say missing=).  Floating input becomes float32
    and NaN means missing.  missing: optional bool mask [n] of the documents without a value.  Host logic only."""
    v = values.detach().cpu().numpy() if _is_torch(values) else np.asarray(values)
    v = np.atleast_1d(v)
    if v.ndim != 1:
        raise ValueError(f"{what} must be 1-D (one value per document), got {v.ndim} dimensions")
    if v.dtype == np.bool_ or v.dtype.kind not in "iuf":
        raise TypeError(f"{what} must be integers or floats, got {v.dtype}")
    m = None
    if missing is not None:
        m = missing.detach().cpu().numpy() if _is_torch(missing) else np.asarray(missing)
        if m.dtype != np.bool_ or m.shape != v.shape:
            raise ValueError(f"missing must be a bool mask of shape {v.shape}, got {m.dtype} {m.shape}")
        v = np.where(m, v.dtype.type(0), v)                       # (what a masked entry holds is not looked at)
    if v.dtype.kind in "iu":
        if v.size and (int(v.min()) <= INT32_MISSING or int(v.max()) > 0x7FFFFFFF):
            raise ValueError(f"{what}: an integer field holds [-2^31 + 1, 2^31 - 1] (-2^31 marks a missing value: pass missing=)")
        out = v.astype(np.int32)
    else:
        with np.errstate(over="ignore"):
            out = v.astype(np.float32)
    if m is not None:
        out[m] = INT32_MISSING if out.dtype == np.int32 else np.nan
    return np.ascontiguousarray(out)


def _value_dtype(values):
    """numpy / torch values -> VS_VAL_F32 or VS_VAL_I32 (TypeError for anything else: value_column converts)"""
    dt = str(values.dtype).replace("torch.", "")
    if dt == "float32":
        return nat.VAL_F32
    if dt == "int32":
        return nat.VAL_I32
    raise TypeError(f"a value column is float32 or int32 (value_column() converts), got {values.dtype}")


def _value_args(values, n_rows, rows_per_chunk=0):
    """Argument checks of a value call that need no device -> (vs dtype, rows_per_chunk)"""
    if isinstance(rows_per_chunk, bool) or not isinstance(rows_per_chunk, (int, np.integer)):
        raise TypeError(f"rows_per_chunk must be an int, got {type(rows_per_chunk).__name__}")
    if rows_per_chunk < 0 or rows_per_chunk % 64:
        raise ValueError(f"rows_per_chunk must be 0 (automatic) or a positive multiple of 64, got {rows_per_chunk}")
    if not hasattr(values, "shape") or len(values.shape) != 1 or int(values.shape[0]) != int(n_rows):
        raise ValueError(f"values must hold one entry per row ({int(n_rows)}), got shape {tuple(getattr(values, 'shape', ()))}")
    return _value_dtype(values), int(rows_per_chunk)


def _np_value_dtype(dt):
    return np.float32 if dt == nat.VAL_F32 else np.int32


def _value_bounds(lo, hi, dt):
    """lo / hi of a range (None = an open end; scalars, or sequences of B) -> (lo [B], hi [B] in the field's type, scalar?).  A bound that is
    missing (NaN), or an integer bound outside the field's range, raises."""
    npdt = _np_value_dtype(dt)
    open_lo, open_hi = (-np.inf, np.inf) if dt == nat.VAL_F32 else (INT32_MISSING + 1, 0x7FFFFFFF)
    def one(x, opened, name):
        if x is None:
            return np.asarray([opened]), True
        a = x.detach().cpu().numpy() if _is_torch(x) else np.asarray([opened if e is None else e for e in x] if isinstance(x, (list, tuple)) else x)
        scalar = a.ndim == 0
        a = np.atleast_1d(a)
        if a.ndim != 1 or a.dtype == np.bool_ or a.dtype.kind not in "iuf":
            raise TypeError(f"{name}: a number, None, or a 1-D sequence of them")
        if a.dtype.kind == "f" and np.isnan(a).any():
            raise ValueError(f"{name}: NaN is no bound (None is an open end)")
        if dt == nat.VAL_I32:
            if a.dtype.kind == "f":                               # lo <= v over integers v: round the bound inwards
                a = np.ceil(a) if name == "lo" else np.floor(a)
                a = np.where(np.isinf(a), np.where(a < 0, open_lo, open_hi), a)      # (+-inf: an open end)
            if (a < open_lo).any() or (a > open_hi).any():
                raise ValueError(f"{name}: a bound of an integer field lies in [-2^31 + 1, 2^31 - 1] (None is an open end)")
            a = a.astype(np.int64)
        return a, scalar
    l, sl = one(lo, open_lo, "lo")
    h, sh = one(hi, open_hi, "hi")
    B = max(l.shape[0], h.shape[0])
    if l.shape[0] not in (1, B) or h.shape[0] not in (1, B):
        raise ValueError(f"lo holds {l.shape[0]} bounds, hi {h.shape[0]}")
    if not 1 <= B <= MAX_VALUE_RANGES:
        raise ValueError(f"the number of ranges must be in 1..{MAX_VALUE_RANGES}, got {B}")
    with np.errstate(over="ignore"):
        l, h = np.broadcast_to(l, (B,)).astype(npdt), np.broadcast_to(h, (B,)).astype(npdt)
    return np.ascontiguousarray(l), np.ascontiguousarray(h), sl and sh


def _value_edges(edges, dt):
    """edges of a histogram -> ndarray [E] in the field's type: 2..1025 of them, strictly ascending, none missing"""
    e = edges.detach().cpu().numpy() if _is_torch(edges) else np.asarray(edges)
    if e.ndim != 1 or e.dtype == np.bool_ or e.dtype.kind not in "iuf":
        raise TypeError("edges: a 1-D sequence of numbers")
    if not 2 <= e.shape[0] <= MAX_VALUE_EDGES:
        raise ValueError(f"a histogram takes 2..{MAX_VALUE_EDGES} edges, got {e.shape[0]}")
    if e.dtype.kind == "f" and np.isnan(e).any():
        raise ValueError("edges: NaN is no edge")
    if dt == nat.VAL_I32:
        if e.dtype.kind == "f" and (e != np.floor(e)).any():
            raise ValueError("edges of an integer field must be integers")
        if int(e.min()) <= INT32_MISSING or int(e.max()) > 0x7FFFFFFF:
            raise ValueError("edges of an integer field lie in [-2^31 + 1, 2^31 - 1]")
    with np.errstate(over="ignore"):
        out = np.ascontiguousarray(e.astype(_np_value_dtype(dt)))
    if not (out[1:] > out[:-1]).all():
        raise ValueError("edges must be strictly ascending (in the field's type)")
    return out


def _value_topk_args(k, descending=True):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"k must be an int, got {type(k).__name__}")
    if not 1 <= int(k) <= MAX_VALUE_TOPK:
        raise ValueError(f"k must be in 1..{MAX_VALUE_TOPK}, got {int(k)}")
    return int(k), 1 if descending else 0


def _values_on(values, device: int):
    """values (numpy / torch, float32 or int32) -> contiguous tensor on GPU `device` (the tensor itself when it is one already)"""
    import torch
    t = values.detach() if _is_torch(values) else torch.from_numpy(np.ascontiguousarray(values))
    return t.to(torch.device("cuda", device)).contiguous()


def _value_keys(t):
    """The uint32 order keys of a float32 / int32 tensor, as int64 (0 = missing): the rule of value_check.h, for merging shard results"""
    import torch
    u = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if t.dtype == torch.int32:
        return u ^ 0x80000000
    mag = u & 0x7FFFFFFF
    u = torch.where(mag == 0, torch.zeros_like(u), u)
    key = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
    return torch.where(mag > 0x7F800000, torch.zeros_like(key), key)


def value_range_bitmaps(values, lo, hi, bit0: int = 0, ld_words=None, device: int = 0):
    """Per range the bitmap of the rows whose value lies in it (vs_value_range_bitmaps) -> words int32 [B, ld_words]: bit bit0 + r of row b
    is set iff row r has a value and lo[b] <= v <= hi[b]; None is an open end.  values: float32 / int32 [n_rows]; numpy in -> numpy out
    (words behind the span are zero), torch CUDA in -> a tensor on `device`, on torch's current stream."""
    if not hasattr(values, "shape") or len(values.shape) != 1 or int(values.shape[0]) < 1:
        raise ValueError("values must be a non-empty 1-D array")
    dt = _value_dtype(values)
    l, h, _ = _value_bounds(lo, hi, dt)
    n, B = int(values.shape[0]), int(l.shape[0])
    if isinstance(bit0, bool) or not isinstance(bit0, (int, np.integer)) or bit0 < 0:
        raise ValueError(f"bit0 must be an int >= 0, got {bit0!r}")
    span = (int(bit0) + n + 31) // 32
    ld = span if ld_words is None else int(ld_words)
    if ld < span:
        raise ValueError(f"ld_words = {ld} is shorter than the {span} words a bitmap spans")
    nat.require_device()
    if _is_torch(values) and values.is_cuda:
        import torch
        v = values.detach().contiguous()
        ld_, hd_ = torch.from_numpy(np.stack([l, h])).to(v.device)                  # (one upload for both bounds)
        out = torch.zeros((B, ld), dtype=torch.int32, device=v.device) if ld > span else torch.empty((B, ld), dtype=torch.int32, device=v.device)
        nat.check(nat.lib().vs_value_range_bitmaps(_ptr(v), dt, n, _ptr(ld_), _ptr(hd_), B, int(bit0), _ptr(out), ld, int(device),
                                                   current_stream(int(device))))
        return out
    v = np.ascontiguousarray(_host(values))
    out = np.zeros((B, ld), dtype=np.int32)
    nat.check(nat.lib().vs_value_range_bitmaps(_ptr(v), dt, n, _ptr(l), _ptr(h), B, int(bit0), _ptr(out), ld, int(device), None))
    return out


def _doc_set(filter, n_rows, device):
    """filter= of an aggregation -> None or a DocFilter on `device`"""
    if filter is None:
        return None
    from .doc_filter import as_doc_filter
    return as_doc_filter(filter, n_rows, device=device)


_value_set = _doc_set                                  # (its name before every aggregation used it)


def _set_args(f, bit0):
    """the set of a raw call -> (B, (words, bit0, ld_words, B)): f None (every live row) or a DocFilter on the call's GPU, read from bit `bit0` on"""
    B = f.n_queries if (f is not None and f.per_query) else 1
    return B, (_ptr(f.words) if f is not None else None, int(bit0), f.ld if f is not None else 0, B)


# ---- breakdowns: a numeric field's stats and histogram per facet label (vs_facet_value_stats, vs_facet_value_histogram) ---------------------
class FacetValueStats(NamedTuple):
    """facet_value_stats: per (query, label) the ValueStats of the set's documents with that label -- count, missing, sum int64 [B, L], min /
    max [B, L] in the field's type (the missing sentinel where count is 0) -- with the size of the set (total [B]) and its documents whose
    label is outside [0, L) (other [B]): count.sum(1) + missing.sum(1) + other == total, and count + missing is facet_counts' counts."""
    count: Any
    missing: Any
    min: Any
    max: Any
    sum: Any
    total: Any
    other: Any

    def mean(self):
        """the mean value per (query, label) in fp64 (NaN for a cell without values)"""
        return ValueStats(self.count, self.missing, self.min, self.max, self.sum).mean()


class FacetValueHistogram(NamedTuple):
    """facet_value_histogram: counts int64 [B, L, E - 1] -- bin i of (b, l) holds the set's documents with label l and edges[i] <= v <
    edges[i + 1]; below / above / missing int64 [B, L] as in ValueHistogram; total / other int64 [B] as in FacetCounts: counts.sum((1, 2)) +
    below.sum(1) + above.sum(1) + missing.sum(1) + other == total."""
    counts: Any
    below: Any
    above: Any
    missing: Any
    total: Any
    other: Any


def facet_value_plan(n_rows: int, B: int, n_labels: int, n_slots: int, per_query: bool, rows_per_chunk: int = 0):
    """The launch vs_facet_value_stats (n_slots = 0) / vs_facet_value_histogram (n_slots = n_edges + 2) take for these arguments
    (vs_facet_value_plan; pure host arithmetic, no GPU needed) -> (regime, qt, chunks, rows_per_chunk): regime 0 = LDS records / bins, 1 =
    global atomics; qt = queries a workgroup serves."""
    regime, qt, chunks, rpc = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_facet_value_plan(int(n_rows), int(B), int(n_labels), int(n_slots), 1 if per_query else 0, int(rows_per_chunk),
                                            C.byref(regime), C.byref(qt), C.byref(chunks), C.byref(rpc)))
    return regime.value, qt.value, chunks.value, rpc.value


def _facet_value_args(labels, n_labels, values, n_rows, rows_per_chunk=0, edges=None):
    """Argument checks of a breakdown that need no device -> (n_labels, vs dtype, rows_per_chunk, edges in the field's type | None)"""
    n_labels, rows_per_chunk = _facet_args(labels, n_labels, n_rows, rows_per_chunk)
    dt, _ = _value_args(values, n_rows, rows_per_chunk)
    e = None
    if edges is not None:
        e = _value_edges(edges, dt)
        if n_labels * (int(e.shape[0]) + 2) > nat.FACET_VALUE_MAX_CELLS:
            raise ValueError(f"n_labels x (n_edges + 2) = {n_labels * (int(e.shape[0]) + 2)} is more than the {nat.FACET_VALUE_MAX_CELLS} cells a query takes")
    return n_labels, dt, rows_per_chunk, e


# ---- percentiles: exact order statistics of a numeric field (vs_value_quantiles, vs_value_radix_counts, vs_value_radix_step) ----------------
MAX_VALUE_RANKS = nat.VALUE_MAX_RANKS
QUANTILE_METHODS = {"lower": nat.QUANTILE_LOWER, "higher": nat.QUANTILE_HIGHER, "nearest": nat.QUANTILE_NEAREST}


class ValueQuantiles(NamedTuple):
    """value_quantiles: per query and rank the order statistic of the set's values -- values [B, R] in the field's type (the missing
    sentinel, NaN / INT32_MIN, where there is no answer), ranks int64 [B, R] the 0-based ascending ranks they stand at (-1: no answer);
    count / missing int64 [B]: the documents of the set with / without a value."""
    values: Any
    ranks: Any
    count: Any
    missing: Any


class ValuePercentiles(NamedTuple):
    """percentiles / median: values [B, P] -- float64 for method "linear" (NaN where there is no answer), else the field's type (the missing
    sentinel there); count / missing int64 [B]: the documents of the set with / without a value."""
    values: Any
    count: Any
    missing: Any


PERCENTILE_METHODS = ("linear", "lower", "higher", "nearest")


def _percentile_args(pcts, method):
    """pcts of percentiles() -> the quantiles q = pcts / 100, float64 [P]; a percentile outside 0..100 or NaN raises"""
    if method not in PERCENTILE_METHODS:
        raise ValueError(f'method must be one of {PERCENTILE_METHODS}, got {method!r}')
    p = np.asarray(pcts.detach().cpu().numpy() if _is_torch(pcts) else pcts)
    if p.dtype == np.bool_ or p.dtype.kind not in "iuf":
        raise TypeError("pcts: a number or a 1-D sequence of numbers in 0..100")
    p = np.atleast_1d(p).astype(np.float64)
    if p.ndim != 1 or p.shape[0] < 1:
        raise ValueError("pcts: a number or a non-empty 1-D sequence of numbers")
    if not ((p >= 0.0) & (p <= 100.0)).all():
        raise ValueError("pcts must lie in 0..100")
    return np.ascontiguousarray(p / 100.0)


def value_quantile_plan(n_rows: int, B: int, R: int, per_query: bool, rows_per_chunk: int = 0):
    """The launch of the counting kernel of vs_value_quantiles for these arguments (vs_value_quantile_plan; pure host arithmetic, no GPU
    needed) -> (qt, chunks, rows_per_chunk): qt = queries a workgroup serves, by the number of ranks R."""
    qt, chunks, rpc = C.c_int32(0), C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_value_quantile_plan(int(n_rows), int(B), int(R), 1 if per_query else 0, int(rows_per_chunk), C.byref(qt), C.byref(chunks),
                                               C.byref(rpc)))
    return qt.value, chunks.value, rpc.value


def _quantile_args(q, method, ranks):
    """Argument checks of a quantile call that need no device -> (q float64 [R] | None, method code, ranks int64 [R] or [B, R] | None)"""
    if (q is None) == (ranks is None):
        raise ValueError("exactly one of q (quantiles in [0, 1]) and ranks (0-based ascending ranks) must be given")
    if method not in QUANTILE_METHODS:
        raise ValueError(f'method must be "lower", "higher" or "nearest", got {method!r}')
    if q is not None:
        a = np.atleast_1d(np.asarray(q.detach().cpu().numpy() if _is_torch(q) else q, dtype=np.float64))
        if a.ndim != 1 or a.shape[0] < 1:
            raise ValueError("q must be a number or a non-empty 1-D sequence of numbers")
        if not ((a >= 0.0) & (a <= 1.0)).all():
            raise ValueError("q must lie in [0, 1]")
        return np.ascontiguousarray(a), QUANTILE_METHODS[method], None
    r = np.asarray(ranks.detach().cpu().numpy() if _is_torch(ranks) else ranks)
    if r.dtype == np.bool_ or r.dtype.kind not in "iu":
        raise TypeError(f"ranks must be integers, got {r.dtype}")
    r = np.atleast_1d(r).astype(np.int64)
    if r.ndim not in (1, 2) or r.shape[-1] < 1:
        raise ValueError("ranks must be a non-empty [R] or [B, R] array")
    if (r < 0).any():
        raise ValueError("ranks must be >= 0 (0-based, ascending)")
    return None, QUANTILE_METHODS[method], np.ascontiguousarray(r)


def _quantile_ranks_for(ranks, B):
    """ranks [R] or [B, R] -> int64 [B, R]"""
    if ranks.ndim == 1:
        return np.ascontiguousarray(np.broadcast_to(ranks[None, :], (B, ranks.shape[0])))
    if ranks.shape[0] != B:
        raise ValueError(f"ranks holds {ranks.shape[0]} rows for {B} queries")
    return ranks


def quantile_lerp(lo, hi, frac):
    """The linear interpolation of ``percentiles(method="linear")`` in fp64: lo + (hi - lo) * frac, and exactly lo where lo == hi (so that
    +-inf does not give NaN).  numpy arrays in, float64 out; a missing end (NaN) gives NaN."""
    lo, hi, frac = np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(frac, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(lo == hi, lo, lo + (hi - lo) * frac)


def value_radix_step(level: int, counts, R: int, state=None, q=None, method: int = 0, ranks=None, dtype=None, device: int = 0):
    """One step of the radix select on a level's counts (vs_value_radix_step; CUDA tensors on `device`, torch's current stream).  counts:
    int64 [B, S, bins], summed over the shards; state: the dict the step of the level above returned (None at level 0); q float64 [R] with
    the method code, or ranks int64 [B, R], at level 0 -> dict(rank_res, rank_slot, rank_prefix, slot_prefix, n_slots) and, from level 0 on,
    count [B] and ranks [B, R]; after level 2, values [B, R] of `dtype`."""
    import torch
    dev = torch.device("cuda", device)
    B = int(counts.shape[0])
    if state is None:
        state = dict(rank_res=torch.empty((B, R), dtype=torch.int64, device=dev), rank_slot=torch.empty((B, R), dtype=torch.int32, device=dev),
                     rank_prefix=torch.empty((B, R), dtype=torch.int32, device=dev), slot_prefix=torch.empty((B, R), dtype=torch.int32, device=dev),
                     n_slots=torch.empty(B, dtype=torch.int32, device=dev), count=torch.empty(B, dtype=torch.int64, device=dev),
                     ranks=torch.empty((B, R), dtype=torch.int64, device=dev))
    last = level == nat.VALUE_RADIX_LEVELS - 1
    if last:
        state["values"] = torch.empty((B, R), dtype=dtype, device=dev)
    counts = counts.contiguous()
    nat.check(nat.lib().vs_value_radix_step(int(level), _ptr(counts), B, int(R), _ptr(q) if q is not None else None, int(method),
                                            _ptr(ranks) if ranks is not None else None, _ptr(state["rank_res"]), _ptr(state["rank_slot"]),
                                            _ptr(state["rank_prefix"]), _ptr(state["slot_prefix"]), _ptr(state["n_slots"]), _ptr(state["count"]),
                                            _ptr(state["ranks"]), _ptr(state["values"]) if last else None,
                                            nat.VAL_F32 if dtype == torch.float32 else nat.VAL_I32, int(device), current_stream(int(device))))
    return state


def _quantile_batches(q, ranks, B, call):
    """more than 16 ranks are served in batches of 16: call(q batch | None, ranks batch | None, R) -> (values, ranks, count, missing)"""
    import torch
    P = q.shape[0] if q is not None else ranks.shape[1]
    parts = []
    for j0 in range(0, P, MAX_VALUE_RANKS):
        j1 = min(P, j0 + MAX_VALUE_RANKS)
        parts.append(call(np.ascontiguousarray(q[j0:j1]) if q is not None else None,
                          np.ascontiguousarray(ranks[:, j0:j1]) if ranks is not None else None, j1 - j0))
    if len(parts) == 1:
        return parts[0]
    return torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts], dim=1), parts[0][2], parts[0][3]


# ---- per-label percentiles: order statistics of a numeric field per facet label (vs_facet_value_quantiles, vs_facet_value_radix_counts) ------
class FacetValueQuantiles(NamedTuple):
    """facet_value_quantiles: per (query, label, rank) the order statistic of the values of the set's documents with that label -- values
    [B, L, R] in the field's type (the missing sentinel where there is no answer), ranks int64 [B, L, R] (-1: no answer); count / missing
    int64 [B, L]: those documents with / without a value; total / other int64 [B] as in FacetCounts: count.sum(1) + missing.sum(1) + other ==
    total."""
    values: Any
    ranks: Any
    count: Any
    missing: Any
    total: Any
    other: Any


class FacetValuePercentiles(NamedTuple):
    """percentiles_by_facet / median_by_facet: values [B, L, P] -- float64 for method "linear" (NaN where there is no answer), else the
    field's type (the missing sentinel there); count / missing int64 [B, L]; total / other int64 [B]."""
    values: Any
    count: Any
    missing: Any
    total: Any
    other: Any


def facet_value_quantile_plan(n_rows: int, B: int, n_labels: int, R: int, level: int, per_query: bool, rows_per_chunk: int = 0):
    """The launch of the counting kernel of vs_facet_value_quantiles at a radix level (vs_facet_value_quantile_plan; pure host arithmetic, no
    GPU needed) -> (regime, qt, tile_labels, label_tiles, chunks, rows_per_chunk): regime 0 = LDS histograms of qt queries x tile_labels labels
    a workgroup, label_tiles tiles; 1 = global atomics."""
    regime, qt, tl, lt, chunks, rpc = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_facet_value_quantile_plan(int(n_rows), int(B), int(n_labels), int(R), int(level), 1 if per_query else 0, int(rows_per_chunk),
                                                     C.byref(regime), C.byref(qt), C.byref(tl), C.byref(lt), C.byref(chunks), C.byref(rpc)))
    return regime.value, qt.value, tl.value, lt.value, chunks.value, rpc.value


def _facet_quantile_args(q, method, ranks, n_labels):
    """Argument checks of a per-label quantile call that need no device -> (q float64 [R] | None, method code, ranks int64 [R] or [B, L, R] |
    None)"""
    if ranks is not None and q is None:
        r = np.asarray(ranks.detach().cpu().numpy() if _is_torch(ranks) else ranks)
        if r.ndim == 3:
            if r.shape[1] != n_labels:
                raise ValueError(f"ranks holds {r.shape[1]} labels for n_labels = {n_labels}")
            _, m, flat = _quantile_args(None, method, r.reshape(-1, r.shape[2]))
            return None, m, flat.reshape(r.shape)
        if r.ndim != 1:
            raise ValueError("ranks must be a non-empty [R] or [B, n_labels, R] array")
        ranks = r
    return _quantile_args(q, method, ranks)


def _facet_quantile_batches(q, ranks, cells, call):
    """The ranks are served in batches of min(16, 65536 // cells) -- cells = B x n_labels; 65536 x 2048 bins are the 2^27 counts of a call:
    call(q batch | None, ranks batch [B, L, Rb] | None, Rb) -> the six tensors"""
    import torch
    P = q.shape[0] if q is not None else ranks.shape[2]
    step = max(1, min(MAX_VALUE_RANKS, (1 << 16) // max(cells, 1)))
    parts = []
    for j0 in range(0, P, step):
        j1 = min(P, j0 + step)
        parts.append(call(np.ascontiguousarray(q[j0:j1]) if q is not None else None,
                          np.ascontiguousarray(ranks[:, :, j0:j1]) if ranks is not None else None, j1 - j0))
    if len(parts) == 1:
        return parts[0]
    return (torch.cat([p[0] for p in parts], dim=2), torch.cat([p[1] for p in parts], dim=2)) + tuple(parts[0][2:])


KMEANS_UPDATE_BATCH = 64                               # clusters a term_sums call took when the update went through from_labels (kept: callers batch by it)
KMEANS_METRICS = ("dot", "l2")


class KMeansResult(NamedTuple):
    """kmeans / cluster: centroids float32 [K, V]; labels int32 [N] and values float32 [N], the assignment UNDER these centroids (-1 / -inf
    for a deleted or filtered-out document); counts int64 [K], the documents of each cluster; n_iter, the iterations run; changed, per
    iteration the documents whose label differed from the previous assignment (the first entry: the documents assigned)."""
    centroids: Any
    labels: Any
    values: Any
    counts: Any
    n_iter: int
    changed: list


def _kmeans_args(n_clusters, iters, metric, init=None, n_cols=None):
    """Argument checks of kmeans that need no device -> (K, iters).  init: None, int64 row ids [K] or float32 centroids [K, V]."""
    for name, v in (("n_clusters", n_clusters), ("iters", iters)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
    K, iters = int(n_clusters), int(iters)
    if not 1 <= K <= MAX_ASSIGN_K:
        raise ValueError(f"n_clusters must be in 1..{MAX_ASSIGN_K}, got {K}")
    if iters < 0:
        raise ValueError(f"iters must be >= 0, got {iters}")
    if metric not in KMEANS_METRICS:
        raise ValueError(f'metric must be "dot" or "l2", got {metric!r}')
    if init is not None:
        if not hasattr(init, "shape") or len(init.shape) not in (1, 2) or int(init.shape[0]) != K:
            raise ValueError(f"init must be {K} row ids [K] or {K} centroids [K, V]")
        floating = init.is_floating_point() if _is_torch(init) else np.issubdtype(np.asarray(init).dtype, np.floating)
        if len(init.shape) == 1 and floating:
            raise TypeError("init row ids must be integers")
        if len(init.shape) == 2:
            if not floating:
                raise TypeError("init centroids must be floating point")
            if n_cols is not None and int(init.shape[1]) != int(n_cols):
                raise ValueError(f"init centroids have {int(init.shape[1])} columns, the index has {int(n_cols)}")
            on_gpu = _is_torch(init) and init.is_cuda
            if not on_gpu and not bool(np.isfinite(_host(init) if _is_torch(init) else np.asarray(init)).all()):
                raise ValueError("init centroids must be finite")
    return K, iters


def kmeans_loop(target, centroids, iters: int, metric: str = "l2", filter=None):
    """Lloyd's iteration over the rows of `target` (a DeviceIndex or a ShardGroup) from float32 start centroids [K, V] on its GPU ->
    (centroids, labels, values, n_iter, changed).  Per iteration: bias = -half_norms(C) under "l2" (none under "dot"); labels, values =
    assign(C, bias, filter); changed = the rows whose label differs from the previous assignment (first: the rows assigned); stop when
    nothing changed; else C = label_term_sums(labels, K, filter).mean() -- the sums of all K clusters in one pass, bit for bit those of
    term_sums(filter=from_labels(labels, [j]) & filter) -- where the cluster has rows; an empty cluster keeps its centroid.  Where K x V is
    more than the 2^27 cells of one call (label_term_slices) the update takes a slice of the clusters a pass: any K <= 4096 serves at any V.  The labels returned are the assignment under the centroids returned (one
    closing assign when the loop ends on `iters`).  Deterministic: every step is pinned bit for bit."""
    import torch
    dev = torch.device("cuda", target.device)
    C_ = centroids.detach().to(dev).to(torch.float32).contiguous().clone()
    K = int(C_.shape[0])

    def step():
        bias = -target.half_norms(C_) if metric == "l2" else None
        return target.assign(C_, bias=bias, filter=filter)

    prev, changed, stale = None, [], True
    for _ in range(int(iters)):
        cur = step()
        stale = False
        n_changed = int((cur.labels >= 0).sum()) if prev is None else int((cur.labels != prev.labels).sum())
        changed.append(n_changed)
        prev = cur
        if n_changed == 0:
            break
        for l0, n in label_term_slices(K, int(C_.shape[1])):          # all K clusters in one pass (a row outside the filter carries -1) -- a
            lab = cur.labels if n == K else cur.labels - l0           # slice a pass where K x V is more than one call's 2^27 cells
            ts = target.label_term_sums(lab, n, filter=filter)
            C_[l0:l0 + n] = torch.where((ts.total > 0).reshape(-1, 1), ts.mean(), C_[l0:l0 + n])
        stale = True
    if stale:
        prev = step()
    return C_, prev.labels, prev.values, len(changed), changed


def _host(x):
    return x.detach().numpy() if _is_torch(x) else x


def _numel(x):
    return int(x.numel()) if _is_torch(x) else int(x.size)


def _n_cols_of(obj) -> int:
    return obj._n_cols() if isinstance(obj, DeviceIndex) else int(obj._shards[0].info().n_cols)


def _candidate_row_ends(obj, flat_ids):
    """indptr int64 [n + 1] (on the device) of the compact rows of flat_ids: the sizing pass of get_rows alone"""
    import torch
    n = int(flat_ids.shape[0])
    indptr = torch.empty(n + 1, dtype=torch.int64, device=flat_ids.device)
    if isinstance(obj, ShardGroup):
        nat.check(nat.lib().vs_shard_group_get_rows(obj._h, _ptr(flat_ids), n, _ptr(indptr), None, None))
    else:
        nat.check(nat.lib().vs_index_get_rows(obj._h, _ptr(flat_ids), n, 0, _ptr(indptr), None, None, current_stream(obj.device)))
    return indptr


def _diversify(obj, ids, scores, k, lam, sim, max_row_bytes=None, chunks_out=None):
    """MMR over the hit lists ids / scores [B, kk] with the rows obj stores: the batch is cut into runs of queries whose
    candidate rows (8 bytes a non-zero, sized by the first pass of get_rows) stay under max_row_bytes -- a run is never shorter than one
    query --, and every run is get_rows -> vs_mmr_select_csr.  obj: a DeviceIndex or a ShardGroup.  chunks_out: a list that receives the
    number of runs (tests, tools/probe_mmr.py)."""
    import torch
    k, _, mode = _diverse_args(k, None, sim)
    if not hasattr(ids, "ndim") or ids.ndim != 2 or tuple(scores.shape) != tuple(ids.shape):
        raise ValueError("ids and scores must be [B, kk] arrays of one shape")
    B, kk = int(ids.shape[0]), int(ids.shape[1])
    if not 1 <= kk <= MAX_MMR_DEPTH:
        raise ValueError(f"a hit list must hold 1..{MAX_MMR_DEPTH} candidates, got {kk}")
    if k > MAX_MMR_DEPTH:
        raise ValueError(f"k must be at most {MAX_MMR_DEPTH}, got {k}")
    _int64_ids(ids, 2)
    lam_h = _lam_array(lam, B)
    max_row_bytes = DEFAULT_MMR_ROW_BYTES if max_row_bytes is None else int(max_row_bytes)
    if max_row_bytes < 1:
        raise ValueError(f"max_row_bytes must be positive, got {max_row_bytes}")
    nat.require_device()
    device = int(obj.device)
    dev = torch.device("cuda", device)
    V = _n_cols_of(obj)
    if V > nat.MMR_MAX_COLS:
        raise NotImplementedError(f"the index has {V} columns, diversified search serves at most {nat.MMR_MAX_COLS}")
    sharded = isinstance(obj, ShardGroup)
    host_kind = None if (_is_torch(ids) and ids.is_cuda) else ("torch" if _is_torch(ids) else "numpy")
    as_t = lambda x: x if _is_torch(x) else torch.from_numpy(np.ascontiguousarray(x))
    ids_d = as_t(ids).to(dev).contiguous()
    sc_d = as_t(scores).to(dev).to(torch.float32).contiguous()
    out = tuple(torch.empty((B, k), dtype=dt, device=dev) for dt in (torch.int64, torch.float32, torch.int32, torch.float32, torch.float32))
    flat = ids_d.reshape(-1)
    sync = torch.cuda.current_stream(device).synchronize
    if sharded:
        sync()                                                           # (the group runs on its own streams)
    ends = _candidate_row_ends(obj, flat)
    per_query = ((ends[kk::kk] - ends[:-1:kk]) * 8).tolist()             # bytes of each query's candidate rows (synchronises)
    runs, b0, held = [], 0, 0
    for b, nbytes in enumerate(per_query):
        if b > b0 and held + nbytes > max_row_bytes:
            runs.append((b0, b))
            b0, held = b, 0
        held += nbytes
    runs.append((b0, B))
    for b0, b1 in runs:
        if sharded:
            sync()
        indptr, indices, values = obj.get_rows(flat[b0 * kk:b1 * kk])
        mmr_select(indptr, indices, values, ids_d[b0:b1], sc_d[b0:b1], k, lam_h[b0:b1], sim, V, device, out=tuple(o[b0:b1] for o in out))
    if chunks_out is not None:
        chunks_out.append(len(runs))
    res = DiverseResults(*out[:4])
    if host_kind is not None:
        sync()
        res = DiverseResults(*(t.cpu() if host_kind == "torch" else t.cpu().numpy() for t in res))
    return res


def _search_diverse(obj, q, k, lam=0.5, depth=None, sim="cosine", filter=None, max_row_bytes=None, chunks_out=None):
    """search(q, depth, filter=) -> _diversify of its lists.  depth defaults to min(n_rows, 1024, max(4 k, k + 16)): a starting point, not
    a measured optimum.  Deleted rows and the filter act through the search.  obj: a DeviceIndex or a ShardGroup."""
    import torch
    k, depth, _ = _diverse_args(k, depth, sim)
    if q.ndim != 2:
        raise ValueError("queries must be [B, V]")
    _lam_array(lam, int(q.shape[0]))                                     # (argument errors before any device work)
    if depth is None:
        depth = max(k, min(int(obj.n_rows), MAX_MMR_DEPTH, max(4 * k, k + 16)))      # (k > n_rows: the search raises as it does for any query)
        if depth > MAX_MMR_DEPTH:
            raise ValueError(f"k must be at most {MAX_MMR_DEPTH} (the deepest candidate list), got {k}")
    nat.require_device()
    device = int(obj.device)
    as_numpy = not _is_torch(q)
    on_host = as_numpy or not q.is_cuda
    qd = (torch.from_numpy(np.ascontiguousarray(q)) if as_numpy else q).to(torch.device("cuda", device))
    if isinstance(obj, ShardGroup):
        torch.cuda.current_stream(device).synchronize()
    ids, sc = obj.search(qd, depth, filter=filter)
    res = _diversify(obj, ids, sc, k, lam, sim, max_row_bytes, chunks_out)
    if on_host:
        torch.cuda.current_stream(device).synchronize()
        res = DiverseResults(*(t.cpu().numpy() if as_numpy else t.cpu() for t in res))
    return res


def _queries_from_rows(call, ids, weights, q, alpha, B, m, V, device, stream):
    """the shared body of DeviceIndex / ShardGroup .queries_from_rows: call(ids, B, m, ld_ids, w, ldw, q, q_dtype, ldq, alpha, out, ldo[, stream])"""
    p_ids, _, k1 = as_arg(ids, (nat.VS_I64,))
    p_w, _, k2 = as_arg(weights, (nat.VS_F32,))
    p_q, dt, k3 = as_arg(q, (nat.VS_F32, nat.VS_F16))
    ldq = int(q.shape[1]) if q is not None else 0
    if q is None:
        dt = nat.VS_F32
    if device is not None:
        import torch
        out = torch.empty((B, V), dtype=torch.float32, device=torch.device("cuda", device))
        args = (p_ids, B, m, m, p_w, m, p_q, dt, ldq, float(alpha), C.c_void_p(out.data_ptr()), V)
        nat.check(call(*args, current_stream(device)) if stream else call(*args))
        return out
    out = np.empty((B, V), dtype=np.float32)
    args = (p_ids, B, m, m, p_w, m, p_q, dt, ldq, float(alpha), C.c_void_p(out.ctypes.data), V)
    nat.check(call(*args, None) if stream else call(*args))
    if _is_torch(ids) or _is_torch(q) or _is_torch(weights):
        import torch
        return torch.from_numpy(out)
    return out

def _term_args(cols, thr=None):
    """Terms of term_bitmaps() / doc_freq() -> (int32 [T] columns, float32 [T] thresholds or None).  cols: integer column ids (a
    list / ndarray / tensor, or one int); thr: None, a dict {column: threshold}, or one threshold per term (None / NaN: no threshold).
    Pure host work: argument errors come before any device work."""
    if _is_torch(cols):
        cols = cols.detach().cpu().numpy()
    c = np.atleast_1d(np.asarray(cols))
    if c.ndim != 1 or c.size == 0:
        raise ValueError("cols must be a non-empty 1-D list of column ids")
    if c.dtype == np.bool_ or not np.issubdtype(c.dtype, np.integer):
        raise TypeError(f"cols must be integer column ids, got {c.dtype}")
    if c.size > nat.TERM_FILTER_TERMS:
        raise ValueError(f"at most {nat.TERM_FILTER_TERMS} terms a call, got {c.size}")
    if int(c.min()) < 0 or int(c.max()) > 0x7FFFFFFF:
        raise ValueError(f"column {int(c.min()) if int(c.min()) < 0 else int(c.max())} is not a column of the index")
    c = np.ascontiguousarray(c, dtype=np.int32)
    if thr is None:
        return c, None
    if isinstance(thr, dict):
        t = np.array([float(thr.get(int(x), np.nan)) for x in c], dtype=np.float32)
    else:
        if _is_torch(thr):
            thr = thr.detach().cpu().numpy()
        t = np.array([np.nan if x is None else float(x) for x in np.atleast_1d(np.asarray(thr, dtype=object))], dtype=np.float32)
        if t.shape != c.shape:
            raise ValueError(f"thr has {t.size} entries, cols {c.size}")
    return c, (None if bool(np.isnan(t).all()) else np.ascontiguousarray(t))


def _term_bitmaps(call, n_rows, n_cols, device, cols, thr, want_df=False, live_only=True, ld=None, stream=True):
    """the shared body of DeviceIndex / ShardGroup .term_bitmaps / .doc_freq: call(cols, thr, T, words, ld, df, live_only[, stream])
    -> (int32 CUDA tensor [T, ld], int64 CUDA tensor [T] or None)"""
    import torch
    c, t = _term_args(cols, thr)
    if int(c.max()) >= n_cols:
        raise ValueError(f"column {int(c.max())} is outside [0, {n_cols})")
    nat.require_device()
    T, W = int(c.shape[0]), (int(n_rows) + 31) // 32
    ld = W if ld is None else int(ld)
    dev = torch.device("cuda", device)
    words = torch.zeros((T, max(ld, 1)), dtype=torch.int32, device=dev) if ld > W else torch.empty((T, max(ld, 1)), dtype=torch.int32, device=dev)
    df = torch.zeros(T, dtype=torch.int64, device=dev) if want_df else None
    args = (C.c_void_p(c.ctypes.data), C.c_void_p(t.ctypes.data) if t is not None else None, T, C.c_void_p(words.data_ptr()), ld,
            C.c_void_p(df.data_ptr()) if want_df else None, 1 if live_only else 0)
    if stream:
        nat.check(call(*args, current_stream(device)))
    else:
        torch.cuda.current_stream(device).synchronize()             # (the group runs on its own streams)
        nat.check(call(*args))
    return words, df


# ---- aggregations, each written once over the parts of obj: a DeviceIndex is one part at row 0, a ShardGroup one part a shard ---------------------
# A feature is a raw call (DeviceIndex._*_call), a merge rule (_add_parts, _merge_stats, torch.cat, _merge_value_topk) and a function below.
def _lab(labels):
    """a label column of _shard_parts: (conversion, kind, array)"""
    return _labels_on, "labels", labels


def _val(values):
    """a value column of _shard_parts"""
    return _values_on, "values", values


def _shard_parts(obj, filter, columns, call, n_rows=None):
    """call(shard, *its slices of the per-row columns, its filter, its first row) for every part of obj -> the parts' tuples on obj's GPU.
    filter: filter= as given (resolved once, on obj's GPU; n_rows: obj.n_rows where the caller has it) -- a part's rows are bits [row0,
    row0 + n) of it; columns: (conversion, kind, array) each (``_lab``, ``_val``).  A part on obj's GPU is returned as the call made it."""
    dev = obj.device
    f = None if filter is None else _doc_set(filter, obj.n_rows if n_rows is None else n_rows, dev)
    out = []
    for (sh, row0), *xs in zip(obj._parts, *[obj._slices(*c) for c in columns]):
        part = call(sh, *xs, f if f is None else f.to(sh.device), row0)
        out.append(part if sh.device == dev else tuple(t.to(f"cuda:{dev}") for t in part))
    return out


def _add_parts(parts):
    """the parts' integer tensors (counts, sums, histograms) added field by field; one part is returned as it is"""
    return parts[0] if len(parts) == 1 else tuple(sum(x[1:], x[0]) for x in zip(*parts))


def _merge_stats(parts):
    """the parts' (count, missing, min, max, *sums), [B] or [B, L] alike -> one: the integers added, min and max taken on the order keys (an
    int32 value never passes through a float) among the parts whose count is not 0; one part is returned as it is"""
    if len(parts) == 1:
        return parts[0]
    import torch
    count, lo, hi = (torch.stack([p[i] for p in parts]) for i in (0, 2, 3))
    has = count > 0
    klo = torch.where(has, _value_keys(lo), torch.full_like(count, 1 << 32))
    khi = torch.where(has, _value_keys(hi), torch.zeros_like(count))
    added = _add_parts([p[:2] + p[4:] for p in parts])
    return added[:2] + (lo.gather(0, klo.argmin(0, keepdim=True))[0], hi.gather(0, khi.argmax(0, keepdim=True))[0]) + added[2:]


def _merge_value_topk(parts, k, descending):
    """the shards' (ids, values) lists [B, k], each with its id offset -> the k best by (order key, id)"""
    import torch
    ids, vals = (torch.cat(x, dim=1) for x in zip(*parts))                          # [B, S * k]: ids ascend from shard to shard
    key = _value_keys(vals)
    key = torch.where(ids < 0, torch.full_like(key, -1), key if descending else 0xFFFFFFFF - key)
    # a shard's list is in (key descending, id ascending) order and the shards' id ranges ascend: order by id first, then -- stably -- by key
    by_id = torch.where(ids < 0, torch.full_like(ids, 1 << 62), ids).argsort(dim=1, stable=True)
    order = by_id.gather(1, key.gather(1, by_id).argsort(dim=1, descending=True, stable=True))[:, :k]
    return ids.gather(1, order), vals.gather(1, order)


def _facet_sums(obj, labels, n_labels, filter, rows_per_chunk):
    n = obj.n_rows
    n_labels, rows_per_chunk = _facet_args(labels, n_labels, n, rows_per_chunk)
    nat.require_device()
    return _add_parts(_shard_parts(obj, filter, (_lab(labels),), lambda sh, l, f, row0: sh._facet_call(l, n_labels, f, row0, rows_per_chunk), n))


def _facet_counts(obj, labels, n_labels, filter, rows_per_chunk):
    return FacetCounts(*_facet_out(labels, *_facet_sums(obj, labels, n_labels, filter, rows_per_chunk)))


def _top_facets(obj, labels, n_labels, topn, filter, min_count):
    topn, min_count = _topn_args(topn, min_count)
    counts, total, other = _facet_sums(obj, labels, n_labels, filter, 0)
    top_l, top_c = facet_topn(counts, topn, min_count, device=obj.device)
    return TopFacets(*_facet_out(labels, top_l, top_c, total, other))


def _value_range_filter(obj, values, lo, hi):
    import torch
    from .doc_filter import DocFilter
    n = obj.n_rows
    dt, _ = _value_args(values, n)
    l, _, scalar = _value_bounds(lo, hi, dt)
    nat.require_device()
    parts = _shard_parts(obj, None, (_val(values),), lambda sh, v, f, row0: (value_range_bitmaps(v, lo, hi, bit0=row0 & 31, device=sh.device),))
    words = parts[0][0]
    if len(parts) > 1:                                             # a part's words are zero below its first bit and past its last
        words = torch.zeros((int(l.shape[0]), (n + 31) // 32), dtype=torch.int32, device=words.device)
        for (part,), (_, row0) in zip(parts, obj._parts):
            words[:, (row0 >> 5):(row0 >> 5) + part.shape[1]] |= part
    return DocFilter(words[0] if scalar else words, n)


def _value_stats(obj, values, filter, rows_per_chunk):
    n = obj.n_rows
    dt, rows_per_chunk = _value_args(values, n, rows_per_chunk)
    nat.require_device()
    parts = _shard_parts(obj, filter, (_val(values),), lambda sh, v, f, row0: sh._value_stats_call(v, dt, f, row0, rows_per_chunk), n)
    return ValueStats(*_facet_out(values, *_merge_stats(parts)))


def _value_histogram(obj, values, edges, filter, rows_per_chunk):
    n = obj.n_rows
    dt, rows_per_chunk = _value_args(values, n, rows_per_chunk)
    e = _value_edges(edges, dt)
    nat.require_device()
    parts = _shard_parts(obj, filter, (_val(values),),
                         lambda sh, v, f, row0: sh._value_hist_call(v, dt, _values_on(e, sh.device), f, row0, rows_per_chunk), n)
    c, below, above, missing = _add_parts(parts)
    return ValueHistogram(*_facet_out(values, c, below, above, missing, c.sum(1) + below + above + missing))


def _value_topk(obj, values, k, descending, filter, id_offset, rows_per_chunk):
    n = obj.n_rows
    dt, rows_per_chunk = _value_args(values, n, rows_per_chunk)
    k, descending = _value_topk_args(k, descending)
    nat.require_device()
    parts = _shard_parts(obj, filter, (_val(values),),
                         lambda sh, v, f, row0: sh._value_topk_call(v, dt, k, descending, id_offset + row0, f, row0, rows_per_chunk), n)
    return SortedResults(*_facet_out(values, *(parts[0] if len(parts) == 1 else _merge_value_topk(parts, k, descending))))


def _facet_value_stats(obj, labels, n_labels, values, filter, rows_per_chunk):
    n = obj.n_rows
    n_labels, dt, rows_per_chunk, _ = _facet_value_args(labels, n_labels, values, n, rows_per_chunk)
    nat.require_device()
    parts = _shard_parts(obj, filter, (_lab(labels), _val(values)),
                         lambda sh, l, v, f, row0: sh._facet_value_stats_call(l, n_labels, v, dt, f, row0, rows_per_chunk), n)
    return FacetValueStats(*_facet_out(labels, *_merge_stats(parts)))


def _facet_value_histogram(obj, labels, n_labels, values, edges, filter, rows_per_chunk):
    n = obj.n_rows
    n_labels, dt, rows_per_chunk, e = _facet_value_args(labels, n_labels, values, n, rows_per_chunk, edges)
    nat.require_device()
    parts = _shard_parts(obj, filter, (_lab(labels), _val(values)),
                         lambda sh, l, v, f, row0: sh._facet_value_hist_call(l, n_labels, v, dt, _values_on(e, sh.device), f, row0, rows_per_chunk), n)
    return FacetValueHistogram(*_facet_out(labels, *_add_parts(parts)))


def _value_quantiles(obj, values, q, method, ranks, filter, rows_per_chunk):
    """One part: the one call that runs the three levels on its GPU.  More: three rounds of level calls -- the parts' digit counts added on obj's
    GPU, one step there picks each rank's bin and names the next level's slots."""
    import torch
    n = obj.n_rows
    dt, rows_per_chunk = _value_args(values, n, rows_per_chunk)
    qa, method, ra = _quantile_args(q, method, ranks)
    nat.require_device()
    dev = torch.device("cuda", obj.device)
    f = _doc_set(filter, n, obj.device)
    B = _set_args(f, 0)[0]
    if ra is not None:
        ra = _quantile_ranks_for(ra, B)
    tdt = torch.float32 if dt == nat.VAL_F32 else torch.int32
    up = lambda a: torch.from_numpy(a).to(dev) if a is not None else None
    if len(obj._parts) == 1:
        fused = lambda sh, v, fs, row0: _quantile_batches(
            qa, ra, B, lambda qb, rb, R: sh._value_quantiles_call(v, dt, up(qb), method, up(rb), R, fs, row0, rows_per_chunk))
        return ValueQuantiles(*_facet_out(values, *_shard_parts(obj, f, (_val(values),), fused, n)[0]))

    def batch(qb, rb, R):
        q_dev, r_dev = up(qb), up(rb)
        state = missing = None
        for level in range(nat.VALUE_RADIX_LEVELS):
            def one(sh, v, fs, row0):
                d = torch.device("cuda", sh.device)
                sp, ns = (state["slot_prefix"].to(d), state["n_slots"].to(d)) if level else (None, None)
                return sh._value_radix_counts_call(v, dt, level, R, sp, ns, fs, row0, rows_per_chunk)
            counts, *rest = _add_parts(_shard_parts(obj, f, (_val(values),), one, n))
            if level == 0:
                missing = rest[0]
            state = value_radix_step(level, counts, R, state, q_dev, method, r_dev, tdt, obj.device)
        return state["values"], state["ranks"], state["count"], missing
    return ValueQuantiles(*_facet_out(values, *_quantile_batches(qa, ra, B, batch)))


def _facet_value_quantiles(obj, labels, n_labels, values, q, method, ranks, filter, rows_per_chunk):
    """_value_quantiles with a (query, label) cell where that has a query: one part runs the one call; more parts count each level on their
    GPUs, the counts are added on obj's GPU and one value_radix_step over B x n_labels cells runs there."""
    import torch
    n = obj.n_rows
    n_labels, dt, rows_per_chunk, _ = _facet_value_args(labels, n_labels, values, n, rows_per_chunk)
    qa, method, ra = _facet_quantile_args(q, method, ranks, n_labels)
    nat.require_device()
    dev = torch.device("cuda", obj.device)
    f = _doc_set(filter, n, obj.device)
    B = _set_args(f, 0)[0]
    L = n_labels
    if ra is not None:
        if ra.ndim == 1:
            ra = np.ascontiguousarray(np.broadcast_to(ra[None, None, :], (B, L, ra.shape[0])))
        elif ra.shape[0] != B:
            raise ValueError(f"ranks holds {ra.shape[0]} rows for {B} queries")
    tdt = torch.float32 if dt == nat.VAL_F32 else torch.int32
    up = lambda a: torch.from_numpy(a).to(dev) if a is not None else None
    cols = (_lab(labels), _val(values))
    if len(obj._parts) == 1:
        fused = lambda sh, l, v, fs, row0: _facet_quantile_batches(
            qa, ra, B * L, lambda qb, rb, R: sh._facet_value_quantiles_call(l, L, v, dt, up(qb), method, up(rb), R, fs, row0, rows_per_chunk))
        return FacetValueQuantiles(*_facet_out(labels, *_shard_parts(obj, f, cols, fused, n)[0]))

    def batch(qb, rb, R):
        q_dev, r_dev = up(qb), up(rb)
        state = tail = None
        for level in range(nat.VALUE_RADIX_LEVELS):
            def one(sh, l, v, fs, row0):
                d = torch.device("cuda", sh.device)
                sp, ns = (state["slot_prefix"].to(d), state["n_slots"].to(d)) if level else (None, None)
                return sh._facet_value_radix_counts_call(l, L, v, dt, level, R, sp, ns, fs, row0, rows_per_chunk)
            counts, *rest = _add_parts(_shard_parts(obj, f, cols, one, n))
            if level == 0:
                tail = rest                                        # missing [B, L], total, other [B]
            state = value_radix_step(level, counts.reshape(B * L, counts.shape[2], counts.shape[3]), R, state, q_dev, method,
                                     r_dev.reshape(B * L, R) if r_dev is not None else None, tdt, obj.device)
        return (state["values"].reshape(B, L, R), state["ranks"].reshape(B, L, R), state["count"].reshape(B, L)) + tuple(tail)
    return FacetValueQuantiles(*_facet_out(labels, *_facet_quantile_batches(qa, ra, B * L, batch)))


def _term_agg(obj, spec, filter, ids, rows_per_chunk, extra=()):
    """term_counts / term_sums: the set from `filter`, from `ids` or every live document -> spec.result on obj's GPU.  Every part takes its bit
    range of the filter, or the ids with its first row as the id offset.  A host id list is checked by the library before it is staged (an
    index) or here (a group, whose shards skip the ids they do not own).  extra: the arguments behind rows_per_chunk (term sums: tile_cols)."""
    if ids is None:
        nat.require_device()
        return spec.result(*_add_parts(_shard_parts(obj, filter, (), lambda sh, f, row0: sh._term_set_call(spec, f, row0, rows_per_chunk, extra))))
    import torch
    group = isinstance(obj, ShardGroup)
    ids = _term_ids(ids)
    on_dev = _is_torch(ids) and ids.is_cuda
    t = ids if _is_torch(ids) else torch.from_numpy(np.ascontiguousarray(ids))
    if group and not on_dev and t.numel() and (int(t.min()) < -1 or int(t.max()) >= obj.n_rows):
        raise ValueError(f"an id lies outside [-1, {obj.n_rows})")
    nat.require_device()
    if not group and not on_dev:
        h = np.ascontiguousarray(_host(ids))
        B, m, V = h.shape[0], h.shape[1], obj._n_cols()
        out, total = np.empty((B, V), dtype=np.int64), np.empty(B, dtype=np.int64)
        nat.check(getattr(nat.lib(), spec.ids)(obj._h, _ptr(h), B, m, m, 0, 1, *extra, _ptr(out), V, _ptr(total), None))
        dev = torch.device("cuda", obj.device)
        return spec.result(torch.from_numpy(out).to(dev), torch.from_numpy(total).to(dev))

    def one(sh, f, row0):
        ts = t.to(torch.device("cuda", sh.device))
        rows_ok = not group and ts.stride(1) == 1 and ts.stride(0) >= ts.shape[1]   # (an index reads a column slice of a wider hit list in place)
        return sh._term_ids_call(spec, ts if rows_ok else ts.contiguous(), row0, not group, extra)
    return spec.result(*_add_parts(_shard_parts(obj, None, (), one)))


def _term_counts(obj, filter, ids, rows_per_chunk):
    if filter is not None and ids is not None:
        raise ValueError("the set is given by `filter` or by `ids`, not both")
    return _term_agg(obj, _TERM_COUNTS, filter, ids, _rows_per_chunk_arg(rows_per_chunk))


def _term_sums(obj, filter, ids, rows_per_chunk, tile_cols):
    if filter is not None and ids is not None:
        raise ValueError("the set is given by `filter` or by `ids`, not both")
    rows_per_chunk, tile_cols = _term_sum_args(rows_per_chunk, tile_cols)
    return _term_agg(obj, _TERM_SUMS, filter, ids, rows_per_chunk, (tile_cols,))


def _one_set(obj, filter, what):
    """filter= of a call that takes ONE document set -> (None | a shared DocFilter on obj's GPU, n_rows | None)"""
    n = None if filter is None else obj.n_rows
    f = _doc_set(filter, n, obj.device)
    if f is not None and f.per_query:
        raise ValueError(f"{what} takes ONE document set, not a per-query filter")
    return f, n


def _label_terms(obj, fn, result, labels, n_labels, filter, rows_per_item, tile_cols):
    """label_term_sums / label_term_counts: every part takes its slice of the labels and its bit range of the set; the integer outputs are
    added on obj's GPU -> result(matrix [L, V], total [L], other [1])"""
    n_labels, rows_per_item, tile_cols = _label_term_args(labels, n_labels, obj.n_rows, _n_cols_of(obj), rows_per_item, tile_cols)
    f, n = _one_set(obj, filter, fn)
    nat.require_device()
    import torch

    def one(sh, l, fs, row0):
        with torch.cuda.device(torch.device("cuda", sh.device)):   # (a shard of a group runs with its GPU current)
            return sh._label_term_call(fn, l, n_labels, fs, row0, rows_per_item, tile_cols)
    return result(*_facet_out(labels, *_add_parts(_shard_parts(obj, f, (_lab(labels),), one, n))))


def _label_order(obj, labels, n_labels, filter):
    """label_order: the parts' orders, each over its own rows, placed label by label behind one another (a part's rows + its first row)"""
    n_labels, _, _ = _label_term_args(labels, n_labels, obj.n_rows)
    f, n = _one_set(obj, filter, "label_order")
    nat.require_device()
    import torch
    dev = torch.device("cuda", obj.device)

    def one(sh, l, fs, row0):
        with torch.cuda.device(torch.device("cuda", sh.device)):
            ptr, rows, other = sh._label_order_call(l, n_labels, fs, row0)
        return ptr, (rows[:int(ptr[-1])].to(torch.int64) & 0xFFFFFFFF) + row0, other
    parts = _shard_parts(obj, f, (_lab(labels),), one, n)
    if len(parts) == 1:
        return LabelOrder(*_facet_out(labels, *parts[0]))
    cnts = [p[0][1:] - p[0][:-1] for p in parts]
    ptr = torch.zeros(n_labels + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(sum(cnts[1:], cnts[0]), 0)
    rows = torch.empty(int(ptr[-1]), dtype=torch.int64, device=dev)
    before = torch.zeros(n_labels, dtype=torch.int64, device=dev)
    ar = torch.arange(n_labels, device=dev)
    for (p_ptr, p_rows, _), cnt in zip(parts, cnts):
        lab = torch.repeat_interleave(ar, cnt)                     # the label of every entry of the part's order
        at = torch.arange(p_rows.numel(), device=dev) - p_ptr[:-1][lab]
        rows[ptr[:-1][lab] + before[lab] + at] = p_rows
        before += cnt
    return LabelOrder(*_facet_out(labels, ptr, rows, sum((p[2] for p in parts[1:]), parts[0][2])))


def _label_top_weights(obj, labels, n_labels, filter, topn, min_count):
    """label_term_sums of the set (and its label_term_counts when min_count asks for them: a second pass over the set and the cells, the
    label order built again), then the top-n of every label on obj's first GPU -> TopWeights [n_labels, topn]"""
    import torch
    topn, min_count = _weight_topn_args(topn, min_count)
    lab = labels if _is_torch(labels) else torch.from_numpy(np.ascontiguousarray(labels))
    parts = []
    for l0, n in label_term_slices(int(n_labels), _n_cols_of(obj)):                  # (one slice unless n_labels x V is more than one call holds)
        sl = lab if n == int(n_labels) else lab - l0
        res = obj.label_term_sums(sl, n, filter=filter)
        counts = obj.label_term_counts(sl, n, filter=filter).counts if min_count > 0 else None       # (a second pass, label order included)
        parts.append(term_sum_topn(res.sums, res.total, topn, counts=counts, min_count=min_count, device=obj.device) + (res.total,))
    return TopWeights(*(parts[0] if len(parts) == 1 else (torch.cat(x) for x in zip(*parts))))


def _label_top_terms(obj, labels, n_labels, filter, topn, method, min_count, background):
    """label_term_counts of the set, then every label's top-n against the background -> TopTerms [n_labels, topn]"""
    import torch
    topn, method, min_count = _term_topn_args(topn, method, min_count)
    _background_arg(background)
    lab = labels if _is_torch(labels) else torch.from_numpy(np.ascontiguousarray(labels))
    fg = obj.label_term_counts(lab, n_labels, filter=filter)
    return _top_terms_of(obj, TermCounts(fg.counts, fg.total), topn, method, min_count, background)


def _assign(obj, centroids, bias, filter, rows_per_chunk):
    c, b, rows_per_chunk = _assign_args(centroids, bias, _n_cols_of(obj), rows_per_chunk)
    import torch
    nat.require_device()
    n = None if filter is None else obj.n_rows
    f = _doc_set(filter, n, obj.device)
    if f is not None and f.per_query:
        raise ValueError("assign takes ONE document set, not a per-query filter")

    def one(sh, fs, row0):
        sdev = torch.device("cuda", sh.device)
        with torch.cuda.device(sdev):                              # (a shard of a group runs with its GPU current)
            return sh._assign_call(c.to(sdev).contiguous(), b.to(sdev).contiguous() if b is not None else None, fs, row0, rows_per_chunk)
    parts = _shard_parts(obj, f, (), one, n)
    return Assignment(*(parts[0] if len(parts) == 1 else (torch.cat(x) for x in zip(*parts))))


# ---- scores as a field: the exact score of every row of a document set (vs_index_set_scores) -------------------------------------------------
def set_score_plan(n_rows: int, B: int, n_cols: int, per_query: bool = True, rows_per_chunk: int = 0):
    """The launch vs_index_set_scores takes for these arguments (vs_set_score_plan; pure host arithmetic, no GPU needed) -> (chunks,
    rows_per_chunk): a work item is one query's chunk of rows."""
    chunks, rpc = C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_set_score_plan(int(n_rows), int(B), int(n_cols), 1 if per_query else 0, int(rows_per_chunk), C.byref(chunks), C.byref(rpc)))
    return chunks.value, rpc.value


def _set_scores(obj, q, filter, rows_per_chunk):
    rows_per_chunk = _rows_per_chunk_arg(rows_per_chunk)
    if not hasattr(q, "ndim") or q.ndim != 2:
        raise ValueError("queries must be [B, V]")
    import torch
    nat.require_device()
    qt = q.detach() if _is_torch(q) else torch.from_numpy(np.ascontiguousarray(q))
    n = obj.n_rows
    f = None
    if filter is not None:
        from .doc_filter import as_doc_filter
        f = as_doc_filter(filter, n, device=obj.device, batch=int(qt.shape[0]))

    def one(sh, fs, row0):
        sdev = torch.device("cuda", sh.device)
        with torch.cuda.device(sdev):                              # (a shard of a group runs with its GPU current)
            return (sh._set_scores_call(qt.to(sdev).contiguous(), fs, row0, rows_per_chunk),)
    parts = _shard_parts(obj, f, (), one, n)
    return parts[0][0] if len(parts) == 1 else torch.cat([p[0] for p in parts], dim=1)


# ---- set egress: the size, the members, a page and a sample of a document set; id lists back to bitmaps (vs_set_*) ------------------------------
class SetIds(NamedTuple):
    """set_ids / DocFilter.ids: per query the set's documents in ascending order -- ranks [offset, offset + limit) of that list, ids int64
    [B, limit], -1 behind the last member -- and the full size of the set, counts int64 [B], whatever the window"""
    ids: object
    counts: object


class SetSample(NamedTuple):
    """set_sample / DocFilter.sample: per query n documents of the set, uniformly and without replacement -- the n with the smallest (hash of
    the seed and the id, id), in that order, ids int64 [B, n], -1 behind the last when the set holds fewer -- and the size of the set"""
    ids: object
    counts: object


MAX_SET_SAMPLE = nat.SET_MAX_SAMPLE
MAX_SET_IDS = nat.SET_MAX_OUT_IDS


def set_list_plan(n_rows: int, B: int, per_query: bool = True, rows_per_chunk: int = 0):
    """The launch vs_set_count / vs_set_ids / vs_set_sample take for these arguments (vs_set_list_plan; pure host arithmetic, no GPU needed) ->
    (chunks, rows_per_chunk, spans): a work item is one query's chunk of rows, a wave counts and lists 2048-row spans."""
    chunks, rpc, spans = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    nat.check(nat.lib().vs_set_list_plan(int(n_rows), int(B), 1 if per_query else 0, int(rows_per_chunk), C.byref(chunks), C.byref(rpc), C.byref(spans)))
    return chunks.value, rpc.value, spans.value


def set_sample_hash(seed: int, id: int) -> int:
    """The pinned hash vs_set_sample orders a set by (vs_set_sample_hash, on the host): uint32 of (seed, global id)"""
    return int(nat.lib().vs_set_sample_hash(int(seed) & 0xFFFFFFFFFFFFFFFF, int(id)))


def _is_int(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def _set_window_args(offset, limit):
    """offset: an int >= 0 or a sequence of them, one per query; limit: None (the largest count) or an int >= 0 -> (int | int64 ndarray, limit)"""
    if _is_int(offset):
        off = int(offset)
        bad = off < 0
    else:
        off = np.asarray(offset.detach().cpu().numpy() if _is_torch(offset) else offset)
        if off.ndim != 1 or off.shape[0] < 1 or off.dtype.kind not in "iu":
            raise TypeError("offset: an int, or one int per query")
        off = np.ascontiguousarray(off, dtype=np.int64)
        bad = bool((off < 0).any())
    if bad:
        raise ValueError("offset must be >= 0")
    if limit is not None and (not _is_int(limit) or limit < 0):
        raise ValueError(f"limit must be None or an int >= 0, got {limit!r}")
    return off, None if limit is None else int(limit)


def _set_sample_args(n, seed):
    if not _is_int(n) or not 1 <= n <= MAX_SET_SAMPLE:
        raise ValueError(f"n must be in 1..{MAX_SET_SAMPLE}, got {n!r}")
    if not _is_int(seed):
        raise TypeError(f"seed must be an int, got {type(seed).__name__}")
    return int(n), int(seed)


def _sample_seeds(seed: int, B: int):
    """query b samples under seed + b (modulo 2^64) -> int64 ndarray [B] holding the uint64 bits"""
    return np.array([(seed + b) & 0xFFFFFFFFFFFFFFFF for b in range(B)], dtype=np.uint64).view(np.int64)


def _offsets_for(off, B):
    """the offsets of a call for B queries -> None (all 0) or an int64 ndarray [B]"""
    if isinstance(off, int):
        return None if off == 0 else np.full(B, off, dtype=np.int64)
    if off.shape[0] != B:
        raise ValueError(f"{off.shape[0]} offsets, the filter is for {B} queries")
    return off


def _set_count_call(h, device, n_rows, f, bit0, rows_per_chunk):
    """One vs_set_count (h None: the bitmap as it is) or vs_index_set_count (tombstones in) call on torch's current stream -> (counts int64
    [B],) on `device`.  f: None (every row) or a DocFilter there, read from bit `bit0` on."""
    import torch
    B, (w, b0, ld, _) = _set_args(f, bit0)
    counts = torch.empty(B, dtype=torch.int64, device=torch.device("cuda", device))
    if h is None:
        nat.check(nat.lib().vs_set_count(w, b0, ld, None, B, int(n_rows), rows_per_chunk, _ptr(counts), device, current_stream(device)))
    else:
        nat.check(nat.lib().vs_index_set_count(h, w, b0, ld, B, rows_per_chunk, _ptr(counts), current_stream(device)))
    return (counts,)


def _set_ids_call(h, device, n_rows, f, bit0, offsets_dev, limit, id_offset, rows_per_chunk):
    """One vs_set_ids / vs_index_set_ids call -> (ids int64 [B, limit], counts int64 [B]); offsets_dev: None or an int64 tensor [B] there"""
    import torch
    dev = torch.device("cuda", device)
    B, (w, b0, ld, _) = _set_args(f, bit0)
    ids = torch.empty((B, limit), dtype=torch.int64, device=dev)
    counts = torch.empty(B, dtype=torch.int64, device=dev)
    if h is None:
        nat.check(nat.lib().vs_set_ids(w, b0, ld, None, B, int(n_rows), _ptr(offsets_dev), limit, int(id_offset), rows_per_chunk, _ptr(ids),
                                       _ptr(counts), device, current_stream(device)))
    else:
        nat.check(nat.lib().vs_index_set_ids(h, w, b0, ld, B, _ptr(offsets_dev), limit, int(id_offset), rows_per_chunk, _ptr(ids), _ptr(counts),
                                             current_stream(device)))
    return ids, counts


def _set_sample_call(h, device, n_rows, f, bit0, seeds_dev, n, id_offset, rows_per_chunk):
    """One vs_set_sample / vs_index_set_sample call -> (ids int64 [B, n], hashes int64 [B, n] in 0..2^32 - 1, counts int64 [B]); seeds_dev:
    an int64 tensor [B] there holding the uint64 seeds' bits"""
    import torch
    dev = torch.device("cuda", device)
    B, (w, b0, ld, _) = _set_args(f, bit0)
    ids = torch.empty((B, n), dtype=torch.int64, device=dev)
    hs = torch.empty((B, n), dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int64, device=dev)
    if h is None:
        nat.check(nat.lib().vs_set_sample(w, b0, ld, None, B, int(n_rows), _ptr(seeds_dev), n, int(id_offset), rows_per_chunk, _ptr(ids), _ptr(hs),
                                          _ptr(counts), device, current_stream(device)))
    else:
        nat.check(nat.lib().vs_index_set_sample(h, w, b0, ld, B, _ptr(seeds_dev), n, int(id_offset), rows_per_chunk, _ptr(ids), _ptr(hs), _ptr(counts),
                                                current_stream(device)))
    return ids, hs.to(torch.int64) & 0xFFFFFFFF, counts


def set_from_ids(ids, n_rows: int, bit0: int = 0, allow: bool = True, ld_words=None, device: int = 0):
    """vs_set_from_ids on torch's current stream: ids an int64 tensor [B, m] on `device` (entries < 0 are padding; an id at or above n_rows is
    ignored) -> int32 words [B, ld_words] there, bit bit0 + id set for every listed id -- or, allow=False, for every other row"""
    import torch
    B, m = int(ids.shape[0]), int(ids.shape[1])
    nw = (int(bit0) + int(n_rows) + 31) // 32
    ld = nw if ld_words is None else int(ld_words)
    words = torch.empty((B, ld), dtype=torch.int32, device=torch.device("cuda", device))
    ids = ids.contiguous()
    nat.check(nat.lib().vs_set_from_ids(_ptr(ids) if m else None, B, m, m, int(n_rows), int(bit0), 1 if allow else 0, _ptr(words), ld, int(device),
                                        current_stream(device)))
    return words


def _on(x, device: int):
    """a small host array -> a tensor on GPU `device`"""
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{device}")


def _doc_filter_count(f, rows_per_chunk=0):
    nat.require_device()
    return _set_count_call(None, f.device.index, f.n_rows, f, 0, _rows_per_chunk_arg(rows_per_chunk))[0]


def _doc_filter_ids(f, offset, limit, rows_per_chunk=0):
    off, limit = _set_window_args(offset, limit)
    rpc = _rows_per_chunk_arg(rows_per_chunk)
    nat.require_device()
    dev, B = f.device.index, f.n_queries or 1
    if limit is None:                                              # one count round first
        limit = int(_set_count_call(None, dev, f.n_rows, f, 0, rpc)[0].max())
    return SetIds(*_set_ids_call(None, dev, f.n_rows, f, 0, _on(_offsets_for(off, B), dev), limit, 0, rpc))


def _doc_filter_sample(f, n, seed, rows_per_chunk=0):
    n, seed = _set_sample_args(n, seed)
    rpc = _rows_per_chunk_arg(rows_per_chunk)
    nat.require_device()
    dev, B = f.device.index, f.n_queries or 1
    ids, _, counts = _set_sample_call(None, dev, f.n_rows, f, 0, _on(_sample_seeds(seed, B), dev), n, 0, rpc)
    return SetSample(ids, counts)


def _set_batch(obj, filter, n):
    """filter= resolved once on obj's GPU -> (DocFilter | None, the B of the calls)"""
    f = _doc_set(filter, n, obj.device)
    return f, (f.n_queries if (f is not None and f.per_query) else 1)


def _set_count(obj, filter, rows_per_chunk):
    n = obj.n_rows
    rpc = _rows_per_chunk_arg(rows_per_chunk)
    nat.require_device()
    return _add_parts(_shard_parts(obj, filter, (), lambda sh, f, row0: sh._set_count_call(f, row0, rpc), n))[0]


def _set_ids(obj, filter, offset, limit, rows_per_chunk):
    """The shard rule of the list: after a count round, shard s lists its local window [offset - C_s, offset - C_s + limit) clipped at 0 -- C_s
    the count of the shards before it -- with its first row as the id offset, and the pieces are placed one behind the other."""
    import torch
    n = obj.n_rows
    off, limit = _set_window_args(offset, limit)
    rpc = _rows_per_chunk_arg(rows_per_chunk)
    nat.require_device()
    f, B = _set_batch(obj, filter, n)
    off = _offsets_for(off, B)
    parts = obj._parts
    if len(parts) == 1 and limit is not None:                      # one part: its window is the window
        sh = parts[0][0]
        return SetIds(*sh._set_ids_call(f, 0, _on(off, sh.device), limit, 0, rpc))
    counts = torch.stack([p[0] for p in _shard_parts(obj, f, (), lambda sh, fs, row0: sh._set_count_call(fs, row0, rpc), n)])      # [S, B]
    total = counts.sum(0)
    if limit is None:
        limit = int(total.max())
    before = counts.cumsum(0) - counts                             # C_s: the exclusive prefix of the shards' counts
    want = _on(off, obj.device) if off is not None else torch.zeros(B, dtype=torch.int64, device=total.device)
    local = {row0: (want - before[s]).clamp_(min=0) for s, (_, row0) in enumerate(parts)}
    pieces = _shard_parts(obj, f, (), lambda sh, fs, row0: sh._set_ids_call(fs, row0, local[row0].to(f"cuda:{sh.device}"), limit, row0, rpc), n)
    if len(pieces) == 1:
        return SetIds(pieces[0][0], total)
    out = torch.full((B, limit), -1, dtype=torch.int64, device=total.device)
    slot = torch.arange(limit, device=total.device)[None, :]
    for s, (ids, _) in enumerate(pieces):
        dest = slot + (before[s] - want).clamp_(min=0)[:, None]    # a shard's piece starts where the shards before it end
        take = (ids >= 0) & (dest < limit)
        out[take.nonzero(as_tuple=True)[0], dest[take]] = ids[take]
    return SetIds(out, total)


def _merge_set_samples(parts, n):
    """the shards' (ids, hashes, counts), each sampled with its id offset -> the n smallest by (hash, id), and the counts added"""
    import torch
    ids, hs = (torch.cat([p[i] for p in parts], dim=1) for i in (0, 1))
    gone = ids < 0
    by_id = torch.where(gone, torch.full_like(ids, 1 << 62), ids).argsort(dim=1, stable=True)
    h = torch.where(gone, torch.full_like(hs, 1 << 32), hs)
    order = by_id.gather(1, h.gather(1, by_id).argsort(dim=1, stable=True))[:, :n]
    return ids.gather(1, order), sum(p[2] for p in parts[1:]) + parts[0][2]


def _set_sample(obj, filter, n, seed, rows_per_chunk):
    n_rows = obj.n_rows
    n, seed = _set_sample_args(n, seed)
    rpc = _rows_per_chunk_arg(rows_per_chunk)
    nat.require_device()
    f, B = _set_batch(obj, filter, n_rows)
    seeds = _sample_seeds(seed, B)
    parts = _shard_parts(obj, f, (), lambda sh, fs, row0: sh._set_sample_call(fs, row0, _on(seeds, sh.device), n, row0, rpc), n_rows)
    if len(parts) == 1:
        return SetSample(parts[0][0], parts[0][2])
    return SetSample(*_merge_set_samples(parts, n))


class DeviceIndex:
    """Owner of one device-resident index shard (CSR packets or dense)."""

    def __init__(self, handle):
        self._h = handle
        self._device = None        # cached: info() reads device-side search statistics and therefore synchronises

    @property
    def device(self) -> int:
        if self._device is None:
            self._device = int(self.info().device)
        return self._device

    @property
    def _parts(self):
        """(shard, its first row) of every part an aggregation runs over: an index is one part at row 0"""
        return ((self, 0),)

    def _slices(self, on, kind, x):
        """every part's slice of a per-row column, made a tensor on its GPU by `on` (_labels_on | _values_on)"""
        return (on(x, self.device),)

    # ---- constructors -------------------------------------------------------------------------
    @classmethod
    def from_csr(cls, indptr, indices, data, n_cols, store_dtype=None, device=0):
        """CSR arrays (numpy or torch, host or device). data=None -> binary index.
        store_dtype: VS_F32 | VS_F16 | VS_NONE; default = dtype of `data` (binary when data is None)."""
        nat.require_device()
        p_rp, dt_rp, k1 = as_arg(indptr, (nat.VS_I32, nat.VS_I64))
        p_ci, dt_ci, k2 = as_arg(indices, (nat.VS_I32, nat.VS_I64))
        p_v, dt_v, k3 = as_arg(data, (nat.VS_F32, nat.VS_F16))
        n_rows = int(indptr.shape[0]) - 1
        if store_dtype is None:
            store_dtype = dt_v if data is not None else nat.VS_NONE
        h = C.c_void_p()
        nat.check(nat.lib().vs_index_create_csr(p_rp, dt_rp, p_ci, dt_ci, p_v, dt_v if data is not None else nat.VS_F32,
                                                store_dtype, n_rows, int(n_cols), int(device), C.byref(h)))
        del k1, k2, k3
        return cls(h)

    @classmethod
    def reserved(cls, rows_cap, packets_cap, n_cols, store_dtype, device=0):
        """Empty CSR index with room for rows_cap rows / packets_cap 8-nnz packets; fill with append_csr()."""
        nat.require_device()
        h = C.c_void_p()
        nat.check(nat.lib().vs_index_create_reserved(int(rows_cap), int(packets_cap), int(n_cols), int(store_dtype), int(device), C.byref(h)))
        return cls(h)

    def append_csr(self, indptr, indices, data):
        """Append a block of CSR rows (a shard) behind the rows already in the index."""
        p_rp, dt_rp, k1 = as_arg(indptr, (nat.VS_I32, nat.VS_I64))
        p_ci, dt_ci, k2 = as_arg(indices, (nat.VS_I32, nat.VS_I64))
        p_v, dt_v, k3 = as_arg(data, (nat.VS_F32, nat.VS_F16))
        nat.check(nat.lib().vs_index_append_csr(self._h, p_rp, dt_rp, p_ci, dt_ci, p_v, dt_v if data is not None else nat.VS_F32,
                                                int(indptr.shape[0]) - 1))

    def slice_rows(self, row0: int, n_rows: int, device: int = None) -> "DeviceIndex":
        """Rows [row0, row0 + n_rows) as a new CSR index on GPU `device` (default: this index's): a device-to-device (peer) copy of
        the packets -- what row-range sharding deals out (vs_index_slice_rows)."""
        h = C.c_void_p()
        nat.check(nat.lib().vs_index_slice_rows(self._h, int(row0), int(n_rows), int(self.device if device is None else device), C.byref(h)))
        return DeviceIndex(h)

    def append_npz(self, path: str, shift: int = 0):
        """Append a scipy.sparse.save_npz CSR shard read natively (zip + npy parsed in the library): columns below `shift` dropped,
        ids moved down by `shift`, sorted within a row.  NotImplementedError for non-CSR files; NotBinaryError when a binary
        (bag-of-token) index meets a value other than 1."""
        try:
            nat.check(nat.lib().vs_index_append_npz(self._h, str(path).encode(), int(shift)))
        except ValueError as e:
            if "expects a binary matrix" in str(e):
                raise NotBinaryError(str(e)) from None
            raise

    def save_npz(self, path: str, compressed: bool = False):
        """Write the index as a scipy.sparse.save_npz file (CSR, int64 ids, fp32 data) without scipy."""
        nat.check(nat.lib().vs_index_save_npz(self._h, str(path).encode(), 1 if compressed else 0))

    def save_native(self, path: str):
        """Write the device format verbatim (.vsx shard file)."""
        nat.check(nat.lib().vs_index_save_native(self._h, str(path).encode()))

    @classmethod
    def load_native(cls, path: str, device=0):
        nat.require_device()
        h = C.c_void_p()
        nat.check(nat.lib().vs_index_load_native(str(path).encode(), int(device), C.byref(h)))
        return cls(h)

    @classmethod
    def from_dense(cls, mat, store_dtype=None, device=0, max_density=0.0):
        """Dense [N, V] index. max_density > 0: store as CSR packets when the matrix is that sparse
        (sparsity-aware dense index: same results, searched by the CSR scan)."""
        nat.require_device()
        p, dt, keep = as_arg(mat, (nat.VS_F32, nat.VS_F16))
        n_rows, n_cols = int(mat.shape[0]), int(mat.shape[1])
        h = C.c_void_p()
        nat.check(nat.lib().vs_index_create_dense_auto(p, dt, dt if store_dtype is None else store_dtype, n_rows, n_cols, n_cols,
                                                       float(max_density), int(device), C.byref(h)))
        del keep
        return cls(h)

    @classmethod
    def synthetic(cls, seed, row0, n_rows, n_cols=29523, nnz=768, kind=0, val_law=0, store_dtype=nat.VS_F32, device=0):
        nat.require_device()
        h = C.c_void_p()
        nat.check(nat.lib().vs_index_create_synthetic(C.c_uint64(seed), int(row0), int(n_rows), int(n_cols), int(nnz), int(kind),
                                                      int(val_law), int(store_dtype), int(device), C.byref(h)))
        return cls(h)

    # ---- lifetime -------------------------------------------------------------------------------
    def prepare(self):
        """Build now what the first sparse search would build inside the call (vs_index_prepare)."""
        nat.check(nat.lib().vs_index_prepare(self._h, None))
        return self

    def close(self):
        if self._h is not None and self._h.value:
            nat.lib().vs_index_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- queries --------------------------------------------------------------------------------
    def info(self) -> nat.IndexInfo:
        out = nat.IndexInfo()
        nat.check(nat.lib().vs_index_info(self._h, C.byref(out)))
        return out

    def set_queries_per_pass(self, qt: int):
        """0 = auto (tiles of 8 sparse queries per index pass when the batch qualifies), 1 = one query per pass."""
        nat.check(nat.lib().vs_index_set_queries_per_pass(self._h, int(qt)))

    def set_option(self, name: str, value: int):
        """Tuning / test options: "blocked_postings" (-1 auto, 0 off, 1 on), "mq_variant" (-1 auto, 0 plain, 1 shared columns)."""
        nat.check(nat.lib().vs_index_set_option(self._h, name.encode(), int(value)))

    def _q_args(self, q):
        if q.ndim != 2:
            raise ValueError("queries must be [B, V]")
        p, dt, keep = as_arg(q, (nat.VS_F32, nat.VS_F16))
        return p, dt, keep, int(q.shape[0]), int(q.shape[1])

    def _filter_arg(self, filter, B):
        """`filter=` -> (words pointer on this index's device, filter_ld, keep-alive DocFilter); (None, 0, None) without one."""
        if filter is None:
            return None, 0, None
        from .doc_filter import as_doc_filter
        f = as_doc_filter(filter, int(self.info().n_rows), device=self.device, batch=B)
        return C.c_void_p(f.words.data_ptr()), f.ld, f

    def search(self, q, k: int, id_offset: int = 0, filter=None):
        """Top-k per query -> (ids int64 [B,k], scores float32 [B,k]); canonical order (score desc, id asc).
        Device queries: the call returns once the kernels are enqueued on torch's current stream (no host synchronisation on
        the postings filter path); host queries / outputs are copied and the call blocks.
        filter: a DocFilter, a bool mask [N] / [B, N] or integer row ids to allow (vsearch_amd.doc_filter) -- the top k of the allowed
        rows only; positions beyond them hold id -1, score -inf."""
        p, dt, keep, B, ldq = self._q_args(q)
        k = int(k)
        fp, fld, fkeep = self._filter_arg(filter, B)
        if _is_torch(q) and q.is_cuda:
            import torch
            dev = torch.device("cuda", self.device)
            ids = torch.empty((B, k), dtype=torch.int64, device=dev)
            scores = torch.empty((B, k), dtype=torch.float32, device=dev)
            stream = current_stream(self.device)
            if fp is None:
                nat.check(nat.lib().vs_index_search(self._h, p, dt, ldq, B, k, int(id_offset), C.c_void_p(ids.data_ptr()),
                                                    C.c_void_p(scores.data_ptr()), stream))
            else:
                nat.check(nat.lib().vs_index_search_filtered(self._h, p, dt, ldq, B, k, fp, 0, fld, int(id_offset), C.c_void_p(ids.data_ptr()),
                                                             C.c_void_p(scores.data_ptr()), stream))
            return ids, scores
        ids = np.empty((B, k), dtype=np.int64)
        scores = np.empty((B, k), dtype=np.float32)
        if fp is None:
            nat.check(nat.lib().vs_index_search(self._h, p, dt, ldq, B, k, int(id_offset), C.c_void_p(ids.ctypes.data),
                                                C.c_void_p(scores.ctypes.data), None))
        else:
            import torch
            torch.cuda.current_stream(self.device).synchronize()     # (the bitmap was packed on torch's stream; this call runs on the null stream)
            nat.check(nat.lib().vs_index_search_filtered(self._h, p, dt, ldq, B, k, fp, 0, fld, int(id_offset), C.c_void_p(ids.ctypes.data),
                                                         C.c_void_p(scores.ctypes.data), None))
        if _is_torch(q):
            import torch
            return torch.from_numpy(ids), torch.from_numpy(scores)
        return ids, scores

    def explain(self, q, ids, topn: int = 10, id_offset: int = 0) -> Explanation:
        """Score and explain the pairs (query b, document ids[b, j]) from the stored rows (vs_index_explain): per pair the top `topn`
        columns by contribution q[c] * v, the score (bit-identical to the exact search paths' score on a CSR index) and the number of
        matched terms.  q: [B, V] queries as in search(), or None to rank each row's own stored values (disentangle).  ids: int64 [B, k]
        (id -1 = a filtered search's padding: cols -1, score -inf, 0 matched); ids are global, rows start at id_offset.
        numpy in -> numpy out; torch CUDA in -> tensors on the index's device, enqueued on torch's current stream."""
        B, k, topn, on_dev = _explain_args(q, ids, topn)
        nat.require_device()
        p, dt, keep, ldq = None, nat.VS_F32, None, 0
        if q is not None:
            p, dt, keep, _, ldq = self._q_args(q)
        p_ids, _, keep_ids = as_arg(ids, (nat.VS_I64,))
        out, ptrs = _explain_outputs(B, k, topn, self.device if on_dev else None)
        if k == 0:
            return Explanation(*out)
        stream = current_stream(self.device) if on_dev else None
        nat.check(nat.lib().vs_index_explain(self._h, p, dt, ldq, B, p_ids, k, k, int(id_offset), topn, *ptrs, stream))
        if not on_dev and (_is_torch(ids) or _is_torch(q)):
            import torch
            out = tuple(torch.from_numpy(a) for a in out)
        return Explanation(*out)

    # ---- mutable index: delete / restore / compact --------------------------------------------------
    def _tombstones(self, fn, ids):
        ids, on_dev = _row_ids(ids)
        nat.require_device()
        n = int(ids.shape[0])
        if n == 0:
            return
        fn = getattr(nat.lib(), fn)
        if on_dev:
            nat.check(fn(self._h, C.c_void_p(ids.data_ptr()), n, 0, current_stream(self.device)))
        else:
            nat.check(fn(self._h, C.c_void_p(ids.ctypes.data), n, 0, None))

    def delete_rows(self, ids):
        """Mark rows deleted (vs_index_delete_rows): from now on no search of this handle returns them -- search, search_by_example and
        the shards of a group apply the handle's live bitmap like a deny DocFilter, ANDed with a `filter=` of the call.  Ids do not move and
        the rows stay stored (explain / get_rows still answer; restore_rows brings them back) until compact().  ids: integers, 1-D; -1 is
        ignored, deleting twice is a no-op; an id outside the index raises ValueError (CUDA tensors are not checked: such ids are skipped,
        and the call only enqueues on torch's current stream)."""
        self._tombstones("vs_index_delete_rows", ids)

    def restore_rows(self, ids=None):
        """Undo delete_rows for `ids`; None restores every row (the handle then searches exactly as one that never had deletions)."""
        if ids is None:
            nat.require_device()
            nat.check(nat.lib().vs_index_restore_rows(self._h, None, 0, 0, None))
            return
        self._tombstones("vs_index_restore_rows", ids)

    @property
    def n_live(self) -> int:
        """rows not deleted (synchronises)"""
        out = C.c_int64(0)
        nat.check(nat.lib().vs_index_live_rows(self._h, C.byref(out)))
        return out.value

    def live_mask(self):
        """bool tensor [n_rows] on the index's device: True = live (vs_index_live_bitmap, unpacked)"""
        import torch
        nat.require_device()
        n = self.n_rows
        dev = torch.device("cuda", self.device)
        words = torch.zeros(max((n + 31) // 32, 1), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(self.device).synchronize()
        nat.check(nat.lib().vs_index_live_bitmap(self._h, C.c_void_p(words.data_ptr()), int(words.numel())))
        bits = (words[:, None] >> torch.arange(32, device=dev, dtype=torch.int32)[None, :]) & 1
        return bits.reshape(-1)[:n].to(torch.bool)

    def compact(self, rows_extra: int = 0, packets_extra: int = 0, device: int = None):
        """-> (new DeviceIndex holding the live rows in order, old_ids int64 numpy [n_live]: the row of this index each new row was), with
        room for rows_extra more rows / packets_extra more 8-nnz packets of append_csr (vs_index_compact).  This index is untouched.  If HBM
        cannot hold both, this index's postings copy is dropped (prepare() rebuilds it) and the call retried once."""
        rows_extra, packets_extra = _compact_args(rows_extra, packets_extra)
        nat.require_device()
        device = self.device if device is None else int(device)
        old = np.empty(self.n_live, dtype=np.int64)
        h = C.c_void_p()
        args = (self._h, rows_extra, packets_extra, device, C.byref(h), C.c_void_p(old.ctypes.data) if old.size else None)
        _new_index_call(nat.lib().vs_index_compact, args, (self,))
        return DeviceIndex(h), old

    def prune(self, topk=None, min_value=None, keep_cols=None, drop_cols=None, protect=None, rows_extra: int = 0, packets_extra: int = 0,
              device: int = None):
        """-> (new DeviceIndex, kept int32 numpy [n_rows]: the cells every row keeps).  The new index holds, for every row, the stored cells
        that are eligible -- column in keep_cols (ids or a bool mask [n_cols]; None: all) and not in drop_cols, value >= min_value -- and either
        among the row's topk largest eligible values (ties: the earlier stored cell) or stored by the same row of `protect` (a DeviceIndex of
        the same shape on the same GPU, binary or valued: the reference's bow_mask | topk_mask); cells keep their stored order and bits
        (vs_index_prune).  Rows keep their ids, deleted rows stay deleted; this index is untouched.  topk / min_value on a binary index raise
        ValueError, a dense matrix index NotImplementedError.  rows_extra / packets_extra / device as in compact(), and compact()'s retry: if
        HBM cannot hold both, this index's postings copy is dropped (prepare() rebuilds it) and the call retried once."""
        topk, min_value = _prune_args(topk, min_value)
        rows_extra, packets_extra = _compact_args(rows_extra, packets_extra)
        if protect is not None and not isinstance(protect, DeviceIndex):
            raise TypeError(f"protect must be a DeviceIndex, got {type(protect).__name__}")
        nat.require_device()
        info = self.info()
        words = _col_keep_words(int(info.n_cols), keep_cols, drop_cols)
        device = self.device if device is None else int(device)
        kept = np.zeros(int(info.n_rows), dtype=np.int32)
        h = C.c_void_p()
        args = (self._h, topk, C.c_float(min_value), C.c_void_p(words.ctypes.data) if words is not None else None,
                protect._h if protect is not None else None, rows_extra, packets_extra, device, C.byref(h),
                C.c_void_p(kept.ctypes.data) if kept.size else None)
        _new_index_call(nat.lib().vs_index_prune, args, (self,))
        return DeviceIndex(h), kept

    def select_rows(self, ids, rows_extra: int = 0, packets_extra: int = 0, device: int = None, id_offset: int = 0) -> "DeviceIndex":
        """-> a new DeviceIndex whose row j is row ids[j] - id_offset of this one (vs_index_select_rows): any order, repeats kept, packets copied
        whole -- a row scores bit for bit what it scores here.  ids: integers, 1-D, numpy or torch, on the host or on this index's GPU (a
        tensor on another GPU is moved); an id outside the index -- -1 included -- and an empty list raise ValueError.  Deleted rows are
        carried as deleted.  This index is untouched.  rows_extra / packets_extra / device as in compact(), and compact()'s retry: if HBM
        cannot hold both, this index's postings copy is dropped (prepare() rebuilds it) and the call retried once."""
        ids, on_dev = _select_ids(ids)
        rows_extra, packets_extra = _compact_args(rows_extra, packets_extra)
        nat.require_device()
        if on_dev and ids.device.index != self.device:
            ids = ids.to(f"cuda:{self.device}")
        device = self.device if device is None else int(device)
        h = C.c_void_p()
        args = (self._h, C.c_void_p(ids.data_ptr() if on_dev else ids.ctypes.data), int(ids.shape[0]), int(id_offset), rows_extra, packets_extra, device,
                C.byref(h))
        if on_dev:
            import torch
            torch.cuda.current_stream(self.device).synchronize()    # (the ids were made on torch's stream; the call runs on the null stream)
        _new_index_call(nat.lib().vs_index_select_rows, args, (self,))
        return DeviceIndex(h)

    # ---- reweighted index ------------------------------------------------------------------------------
    def row_stats(self) -> RowStats:
        """-> RowStats(cells, nonzero, l1, sumsq, max): tensors [n_rows] on the index's device, one entry a stored row, deleted rows included
        (vs_index_row_stats).  l1 and sumsq are float64 sums in the pinned order of the exact scores -- bit-reproducible; the root of sumsq is
        the caller's (Index.row_norms).  A dense matrix index raises NotImplementedError.  Blocking."""
        import torch
        nat.require_device()
        n = self.n_rows
        dev = torch.device("cuda", self.device)
        out = RowStats(torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                       torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev),
                       torch.full((n,), float("nan"), dtype=torch.float32, device=dev))
        torch.cuda.current_stream(self.device).synchronize()    # (the outputs were made on torch's stream; the call runs on the null stream)
        nat.check(nat.lib().vs_index_row_stats(self._h, *[C.c_void_p(t.data_ptr()) if n else None for t in out]))
        return out

    def rescale_plan(self, row_scale=None, col_scale=None, dtype=None):
        """what rescale() with these arguments would take -> (scratch_bytes, lds_bytes, col_route: "none" | "lds" | "memory"); scales are
        only tested for None (vs_rescale_plan: pure host arithmetic)"""
        info = self.info()
        return rescale_plan(info.n_rows, info.n_packets, info.n_cols, info.store_dtype, _rescale_dtype(dtype, int(info.store_dtype)),
                            row_scale is not None, col_scale is not None)

    def rescale(self, row_scale=None, col_scale=None, dtype=None, rows_extra: int = 0, packets_extra: int = 0, device: int = None) -> "DeviceIndex":
        """-> a new DeviceIndex with this one's rows, cells and column ids whose stored values are value * row_scale[row] * col_scale[column]
        (vs_index_rescale): products in float64, left to right, rounded once to float32 and then, for dtype "fp16", to float16; with one scale
        that is numpy's float32 product.  row_scale [n_rows], col_scale [n_cols]: numbers, numpy or torch, on the host or on a GPU (moved to
        this index's); None = 1, not multiplied in.  dtype: "fp32" | "fp16" | None = the source's (a binary index, whose cells all hold 1, then
        raises ValueError).  Padding cells stay 0 whatever the scales.  Deleted rows are carried as deleted; this index is untouched.
        rows_extra / packets_extra / device as in compact(), and compact()'s retry: if HBM cannot hold both, this index's postings copy is
        dropped (prepare() rebuilds it) and the call retried once.  A dense matrix index raises NotImplementedError."""
        rows_extra, packets_extra = _compact_args(rows_extra, packets_extra)
        nat.require_device()
        info = self.info()
        out_dtype = _rescale_dtype(dtype, int(info.store_dtype))
        rs, p_rs = _scale_arg(row_scale, int(info.n_rows), "row_scale", self.device)
        cs, p_cs = _scale_arg(col_scale, int(info.n_cols), "col_scale", self.device)
        device = self.device if device is None else int(device)
        if _is_torch(rs) or _is_torch(cs):
            import torch
            torch.cuda.current_stream(self.device).synchronize()    # (the scales were made on torch's stream; the call runs on the null stream)
        h = C.c_void_p()
        args = (self._h, p_rs, p_cs, out_dtype, rows_extra, packets_extra, device, C.byref(h))
        _new_index_call(nat.lib().vs_index_rescale, args, (self,))
        return DeviceIndex(h)

    # ---- combined index ---------------------------------------------------------------------------------
    def combine_plan(self, other, dtype=None) -> CombinePlan:
        """what combine() with `other` would take -> CombinePlan (vs_combine_plan: pure host arithmetic)"""
        if not isinstance(other, DeviceIndex):
            raise TypeError(f"other must be a DeviceIndex, got {type(other).__name__}")
        a, b = self.info(), other.info()
        return combine_plan(a.n_rows, a.n_packets, b.n_packets, a.n_cols, a.store_dtype, b.store_dtype,
                            _combine_dtype(dtype, int(a.store_dtype), int(b.store_dtype)))

    def combine(self, other, wa=1.0, wb=1.0, dtype=None, rows_extra: int = 0, packets_extra: int = 0, device: int = None) -> "DeviceIndex":
        """-> a new DeviceIndex whose row r is wa * (row r of this index) + wb * (row r of `other`), cell by cell (vs_index_combine): the
        columns of a row are the union of the columns either row stores, in ascending order -- a stored zero is a cell, a sum that cancels
        stays one --; a value is np.float32(np.float64(wa) * a + np.float64(wb) * b), the one product where one side lacks the column, a
        binary side counting 1, then rounded to float16 for dtype "fp16".  A score is linear in the cells, so searching the result ranks by
        wa * (this index's score) + wb * (other's score) over every row.  other: a DeviceIndex of the same rows and columns on the same GPU
        (any store; `self` itself is allowed).  dtype: "fp32" | "fp16" | None = fp32 unless both sources are fp16.  A row that stores a
        column twice raises ValueError naming it; a dense matrix index NotImplementedError.  Deleted rows: either side's.  Both indexes are
        untouched.  rows_extra / packets_extra / device as in compact(), and prune()'s retry: if HBM cannot hold all three, the sources'
        postings copies are dropped (prepare() rebuilds them) and the call retried once."""
        if not isinstance(other, DeviceIndex):
            raise TypeError(f"other must be a DeviceIndex, got {type(other).__name__}")
        wa, wb = _combine_weight(wa, "wa"), _combine_weight(wb, "wb")
        rows_extra, packets_extra = _compact_args(rows_extra, packets_extra)
        nat.require_device()
        out_dtype = _combine_dtype(dtype, int(self.info().store_dtype), int(other.info().store_dtype))
        device = self.device if device is None else int(device)
        h = C.c_void_p()
        args = (self._h, other._h, C.c_float(wa), C.c_float(wb), out_dtype, rows_extra, packets_extra, device, C.byref(h))
        _new_index_call(nat.lib().vs_index_combine, args, (self, other))
        return DeviceIndex(h)

    # ---- joined index -----------------------------------------------------------------------------------
    def concat_plan(self, others, dtype=None) -> ConcatPlan:
        """what concat() with `others` would take -> ConcatPlan (vs_concat_plan: pure host arithmetic)"""
        infos = [x.info() for x in _concat_sources(self, others, DeviceIndex)]
        dts = [int(i.store_dtype) for i in infos]
        return concat_plan([i.n_rows for i in infos], [i.n_packets for i in infos], infos[0].n_cols, dts, _concat_dtype(dtype, dts))

    def concat(self, others, dtype=None, rows_extra: int = 0, packets_extra: int = 0, device: int = None) -> "DeviceIndex":
        """-> a new DeviceIndex whose rows are this index's, then those of others[0], and so on (vs_index_concat): packets are copied whole,
        so a row scores bit for bit what it scored in a source of the result's dtype.  others: a DeviceIndex or a sequence of them (up to
        256 sources in all), on this index's GPU, of the same n_cols; fp32, fp16 and binary stores may be mixed, the same index may appear
        more than once, an index without rows contributes nothing.  dtype: "fp32" | "fp16" | "binary" | None = binary if all sources are
        binary, fp16 if all valued sources store fp16, else fp32.  A source of another store is converted cell by cell: fp16 -> fp32 exactly,
        fp32 -> fp16 rounded once to nearest even, a binary cell becomes 1; "binary" with a valued source raises ValueError.  Deleted rows
        are carried as deleted.  Every source is untouched.  A dense matrix index raises NotImplementedError.  rows_extra / packets_extra /
        device as in compact(), and prune()'s retry: if HBM cannot hold them all, the sources' postings copies are dropped (prepare()
        rebuilds them) and the call retried once."""
        srcs = _concat_sources(self, others, DeviceIndex)
        rows_extra, packets_extra = _compact_args(rows_extra, packets_extra)
        nat.require_device()
        out_dtype = _concat_dtype(dtype, [int(x.info().store_dtype) for x in srcs])
        device = self.device if device is None else int(device)
        arr = (C.c_void_p * len(srcs))(*[x._h for x in srcs])
        h = C.c_void_p()
        args = (arr, len(srcs), out_dtype, rows_extra, packets_extra, device, C.byref(h))
        _new_index_call(nat.lib().vs_index_concat, args, srcs)
        return DeviceIndex(h)

    # ---- term constraints (vsearch_amd.doc_filter.DocFilter.from_terms) ------------------------------
    def _term_words(self, cols, thr=None, want_df=False, live_only=True, ld=None):
        info = self.info()
        return _term_bitmaps(lambda *a: nat.lib().vs_index_term_bitmaps(self._h, *a), info.n_rows, info.n_cols, self.device, cols, thr,
                             want_df, live_only, ld, True)

    def term_bitmaps(self, cols, thr=None):
        """One bitmap of rows per term (vs_index_term_bitmaps) -> int32 CUDA tensor [T, W], W = ceil(n_rows / 32): bit r of bitmap t is set
        iff row r stores column cols[t] with a non-zero value -- with a threshold, iff the stored value is >= it.  thr: a dict {column:
        threshold} or one threshold per term (None / NaN: none).  A deleted row still reports its terms.  A column outside [0, V) raises
        ValueError.  Enqueued on torch's current stream."""
        return self._term_words(cols, thr)[0]

    def doc_freq(self, cols, thr=None, live_only=True):
        """Rows that have each term -> int64 CUDA tensor [T]; live_only: deleted rows do not count."""
        return self._term_words(cols, thr, True, live_only)[1]

    # ---- query by example ------------------------------------------------------------------------
    @property
    def n_rows(self) -> int:
        return int(self.info().n_rows)

    def _n_cols(self) -> int:
        if getattr(self, "_cols", None) is None:
            self._cols = int(self.info().n_cols)
        return self._cols

    def get_rows(self, ids, id_offset: int = 0):
        """The stored rows of ids (int64 [n]; -1 = an empty row) -> (indptr int64 [n + 1], indices int32, values float32): columns ascending,
        fp16 values widened exactly, 1 for a binary index, the non-zeros of a dense row (vs_index_get_rows).  An id outside [-1, N) raises
        ValueError.  numpy in -> numpy out; torch CUDA in -> tensors on the index's device.  Blocking."""
        on_dev = _int64_ids(ids, 1)
        nat.require_device()
        n = int(ids.shape[0])
        p_ids, _, keep = as_arg(ids, (nat.VS_I64,))
        if on_dev:
            import torch
            dev = torch.device("cuda", self.device)
            stream = current_stream(self.device)
            indptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
            nat.check(nat.lib().vs_index_get_rows(self._h, p_ids, n, int(id_offset), C.c_void_p(indptr.data_ptr()), None, None, stream))
            nnz = int(indptr[-1])
            indices = torch.empty(nnz, dtype=torch.int32, device=dev)
            values = torch.empty(nnz, dtype=torch.float32, device=dev)
            if nnz:
                nat.check(nat.lib().vs_index_get_rows(self._h, p_ids, n, int(id_offset), C.c_void_p(indptr.data_ptr()),
                                                      C.c_void_p(indices.data_ptr()), C.c_void_p(values.data_ptr()), stream))
            return indptr, indices, values
        indptr = np.empty(n + 1, dtype=np.int64)
        nat.check(nat.lib().vs_index_get_rows(self._h, p_ids, n, int(id_offset), C.c_void_p(indptr.ctypes.data), None, None, None))
        nnz = int(indptr[-1])
        indices = np.empty(nnz, dtype=np.int32)
        values = np.empty(nnz, dtype=np.float32)
        if nnz:
            nat.check(nat.lib().vs_index_get_rows(self._h, p_ids, n, int(id_offset), C.c_void_p(indptr.ctypes.data), C.c_void_p(indices.ctypes.data),
                                                  C.c_void_p(values.ctypes.data), None))
        if _is_torch(ids):
            import torch
            return torch.from_numpy(indptr), torch.from_numpy(indices), torch.from_numpy(values)
        return indptr, indices, values

    def queries_from_rows(self, ids, weights=None, q=None, alpha: float = 1.0):
        """Dense fp32 queries [B, V] from stored rows (vs_index_queries_from_rows): row b is fl32(alpha * q[b]) (0 without q) plus
        fl32(weights[b, j] * row ids[b, j]) for j = 0 .. m-1 in order, each add rounded to fp32; id -1 adds nothing.  ids: int64 [B, m];
        weights: float32 [B, m] (default 1); q: [B, V] fp32 | fp16.  numpy in -> numpy out; torch CUDA in -> a tensor on the index's
        device, enqueued on torch's current stream."""
        B, m, on_dev = _by_example_args(ids, weights, q)
        nat.require_device()
        V = self._n_cols()
        return _queries_from_rows(lambda *args: nat.lib().vs_index_queries_from_rows(self._h, *args), ids, weights, q, alpha, B, m, V,
                                  self.device if on_dev else None, True)

    def search_by_example(self, ids, k: int, weights=None, q=None, alpha: float = 1.0, a=None, exclude: bool = True, filter=None):
        """Search with stored rows as queries: queries_from_rows(ids, weights, q, alpha), then (a = int) only the a largest entries of
        each query (vs_topk_mask), then the top k -- without each query's own example ids when `exclude` (the search takes k + m and
        vs_topk_exclude drops them: exact).  filter: as search().  -> (ids, scores); fewer than k rows left: id -1, score -inf."""
        return _search_by_example(self, ids, k, weights, q, alpha, a, exclude, filter)

    def search_grouped(self, q, k: int, groups, per_group: int = 1, filter=None, depth=None) -> GroupedResults:
        """The top k GROUPS per query, each with its best `per_group` rows: the collapse of the complete canonical ranking (live rows allowed
        by `filter`), exact -- searches of doubling depth, each collapsed on the GPU (vs_topk_collapse), the next one filtered to the rows
        that can still matter (vs_group_filter), until every query is proven complete.  groups: int32 [n_rows], values >= 0 (rows with
        equal values form a group).  depth: the first search's depth (default min(n_rows, 2 k per_group)); the result does not depend
        on it.  filter: as search().  k <= 1024, per_group <= 64, k * per_group <= 8192.  numpy queries -> numpy results; CUDA tensors ->
        tensors on the index's device, on torch's current stream."""
        return _search_grouped(self, q, k, per_group, groups, filter, depth)

    def search_diverse(self, q, k: int, lam=0.5, depth=None, sim: str = "cosine", filter=None, max_row_bytes=None) -> DiverseResults:
        """Diversified top k: Maximal Marginal Relevance over the top `depth` of search(q, depth, filter=) -- each pick is the candidate
        with the largest lam * relevance - (1 - lam) * (largest similarity to a hit already picked), similarities taken between the stored
        rows on the GPU (vs_mmr_select_csr; the exact numerics: include/vsearch_hip.h).  lam in [0, 1], one number or one per query: 1 is
        the plain top k, 0 ranks by novelty alone.  sim: "cosine" (relevance = score / best score) | "dot" (raw scores and dot products).
        depth: candidates per query, k <= depth <= 1024 (default min(n_rows, 1024, max(4 k, k + 16)), a starting point).  The candidate
        rows pass through HBM at most max_row_bytes at a time (default 1 GiB).  n_cols <= 32 768.  numpy queries -> numpy results; CUDA
        tensors -> tensors on the index's device, on torch's current stream."""
        return _search_diverse(self, q, k, lam, depth, sim, filter, max_row_bytes)

    def search_fused(self, qs, k: int, mode: str = "rrf", weights=None, c: float = 60.0, depth=None, filter=None) -> FusedResults:
        """Several queries for one answer: every query batch of qs ([L, B, V], or a list of L batches [B, V]: paraphrases, a feedback query
        next to the original) is searched at depth `depth`, and the L hit lists of a query are fused on the GPU (fuse_topk / vs_fuse_topk:
        "rrf" reciprocal rank fusion, "sum" / "mnz" min-max normalised CombSUM / CombMNZ, "raw" the weighted sum of the scores).  depth:
        default min(n_rows, 1024, 4096 / L, max(4 k, k + 16)), a starting point.  filter: as search(), applied to every search.  A fusion
        of the lists' candidates, not a proven top k of a summed score over all rows.  numpy queries -> numpy results; CUDA tensors ->
        tensors on the index's device, on torch's current stream."""
        return _search_fused(self, qs, k, mode, weights, c, depth, filter)

    def diversify(self, ids, scores, k: int, lam=0.5, sim: str = "cosine", max_row_bytes=None) -> DiverseResults:
        """search_diverse's selection over hit lists the caller already has (ids int64 / scores [B, kk], kk <= 1024; a reranked or a
        filtered list: anything after a list's first id -1 is ignored).  Rows are read as stored, deleted ones included."""
        return _diversify(self, ids, scores, k, lam, sim, max_row_bytes)

    # ---- range search: every document scoring at least a threshold (vs_index_search_range) -------------------------------------------
    def _range_call(self, q, thr, max_hits, filter, id_offset, want_words, filter_bit0=0, boost=None):
        """One vs_index_search_range call -> (ids, scores, counts, words | None).  A torch CUDA q runs on device buffers and torch's current
        stream; anything else on host buffers (blocking).  thr: float32 ndarray [B]; filter: None or a DocFilter on this index's device.
        boost: None, or _boost_args' tuple -- then the call is vs_index_search_boosted, its columns and weights in the kind of the call."""
        p, dt, keep, B, ldq = self._q_args(q)
        n = int(self.info().n_rows)
        W = (n + 31) // 32
        K = int(max_hits)
        fn = nat.lib().vs_index_search_range if boost is None else nat.lib().vs_index_search_boosted
        if _is_torch(q) and q.is_cuda:
            import torch
            dev = torch.device("cuda", self.device)
            t_thr = torch.from_numpy(thr).to(dev)
            ids = torch.empty((B, K), dtype=torch.int64, device=dev)
            scores = torch.empty((B, K), dtype=torch.float32, device=dev)
            counts = torch.empty(B, dtype=torch.int64, device=dev)
            words = torch.empty((B, W), dtype=torch.int32, device=dev) if want_words else None
            fp = C.c_void_p(filter.words.data_ptr()) if filter is not None else None
            extra, keep_boost = _boost_c_args(boost, dev) if boost is not None else ((), None)
            nat.check(fn(self._h, p, dt, ldq, B, C.c_void_p(t_thr.data_ptr()), K, fp, int(filter_bit0), filter.ld if filter is not None else 0,
                         int(id_offset), _ptr(ids) if K else None, _ptr(scores) if K else None, _ptr(counts), _ptr(words) if want_words else None, W,
                         *extra, current_stream(self.device)))
            return ids, scores, counts, words
        if filter is not None or _boost_on_device(boost):
            # the filter's words live on the GPU and the call takes all-host or all-device buffers: run on the device, bring the results back
            import torch
            qd = (q if _is_torch(q) else torch.from_numpy(np.ascontiguousarray(q))).to(torch.device("cuda", self.device))
            out = self._range_call(qd, thr, K, filter, id_offset, want_words, filter_bit0, boost)
            out = tuple(t.cpu() if t is not None else None for t in out)
            return out if _is_torch(q) else tuple(t.numpy() if t is not None else None for t in out)
        ids = np.empty((B, K), dtype=np.int64)
        scores = np.empty((B, K), dtype=np.float32)
        counts = np.empty(B, dtype=np.int64)
        words = np.empty((B, W), dtype=np.int32) if want_words else None
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size else None
        extra, keep_boost = _boost_c_args(boost, None) if boost is not None else ((), None)
        nat.check(fn(self._h, p, dt, ldq, B, ptr(thr), K, None, 0, 0, int(id_offset), ptr(ids), ptr(scores), ptr(counts), ptr(words), W, *extra, None))
        if _is_torch(q):
            import torch
            return (torch.from_numpy(ids), torch.from_numpy(scores), torch.from_numpy(counts), torch.from_numpy(words) if want_words else None)
        return ids, scores, counts, words

    def _range(self, q, min_score, max_hits, filter, id_offset, want_words):
        B, thr, K = _range_args(q, min_score, max_hits)
        nat.require_device()
        f = None
        if filter is not None:
            from .doc_filter import as_doc_filter
            f = as_doc_filter(filter, int(self.info().n_rows), device=self.device, batch=B)
        return self._range_call(q, thr, K, f, id_offset, want_words)

    def _boosted(self, q, boosts, weights, mode, min_score, max_hits, filter, id_offset, want_words):
        B, thr, K, boost = _boost_args(q, boosts, weights, mode, min_score, max_hits, int(self.info().n_rows))
        nat.require_device()
        f = None
        if filter is not None:
            from .doc_filter import as_doc_filter
            f = as_doc_filter(filter, int(self.info().n_rows), device=self.device, batch=B)
        return self._range_call(q, thr, K, f, id_offset, want_words, boost=boost)

    def search_boosted(self, q, boosts, weights, mode: str = "add", min_score=None, max_hits: int = 100, filter=None,
                       id_offset: int = 0) -> RangeResults:
        """search_range with a BOOSTED score in the place of the score: relevance plus ("add") or times ("mul") a weighted sum of up to 4
        numeric fields, exact -- every live, allowed document is scored, so with min_score=None the list is the exact top max_hits by
        boosted score, not a rescore window.  boosts: a list of value columns [n_rows] (float32 / int32, value_column() converts; NaN /
        INT32_MIN = no value, which is neutral); weights: one per field, or [B, F].  S = the fp64 row sum of search_range before its
        rounding, t_j = fp64(w_j) * fp64(value_j) (0 for w_j == 0 or a missing value); "add": fl32(((S + t_0) + t_1) ...), "mul":
        fl32(S * (((1 + t_0) + t_1) ...)); a NaN result matches nothing.  With every weight 0 it is search_range bit for bit.  min_score:
        a floor on the boosted score (None: none).  -> RangeResults(ids, boosted scores, counts) as search_range."""
        ids, scores, counts, _ = self._boosted(q, boosts, weights, mode, min_score, max_hits, filter, id_offset, False)
        return RangeResults(ids, scores, counts)

    def count_boosted(self, q, boosts, weights, mode: str = "add", min_score=None, filter=None):
        """The number of live, allowed documents whose boosted score is at least min_score, per query: int64 [B]."""
        return self._boosted(q, boosts, weights, mode, min_score, 0, filter, 0, False)[2]

    def boosted_filter(self, q, boosts, weights, mode: str = "add", min_score=None, filter=None):
        """The documents search_boosted matches, as a per-query DocFilter [B, W] on the index's device (as match_filter)."""
        from .doc_filter import DocFilter
        import torch
        _boost_args(q, boosts, weights, mode, min_score, 0)
        dev = torch.device("cuda", self.device)
        qd = q.to(dev) if _is_torch(q) else torch.from_numpy(np.ascontiguousarray(q)).to(dev)
        words = self._boosted(qd, boosts, weights, mode, min_score, 0, filter, 0, True)[3]
        return DocFilter(words, int(self.info().n_rows))

    def last_range_plan(self):
        """(row chunks, rows a chunk) of the scan the most recent range search on this index took (vs_index_last_range_plan)"""
        chunks, rpc = C.c_int32(0), C.c_int64(0)
        nat.check(nat.lib().vs_index_last_range_plan(self._h, C.byref(chunks), C.byref(rpc)))
        return chunks.value, rpc.value

    def search_range(self, q, min_score, max_hits: int = 100, filter=None, id_offset: int = 0) -> RangeResults:
        """Every live, allowed document scoring at least min_score (one number, or one per query), counted -> RangeResults(ids, scores,
        counts): counts [B] is exact whatever max_hits is; ids / scores [B, max_hits] hold the matches in the canonical order -- all of
        them when counts[b] <= max_hits, else the top max_hits -- with id -1 / score -inf behind them.  The score is the library's exact
        numerics on every path (what explain() reports for the pair), so membership does not depend on the kernel that served the call.
        max_hits in 0..2048; filter as in search().  numpy in -> numpy out; torch CUDA in -> tensors on the index's device."""
        ids, scores, counts, _ = self._range(q, min_score, max_hits, filter, id_offset, False)
        return RangeResults(ids, scores, counts)

    def count_matches(self, q, min_score, filter=None):
        """The number of live, allowed documents scoring at least min_score, per query: int64 [B] (search_range with max_hits = 0)."""
        return self._range(q, min_score, 0, filter, 0, False)[2]

    def match_filter(self, q, min_score, filter=None):
        """The documents search_range matches, as a per-query DocFilter [B, W] on the index's device: the uncapped result, ready for
        ``search(filter=)`` and for ``&``, ``|``, ``~`` with any other filter."""
        from .doc_filter import DocFilter
        import torch
        _range_args(q, min_score, 0)
        dev = torch.device("cuda", self.device)
        qd = q.to(dev) if _is_torch(q) else torch.from_numpy(np.ascontiguousarray(q)).to(dev)
        words = self._range(qd, min_score, 0, filter, 0, True)[3]
        return DocFilter(words, int(self.info().n_rows))

    # ---- facet counts: how a document set spreads over per-row labels (vs_index_facet_counts) ---------------------------------------------
    def _facet_call(self, labels_dev, n_labels, f, bit0, rows_per_chunk):
        """One vs_index_facet_counts call on device buffers and torch's current stream -> (counts [B, L], total [B], other [B]) int64 CUDA
        tensors.  labels_dev: int32 CUDA tensor [n_rows] on this index's device; f: None or a DocFilter there, read from bit `bit0` on."""
        import torch
        dev = torch.device("cuda", self.device)
        B, set_args = _set_args(f, bit0)
        counts = torch.empty((B, n_labels), dtype=torch.int64, device=dev)
        total = torch.empty(B, dtype=torch.int64, device=dev)
        other = torch.empty(B, dtype=torch.int64, device=dev)
        nat.check(nat.lib().vs_index_facet_counts(self._h, *set_args, _ptr(labels_dev), n_labels, rows_per_chunk, _ptr(counts), n_labels,
                                                  _ptr(total), _ptr(other), current_stream(self.device)))
        return counts, total, other

    def facet_counts(self, labels, n_labels: int, filter=None, rows_per_chunk: int = 0) -> FacetCounts:
        """How a document set spreads over per-document labels -> FacetCounts(counts [B, n_labels], total [B], other [B]), int64.  labels:
        integer codes [n_rows] (numpy, or a tensor -- an int32 tensor on the index's GPU is read in place); a label outside [0, n_labels),
        -1 = "no label" included, counts into `other`.  filter: what search(filter=) accepts -- a per-query DocFilter (match_filter's result)
        gives one row per query, a shared one B = 1, None every live document.  Deleted documents never count.  rows_per_chunk: 0 =
        automatic, else a multiple of 64 (a tuning knob: the result does not depend on it).  numpy labels -> numpy out; tensor labels ->
        tensors on the index's device, enqueued on torch's current stream."""
        return _facet_counts(self, labels, n_labels, filter, rows_per_chunk)

    def top_facets(self, labels, n_labels: int, topn: int, filter=None, min_count: int = 1) -> TopFacets:
        """facet_counts, then per query the `topn` labels with the most documents (vs_facet_topn): count descending, label ascending, only
        labels with at least max(min_count, 1) documents; unused slots label -1 / count 0.  topn in 1..1024."""
        return _top_facets(self, labels, n_labels, topn, filter, min_count)

    # ---- numeric fields: range filters, stats, histograms and sort by value (vs_index_value_stats / _histogram / _topk) --------------------
    def _value_stats_call(self, vals_dev, dt, f, bit0, rows_per_chunk):
        """One vs_index_value_stats call on device buffers and torch's current stream -> (count, missing, min, max, sum) CUDA tensors [B].
        vals_dev: float32 / int32 CUDA tensor [n_rows] on this index's device; f: None or a DocFilter there, read from bit `bit0` on."""
        import torch
        dev = torch.device("cuda", self.device)
        B, set_args = _set_args(f, bit0)
        count, missing, total = (torch.empty(B, dtype=torch.int64, device=dev) for _ in range(3))
        lo, hi = (torch.empty(B, dtype=vals_dev.dtype, device=dev) for _ in range(2))
        nat.check(nat.lib().vs_index_value_stats(self._h, *set_args, _ptr(vals_dev), dt, rows_per_chunk, _ptr(count), _ptr(missing), _ptr(lo),
                                                 _ptr(hi), _ptr(total), current_stream(self.device)))
        return count, missing, lo, hi, total

    def _value_hist_call(self, vals_dev, dt, edges_dev, f, bit0, rows_per_chunk):
        """One vs_index_value_histogram call -> (counts [B, E - 1], below, above, missing [B]) int64 CUDA tensors"""
        import torch
        dev = torch.device("cuda", self.device)
        B, set_args = _set_args(f, bit0)
        E = int(edges_dev.shape[0])
        counts = torch.empty((B, E - 1), dtype=torch.int64, device=dev)
        below, above, missing = (torch.empty(B, dtype=torch.int64, device=dev) for _ in range(3))
        nat.check(nat.lib().vs_index_value_histogram(self._h, *set_args, _ptr(vals_dev), dt, _ptr(edges_dev), E, rows_per_chunk, _ptr(counts), E - 1,
                                                     _ptr(below), _ptr(above), _ptr(missing), current_stream(self.device)))
        return counts, below, above, missing

    def _value_topk_call(self, vals_dev, dt, k, descending, id_offset, f, bit0, rows_per_chunk):
        """One vs_index_value_topk call -> (ids int64 [B, k], values [B, k]) CUDA tensors"""
        import torch
        dev = torch.device("cuda", self.device)
        B, set_args = _set_args(f, bit0)
        ids = torch.empty((B, k), dtype=torch.int64, device=dev)
        vals = torch.empty((B, k), dtype=vals_dev.dtype, device=dev)
        nat.check(nat.lib().vs_index_value_topk(self._h, *set_args, _ptr(vals_dev), dt, k, descending, int(id_offset), rows_per_chunk, _ptr(ids),
                                                _ptr(vals), current_stream(self.device)))
        return ids, vals

    def value_range_filter(self, values, lo=None, hi=None):
        """The documents whose value lies in [lo, hi], both ends inclusive, as a DocFilter on the index's device (vs_value_range_bitmaps): for
        ``search(filter=)`` and for ``&``, ``|``, ``~`` with any other filter.  values: float32 / int32 [n_rows] (``value_column`` converts);
        None is an open end; sequences of B bounds give a per-query filter.  A document without a value never matches."""
        return _value_range_filter(self, values, lo, hi)

    def value_stats(self, values, filter=None, rows_per_chunk: int = 0) -> ValueStats:
        """Count, missing, min, max and sum of a numeric field over a document set -> ValueStats, one entry per query.  values: float32 /
        int32 [n_rows] (numpy, or a tensor -- one on the index's GPU is read in place).  filter: what search(filter=) accepts -- a per-query
        DocFilter gives one entry per query, a shared one B = 1, None every live document.  Deleted documents never count.  numpy values ->
        numpy out; tensor values -> tensors on the index's device, enqueued on torch's current stream."""
        return _value_stats(self, values, filter, rows_per_chunk)

    def value_histogram(self, values, edges, filter=None, rows_per_chunk: int = 0) -> ValueHistogram:
        """How a document set spreads over the bins [edges[i], edges[i + 1]) of a numeric field -> ValueHistogram(counts [B, E - 1], below,
        above, missing, total), int64.  edges: 2..1025 strictly ascending numbers.  values, filter, outputs as in ``value_stats``."""
        return _value_histogram(self, values, edges, filter, rows_per_chunk)

    def value_topk(self, values, k: int, descending: bool = True, filter=None, id_offset: int = 0, rows_per_chunk: int = 0) -> SortedResults:
        """Per query the k documents of the set with the largest (descending) or smallest values of a numeric field, ties by id ascending ->
        SortedResults(ids [B, k], values [B, k]); documents without a value are never listed; id -1 / the missing sentinel behind the last.
        k in 1..1024.  values, filter, outputs as in ``value_stats``."""
        return _value_topk(self, values, k, descending, filter, id_offset, rows_per_chunk)

    # ---- breakdowns: a numeric field by facet label (vs_index_facet_value_stats / _histogram) --------------------------------------------------
    def _facet_value_stats_call(self, labels_dev, n_labels, vals_dev, dt, f, bit0, rows_per_chunk):
        """One vs_index_facet_value_stats call on device buffers and torch's current stream -> (count, missing, min, max, sum [B, L], total,
        other [B]) CUDA tensors.  labels_dev / vals_dev: int32 and float32 / int32 CUDA tensors [n_rows] on this index's device; f: None or a
        DocFilter there, read from bit `bit0` on."""
        import torch
        dev = torch.device("cuda", self.device)
        B, set_args = _set_args(f, bit0)
        count, missing, total_sum = (torch.empty((B, n_labels), dtype=torch.int64, device=dev) for _ in range(3))
        lo, hi = (torch.empty((B, n_labels), dtype=vals_dev.dtype, device=dev) for _ in range(2))
        total, other = (torch.empty(B, dtype=torch.int64, device=dev) for _ in range(2))
        nat.check(nat.lib().vs_index_facet_value_stats(self._h, *set_args, _ptr(labels_dev), n_labels, _ptr(vals_dev), dt, rows_per_chunk,
                                                       _ptr(count), _ptr(missing), _ptr(lo), _ptr(hi), _ptr(total_sum), n_labels, _ptr(total),
                                                       _ptr(other), current_stream(self.device)))
        return count, missing, lo, hi, total_sum, total, other

    def _facet_value_hist_call(self, labels_dev, n_labels, vals_dev, dt, edges_dev, f, bit0, rows_per_chunk):
        """One vs_index_facet_value_histogram call -> (counts [B, L, E - 1], below, above, missing [B, L], total, other [B]) int64 CUDA tensors"""
        import torch
        dev = torch.device("cuda", self.device)
        B, set_args = _set_args(f, bit0)
        E = int(edges_dev.shape[0])
        counts = torch.empty((B, n_labels, E - 1), dtype=torch.int64, device=dev)
        below, above, missing = (torch.empty((B, n_labels), dtype=torch.int64, device=dev) for _ in range(3))
        total, other = (torch.empty(B, dtype=torch.int64, device=dev) for _ in range(2))
        nat.check(nat.lib().vs_index_facet_value_histogram(self._h, *set_args, _ptr(labels_dev), n_labels, _ptr(vals_dev), dt, _ptr(edges_dev), E,
                                                           rows_per_chunk, _ptr(counts), E - 1, _ptr(below), _ptr(above), _ptr(missing),
                                                           _ptr(total), _ptr(other), current_stream(self.device)))
        return counts, below, above, missing, total, other

    def facet_value_stats(self, labels, n_labels: int, values, filter=None, rows_per_chunk: int = 0) -> FacetValueStats:
        """Count, missing, min, max and sum of a numeric field per facet label over a document set, in one pass -> FacetValueStats (matrices
        [B, n_labels], total / other [B]); ``.mean()`` in fp64.  labels as in ``facet_counts`` (a label outside [0, n_labels) counts into
        `other` and nothing else), values as in ``value_stats``; filter: what search(filter=) accepts.  Deleted documents never count.
        numpy in -> numpy out; tensors in -> tensors on the index's device, enqueued on torch's current stream."""
        return _facet_value_stats(self, labels, n_labels, values, filter, rows_per_chunk)

    def facet_value_histogram(self, labels, n_labels: int, values, edges, filter=None, rows_per_chunk: int = 0) -> FacetValueHistogram:
        """How the documents of each facet label spread over the bins [edges[i], edges[i + 1]) of a numeric field, over a document set, in one
        pass (a cross-tab) -> FacetValueHistogram(counts [B, n_labels, E - 1], below, above, missing [B, n_labels], total, other [B]).
        edges: 2..1025 strictly ascending numbers, n_labels x (E + 2) <= 2^22.  labels, values, filter, outputs as in ``facet_value_stats``."""
        return _facet_value_histogram(self, labels, n_labels, values, edges, filter, rows_per_chunk)

    # ---- percentiles (vs_index_value_quantiles, vs_index_value_radix_counts) ------------------------------------------------------------------
    def _value_quantiles_call(self, vals_dev, dt, q_dev, method, ranks_dev, R, f, bit0, rows_per_chunk):
        """One vs_index_value_quantiles call on device buffers -> (values [B, R], ranks int64 [B, R], count, missing int64 [B]) CUDA tensors.
        q_dev: float64 [R] or None; ranks_dev: int64 [B, R] or None."""
        import torch
        dev = torch.device("cuda", self.device)
        B, set_args = _set_args(f, bit0)
        vals = torch.empty((B, R), dtype=vals_dev.dtype, device=dev)
        ranks = torch.empty((B, R), dtype=torch.int64, device=dev)
        count, missing = (torch.empty(B, dtype=torch.int64, device=dev) for _ in range(2))
        nat.check(nat.lib().vs_index_value_quantiles(self._h, *set_args, _ptr(vals_dev), dt, _ptr(q_dev) if q_dev is not None else None, method,
                                                     _ptr(ranks_dev) if ranks_dev is not None else None, R, rows_per_chunk, _ptr(vals), _ptr(ranks),
                                                     _ptr(count), _ptr(missing), current_stream(self.device)))
        return vals, ranks, count, missing

    def _value_radix_counts_call(self, vals_dev, dt, level, R, slot_prefix, n_slots, f, bit0, rows_per_chunk):
        """One vs_index_value_radix_counts call -> (counts int64 [B, S, bins], missing int64 [B]) CUDA tensors; missing only at level 0.
        slot_prefix int32 [B, R] / n_slots int32 [B]: the state of the step above, on this index's device (None at level 0)."""
        import torch
        dev = torch.device("cuda", self.device)
        B, set_args = _set_args(f, bit0)
        bins = nat.VALUE_RADIX_BINS if level < 2 else nat.VALUE_RADIX_BINS // 2
        counts = torch.empty((B, 1 if level == 0 else R, bins), dtype=torch.int64, device=dev)
        missing = torch.empty(B, dtype=torch.int64, device=dev) if level == 0 else None
        nat.check(nat.lib().vs_index_value_radix_counts(self._h, *set_args, _ptr(vals_dev), dt, level, R,
                                                        _ptr(slot_prefix) if level else None, _ptr(n_slots) if level else None, rows_per_chunk,
                                                        _ptr(counts), _ptr(missing) if level == 0 else None, current_stream(self.device)))
        return (counts, missing) if level == 0 else (counts,)

    def value_quantiles(self, values, q=None, method: str = "lower", ranks=None, filter=None, rows_per_chunk: int = 0) -> ValueQuantiles:
        """Exact order statistics of a numeric field over a document set -> ValueQuantiles(values [B, R], ranks [B, R], count, missing).
        q: quantiles in [0, 1] shared by the queries, turned into ranks by pos = q * (count - 1) and method "lower" (floor), "higher" (ceil)
        or "nearest" (half to even); or ranks: 0-based ascending ranks, [R] or [B, R].  A rank outside the set's values gives the missing
        sentinel and rank -1.  No interpolation, no sort: three counting passes over the set.  More than 16 ranks are served in batches of
        16.  values, filter, outputs as in ``value_stats``."""
        return _value_quantiles(self, values, q, method, ranks, filter, rows_per_chunk)

    # ---- per-label percentiles (vs_index_facet_value_quantiles, vs_index_facet_value_radix_counts) ------------------------------------------
    def _facet_value_quantiles_call(self, labels_dev, n_labels, vals_dev, dt, q_dev, method, ranks_dev, R, f, bit0, rows_per_chunk):
        """One vs_index_facet_value_quantiles call on device buffers -> (values [B, L, R], ranks int64 [B, L, R], count, missing int64 [B, L],
        total, other int64 [B]) CUDA tensors.  q_dev: float64 [R] or None; ranks_dev: int64 [B, L, R] or None."""
        import torch
        dev = torch.device("cuda", self.device)
        B, set_args = _set_args(f, bit0)
        vals = torch.empty((B, n_labels, R), dtype=vals_dev.dtype, device=dev)
        ranks = torch.empty((B, n_labels, R), dtype=torch.int64, device=dev)
        count, missing = (torch.empty((B, n_labels), dtype=torch.int64, device=dev) for _ in range(2))
        total, other = (torch.empty(B, dtype=torch.int64, device=dev) for _ in range(2))
        nat.check(nat.lib().vs_index_facet_value_quantiles(self._h, *set_args, _ptr(labels_dev), n_labels, _ptr(vals_dev), dt,
                                                           _ptr(q_dev) if q_dev is not None else None, method,
                                                           _ptr(ranks_dev) if ranks_dev is not None else None, R, rows_per_chunk, _ptr(vals),
                                                           _ptr(ranks), _ptr(count), _ptr(missing), _ptr(total), _ptr(other),
                                                           current_stream(self.device)))
        return vals, ranks, count, missing, total, other

    def _facet_value_radix_counts_call(self, labels_dev, n_labels, vals_dev, dt, level, R, slot_prefix, n_slots, f, bit0, rows_per_chunk):
        """One vs_index_facet_value_radix_counts call -> (counts int64 [B, L, S, bins], missing int64 [B, L], total, other int64 [B]) CUDA
        tensors; only counts below level 0.  slot_prefix int32 [B x L, R] / n_slots int32 [B x L]: the state of the step above, on this
        index's device (None at level 0)."""
        import torch
        dev = torch.device("cuda", self.device)
        B, set_args = _set_args(f, bit0)
        bins = nat.VALUE_RADIX_BINS if level < 2 else nat.VALUE_RADIX_BINS // 2
        counts = torch.empty((B, n_labels, 1 if level == 0 else R, bins), dtype=torch.int64, device=dev)
        missing = torch.empty((B, n_labels), dtype=torch.int64, device=dev) if level == 0 else None
        total, other = (torch.empty(B, dtype=torch.int64, device=dev) if level == 0 else None for _ in range(2))
        opt = lambda t, use: _ptr(t) if use else None
        nat.check(nat.lib().vs_index_facet_value_radix_counts(self._h, *set_args, _ptr(labels_dev), n_labels, _ptr(vals_dev), dt, level, R,
                                                              opt(slot_prefix, level), opt(n_slots, level), rows_per_chunk, _ptr(counts),
                                                              opt(missing, level == 0), opt(total, level == 0), opt(other, level == 0),
                                                              current_stream(self.device)))
        return (counts, missing, total, other) if level == 0 else (counts,)

    def facet_value_quantiles(self, labels, n_labels: int, values, q=None, method: str = "lower", ranks=None, filter=None,
                              rows_per_chunk: int = 0) -> FacetValueQuantiles:
        """Exact order statistics of a numeric field per facet label over a document set, three counting passes for all labels ->
        FacetValueQuantiles(values, ranks [B, n_labels, R], count, missing [B, n_labels], total, other [B]).  q / method / ranks as in
        ``value_quantiles`` (ranks: [R] or [B, n_labels, R]), applied to each label's count; labels, values, filter, outputs as in
        ``facet_value_stats``.  The ranks are served in batches of min(16, 65536 // (B x n_labels)), so that the counts of a batch stay
        within 2^27 (the percentiles' 1 GiB rule); B x n_labels itself may not pass 65536."""
        return _facet_value_quantiles(self, labels, n_labels, values, q, method, ranks, filter, rows_per_chunk)

    def facet_value_radix_counts(self, labels, n_labels: int, values, level: int, R: int, slot_prefix=None, n_slots=None, filter=None,
                                 rows_per_chunk: int = 0):
        """One radix level's digit counts per (query, label) (vs_index_facet_value_radix_counts) -> (counts int64 [B, n_labels, S, bins],
        missing [B, n_labels], total, other [B]) at level 0, (counts,) below.  slot_prefix int32 [B x n_labels, R] / n_slots int32 [B x
        n_labels]: the state ``value_radix_step`` returned for the level above, taken over B x n_labels cells."""
        n_labels, dt, rows_per_chunk, _ = _facet_value_args(labels, n_labels, values, self.n_rows, rows_per_chunk)
        nat.require_device()
        to = lambda t: None if t is None else (t if _is_torch(t) else _on(t, self.device)).to(f"cuda:{self.device}").contiguous()
        one = lambda sh, l, v, f, row0: sh._facet_value_radix_counts_call(l, n_labels, v, dt, int(level), int(R), to(slot_prefix), to(n_slots), f,
                                                                          row0, rows_per_chunk)
        return _facet_out(labels, *_shard_parts(self, filter, (_lab(labels), _val(values)), one, self.n_rows)[0])

    # ---- term aggregations: what a document set is about (vs_index_term_counts, vs_index_term_counts_ids) ---------------------------------
    def _term_set_call(self, spec, f, bit0, rows_per_chunk, extra=()):
        """One bitmap-driven call of a term aggregation (spec.bitmap) on device buffers and torch's current stream -> ([B, V], total [B]) int64
        CUDA tensors.  f: None or a DocFilter on this index's device, read from bit `bit0` on; extra: the arguments behind rows_per_chunk."""
        import torch
        dev = torch.device("cuda", self.device)
        (B, set_args), V = _set_args(f, bit0), self._n_cols()
        out = torch.empty((B, V), dtype=torch.int64, device=dev)
        total = torch.empty(B, dtype=torch.int64, device=dev)
        nat.check(getattr(nat.lib(), spec.bitmap)(self._h, *set_args, int(rows_per_chunk), *extra, _ptr(out), V, _ptr(total),
                                                  current_stream(self.device)))
        return out, total

    def _term_ids_call(self, spec, ids_dev, id_offset, strict, extra=()):
        """One id-list-driven call of a term aggregation (spec.ids): ids_dev int64 CUDA tensor [B, m] on this index's device"""
        import torch
        B, m, V = int(ids_dev.shape[0]), int(ids_dev.shape[1]), self._n_cols()
        out = torch.empty((B, V), dtype=torch.int64, device=ids_dev.device)
        total = torch.empty(B, dtype=torch.int64, device=ids_dev.device)
        nat.check(getattr(nat.lib(), spec.ids)(self._h, _ptr(ids_dev), B, m, int(ids_dev.stride(0)), int(id_offset), 1 if strict else 0, *extra,
                                               _ptr(out), V, _ptr(total), current_stream(self.device)))
        return out, total

    def _term_counts_call(self, f, bit0, rows_per_chunk):
        return self._term_set_call(_TERM_COUNTS, f, bit0, rows_per_chunk)

    def _term_counts_ids_call(self, ids_dev, id_offset, strict):
        return self._term_ids_call(_TERM_COUNTS, ids_dev, id_offset, strict)

    def _term_sums_call(self, f, bit0, rows_per_chunk, tile_cols):
        return self._term_set_call(_TERM_SUMS, f, bit0, rows_per_chunk, (int(tile_cols),))

    def _term_sums_ids_call(self, ids_dev, id_offset, strict, tile_cols):
        return self._term_ids_call(_TERM_SUMS, ids_dev, id_offset, strict, (int(tile_cols),))

    def term_counts(self, filter=None, ids=None, rows_per_chunk: int = 0) -> TermCounts:
        """For a document set, how many of its documents have each vocabulary column -> TermCounts(counts [B, V], total [B]), int64 tensors
        on the index's device, enqueued on torch's current stream.  A document has a column iff it stores it with a non-zero value (the
        term constraints' definition).  The set: `filter` -- what search(filter=) accepts: a per-query DocFilter (match_filter's result)
        gives one row per query, a shared one B = 1 -- or `ids`, int64 [B, m] hit lists (``search``'s ids: -1 is skipped, an id listed
        twice counts twice, an id outside the index raises ValueError when the list is on the host and is skipped when it is on the
        device); neither: every live document (the document frequency of all columns in one pass).  Deleted documents never count.
        rows_per_chunk: 0 = automatic, else a multiple of 64 (a tuning knob: the result does not depend on it)."""
        return _term_counts(self, filter, ids, rows_per_chunk)

    def top_terms(self, filter=None, ids=None, topn: int = 20, method: str = "jlh", min_count: int = 1, background=None) -> TopTerms:
        """term_counts of the set, then per query its `topn` most significant columns against a background (vs_term_topn; see
        ``term_topn``): method "jlh" | "lift", or "count" -- the columns most documents of the set have, ordered by the exact integers
        (vs_facet_topn; scores are the counts, bg is 0 unless a background is given).  background: a TermCounts with one row (e.g. a kept
        ``term_counts()``); None counts every live document in this call.  topn in 1..1024."""
        return _top_terms(self, filter, ids, topn, method, min_count, background)

    # ---- term sums: the weight a document set puts on each column (vs_index_term_sums, vs_index_term_sums_ids) ----------------------------------
    def term_sums(self, filter=None, ids=None, rows_per_chunk: int = 0, tile_cols: int = 0) -> TermSums:
        """For a document set, how much weight it puts on each vocabulary column -> TermSums(sums [B, V], total [B]), int64 tensors on the
        index's device, enqueued on torch's current stream.  sums are fixed point: every stored cell adds its value (clamped to +-2^20)
        times 2^24, rounded to nearest even -- exact for fp16 and binary stores, and independent of the order of the additions;
        ``.values()`` gives them as float64, ``.mean()`` the set's centroid as float32.  The set is ``term_counts``'s: `filter`, or `ids`
        (int64 [B, m] hit lists: -1 is skipped, an id listed twice counts twice, an id outside the index raises ValueError when the list is
        on the host and is skipped when it is on the device), or neither: every live document.  Deleted documents never contribute.
        rows_per_chunk: 0 = automatic, else a multiple of 64; tile_cols: 0 = automatic, else the columns of a workgroup's tile, at most
        18 432 (tuning knobs: the result does not depend on them)."""
        return _term_sums(self, filter, ids, rows_per_chunk, tile_cols)

    def top_weight_terms(self, filter=None, ids=None, topn: int = 20, min_count: int = 0) -> TopWeights:
        """term_sums of the set, then per query the `topn` columns with the largest mean weight (vs_term_sum_topn; see ``term_sum_topn``):
        only columns with a positive sum; min_count > 0 also takes ``term_counts`` of the set and lists only columns at least min_count of
        its documents have.  topn in 1..1024."""
        return _top_weights(self, filter, ids, topn, min_count)

    # ---- per-label term aggregations (vs_index_label_term_sums, vs_index_label_term_counts, vs_label_order) -------------------------------------
    def _label_term_call(self, fn, labels_dev, n_labels, f, bit0, rows_per_item, tile_cols):
        """One vs_index_label_term_sums / _counts call (fn) on device buffers and torch's current stream -> ([L, V], total [L], other [1]) int64
        CUDA tensors.  labels_dev: int32 CUDA tensor [n_rows] on this index's device; f: None or a shared DocFilter there, read from bit
        `bit0` on."""
        import torch
        dev = torch.device("cuda", self.device)
        V = self._n_cols()
        out = torch.empty((n_labels, V), dtype=torch.int64, device=dev)
        total = torch.empty(n_labels, dtype=torch.int64, device=dev)
        other = torch.empty(1, dtype=torch.int64, device=dev)
        nat.check(getattr(nat.lib(), fn)(self._h, _ptr(f.words) if f is not None else None, int(bit0), _ptr(labels_dev), int(n_labels),
                                         int(rows_per_item), int(tile_cols), _ptr(out), V, _ptr(total), _ptr(other), current_stream(self.device)))
        return out, total, other

    def _label_order_call(self, labels_dev, n_labels, f, bit0):
        """One vs_label_order call on device buffers -> (ptr int64 [L + 1], rows int32 [n_rows] holding uint32 row numbers, other int64 [1])"""
        import torch
        dev = torch.device("cuda", self.device)
        ptr = torch.empty(n_labels + 1, dtype=torch.int64, device=dev)
        rows = torch.empty(self.n_rows, dtype=torch.int32, device=dev)
        other = torch.empty(1, dtype=torch.int64, device=dev)
        nat.check(nat.lib().vs_label_order(self._h, _ptr(f.words) if f is not None else None, int(bit0), _ptr(labels_dev), int(n_labels),
                                           _ptr(ptr), _ptr(rows), _ptr(other), current_stream(self.device)))
        return ptr, rows, other

    def label_term_sums(self, labels, n_labels: int, filter=None, rows_per_item: int = 0, tile_cols: int = 0) -> LabelTermSums:
        """``term_sums`` per label, for every label at once: the centroid of every cluster, category or article of ONE document set ->
        LabelTermSums(sums [n_labels, V], total [n_labels], other [1]), int64; ``.values()`` float64, ``.mean()`` the centroids float32.
        labels: integer codes [n_rows] as for ``facet_counts`` (outside [0, n_labels): counted into `other`, contributes nowhere); n_labels
        <= 65 536 and n_labels x V <= 2^27; filter: one set (a shared DocFilter, a bool mask [N] or ids), None = every live document.  One
        visit per stored cell whatever n_labels; row l is bit for bit ``term_sums(filter=from_labels(labels, [l]) & filter)``.
        rows_per_item: 0 = automatic, else a multiple of 64; tile_cols: as in ``term_sums`` (tuning knobs: no output depends on them).
        numpy labels -> numpy out; tensor labels -> tensors on the index's device, enqueued on torch's current stream."""
        return _label_terms(self, "vs_index_label_term_sums", LabelTermSums, labels, n_labels, filter, rows_per_item, tile_cols)

    def label_term_counts(self, labels, n_labels: int, filter=None, rows_per_item: int = 0, tile_cols: int = 0) -> LabelTermCounts:
        """``term_counts`` per label, for every label at once -> LabelTermCounts(counts [n_labels, V], total [n_labels], other [1]), int64:
        the set's documents of each label that have each column (stored with a non-zero value).  Arguments as ``label_term_sums``."""
        return _label_terms(self, "vs_index_label_term_counts", LabelTermCounts, labels, n_labels, filter, rows_per_item, tile_cols)

    def label_order(self, labels, n_labels: int, filter=None) -> LabelOrder:
        """The documents of one set grouped by label (vs_label_order, the first stage of ``label_term_sums``) -> LabelOrder(ptr int64
        [n_labels + 1], rows int64 [n_set], other [1]): rows[ptr[l]:ptr[l + 1]] are the set's documents of label l, in no specified order.
        BLOCKING, unlike ``label_term_sums``: the number of listed rows is read back from the device to size `rows`."""
        return _label_order(self, labels, n_labels, filter)

    # ---- clustering: the nearest of K centroids for every row (vs_index_assign) ------------------------------------------------------------------
    def _round_f16(self) -> bool:
        return int(self.info().store_dtype) == nat.VS_F16

    def _assign_call(self, c_dev, b_dev, f, bit0, rows_per_chunk, want_values=True):
        """One vs_index_assign call on device buffers and torch's current stream -> (labels int32 [n_rows], values float32 [n_rows] | None).
        c_dev [K, V] / b_dev [K] | None: float32 CUDA tensors on this index's device; f: None or a shared DocFilter there, read from bit
        `bit0` on."""
        import torch
        dev = torch.device("cuda", self.device)
        n = self.n_rows
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        values = torch.empty(n, dtype=torch.float32, device=dev) if want_values else None
        nat.check(nat.lib().vs_index_assign(self._h, _ptr(c_dev), int(c_dev.stride(0)), int(c_dev.shape[0]), _ptr(b_dev),
                                            _ptr(f.words) if f is not None else None, int(bit0), int(rows_per_chunk), _ptr(labels), _ptr(values),
                                            current_stream(self.device)))
        return labels, values

    def assign(self, centroids, bias=None, filter=None, rows_per_chunk: int = 0) -> Assignment:
        """For every live, allowed document the centroid with the largest value -> Assignment(labels int32 [N], values float32 [N]) on the
        index's device, on torch's current stream.  centroids: float32 [K, V], K <= 4096, rounded to the index dtype as a query is; value(j,
        r) = the fp64 sum, in the row's stored cell order, of the fp32 products centroid[j, col] * v, plus bias[j] when a bias [K] is given,
        rounded once to fp32; ties go to the lowest j.  bias = -``half_norms(centroids)`` makes it the nearest centroid in the Euclidean
        sense.  A deleted or filtered-out document gets -1 / -inf.  filter: ONE set (a DocFilter, a bool mask [N] or ids).  One pass over the
        index: no [K, N] matrix is formed.  rows_per_chunk: 0 = automatic, else a multiple of 64 (a tuning knob)."""
        return _assign(self, centroids, bias, filter, rows_per_chunk)

    def half_norms(self, centroids):
        """float32(0.5 * ||c'_j||^2) per centroid, c' rounded to the index dtype (``centroid_half_norms``) -> float32 [K] on the index's device"""
        import torch
        c, _, _ = _assign_args(centroids, None, self._n_cols())
        nat.require_device()
        return centroid_half_norms(c.to(torch.device("cuda", self.device)), round_f16=self._round_f16(), device=self.device)

    # ---- scores as a field (vs_index_set_scores) ---------------------------------------------------------------------------------------------
    def _set_scores_call(self, q_dev, f, bit0, rows_per_chunk):
        """One vs_index_set_scores call on device buffers and torch's current stream -> float32 CUDA tensor [B, n_rows].  q_dev: contiguous
        float32 / float16 CUDA tensor [B, V] on this index's device; f: None or a DocFilter there, read from bit `bit0` on."""
        import torch
        p, dt, keep, B, ldq = self._q_args(q_dev)
        n = self.n_rows
        out = torch.empty((B, n), dtype=torch.float32, device=torch.device("cuda", self.device))
        if n:
            nat.check(nat.lib().vs_index_set_scores(self._h, p, dt, ldq, B, _ptr(f.words) if f is not None else None, int(bit0),
                                                    f.ld if f is not None else 0, rows_per_chunk, _ptr(out), n, current_stream(self.device)))
        return out

    def set_scores(self, q, filter=None, rows_per_chunk: int = 0):
        """The exact score of every document of a set, as a value array -> float32 [B, N] on the index's GPU: row b holds query b's score
        (search_range's and explain's, bit for bit) of every live document of its set, and NaN -- the missing sentinel of the numeric
        fields -- for every document OUTSIDE the set and every deleted one.  A row of it is a float32 field: ``value_stats``,
        ``value_histogram``, ``value_topk``, ``value_quantiles`` and the breakdowns take it as `values`.  q: [B, V] float32 / float16 (numpy
        or tensor); filter: what search(filter=) accepts -- one set shared by the queries, or one per query (match_filter's result); None:
        every live document.  rows_per_chunk: 0 = automatic, else a multiple of 64 (a tuning knob: no result depends on it).  A dense
        index, and one wider than 32 763 columns, raise NotImplementedError.  Enqueued on torch's current stream."""
        return _set_scores(self, q, filter, rows_per_chunk)

    # ---- set egress: count, list, page and sample a document set (vs_index_set_count / _set_ids / _set_sample) --------------------------------
    def _set_count_call(self, f, bit0, rows_per_chunk):
        """One vs_index_set_count call on torch's current stream -> (counts int64 [B],).  f: None (every live row) or a DocFilter on this
        index's device, read from bit `bit0` on."""
        return _set_count_call(self._h, self.device, self.n_rows, f, bit0, rows_per_chunk)

    def _set_ids_call(self, f, bit0, offsets_dev, limit, id_offset, rows_per_chunk):
        """One vs_index_set_ids call -> (ids int64 [B, limit], counts int64 [B])"""
        return _set_ids_call(self._h, self.device, self.n_rows, f, bit0, offsets_dev, limit, id_offset, rows_per_chunk)

    def _set_sample_call(self, f, bit0, seeds_dev, n, id_offset, rows_per_chunk):
        """One vs_index_set_sample call -> (ids int64 [B, n], hashes int64 [B, n], counts int64 [B])"""
        return _set_sample_call(self._h, self.device, self.n_rows, f, bit0, seeds_dev, n, id_offset, rows_per_chunk)

    def set_count(self, filter=None, rows_per_chunk: int = 0):
        """The number of live documents in a set -> int64 tensor [B] on the index's device.  filter: what search(filter=) accepts -- a
        per-query DocFilter gives one entry per query, a shared one B = 1, None every live document.  Deleted documents never count."""
        return _set_count(self, filter, rows_per_chunk)

    def set_ids(self, filter=None, offset=0, limit=None, rows_per_chunk: int = 0) -> SetIds:
        """The live documents of a set as ids in ascending order -> SetIds(ids int64 [B, limit], counts int64 [B]): ranks [offset, offset +
        limit) of each query's list, -1 behind its last member; counts is the full size of the set whatever the window.  offset: an int or one
        per query; limit=None takes the largest count (one count round first); B x limit <= 2^27 -- page through longer lists.  No atomic
        decides a position: the list is sorted by construction."""
        return _set_ids(self, filter, offset, limit, rows_per_chunk)

    def set_sample(self, n: int, filter=None, seed: int = 0, rows_per_chunk: int = 0) -> SetSample:
        """n live documents of a set, uniformly and without replacement -> SetSample(ids int64 [B, n], counts int64 [B]): the n with the
        smallest (hash(seed + b, id), id) for query b, in that order (``set_sample_hash``); -1 behind the last when the set holds fewer.  The
        same seed gives the same sample, on one index and on a ShardGroup of its rows alike.  n in 1..1024."""
        return _set_sample(self, filter, n, seed, rows_per_chunk)

    def scores(self, q):
        """Dense [B, n_rows] fp32 score matrix (what index.py:91 materialises). numpy out."""
        info = self.info()
        p, dt, keep, B, ldq = self._q_args(q)
        out = np.empty((B, info.n_rows), dtype=np.float32)
        nat.check(nat.lib().vs_index_scores(self._h, p, dt, ldq, B, C.c_void_p(out.ctypes.data), None))
        return out

    def export_csr(self, val_dtype=np.float32):
        """-> (indptr int64, indices int64, data) as numpy arrays (host)."""
        info = self.info()
        indptr = np.empty(info.n_rows + 1, dtype=np.int64)
        nat.check(nat.lib().vs_index_export_csr(self._h, C.c_void_p(indptr.ctypes.data), None, None, nat.VS_F32))
        nnz = int(indptr[-1])
        indices = np.empty(nnz, dtype=np.int64)
        data = np.empty(nnz, dtype=val_dtype)
        nat.check(nat.lib().vs_index_export_csr(self._h, C.c_void_p(indptr.ctypes.data), C.c_void_p(indices.ctypes.data),
                                                C.c_void_p(data.ctypes.data), _NP2VS[np.dtype(val_dtype)]))
        return indptr, indices, data

    def export_dense(self, dtype=np.float32):
        info = self.info()
        out = np.empty((info.n_rows, info.n_cols), dtype=dtype)
        nat.check(nat.lib().vs_index_export_dense(self._h, C.c_void_p(out.ctypes.data), _NP2VS[np.dtype(dtype)], info.n_cols))
        return out


class NotBinaryError(ValueError):
    """a binary (bag-of-token) index was given a stored value other than 1"""


class ShardGroup:
    """Row-sharded search inside one process (``vs_shard_group_*``): one DeviceIndex per GPU holding consecutive row ranges of one
    corpus; search() scores the batch on every GPU, gathers B * k pairs per shard on the first shard's GPU and merges there."""

    def __init__(self, shards):
        nat.require_device()
        self._shards = list(shards)                      # keep them alive: the group does not own the handles
        arr = (C.c_void_p * len(self._shards))(*[s._h for s in self._shards])
        h = C.c_void_p()
        nat.check(nat.lib().vs_shard_group_create(arr, len(self._shards), C.byref(h)))
        self._h = h

    @property
    def n_rows(self) -> int:
        return sum(int(s.info().n_rows) for s in self._shards)

    @property
    def device(self) -> int:
        """the first shard's GPU: where the group's results land"""
        return self._shards[0].device

    @property
    def _parts(self):
        """(shard, its first row) of every part an aggregation runs over"""
        parts, row0 = [], 0
        for sh in self._shards:
            parts.append((sh, row0))
            row0 += sh.n_rows
        return parts

    def _slices(self, on, kind, x):
        """every shard's slice of a per-row column (kind: "labels" | "values"), made a tensor on its GPU by `on`; cached per kind and tensor
        (and its version: an in-place edit drops it)"""
        key = (id(x), getattr(x, "_version", None), tuple(x.shape))
        cache = self.__dict__.setdefault("_slice_cache", {})
        cached = cache.get(kind)
        if cached is not None and cached[0] == key and cached[1] is x:
            return cached[2]
        parts = self._parts
        ends = [row0 for _, row0 in parts[1:]] + [None]
        slices = [on(x[row0:end], sh.device) for (sh, row0), end in zip(parts, ends)]
        if _is_torch(x):                                         # (a numpy array has no version to tell an in-place edit by)
            cache[kind] = (key, x, slices)
        return slices

    def search(self, q, k: int, filter=None):
        """filter: as DeviceIndex.search, over the GROUP's rows (global ids); every shard reads its own row range of it."""
        if q.ndim != 2:
            raise ValueError("queries must be [B, V]")
        p, dt, keep = as_arg(q, (nat.VS_F32, nat.VS_F16))
        B, ldq, k = int(q.shape[0]), int(q.shape[1]), int(k)
        fkeep = None
        if filter is not None:
            from .doc_filter import as_doc_filter
            fkeep = as_doc_filter(filter, self.n_rows, device=self._shards[0].device, batch=B)
        def run(ids_p, sc_p):
            if fkeep is None:
                nat.check(nat.lib().vs_shard_group_search(self._h, p, dt, ldq, B, k, ids_p, sc_p))
            else:
                nat.check(nat.lib().vs_shard_group_search_filtered(self._h, p, dt, ldq, B, k, C.c_void_p(fkeep.words.data_ptr()), fkeep.ld,
                                                                   ids_p, sc_p))
        if _is_torch(q) and q.is_cuda:
            import torch
            dev = torch.device("cuda", self._shards[0].device)
            ids = torch.empty((B, k), dtype=torch.int64, device=dev)
            sc = torch.empty((B, k), dtype=torch.float32, device=dev)
            run(C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()))
            return ids, sc
        ids = np.empty((B, k), dtype=np.int64)
        sc = np.empty((B, k), dtype=np.float32)
        run(C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data))
        return ids, sc

    # ---- mutable index ----------------------------------------------------------------------------------
    def _tombstones(self, fn, ids):
        ids, on_dev = _row_ids(ids)
        nat.require_device()
        n = int(ids.shape[0])
        if n == 0:
            return
        fn = getattr(nat.lib(), fn)
        if on_dev:
            import torch
            torch.cuda.current_stream(ids.device).synchronize()
            nat.check(fn(self._h, C.c_void_p(ids.data_ptr()), n))
        else:
            nat.check(fn(self._h, C.c_void_p(ids.ctypes.data), n))

    def delete_rows(self, ids):
        """DeviceIndex.delete_rows with global ids: every shard marks the rows it owns (vs_shard_group_delete_rows).  Blocking."""
        self._tombstones("vs_shard_group_delete_rows", ids)

    def restore_rows(self, ids=None):
        if ids is None:
            nat.require_device()
            nat.check(nat.lib().vs_shard_group_restore_rows(self._h, None, 0))
            return
        self._tombstones("vs_shard_group_restore_rows", ids)

    @property
    def n_live(self) -> int:
        return sum(s.n_live for s in self._shards)

    def compact(self, rows_extra: int = 0, packets_extra: int = 0):
        """Every shard compacted on its own GPU -> (new ShardGroup, old_ids int64 numpy: the GLOBAL id each new global row had).  The spare
        capacity goes to the last shard (rows are appended at the end of the corpus)."""
        rows_extra, packets_extra = _compact_args(rows_extra, packets_extra)
        new, olds, row0 = [], [], 0
        for i, s in enumerate(self._shards):
            last = i == len(self._shards) - 1
            c, old = s.compact(rows_extra if last else 0, packets_extra if last else 0)
            new.append(c)
            olds.append(old + row0)
            row0 += s.n_rows
        return ShardGroup(new), (np.concatenate(olds) if olds else np.zeros(0, dtype=np.int64))

    def prune(self, topk=None, min_value=None, keep_cols=None, drop_cols=None, protect=None, rows_extra: int = 0, packets_extra: int = 0):
        """DeviceIndex.prune on every shard's own GPU -> (new ShardGroup, kept int32 numpy over the group's rows).  protect: a ShardGroup cut
        at the same rows, shard i on shard i's GPU.  The spare capacity goes to the last shard."""
        rows_extra, packets_extra = _compact_args(rows_extra, packets_extra)
        if protect is not None:
            if not isinstance(protect, ShardGroup):
                raise TypeError(f"protect must be a ShardGroup, got {type(protect).__name__}")
            mine, theirs = [s.n_rows for s in self._shards], [s.n_rows for s in protect._shards]
            if mine != theirs:
                raise ValueError(f"the protect group is cut into rows {theirs}, this group into {mine}: shard i protects shard i")
        new, kepts = [], []
        for i, s in enumerate(self._shards):
            last = i == len(self._shards) - 1
            c, kept = s.prune(topk, min_value, keep_cols, drop_cols, protect._shards[i] if protect is not None else None,
                              rows_extra if last else 0, packets_extra if last else 0)
            new.append(c)
            kepts.append(kept)
        return ShardGroup(new), (np.concatenate(kepts) if kepts else np.zeros(0, dtype=np.int32))

    def select_rows(self, ids) -> "ShardGroup":
        """DeviceIndex.select_rows with GLOBAL ids -> a new ShardGroup: the ids are dealt to the shards in the order given
        (split_by_shard), every shard selects its own on its own GPU, and the new group is the new shards side by side; a shard that
        receives no id is left out.  That is the unsharded selection exactly when the shard of ids[j] never decreases along j -- ascending
        ids, every filter's set_ids() -- and anything else raises ValueError: a selection does not move rows across shards."""
        ids, on_dev = _select_ids(ids)
        nat.require_device()
        parts = self._parts
        cuts = [row0 for _, row0 in parts] + [self.n_rows]
        begin = _split_on_device(ids, cuts) if on_dev else split_by_shard(ids, cuts)
        new = []
        for (sh, row0), a, b in zip(parts, begin[:-1], begin[1:]):
            if b > a:
                new.append(sh.select_rows(ids[int(a):int(b)], id_offset=row0))
        return ShardGroup(new)

    # ---- reweighted index -------------------------------------------------------------------------------------
    def row_stats(self) -> RowStats:
        """DeviceIndex.row_stats of every shard on its own GPU, concatenated on the first shard's: every row is independent, so the answer is
        the unsharded one bit for bit."""
        import torch
        dev = torch.device("cuda", self.device)
        parts = [sh.row_stats() for sh in self._shards]
        return RowStats(*[torch.cat([p[i].to(dev) for p in parts]) for i in range(5)])

    def rescale_plan(self, row_scale=None, col_scale=None, dtype=None):
        """DeviceIndex.rescale_plan of every shard -> a list of (scratch_bytes, lds_bytes, col_route)"""
        return [sh.rescale_plan(row_scale, col_scale, dtype) for sh in self._shards]

    def rescale(self, row_scale=None, col_scale=None, dtype=None, rows_extra: int = 0, packets_extra: int = 0) -> "ShardGroup":
        """DeviceIndex.rescale on every shard's own GPU -> a new ShardGroup cut at the same rows.  row_scale [the group's rows] is cut at the
        shard boundaries, col_scale goes to every shard's GPU; every row is independent, so the shards side by side are the unsharded result
        bit for bit.  The spare capacity goes to the last shard."""
        rows_extra, packets_extra = _compact_args(rows_extra, packets_extra)
        n = self.n_rows
        if row_scale is not None:
            if not hasattr(row_scale, "shape"):
                row_scale = np.asarray(row_scale)
            if tuple(row_scale.shape) != (n,):
                raise ValueError(f"row_scale must have shape ({n},), got {tuple(row_scale.shape)}")
        new = []
        for i, (sh, row0) in enumerate(self._parts):
            last = i == len(self._shards) - 1
            rs = row_scale[row0:row0 + sh.n_rows] if row_scale is not None else None
            new.append(sh.rescale(rs, col_scale, dtype, rows_extra if last else 0, packets_extra if last else 0))
        return ShardGroup(new)

    # ---- combined index ---------------------------------------------------------------------------------------
    def _same_cuts(self, other):
        if not isinstance(other, ShardGroup):
            raise TypeError(f"other must be a ShardGroup, got {type(other).__name__}")
        mine, theirs = [s.n_rows for s in self._shards], [s.n_rows for s in other._shards]
        if mine != theirs:
            raise ValueError(f"the other group is cut into rows {theirs}, this group into {mine}: shard i is combined with shard i")

    def combine_plan(self, other, dtype=None):
        """DeviceIndex.combine_plan of every pair of shards -> a list of CombinePlan"""
        self._same_cuts(other)
        return [a.combine_plan(b, dtype) for a, b in zip(self._shards, other._shards)]

    def combine(self, other, wa=1.0, wb=1.0, dtype=None, rows_extra: int = 0, packets_extra: int = 0) -> "ShardGroup":
        """DeviceIndex.combine shard by shard on the shards' own GPUs -> a new ShardGroup cut at the same rows.  other: a ShardGroup cut at
        the same rows, shard i on shard i's GPU (else ValueError).  Every row is independent, so the shards side by side are the unsharded
        result bit for bit.  The spare capacity goes to the last shard."""
        self._same_cuts(other)
        rows_extra, packets_extra = _compact_args(rows_extra, packets_extra)
        new = []
        for i, (a, b) in enumerate(zip(self._shards, other._shards)):
            last = i == len(self._shards) - 1
            new.append(a.combine(b, wa, wb, dtype, rows_extra if last else 0, packets_extra if last else 0))
        return ShardGroup(new)

    # ---- joined index ---------------------------------------------------------------------------------------
    def gathered(self, device: int = None, dtype=None) -> DeviceIndex:
        """-> the group's rows as ONE DeviceIndex on GPU `device` (default: the first shard's), the shards one behind the other: global row
        ids do not change, deleted rows stay deleted.  Every shard that lives elsewhere is brought to the target GPU with the device-to-device
        slice (slice_rows(0, n, device)), then one concat() joins them; dtype as in DeviceIndex.concat.  During the call the target GPU holds
        the moved shards AND the result at once -- twice the group's packets less the target's own shard; the moved copies are freed before
        the call returns.  The group is untouched."""
        nat.require_device()
        device = self.device if device is None else int(device)
        if len(self._shards) > CONCAT_MAX_SOURCES:
            raise ValueError(f"a join takes at most {CONCAT_MAX_SOURCES} sources, the group has {len(self._shards)} shards")
        moved, local = [], []
        try:
            for sh in self._shards:
                if sh.device == device:
                    local.append(sh)
                else:
                    local.append(sh.slice_rows(0, sh.n_rows, device))
                    moved.append(local[-1])
            return local[0].concat(local[1:], dtype=dtype, device=device)
        finally:
            for m in moved:
                m.close()

    # ---- term constraints -----------------------------------------------------------------------------------
    def _term_words(self, cols, thr=None, want_df=False, live_only=True, ld=None):
        n_cols = int(self._shards[0].info().n_cols)
        return _term_bitmaps(lambda *a: nat.lib().vs_shard_group_term_bitmaps(self._h, *a), self.n_rows, n_cols, self._shards[0].device, cols, thr,
                             want_df, live_only, ld, False)

    def term_bitmaps(self, cols, thr=None):
        """DeviceIndex.term_bitmaps over the group's rows (vs_shard_group_term_bitmaps): every shard scans its rows on its own GPU, the first
        shard's GPU ORs the re-based words together; equal to the unsharded index word for word.  Blocking."""
        return self._term_words(cols, thr)[0]

    def doc_freq(self, cols, thr=None, live_only=True):
        """DeviceIndex.doc_freq summed over the shards."""
        return self._term_words(cols, thr, True, live_only)[1]

    def explain(self, q, ids, topn: int = 10) -> Explanation:
        """DeviceIndex.explain over the group's rows (global ids): every shard explains the pairs it owns on its own GPU, the first
        shard's GPU gathers them; equal to explaining the unsharded index.  Blocking (vs_shard_group_explain)."""
        B, k, topn, on_dev = _explain_args(q, ids, topn)
        nat.require_device()
        p, dt, keep, ldq = None, nat.VS_F32, None, 0
        if q is not None:
            p, dt, keep = as_arg(q, (nat.VS_F32, nat.VS_F16))
            ldq = int(q.shape[1])
        p_ids, _, keep_ids = as_arg(ids, (nat.VS_I64,))
        out, ptrs = _explain_outputs(B, k, topn, self._shards[0].device if on_dev else None)
        if k == 0:
            return Explanation(*out)
        nat.check(nat.lib().vs_shard_group_explain(self._h, p, dt, ldq, B, p_ids, k, k, topn, *ptrs))
        if not on_dev and (_is_torch(ids) or _is_torch(q)):
            import torch
            out = tuple(torch.from_numpy(a) for a in out)
        return Explanation(*out)

    def get_rows(self, ids):
        """DeviceIndex.get_rows over the group's rows (global ids): every shard extracts the rows it owns, the first shard's GPU stitches
        them (vs_shard_group_get_rows); equal to the unsharded index.  Blocking."""
        on_dev = _int64_ids(ids, 1)
        nat.require_device()
        n = int(ids.shape[0])
        p_ids, _, keep = as_arg(ids, (nat.VS_I64,))
        if on_dev:
            import torch
            dev = torch.device("cuda", self._shards[0].device)
            alloc = lambda size, dt: torch.empty(size, dtype=dt, device=dev)
            ptr = lambda t: C.c_void_p(t.data_ptr())
            i64, i32, f32 = torch.int64, torch.int32, torch.float32
        else:
            alloc = lambda size, dt: np.empty(size, dtype=dt)
            ptr = lambda a: C.c_void_p(a.ctypes.data)
            i64, i32, f32 = np.int64, np.int32, np.float32
        indptr = alloc(n + 1, i64)
        nat.check(nat.lib().vs_shard_group_get_rows(self._h, p_ids, n, ptr(indptr), None, None))
        nnz = int(indptr[-1])
        indices, values = alloc(nnz, i32), alloc(nnz, f32)
        if nnz:
            nat.check(nat.lib().vs_shard_group_get_rows(self._h, p_ids, n, ptr(indptr), ptr(indices), ptr(values)))
        if not on_dev and _is_torch(ids):
            import torch
            return torch.from_numpy(indptr), torch.from_numpy(indices), torch.from_numpy(values)
        return indptr, indices, values

    def queries_from_rows(self, ids, weights=None, q=None, alpha: float = 1.0):
        """DeviceIndex.queries_from_rows over the group's rows (global ids): the owners extract the rows, the first shard's GPU accumulates
        them with the same numerics -- equal to the unsharded index bit for bit (vs_shard_group_queries_from_rows).  Blocking."""
        B, m, on_dev = _by_example_args(ids, weights, q)
        nat.require_device()
        V = int(self._shards[0].info().n_cols)
        return _queries_from_rows(lambda *args: nat.lib().vs_shard_group_queries_from_rows(self._h, *args), ids, weights, q, alpha, B, m, V,
                                  self._shards[0].device if on_dev else None, False)

    def search_by_example(self, ids, k: int, weights=None, q=None, alpha: float = 1.0, a=None, exclude: bool = True, filter=None):
        """DeviceIndex.search_by_example over the group's rows (global ids)."""
        return _search_by_example(self, ids, k, weights, q, alpha, a, exclude, filter)

    def search_grouped(self, q, k: int, groups, per_group: int = 1, filter=None, depth=None) -> GroupedResults:
        """DeviceIndex.search_grouped over the group's rows: `groups` and the rounds' bitmaps are global and live on the first shard's GPU;
        every round is a search(filter=) of the group.  Equal to the unsharded index bit for bit."""
        return _search_grouped(self, q, k, per_group, groups, filter, depth)

    def search_diverse(self, q, k: int, lam=0.5, depth=None, sim: str = "cosine", filter=None, max_row_bytes=None) -> DiverseResults:
        """DeviceIndex.search_diverse over the group's rows: the group's search, the candidates' rows stitched from their owners on the first
        shard's GPU (get_rows), the selection there.  Equal to the unsharded index bit for bit."""
        return _search_diverse(self, q, k, lam, depth, sim, filter, max_row_bytes)

    def search_fused(self, qs, k: int, mode: str = "rrf", weights=None, c: float = 60.0, depth=None, filter=None) -> FusedResults:
        """DeviceIndex.search_fused over the group's rows: the group's searches, fused on the first shard's GPU.  Equal to the unsharded
        index bit for bit."""
        return _search_fused(self, qs, k, mode, weights, c, depth, filter)

    def diversify(self, ids, scores, k: int, lam=0.5, sim: str = "cosine", max_row_bytes=None) -> DiverseResults:
        """DeviceIndex.diversify with global ids."""
        return _diversify(self, ids, scores, k, lam, sim, max_row_bytes)

    def search_range(self, q, min_score, max_hits: int = 100, filter=None) -> RangeResults:
        """DeviceIndex.search_range over the group's rows (global ids): every shard runs with its id_offset, the lists are merged on the
        first shard's GPU and the counts summed.  Equal to the unsharded index bit for bit."""
        ids, sc, counts, _ = _range_shards(self, q, min_score, max_hits, filter, False)
        return RangeResults(*_range_out(q, ids, sc, counts))

    def count_matches(self, q, min_score, filter=None):
        """DeviceIndex.count_matches over the group's rows: the shards' counts summed."""
        return _range_out(q, _range_shards(self, q, min_score, 0, filter, False)[2])[0]

    def match_filter(self, q, min_score, filter=None):
        """DeviceIndex.match_filter over the group's rows: the shards' bitmaps at their bit offsets, on the first shard's GPU."""
        from .doc_filter import DocFilter
        return DocFilter(_range_shards(self, q, min_score, 0, filter, True)[3], self.n_rows)

    def _boosted(self, q, boosts, weights, mode, min_score, max_hits, filter, want_words):
        _, thr, K, boost = _boost_args(q, boosts, weights, mode, min_score, max_hits, self.n_rows)
        return _range_shards(self, q, thr, K, filter, want_words, boost)

    def search_boosted(self, q, boosts, weights, mode: str = "add", min_score=None, max_hits: int = 100, filter=None) -> RangeResults:
        """DeviceIndex.search_boosted over the group's rows (global ids): search_range's shard rule -- every shard gets its row slice of every
        field, its id_offset and its bit range of the filter; lists merged, counts summed.  Equal to the unsharded index bit for bit."""
        ids, sc, counts, _ = self._boosted(q, boosts, weights, mode, min_score, max_hits, filter, False)
        return RangeResults(*_range_out(q, ids, sc, counts))

    def count_boosted(self, q, boosts, weights, mode: str = "add", min_score=None, filter=None):
        """DeviceIndex.count_boosted over the group's rows: the shards' counts summed."""
        return _range_out(q, self._boosted(q, boosts, weights, mode, min_score, 0, filter, False)[2])[0]

    def boosted_filter(self, q, boosts, weights, mode: str = "add", min_score=None, filter=None):
        """DeviceIndex.boosted_filter over the group's rows: the shards' bitmaps at their bit offsets, on the first shard's GPU."""
        from .doc_filter import DocFilter
        return DocFilter(self._boosted(q, boosts, weights, mode, min_score, 0, filter, True)[3], self.n_rows)

    # ---- facet counts -----------------------------------------------------------------------------------------------------------------------
    def facet_counts(self, labels, n_labels: int, filter=None, rows_per_chunk: int = 0) -> FacetCounts:
        """DeviceIndex.facet_counts over the group's rows: labels and filter are global; every shard counts its own rows with its slice of
        the labels on its own GPU, the counts are summed on the first shard's GPU.  Equal to the unsharded index exactly."""
        return _facet_counts(self, labels, n_labels, filter, rows_per_chunk)

    def top_facets(self, labels, n_labels: int, topn: int, filter=None, min_count: int = 1) -> TopFacets:
        """DeviceIndex.top_facets over the group's rows: the top-n is taken after the shards' counts are summed, never per shard."""
        return _top_facets(self, labels, n_labels, topn, filter, min_count)

    # ---- numeric fields -----------------------------------------------------------------------------------------------------------------------
    def value_range_filter(self, values, lo=None, hi=None):
        """DeviceIndex.value_range_filter over the group's rows: every shard writes the bits of its slice of the values at its bit offset of
        one bitmap on the first shard's GPU."""
        return _value_range_filter(self, values, lo, hi)

    def value_stats(self, values, filter=None, rows_per_chunk: int = 0) -> ValueStats:
        """DeviceIndex.value_stats over the group's rows: values and filter are global; counts and sums are added, min and max combined on
        the order keys (an int32 value never passes through a float).  Equal to the unsharded index exactly."""
        return _value_stats(self, values, filter, rows_per_chunk)

    def value_histogram(self, values, edges, filter=None, rows_per_chunk: int = 0) -> ValueHistogram:
        """DeviceIndex.value_histogram over the group's rows: the shards' bins are added on the first shard's GPU."""
        return _value_histogram(self, values, edges, filter, rows_per_chunk)

    # ---- breakdowns -----------------------------------------------------------------------------------------------------------------------------
    def facet_value_stats(self, labels, n_labels: int, values, filter=None, rows_per_chunk: int = 0) -> FacetValueStats:
        """DeviceIndex.facet_value_stats over the group's rows: labels, values and filter are global; counts and sums are added on the first
        shard's GPU, min and max combined on the order keys over [S, B, L].  Equal to the unsharded index exactly."""
        return _facet_value_stats(self, labels, n_labels, values, filter, rows_per_chunk)

    def facet_value_histogram(self, labels, n_labels: int, values, edges, filter=None, rows_per_chunk: int = 0) -> FacetValueHistogram:
        """DeviceIndex.facet_value_histogram over the group's rows: the shards' bins are added on the first shard's GPU."""
        return _facet_value_histogram(self, labels, n_labels, values, edges, filter, rows_per_chunk)

    def value_topk(self, values, k: int, descending: bool = True, filter=None, rows_per_chunk: int = 0) -> SortedResults:
        """DeviceIndex.value_topk over the group's rows (global ids): every shard lists its k best with its id offset; the lists are merged by
        (order key, id) on the first shard's GPU."""
        return _value_topk(self, values, k, descending, filter, 0, rows_per_chunk)

    def value_quantiles(self, values, q=None, method: str = "lower", ranks=None, filter=None, rows_per_chunk: int = 0) -> ValueQuantiles:
        """DeviceIndex.value_quantiles over the group's rows: three rounds of level calls -- every shard counts the level's digits of its
        slice of the values and its bit range of the filter, the counts are added on the first shard's GPU, one step there picks each rank's
        bin and names the next level's slots.  Integer counts: equal to the unsharded index bit for bit."""
        return _value_quantiles(self, values, q, method, ranks, filter, rows_per_chunk)

    def facet_value_quantiles(self, labels, n_labels: int, values, q=None, method: str = "lower", ranks=None, filter=None,
                              rows_per_chunk: int = 0) -> FacetValueQuantiles:
        """DeviceIndex.facet_value_quantiles over the group's rows: per level every shard counts its slice on its GPU, the counts are added on
        the first shard's GPU, one value_radix_step over B x n_labels cells runs there and its state goes back to the shards.  Equal to the
        unsharded index bit for bit."""
        return _facet_value_quantiles(self, labels, n_labels, values, q, method, ranks, filter, rows_per_chunk)

    # ---- term aggregations ------------------------------------------------------------------------------------------------------------------
    def term_counts(self, filter=None, ids=None, rows_per_chunk: int = 0) -> TermCounts:
        """DeviceIndex.term_counts over the group's rows: filter and ids are global.  Every shard counts on its own GPU -- its bit range of
        the filter, or the ids with its first row as the id offset (ids it does not own are skipped) -- and counts and total are summed on
        the first shard's GPU.  Equal to the unsharded index exactly.  An id outside the group raises ValueError (host lists)."""
        return _term_counts(self, filter, ids, rows_per_chunk)

    def top_terms(self, filter=None, ids=None, topn: int = 20, method: str = "jlh", min_count: int = 1, background=None) -> TopTerms:
        """DeviceIndex.top_terms over the group's rows: the top-n is taken after the shards' counts are summed, never per shard."""
        return _top_terms(self, filter, ids, topn, method, min_count, background)

    def term_sums(self, filter=None, ids=None, rows_per_chunk: int = 0, tile_cols: int = 0) -> TermSums:
        """DeviceIndex.term_sums over the group's rows: filter and ids are global.  Every shard sums on its own GPU -- its bit range of the
        filter, or the ids with its first row as the id offset (ids it does not own are skipped) -- and sums and total are added on the
        first shard's GPU.  The additions are integer: equal to the unsharded index exactly.  An id outside the group raises ValueError
        (host lists)."""
        return _term_sums(self, filter, ids, rows_per_chunk, tile_cols)

    def top_weight_terms(self, filter=None, ids=None, topn: int = 20, min_count: int = 0) -> TopWeights:
        """DeviceIndex.top_weight_terms over the group's rows: the top-n is taken after the shards' sums are added, never per shard."""
        return _top_weights(self, filter, ids, topn, min_count)

    def label_term_sums(self, labels, n_labels: int, filter=None, rows_per_item: int = 0, tile_cols: int = 0) -> LabelTermSums:
        """DeviceIndex.label_term_sums over the group's rows: labels and filter are global.  Every shard takes its slice of the labels and
        its bit range of the filter on its own GPU; sums, total and other are added on the first shard's GPU.  The additions are integer:
        equal to the unsharded index bit for bit."""
        return _label_terms(self, "vs_index_label_term_sums", LabelTermSums, labels, n_labels, filter, rows_per_item, tile_cols)

    def label_term_counts(self, labels, n_labels: int, filter=None, rows_per_item: int = 0, tile_cols: int = 0) -> LabelTermCounts:
        """DeviceIndex.label_term_counts over the group's rows, as ``label_term_sums``."""
        return _label_terms(self, "vs_index_label_term_counts", LabelTermCounts, labels, n_labels, filter, rows_per_item, tile_cols)

    def label_order(self, labels, n_labels: int, filter=None) -> LabelOrder:
        """DeviceIndex.label_order over the group's rows: a label's segment holds the shards' segments one behind the other, global ids.
        Every shard's count of listed rows is read back before the next shard is called: the shards run one after the other (a facade for
        pinning the order, not a hot path -- ``label_term_sums`` keeps the order on the device and only enqueues)."""
        return _label_order(self, labels, n_labels, filter)

    def assign(self, centroids, bias=None, filter=None, rows_per_chunk: int = 0) -> Assignment:
        """DeviceIndex.assign over the group's rows: the centroids and the bias are copied to every shard's GPU, every shard assigns its rows
        under its bit range of the filter, and the answers are concatenated on the first shard's GPU.  A row's value depends on nothing
        but the row: equal to the unsharded index bit for bit."""
        return _assign(self, centroids, bias, filter, rows_per_chunk)

    def set_scores(self, q, filter=None, rows_per_chunk: int = 0):
        """DeviceIndex.set_scores over the group's rows: every shard scores its rows under its bit range of the filter on its own GPU, and
        the slices are placed side by side on the first shard's GPU.  A row's score depends on nothing but the row and the query: equal
        to the unsharded index bit for bit."""
        return _set_scores(self, q, filter, rows_per_chunk)

    # ---- set egress ---------------------------------------------------------------------------------------------------------------------------
    def set_count(self, filter=None, rows_per_chunk: int = 0):
        """DeviceIndex.set_count over the group's rows: every shard counts its bit range of the filter, the counts are added."""
        return _set_count(self, filter, rows_per_chunk)

    def set_ids(self, filter=None, offset=0, limit=None, rows_per_chunk: int = 0) -> SetIds:
        """DeviceIndex.set_ids over the group's rows (global ids): after a count round shard s lists its local window [offset - C_s, offset -
        C_s + limit) clipped at 0 -- C_s the count of the shards before it -- with its first row as the id offset, and the pieces are placed
        one behind the other on the first shard's GPU.  Equal to the unsharded index bit for bit."""
        return _set_ids(self, filter, offset, limit, rows_per_chunk)

    def set_sample(self, n: int, filter=None, seed: int = 0, rows_per_chunk: int = 0) -> SetSample:
        """DeviceIndex.set_sample over the group's rows: every shard samples n with its first row as the id offset -- the GLOBAL id is what
        is hashed -- and the lists merge by (hash, id), cut to n.  Equal to the unsharded index bit for bit."""
        return _set_sample(self, filter, n, seed, rows_per_chunk)

    def half_norms(self, centroids):
        """DeviceIndex.half_norms, on the first shard's GPU (the shards share the store dtype)"""
        return self._shards[0].half_norms(centroids)

    def close(self):
        if self._h:
            nat.lib().vs_shard_group_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merge_topk(cand_ids, cand_scores, k: int, device: int = 0):
    """Canonical top-k of gathered per-shard candidates [B, n_cand] (global ids + scores)."""
    nat.require_device()
    p_i, _, k1 = as_arg(cand_ids, (nat.VS_I64,))
    p_s, _, k2 = as_arg(cand_scores, (nat.VS_F32,))
    B, n = int(cand_ids.shape[0]), int(cand_ids.shape[1])
    if _is_torch(cand_ids) and cand_ids.is_cuda:
        import torch
        ids = torch.empty((B, k), dtype=torch.int64, device=cand_ids.device)
        sc = torch.empty((B, k), dtype=torch.float32, device=cand_ids.device)
        nat.check(nat.lib().vs_merge_topk(p_i, p_s, B, n, int(k), C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()),
                                          int(device), current_stream(device)))
        return ids, sc
    ids = np.empty((B, k), dtype=np.int64)
    sc = np.empty((B, k), dtype=np.float32)
    nat.check(nat.lib().vs_merge_topk(p_i, p_s, B, n, int(k), C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data), int(device), None))
    if _is_torch(cand_ids):
        import torch
        return torch.from_numpy(ids), torch.from_numpy(sc)
    return ids, sc


class Profile:
    """bench.py hook: hipEvent timing of the scoring kernels (vs_profile_*)."""

    @staticmethod
    def enable(on=True):
        nat.check(nat.lib().vs_profile_enable(int(bool(on))))

    @staticmethod
    def reset():
        nat.check(nat.lib().vs_profile_reset())

    @staticmethod
    def read(kernel: str):
        ms, n = C.c_double(0), C.c_int64(0)
        nat.check(nat.lib().vs_profile_read(kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value
