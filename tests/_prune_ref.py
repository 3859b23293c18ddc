"""The numpy reference of index pruning (vs_index_prune, include/vsearch_hip.h), restated cell by cell.

For row r with stored cells (col_t, v_t), t = 0..n-1 in STORED ORDER (the order export_csr returns; padding cells are not cells):
  eligible_t  = col_keep[col_t] and (min_value is None or v_t >= min_value)      -- on the fp32-widened stored value; a NaN is never >=
  key_t       = value_key_f32(bits(v_t))                                         -- -0.0 and +0.0 tie, -inf < finite < +inf, NaN -> 0 (last)
  rank        = position among the eligible cells by (key descending, t ascending);   top_t = rank < topk   (topk 0 / None: no cut)
  protected_t = row r of the protect index stores col_t (whatever its value)
  kept_t      = eligible_t and (top_t or protected_t)
The new row is the kept cells in stored order with their stored bits.  A plain loop over the rows: slow and obviously right."""
import numpy as np


def value_key_f32(values):
    """fp32 values -> the uint32 order keys of the numeric fields (value_check.h): NaN -> 0, -0.0 == +0.0, monotone otherwise"""
    u = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).copy()
    mag = u & np.uint32(0x7FFFFFFF)
    u[mag == 0] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[mag > np.uint32(0x7F800000)] = 0
    return key


def keep_row(cols, vals, topk=None, min_value=None, col_keep=None, protect_cols=None):
    """bool [n]: which cells of one row stay.  vals: the fp32-widened stored values, or None for a binary row (col_keep only)."""
    n = len(cols)
    elig = np.ones(n, dtype=bool)
    if col_keep is not None:
        elig &= np.asarray(col_keep, dtype=bool)[cols]
    if vals is None:
        assert not topk and min_value is None, "a binary index is cut by col_keep alone"
        return elig
    vals = np.asarray(vals, dtype=np.float32)
    if min_value is not None:
        with np.errstate(invalid="ignore"):
            elig &= vals >= np.float32(min_value)
    top = np.ones(n, dtype=bool)
    if topk:
        t = np.nonzero(elig)[0]
        order = t[np.argsort(-value_key_f32(vals[t]).astype(np.int64), kind="stable")]     # (key descending, t ascending)
        top = np.zeros(n, dtype=bool)
        top[order[:topk]] = True
    prot = np.zeros(n, dtype=bool)
    if protect_cols is not None:
        prot = np.isin(cols, protect_cols)
    return elig & (top | prot)


def prune_ref(indptr, indices, data, topk=None, min_value=None, col_keep=None, protect=None):
    """CSR in stored order -> (indptr, indices, data, kept) of the pruned index.  data None: binary.  protect: (indptr, indices) of the
    protect index's rows, or None.  data keeps its dtype and bits."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    n_rows = len(indptr) - 1
    keep = np.zeros(len(indices), dtype=bool)
    for r in range(n_rows):
        a, b = indptr[r], indptr[r + 1]
        pc = None
        if protect is not None:
            pc = np.asarray(protect[1])[protect[0][r]:protect[0][r + 1]]
        vals = None if data is None else np.asarray(data[a:b]).astype(np.float32)
        keep[a:b] = keep_row(indices[a:b], vals, topk, min_value, col_keep, pc)
    kept = np.zeros(n_rows, dtype=np.int32)
    for r in range(n_rows):
        kept[r] = keep[indptr[r]:indptr[r + 1]].sum()
    new_ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(kept, out=new_ptr[1:])
    return new_ptr, indices[keep], (None if data is None else np.asarray(data)[keep]), kept


def dense_to_csr(mat):
    """the non-zeros of a dense [B, V] matrix in column order (Tensor.to_sparse_csr)"""
    mat = np.asarray(mat)
    nz = mat != 0
    indptr = np.zeros(mat.shape[0] + 1, dtype=np.int64)
    np.cumsum(nz.sum(axis=1), out=indptr[1:])
    rows, cols = np.nonzero(nz)
    return indptr, cols.astype(np.int64), mat[rows, cols]
