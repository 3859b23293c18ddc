"""numpy reference of the sub-index (vs_index_select_rows): the CSR row gather, the per-shard split rule of a row-sharded
selection and the order of Index.sorted_by.  Plain numpy; nothing here touches the library."""
import numpy as np


def select_ref(indptr, indices, data, ids):
    """rows `ids` of the CSR (indptr, indices, data) in that order, repeats kept -> (indptr int64, indices, data); data may be None (a binary
    index).  An id outside [0, n_rows) -- -1 included -- raises IndexError: a selected row has to exist."""
    indptr = np.asarray(indptr, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    n_rows = len(indptr) - 1
    if ids.ndim != 1 or ids.size == 0:
        raise ValueError("empty selection")
    if ids.min() < 0 or ids.max() >= n_rows:
        raise IndexError("an id outside the index")
    lengths = indptr[ids + 1] - indptr[ids]
    new_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    # cell t of new row j is cell indptr[ids[j]] + t of the source
    take = np.repeat(indptr[ids] - new_ptr[:-1], lengths) + np.arange(new_ptr[-1], dtype=np.int64)
    return new_ptr, np.asarray(indices)[take], None if data is None else np.asarray(data)[take]


def split_by_shard(ids, cuts):
    """The shard rule: global ids dealt to the shards whose rows are [cuts[s], cuts[s + 1]) IN THE ORDER GIVEN -> the list of (shard, local
    ids) of the shards that receive an id.  The shard of ids[i] must never decrease along i (the unsharded answer is then the shards side by
    side); anything else, and an id outside every shard, raises ValueError."""
    ids = np.asarray(ids, dtype=np.int64)
    cuts = np.asarray(cuts, dtype=np.int64)
    if ids.size and (ids.min() < 0 or ids.max() >= cuts[-1]):
        raise ValueError("an id outside the group")
    shard = np.searchsorted(cuts, ids, side="right") - 1
    if (np.diff(shard) < 0).any():
        raise ValueError("the selection goes back to an earlier shard")
    return [(int(s), ids[shard == s] - cuts[s]) for s in np.unique(shard)]


def order_key(values, labels=False):
    """the uint32 order keys of the numeric fields (value_check.h) as int64, 0 = missing: float32 by value with -0.0 = +0.0 and a NaN missing,
    int32 by value with INT32_MIN missing; labels=True: code + 1, so that -1 = no label is missing"""
    v = np.asarray(values)
    if labels:
        return v.astype(np.int64) + 1
    if v.dtype == np.float32:
        u = v.view(np.uint32).astype(np.int64)
        mag = u & 0x7FFFFFFF
        u = np.where(mag == 0, 0, u)
        key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
        return np.where(mag > 0x7F800000, 0, key)
    if v.dtype == np.int32:
        return (v.view(np.uint32).astype(np.int64)) ^ 0x80000000
    raise TypeError(f"a value field is float32 or int32, got {v.dtype}")


def sort_order(keys, live, descending=False):
    """The order of sorted_by: the live documents by (key, id) -- key descending when asked, the id ascending always -- with the missing
    (key 0) last in id order -> the document ids, int64"""
    keys = np.asarray(keys, dtype=np.int64)
    ids = np.nonzero(np.asarray(live, dtype=bool))[0].astype(np.int64)
    k = keys[ids]
    missing = k == 0
    rank = np.where(missing, 1 << 32, (0xFFFFFFFF - k) if descending else k)
    return ids[np.lexsort((ids, rank))]
