"""numpy reference of the clustering calls (vs_index_assign / vs_centroid_half_norms / vs_label_bitmaps and the k-means loop).

The contract.  c'_j = centroid j rounded to the index dtype as a query is (an fp16 store: to fp16, nearest even, widened again; fp32 and binary stores:
as given).  For a row r with stored cells (col_t, v_t) in STORED order (v = 1 on a binary index; cells carrying the padding id n_cols are skipped):
    S(j, r)     = the fp64 sum, starting at +0.0, in the row's stored cell order, of float64(float32(c'_j[col_t] * v_t))
    value(j, r) = float32(S)  without a bias,  float32(S + float64(bias[j]))  with one;  a NaN value counts -- and is reported -- as -inf, a -0.0 as +0.0
    label(r)    = the lowest j whose value is largest, values compared as floats
A row that is deleted or not allowed gets label -1 / value -inf.  The sum is a plain loop over the cell POSITIONS (vectorised over rows and
centroids, never over the cells of a row), so it is the order of the kernel whatever the values are.
Half norms: hn[j] = float32(0.5 * T_j), T_j from 256 strided fp64 partial sums of float32(c' * c') and a halving tree.
Rows come as a CSR (indptr, indices, values | None), e.g. what get_rows returns."""
import numpy as np

import _term_sum_ref as tref
from _facet_ref import pack, unpack  # noqa: F401

MAX_K = 4096
MAX_VALUES = 4096
UPDATE_BATCH = 64
F32 = np.float32


def round_store(c, store="fp32"):
    """the centroids as the kernel multiplies them: float32, through fp16 on an fp16 store"""
    c = np.asarray(c, dtype=F32)
    return c.astype(np.float16).astype(F32) if store == "fp16" else c


def canon(v):
    """float32 values as the kernel reports them: NaN -> -inf, -0.0 -> +0.0"""
    v = np.asarray(v, dtype=F32).copy()
    v[np.isnan(v)] = -np.inf
    v[v == 0] = 0.0
    return v


def values_matrix(indptr, indices, values, n_cols, centroids, bias=None, store="fp32"):
    """float32 [n_rows, K]: value(j, r) for every row, live or not"""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    vals = np.ones(indices.size, dtype=F32) if values is None else np.asarray(values).astype(F32)
    Ct = np.ascontiguousarray(round_store(centroids, store).T)                     # [n_cols, K]
    n, K = indptr.size - 1, Ct.shape[1]
    lens = np.diff(indptr)
    S = np.zeros((n, K), dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(int(lens.max()) if n else 0):                                   # cell position t of every row that has one
            rows = np.flatnonzero(lens > t)
            at = indptr[rows] + t
            keep = indices[at] < n_cols                                                # the padding id is skipped
            rows, at = rows[keep], at[keep]
            prod = (Ct[indices[at]] * vals[at][:, None]).astype(F32)                   # rounded to fp32, then widened
            S[rows] += prod.astype(np.float64)
        if bias is not None:
            S = S + np.asarray(bias, dtype=F32).astype(np.float64)[None, :]
        return canon(S.astype(F32))


def assign(indptr, indices, values, n_cols, centroids, bias=None, allowed=None, store="fp32"):
    """-> (labels int32 [n_rows], values float32 [n_rows]); allowed: bool [n_rows] (live AND filter) or None"""
    val = values_matrix(indptr, indices, values, n_cols, centroids, bias, store)
    labels = np.argmax(val, axis=1).astype(np.int32)                                   # (the first of equal maxima: the lowest j; -0.0 is gone)
    best = val[np.arange(val.shape[0]), labels]
    if allowed is not None:
        off = ~np.asarray(allowed, dtype=bool)
        labels[off] = -1
        best[off] = -np.inf
    return labels, best.astype(F32)


def assign_loop(indptr, indices, values, n_cols, centroids, bias=None, allowed=None, store="fp32"):
    """the same by a plain triple Python loop over rows, centroids and cells"""
    c = round_store(centroids, store)
    n, K = len(indptr) - 1, c.shape[0]
    labels, best = np.full(n, -1, np.int32), np.full(n, -np.inf, F32)
    old = np.seterr(over="ignore", invalid="ignore")
    for r in range(n):
        if allowed is not None and not allowed[r]:
            continue
        top = None
        for j in range(K):
            s = np.float64(0.0)
            for i in range(int(indptr[r]), int(indptr[r + 1])):
                col = int(indices[i])
                if col >= n_cols:
                    continue
                v = F32(1.0) if values is None else F32(values[i])
                s = s + np.float64(F32(c[j, col] * v))
            if bias is not None:
                s = s + np.float64(F32(bias[j]))
            f = F32(s)
            if np.isnan(f):
                f = F32(-np.inf)
            if f == 0:
                f = F32(0.0)
            if top is None or f > top:
                top, labels[r] = f, j
        best[r] = top
    np.seterr(**old)
    return labels, best


def half_norms(centroids, store="fp32"):
    """float32 [K] in the fixed order: x[t] = sum over columns t, t + 256, ... (ascending) of float64(float32(c' * c')), then the halving tree"""
    c = round_store(centroids, store)
    sq = (c * c).astype(F32).astype(np.float64)
    K, V = sq.shape
    x = np.zeros((K, 256), dtype=np.float64)
    for c0 in range(0, V, 256):
        w = min(256, V - c0)
        x[:, :w] += sq[:, c0:c0 + w]
    h = 128
    while h >= 1:
        x[:, :h] += x[:, h:2 * h]
        h //= 2
    return (0.5 * x[:, 0]).astype(F32)


def half_norms_tree(centroid, store="fp32"):
    """one centroid, the tree spelled out with Python floats"""
    c = round_store(np.asarray(centroid, dtype=F32)[None, :], store)[0]
    x = [0.0] * 256
    for col in range(c.size):
        x[col % 256] = x[col % 256] + float(F32(c[col] * c[col]))
    for h in (128, 64, 32, 16, 8, 4, 2, 1):
        for t in range(h):
            x[t] = x[t] + x[t + h]
    return F32(0.5 * x[0])


def label_bitmaps(labels, values, bit0=0, ld_words=None):
    """uint32 [B, ld_words]: bit bit0 + r of row b set iff labels[r] == values[b]; every other bit of the span's words 0; words behind the span
    (ld_words > span) are 0 here -- the call leaves them alone"""
    labels = np.asarray(labels, dtype=np.int64)
    values = np.atleast_1d(np.asarray(values, dtype=np.int64))
    return pack(labels[None, :] == values[:, None], bit0, 0, ld_words)


def plan(n_rows, K, n_cols, rows_per_chunk=0, auto_chunks=4096, min_rows=256):
    """the plan rule of vs_assign_plan -> (slice_w, slices, chunks, rows_per_chunk, slab_bytes)"""
    w = 64 if K <= 64 else (128 if K <= 128 else 256)
    slices = -(-K // w)
    if rows_per_chunk == 0:
        rows_per_chunk = max(-(-n_rows // auto_chunks), min_rows)
        rows_per_chunk = -(-rows_per_chunk // 64) * 64
    return w, slices, -(-n_rows // rows_per_chunk), rows_per_chunk, (n_cols + 1) * w * slices * 4


def kmeans(indptr, indices, values, n_cols, start, iters, metric="l2", allowed=None, store="fp32"):
    """Lloyd's loop as the library runs it -> (centroids float32 [K, V], labels, values, counts int64 [K], n_iter, changed list).
    start: float32 [K, V].  Update: per cluster the fixed-point term sums of its rows and their mean (tests/_term_sum_ref.py); an empty cluster
    keeps its centroid.  The labels returned are the assignment under the centroids returned."""
    C = np.array(start, dtype=F32, copy=True)
    K = C.shape[0]
    n = len(indptr) - 1
    cells = tref.Cells(indptr, indices, values, n_cols)
    ok = np.ones(n, bool) if allowed is None else np.asarray(allowed, dtype=bool)

    def step():
        bias = -half_norms(C, store) if metric == "l2" else None
        return assign(indptr, indices, values, n_cols, C, bias, ok, store)

    prev, changed, stale = None, [], True
    for _ in range(iters):
        cur = step()
        stale = False
        changed.append(int((cur[0] >= 0).sum()) if prev is None else int((cur[0] != prev[0]).sum()))
        prev = cur
        if changed[-1] == 0:
            break
        for b0 in range(0, K, UPDATE_BATCH):
            batch = np.arange(b0, min(K, b0 + UPDATE_BATCH))
            masks = (cur[0][None, :] == batch[:, None]) & ok[None, :]
            words = pack(masks)
            sums, total = tref.term_sums(words, words.shape[1], 0, cells)
            mean = tref.mean(sums, total)
            C[batch] = np.where((total > 0)[:, None], mean, C[batch])
        stale = True
    if stale:
        prev = step()
    counts = np.bincount(prev[0][prev[0] >= 0], minlength=K).astype(np.int64)
    return C, prev[0], prev[1], counts, len(changed), changed


def grid(rng, shape, lo=-4.0, hi=4.0, denom=256):
    """multiples of 1 / denom (2^-8) in [lo, hi]: products of two are exact in fp32, sums of fewer than 2^16 of them exact in fp64 in any order"""
    return (rng.integers(int(lo * denom), int(hi * denom) + 1, size=shape) / float(denom)).astype(F32)
