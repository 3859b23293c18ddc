"""Numpy references of the term filters (vs_index_term_bitmaps, vs_term_filter_combine; vsearch_amd.doc_filter.DocFilter.from_terms).

A row HAS term c iff it stores column c with a non-zero value; under a threshold t iff the stored value v satisfies v >= t (so a stored
zero counts under t <= 0).  data=None is a binary index: every stored value is 1.  A program allows a row iff it has every must term, no
must_not term and at least min_should of the should terms.

Two independent formulations: term_bitmaps_ref + combine_ref work term by term on the CSR arrays and on packed words (as the library
does); allowed_mask_ref walks the rows one by one with Python sets.  tests/test_term_filter_cpu.py holds them against each other."""
import numpy as np


def pack_bits(mask):
    """bool [..., n] -> uint32 words [..., ceil(n / 32)]: bit r = bit r & 31 of word r >> 5, the bits past n are 0"""
    mask = np.asarray(mask, dtype=bool)
    n = mask.shape[-1]
    W = (n + 31) // 32
    padded = np.zeros(mask.shape[:-1] + (W * 32,), dtype=np.uint8)
    padded[..., :n] = mask
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view(np.uint32).reshape(mask.shape[:-1] + (W,))


def unpack_words(words, n):
    """uint32 / int32 words [..., W] -> bool [..., n]"""
    w = np.ascontiguousarray(words).view(np.uint32)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder="little")
    return bits[..., :n].astype(bool)


def _thr_array(cols, thr):
    """thr: None | dict {column: t} | one entry per term (None / NaN: no threshold) -> float64 [T] with NaN for none"""
    T = len(cols)
    if thr is None:
        return np.full(T, np.nan)
    if isinstance(thr, dict):
        return np.array([float(thr.get(int(c), np.nan)) for c in cols], dtype=np.float64)
    return np.array([np.nan if t is None else float(t) for t in thr], dtype=np.float64)


def term_masks_ref(indptr, indices, data, n_rows, cols, thr=None):
    """bool [T, n_rows]: row r has term cols[t]"""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    row_of = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(indptr[:n_rows + 1]))
    vals = np.ones(indices.shape[0], dtype=np.float32) if data is None else np.asarray(data).astype(np.float32)
    t_arr = _thr_array(cols, thr)
    out = np.zeros((len(cols), n_rows), dtype=bool)
    for t, c in enumerate(cols):
        sel = indices == int(c)
        v = vals[sel]
        ok = (v != 0) if np.isnan(t_arr[t]) else (v >= np.float32(t_arr[t]))
        out[t, row_of[sel][ok]] = True
    return out


def term_bitmaps_ref(indptr, indices, data, n_rows, cols, thr=None):
    """uint32 words [T, ceil(n_rows / 32)]: what vs_index_term_bitmaps writes"""
    return pack_bits(term_masks_ref(indptr, indices, data, n_rows, cols, thr))


def combine_ref(term_words, n_rows, must, must_not, should, min_should):
    """vs_term_filter_combine on packed words: term_words uint32 [T, W]; must / must_not / should int [B, n] of indices into the T bitmaps
    padded with -1; min_should int [B] -> uint32 [B, W]"""
    term_words = np.asarray(term_words).view(np.uint32) if len(term_words) else np.zeros((0, (n_rows + 31) // 32), np.uint32)
    W = (n_rows + 31) // 32
    B = len(min_should)
    tail = np.full(W, 0xFFFFFFFF, dtype=np.uint32)
    if n_rows & 31:
        tail[-1] = (1 << (n_rows & 31)) - 1
    out = np.zeros((B, W), dtype=np.uint32)
    for b in range(B):
        acc = tail.copy()
        for i in must[b]:
            if i >= 0:
                acc &= term_words[i]
        for i in must_not[b]:
            if i >= 0:
                acc &= ~term_words[i]
        ms = int(min_should[b])
        if ms > 0:
            count = np.zeros(W * 32, dtype=np.int32)
            for i in should[b]:
                if i >= 0:
                    count += np.unpackbits(term_words[i].view(np.uint8), bitorder="little")
            acc &= pack_bits(count >= ms)
        out[b] = acc
    return out


def allowed_mask_ref(indptr, indices, data, n_rows, must=None, must_not=None, should=None, min_should=None, thr=None, B=None):
    """Brute force on bool arrays, row by row: bool [B, n_rows] (B = 1 for a shared program).  Each list: column ids, or one list per
    query; min_should None = 1 where the query's should list is non-empty, else 0; thr = {column: t}."""
    def per_query(x):
        if x is None:
            return None
        x = list(x)
        return [list(it) for it in x] if x and all(isinstance(it, (list, tuple, np.ndarray)) for it in x) else None
    lists = {"must": must, "must_not": must_not, "should": should}
    nested = {k: per_query(v) for k, v in lists.items()}
    if B is None:
        sizes = [len(v) for v in nested.values() if v is not None]
        if isinstance(min_should, (list, tuple, np.ndarray)):
            sizes.append(len(min_should))
        B = sizes[0] if sizes else 1
    def of(name, b):
        if nested[name] is not None:
            return [int(c) for c in nested[name][b]]
        return [int(c) for c in (lists[name] if lists[name] is not None else [])]
    thr = thr or {}
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    out = np.zeros((B, n_rows), dtype=bool)
    # the stored entries of the columns any list names, row by row (the other entries cannot matter)
    named = sorted({c for name in lists for b in range(B) for c in of(name, b)})
    row_of = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(indptr[:n_rows + 1]))
    rows_stored = [dict() for _ in range(n_rows)]
    for j in np.nonzero(np.isin(indices, named))[0]:
        rows_stored[int(row_of[j])].setdefault(int(indices[j]), []).append(np.float32(1.0) if data is None else np.float32(data[j]))
    for r in range(n_rows):
        stored = rows_stored[r]
        def has(c):
            vs = stored.get(c, [])
            if c in thr:
                return any(v >= np.float32(thr[c]) for v in vs)
            return any(v != 0 for v in vs)
        for b in range(B):
            sh = set(of("should", b))
            if isinstance(min_should, (list, tuple, np.ndarray)):
                ms = int(min_should[b])
            else:
                ms = (1 if sh else 0) if min_should is None else int(min_should)
            ok = all(has(c) for c in set(of("must", b))) and not any(has(c) for c in set(of("must_not", b)))
            ok = ok and (ms <= 0 or sum(has(c) for c in sh) >= ms)
            out[b, r] = ok
    return out
