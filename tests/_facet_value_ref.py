"""numpy reference of the breakdowns (vs_facet_value_stats / vs_facet_value_histogram) and the case generators of their tests.

The contract: a set is a bitmap as in _facet_ref / _value_ref (bit bit0 + r of the bitmap at words + b * ld stands for row r, ANDed with
`and_words`); labels are int32 [n_rows], values float32 / int32 [n_rows] with the missing sentinel NaN / INT32_MIN.  For a row of query b's set:
    its label is outside [0, n_labels), -1 included:  other[b] += 1 and nothing else, whether or not it has a value
    its label is l and it has a value:                 count[b, l] += 1, min / max[b, l] on the order key, sum[b, l] += fx(v) (modulo 2^64)
    its label is l and it has no value:                missing[b, l] += 1
    total[b] = the size of the set
min / max of a cell with count 0 hold the missing sentinel; of -0.0 and +0.0 the answer is +0.0.  The histogram takes the bin rule of
_value_ref.histogram (searchsorted(side="right")) per label.  Everything is decided on the uint32 order keys (`_value_ref.key`), so every
output is an integer or a 32-bit pattern and compares exactly (`_value_ref.same`).  Plain loops over the rows / np.add.at: tests/
test_facet_value_cpu.py holds this file against _value_ref and _facet_ref label by label."""
import numpy as np

import _value_ref as vref
from _facet_ref import labels_case  # noqa: F401  (random labels with -1 and too-large codes mixed in)
from _value_ref import INT32_MIN, NAN_BITS, edges_case, inset, key, masks_case, pack, same, sentinel, unpack, values_case  # noqa: F401


def unkey(k, dtype):
    """uint32 order keys -> the values they stand for (key 0 -> the missing sentinel), in `dtype`"""
    k = np.asarray(k, dtype=np.uint64)
    if np.dtype(dtype) == np.int32:
        return (k ^ 0x80000000).astype(np.uint32).view(np.int32)
    raw = np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k & 0xFFFFFFFF)
    return np.where(k == 0, NAN_BITS, raw).astype(np.uint32).view(np.float32)


def _rows(words, ld, bit0, n_rows, labels, n_labels, and_words, B):
    m = inset(words, ld, bit0, n_rows, and_words, B)
    lab = np.asarray(labels).astype(np.int64)
    return m, lab, (lab >= 0) & (lab < n_labels)


def stats(words, ld, bit0, n_rows, labels, n_labels, values, and_words=None, B=None):
    """-> (count, missing, min, max, sum [B, n_labels], total, other [B])"""
    v = np.asarray(values)
    m, lab, valid = _rows(words, ld, bit0, n_rows, labels, n_labels, and_words, B)
    k = key(v).astype(np.int64)
    add = vref.fx(v)
    nb = m.shape[0]
    count, missing, total_sum = (np.zeros((nb, n_labels), np.int64) for _ in range(3))
    kmin, kmax = np.full((nb, n_labels), 1 << 32, np.int64), np.zeros((nb, n_labels), np.int64)
    for b in range(nb):
        has = m[b] & valid & (k != 0)
        gone = m[b] & valid & (k == 0)
        np.add.at(count[b], lab[has], 1)
        np.add.at(missing[b], lab[gone], 1)
        np.add.at(total_sum[b], lab[has], add[has])                                  # (int64 wraps modulo 2^64)
        np.minimum.at(kmin[b], lab[has], k[has])
        np.maximum.at(kmax[b], lab[has], k[has])
    lo = unkey(np.where(count > 0, kmin, 0), v.dtype)
    hi = unkey(np.where(count > 0, kmax, 0), v.dtype)
    return count, missing, lo, hi, total_sum, m.sum(axis=1).astype(np.int64), (m & ~valid[None, :]).sum(axis=1).astype(np.int64)


def histogram(words, ld, bit0, n_rows, labels, n_labels, values, edges, and_words=None, B=None):
    """-> (counts [B, n_labels, E - 1], below, above, missing [B, n_labels], total, other [B])"""
    v = np.asarray(values)
    e = np.asarray(edges, dtype=v.dtype)
    m, lab, valid = _rows(words, ld, bit0, n_rows, labels, n_labels, and_words, B)
    k = key(v)
    slot = np.searchsorted(key(e), k, side="right")                                  # 0 = below, E = above
    nb, E = m.shape[0], e.shape[0]
    cells = np.zeros((nb, n_labels, E + 1), np.int64)
    missing = np.zeros((nb, n_labels), np.int64)
    for b in range(nb):
        has = m[b] & valid & (k != 0)
        np.add.at(cells[b], (lab[has], slot[has]), 1)
        np.add.at(missing[b], lab[m[b] & valid & (k == 0)], 1)
    return (cells[:, :, 1:E].copy(), cells[:, :, 0].copy(), cells[:, :, E].copy(), missing, m.sum(axis=1).astype(np.int64),
            (m & ~valid[None, :]).sum(axis=1).astype(np.int64))


def loops(words, bit0, n_rows, labels, n_labels, values, edges, and_words=None):
    """the same with plain Python loops over the raw words and VALUES (no keys): the second opinion -> (stats tuple, histogram tuple)"""
    v = np.asarray(values)
    w = None if words is None else np.atleast_2d(np.ascontiguousarray(words)).view(np.uint32)
    a = None if and_words is None else np.ascontiguousarray(and_words).reshape(-1).view(np.uint32)
    nb, E = 1 if w is None else w.shape[0], len(edges)
    f32 = v.dtype == np.float32
    cnt, mis = (np.zeros((nb, n_labels), np.int64) for _ in range(2))
    exact = [[0] * n_labels for _ in range(nb)]                                      # Python integers: wrapped once at the end
    lo, hi = (np.full((nb, n_labels), sentinel(v.dtype), v.dtype) for _ in range(2))
    hist = np.zeros((nb, n_labels, E + 1), np.int64)
    tot, oth = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    zero = v.dtype.type(0)
    for b in range(nb):
        for r in range(n_rows):
            if not vref._in(w, a, b, bit0 + r):
                continue
            tot[b] += 1
            l, x = int(labels[r]), v[r]
            if not 0 <= l < n_labels:
                oth[b] += 1
                continue
            if (f32 and x != x) or (not f32 and int(x) == INT32_MIN):
                mis[b, l] += 1
                continue
            if cnt[b, l] == 0 or float(x) < float(lo[b, l]):
                lo[b, l] = x + zero
            if cnt[b, l] == 0 or float(hi[b, l]) < float(x):
                hi[b, l] = x + zero
            cnt[b, l] += 1
            exact[b][l] += int(vref.fx(v[r:r + 1])[0])
            hist[b, l, sum(1 for e in edges if not float(x) < float(e))] += 1
    sm = np.array([[(x + (1 << 63)) % (1 << 64) - (1 << 63) for x in row] for row in exact], np.int64).reshape(nb, n_labels)
    return (cnt, mis, lo, hi, sm, tot, oth), (hist[:, :, 1:E].copy(), hist[:, :, 0].copy(), hist[:, :, E].copy(), mis, tot, oth)


# ---- the shard rule: results over row slices -> the result over all rows ----------------------------------------------------------------------
def merge_stats(parts):
    count, missing, lo, hi, sm, total, other = (np.stack(x) for x in zip(*parts))
    klo = np.where(count > 0, key(lo.reshape(-1)).reshape(lo.shape).astype(np.int64), 1 << 32).min(axis=0)
    khi = np.where(count > 0, key(hi.reshape(-1)).reshape(hi.shape).astype(np.int64), 0).max(axis=0)
    c = count.sum(0)
    return (c, missing.sum(0), unkey(np.where(c > 0, klo, 0), lo.dtype), unkey(np.where(c > 0, khi, 0), lo.dtype), sm.sum(0, dtype=np.int64),
            total.sum(0), other.sum(0))


def merge_histogram(parts):
    return tuple(sum(x[1:], x[0]) for x in zip(*parts))


# ---- case generators ------------------------------------------------------------------------------------------------------------------------------
LABEL_SHAPES = ("one", "runs64", "runs64_off1", "random", "mixed", "none")


def labels_shape(kind, n_rows, n_labels, seed=0):
    """int32 labels [n_rows]: "one" -- every row one label (the last); "runs64" -- runs of exactly 64 aligned to the 64-row steps;
    "runs64_off1" -- the same runs offset by one row; "random"; "mixed" -- random with -1 and codes >= n_labels mixed in; "none" -- no row
    has a label (-1 and too-large codes only)"""
    r = np.arange(n_rows, dtype=np.int64)
    if kind == "one":
        return np.full(n_rows, n_labels - 1, np.int32)
    if kind == "runs64":
        return ((r // 64) * 7 % n_labels).astype(np.int32)
    if kind == "runs64_off1":
        return (((r + 63) // 64) * 7 % n_labels).astype(np.int32)
    if kind == "random":
        return labels_case(n_rows, n_labels, seed)
    if kind == "mixed":
        return labels_case(n_rows, n_labels, seed, frac_none=0.15, frac_big=0.1)
    if kind == "none":
        return np.where(r % 3 == 0, -1, np.where(r % 3 == 1, n_labels, (1 << 31) - 1)).astype(np.int32)
    raise ValueError(kind)
