"""numpy reference of the per-label term aggregations (vs_label_order / vs_index_label_term_sums / vs_index_label_term_counts).

The contract.  ONE set of rows -- bit bit0 + r of `words` stands for row r (words None: every row), AND the live bitmap at bit 0 (when given);
bits at or past bit0 + n_rows are ignored -- and one int32 label a row.  For every label l in [0, n_labels):
    sums[l, c]   = the int64 sum of fx(v) over the stored cells (r, c) of the set rows with labels[r] == l     (fx, Cells: _term_sum_ref)
    counts[l, c] = the set rows with labels[r] == l that have column c                                         (has_matrix: _term_agg_ref)
    total[l]     = the set rows with labels[r] == l
and other = the set rows whose label is outside [0, n_labels); they contribute nowhere.  total.sum() + other is the size of the set.  Row l of
either matrix is what _term_sum_ref.term_sums / _term_agg_ref.term_counts give for the set "label == l AND set".  Everything is an integer:
every comparison is exact."""
import numpy as np

from _term_agg_ref import has_matrix, inset, pack, unpack  # noqa: F401  (the sets are the term counts')
from _term_sum_ref import ONE, TILE_COLS, Cells, fx  # noqa: F401

MAX_LABELS = 65536
MAX_CELLS = 1 << 27
LDS_BINS = 16384                                        # labels a workgroup of the label order counts in LDS (the facet counts' boundary)


def members(words, bit0, labels, n_labels, live_words=None):
    """-> (bool [n_labels, n_rows]: row r is in the set and carries label l, other: the set rows outside [0, n_labels))"""
    labels = np.asarray(labels).astype(np.int64)
    m = inset(words, 0, bit0, labels.size, live_words, 1)[0]
    ok = (labels >= 0) & (labels < n_labels)
    out = np.zeros((n_labels, labels.size), dtype=bool)
    rows = np.flatnonzero(m & ok)
    out[labels[rows], rows] = True
    return out, int((m & ~ok).sum())


def label_term_sums(words, bit0, labels, n_labels, cells, live_words=None):
    """-> (sums int64 [n_labels, n_cols], total int64 [n_labels], other int); cells = Cells(...) of the index's rows"""
    mem, other = members(words, bit0, labels, n_labels, live_words)
    sums = np.zeros((n_labels, cells.n_cols), dtype=np.int64)
    lab = np.asarray(labels).astype(np.int64)[cells.rows]
    keep = mem[np.clip(lab, 0, n_labels - 1), cells.rows] & (lab >= 0) & (lab < n_labels)
    with np.errstate(over="ignore"):
        np.add.at(sums, (lab[keep], cells.cols[keep]), cells.fx[keep])
    return sums, mem.sum(axis=1).astype(np.int64), other


def label_term_counts(words, bit0, labels, n_labels, has, live_words=None):
    """-> (counts int64 [n_labels, n_cols], total int64 [n_labels], other int); has = has_matrix(...) of the index's rows"""
    mem, other = members(words, bit0, labels, n_labels, live_words)
    counts = np.zeros((n_labels, has.shape[1]), dtype=np.int64)
    rows, cols = np.nonzero(has)
    lab = np.asarray(labels).astype(np.int64)[rows]
    keep = mem[np.clip(lab, 0, n_labels - 1), rows] & (lab >= 0) & (lab < n_labels)
    np.add.at(counts, (lab[keep], cols[keep]), 1)                  # (what mem @ has gives, without a dense integer product)
    return counts, mem.sum(axis=1).astype(np.int64), other


def label_terms_loop(words, bit0, labels, n_labels, indptr, indices, values, n_cols, live_words=None):
    """(sums, counts, total, other) by a plain Python double loop over rows and cells on the raw words, in Python integers reduced modulo 2^64"""
    w = None if words is None else np.ascontiguousarray(words).reshape(-1).view(np.uint32)
    lw = None if live_words is None else np.ascontiguousarray(live_words).reshape(-1).view(np.uint32)
    n_rows = len(indptr) - 1
    f = [ONE] * len(indices) if values is None else [int(x) for x in fx(values)]
    nz = [True] * len(indices) if values is None else [bool(x != 0) for x in np.asarray(values)]
    sums = [[0] * n_cols for _ in range(n_labels)]
    counts = [[0] * n_cols for _ in range(n_labels)]
    total, other = [0] * n_labels, 0
    for r in range(n_rows):
        bit = bit0 + r
        if w is not None and not (int(w[bit >> 5]) >> (bit & 31)) & 1:
            continue
        if lw is not None and not (int(lw[r >> 5]) >> (r & 31)) & 1:
            continue
        l = int(labels[r])
        if not 0 <= l < n_labels:
            other += 1
            continue
        total[l] += 1
        seen = set()
        for j in range(int(indptr[r]), int(indptr[r + 1])):
            c = int(indices[j])
            if c < n_cols:
                sums[l][c] += f[j]
                if nz[j] and c not in seen:
                    seen.add(c)
                    counts[l][c] += 1
    wrap = lambda x: ((x + (1 << 63)) % (1 << 64)) - (1 << 63)
    return (np.array([[wrap(x) for x in row] for row in sums], dtype=np.int64).reshape(n_labels, n_cols),
            np.array(counts, dtype=np.int64).reshape(n_labels, n_cols), np.array(total, dtype=np.int64), other)


def label_order(words, bit0, labels, n_labels, live_words=None):
    """-> (ptr int64 [n_labels + 1], rows int64 [n_set] with every label's segment ASCENDING, other): the kernel's order inside a segment is
    unspecified -- compare with `sorted_segments`"""
    mem, other = members(words, bit0, labels, n_labels, live_words)
    ptr = np.zeros(n_labels + 1, dtype=np.int64)
    np.cumsum(mem.sum(axis=1), out=ptr[1:])
    ls, rs = np.nonzero(mem)                                       # (row-major: by label, then by row)
    return ptr, rs.astype(np.int64), other


def sorted_segments(ptr, rows):
    """rows with every segment rows[ptr[l]:ptr[l + 1]] sorted ascending"""
    ptr, rows = np.asarray(ptr, dtype=np.int64), np.asarray(rows, dtype=np.int64).copy()
    seg = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    return rows[np.lexsort((rows, seg))] if rows.size else rows


def plan(n_rows, n_labels, n_cols, rows_per_item=0, tile_cols=0, auto_items=1024, span=2048):
    """the plan rule of vs_label_term_plan -> (tiles, tile_cols, rows_per_item, max_items)"""
    if tile_cols == 0:
        tiles = -(-n_cols // TILE_COLS)
        tile_cols = -(-n_cols // tiles)
    else:
        tiles = -(-n_cols // tile_cols)
    if rows_per_item == 0:
        want = max(1, auto_items // tiles)
        rows_per_item = max(-(-n_rows // want), span)
        rows_per_item = -(-rows_per_item // span) * span
    return tiles, tile_cols, rows_per_item, -(-n_rows // rows_per_item) + n_labels


def n_items(total, rows_per_item):
    """the items the table really holds: the sum over the labels of ceil(total / rows_per_item) <= the plan's max_items"""
    return int((-(-np.asarray(total, dtype=np.int64) // rows_per_item)).sum())
