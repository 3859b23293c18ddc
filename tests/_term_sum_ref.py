"""numpy reference of the term sums (vs_index_term_sums / vs_index_term_sums_ids / vs_term_sum_topn).

The contract.  A stored cell of value v (fp16 widened exactly, a binary index stores 1) contributes the integer
    fx(v) = rint(float64(clip(v, -2^20, +2^20)) * 2^24)        (to nearest even; NaN contributes 0; +-inf clamp)
and sums[b, c] is the int64 sum of fx over the stored cells (r, c) of the rows r of query b's set; the padding column n_cols never contributes.
Sums wrap modulo 2^64 as numpy's int64 does.  Rows come as a CSR (indptr, indices, values | None), e.g. what get_rows returns.  Row membership is
that of the term counts (tests/_term_agg_ref.py): bit bit0 + r of the bitmap at words + b * ld stands for row r (ld = 0: one bitmap), AND the live
bitmap at bit 0 (when given); bits at or past bit0 + n_rows are ignored.  total[b] = rows in.
Everything is an integer except the scores of `topn`, which are fp64 arithmetic rounded once to fp32: every comparison is exact."""
import numpy as np

from _term_agg_ref import inset, pack, unpack  # noqa: F401  (the sets are the term counts')

FX_SHIFT, FX_CLAMP_LOG2 = 24, 20
TILE_COLS = 18432
MAX_TOPN = 1024
ONE = 1 << FX_SHIFT


def fx(values):
    """int64 array: the fixed-point image of each value"""
    v = np.asarray(values)
    if v.dtype == np.float16:
        v = v.astype(np.float32)                                    # (widens exactly; 2^20 is no fp16 value)
    with np.errstate(invalid="ignore"):
        x = np.rint(np.clip(v, -2.0 ** FX_CLAMP_LOG2, 2.0 ** FX_CLAMP_LOG2).astype(np.float64) * 2.0 ** FX_SHIFT)
    return np.where(np.isnan(x), 0.0, x).astype(np.int64)


class Cells:
    """the stored cells of an index as the reference reads them: rows, cols and fx of every cell inside [0, n_cols)"""

    def __init__(self, indptr, indices, values, n_cols):
        indptr = np.asarray(indptr, dtype=np.int64)
        indices = np.asarray(indices, dtype=np.int64)
        self.n_rows, self.n_cols = indptr.size - 1, int(n_cols)
        rows = np.repeat(np.arange(self.n_rows), np.diff(indptr))
        f = np.full(indices.size, ONE, dtype=np.int64) if values is None else fx(values)      # values None: a binary index, every cell stores 1
        keep = (indices >= 0) & (indices < n_cols)                                             # the padding id is dropped
        self.rows, self.cols, self.fx = rows[keep], indices[keep], f[keep]

    def rows_sum(self, mult):
        """int64 [n_cols]: the sum over the cells of fx times the multiplicity mult[row] of the cell's row (np.add.at: a column stored twice
        in a row adds twice; int64 wraps modulo 2^64)"""
        out = np.zeros(self.n_cols, dtype=np.int64)
        m = np.asarray(mult, dtype=np.int64)[self.rows]
        with np.errstate(over="ignore"):
            np.add.at(out, self.cols[m != 0], (self.fx * m)[m != 0])
        return out

    def slice(self, r0, r1):
        """the cells of rows [r0, r1) as an index of their own (a row shard)"""
        out = object.__new__(Cells)
        keep = (self.rows >= r0) & (self.rows < r1)
        out.n_rows, out.n_cols = r1 - r0, self.n_cols
        out.rows, out.cols, out.fx = self.rows[keep] - r0, self.cols[keep], self.fx[keep]
        return out


def term_sums(words, ld, bit0, cells, live_words=None, B=None):
    """-> (sums int64 [B, n_cols], total int64 [B]) of the bitmap-driven call; cells = Cells(...) of the index's rows"""
    m = inset(words, ld, bit0, cells.n_rows, live_words, B)
    sums = np.stack([cells.rows_sum(m[b]) for b in range(m.shape[0])])
    return sums, m.sum(axis=1).astype(np.int64)


def term_sums_loop(words, ld, bit0, indptr, indices, values, n_cols, live_words=None):
    """the same, a plain Python double loop over rows and cells on the raw words, in Python integers reduced modulo 2^64"""
    w = np.atleast_2d(np.ascontiguousarray(words)).view(np.uint32)
    lw = None if live_words is None else np.ascontiguousarray(live_words).reshape(-1).view(np.uint32)
    nb, n_rows = w.shape[0], len(indptr) - 1
    f = [ONE] * len(indices) if values is None else [int(x) for x in fx(values)]
    sums = [[0] * n_cols for _ in range(nb)]
    total = [0] * nb
    for b in range(nb):
        for r in range(n_rows):
            bit = bit0 + r
            if not (int(w[b, bit >> 5]) >> (bit & 31)) & 1:
                continue
            if lw is not None and not (int(lw[r >> 5]) >> (r & 31)) & 1:
                continue
            total[b] += 1
            for j in range(int(indptr[r]), int(indptr[r + 1])):
                c = int(indices[j])
                if c < n_cols:
                    sums[b][c] += f[j]
    wrap = lambda x: ((x + (1 << 63)) % (1 << 64)) - (1 << 63)
    return np.array([[wrap(x) for x in row] for row in sums], dtype=np.int64).reshape(nb, n_cols), np.array(total, dtype=np.int64)


def term_sums_ids(ids, id_offset, cells, live=None):
    """-> (sums, total) of the id-list call under strict = 0: ids int64 [B, m], row = id - id_offset; id -1, a row outside the index and a
    deleted row (live bool [n_rows]) are skipped; an id listed twice counts twice; total = the entries counted"""
    ids = np.atleast_2d(np.asarray(ids, dtype=np.int64))
    sums = np.zeros((ids.shape[0], cells.n_cols), dtype=np.int64)
    total = np.zeros(ids.shape[0], dtype=np.int64)
    for b in range(ids.shape[0]):
        rows = ids[b] - id_offset
        ok = (ids[b] != -1) & (rows >= 0) & (rows < cells.n_rows)
        rows = rows[ok]
        if live is not None:
            rows = rows[np.asarray(live, dtype=bool)[rows]]
        total[b] = rows.size
        sums[b] = cells.rows_sum(np.bincount(rows, minlength=cells.n_rows))
    return sums, total


def check_strict(ids, id_offset, n_rows):
    """strict = 1 on a host list: every id is -1 or names a row of the index"""
    ids = np.asarray(ids, dtype=np.int64)
    rows = ids - id_offset
    return bool(((ids == -1) | ((rows >= 0) & (rows < n_rows))).all())


def mean(sums, total):
    """float32 [B, n_cols]: (float64(sums) * 2^-24) / float64(total), each operation rounded once, one rounding to fp32; total = 0: zeros"""
    sums = np.atleast_2d(np.asarray(sums, dtype=np.int64))
    t = np.asarray(total, dtype=np.int64).reshape(-1, 1).astype(np.float64)
    out = np.zeros(sums.shape, dtype=np.float32)
    ok = t[:, 0] > 0
    out[ok] = ((sums[ok].astype(np.float64) * 2.0 ** -FX_SHIFT) / t[ok]).astype(np.float32)
    return out


def topn(sums, total, n, counts=None, min_count=0):
    """-> (cols int32 [B, n], score float32 [B, n], sums int64 [B, n]): per query the n candidates (sum > 0, total > 0, counts >= min_count when
    counts are given) with the largest fp32 mean weight, score descending then column ascending; unused slots -1 / -inf / 0"""
    sums = np.atleast_2d(np.asarray(sums, dtype=np.int64))
    total = np.asarray(total, dtype=np.int64).reshape(-1)
    B, V = sums.shape
    out_c = np.full((B, n), -1, dtype=np.int32)
    out_s = np.full((B, n), -np.inf, dtype=np.float32)
    out_w = np.zeros((B, n), dtype=np.int64)
    s = mean(sums, total)
    for b in range(B):
        cand = (sums[b] > 0) & (total[b] > 0)
        if counts is not None:
            cand &= np.atleast_2d(np.asarray(counts, dtype=np.int64))[b] >= int(min_count)
        cols = np.flatnonzero(cand)
        order = cols[np.lexsort((cols, -s[b][cols].astype(np.float64)))][:n]          # (fp32 -> fp64 is exact: the order is the fp32 one)
        out_c[b, :order.size] = order
        out_s[b, :order.size] = s[b][order]
        out_w[b, :order.size] = sums[b][order]
    return out_c, out_s, out_w


def plan(n_rows, B, n_cols, rows_per_chunk=0, tile_cols=0, auto_items=1024, span=2048):
    """the plan rule of vs_term_sum_plan -> (tiles, tile_cols, chunks, rows_per_chunk)"""
    if tile_cols == 0:
        tiles = -(-n_cols // TILE_COLS)
        tile_cols = -(-n_cols // tiles)
    else:
        tiles = -(-n_cols // tile_cols)
    if rows_per_chunk == 0:
        want = max(1, auto_items // (B * tiles))
        rows_per_chunk = max(-(-n_rows // want), span)
        rows_per_chunk = -(-rows_per_chunk // span) * span
    return tiles, tile_cols, -(-n_rows // rows_per_chunk), rows_per_chunk
