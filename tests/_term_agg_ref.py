"""numpy reference of the term aggregations (vs_index_term_counts / vs_index_term_counts_ids / vs_term_topn) and the case
generators of its tests.

The contract.  A row HAS column c iff it stores c with a non-zero value (a binary index stores 1: every stored cell counts; a stored +0.0 or
-0.0 does not; the packets' padding column n_cols never counts).  Rows come as a CSR (indptr, indices, values | None), e.g. what get_rows
returns.  Row membership is that of the facet counts (tests/_facet_ref.py): bit bit0 + r of the bitmap at words + b * ld stands for row r
(ld = 0: one bitmap), AND the live bitmap at bit 0 (when given); bits at or past bit0 + n_rows are ignored.
    total[b]     = rows in
    counts[b, c] = rows in that have column c, 0 <= c < n_cols
Everything is an integer except the scores of `topn`, which are fp64 arithmetic rounded once to fp32: every comparison is exact."""
import numpy as np

from _facet_ref import pack, unpack  # noqa: F401  (the bitmap layout is the facet counts')

MAX_TOPN = 1024
LIFT, JLH = 0, 1


def has_matrix(indptr, indices, values, n_cols):
    """bool [n_rows, n_cols]: row r has column c.  A column >= n_cols (the padding id) is dropped."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    n = indptr.size - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    keep = (indices >= 0) & (indices < n_cols)
    if values is not None:
        keep &= np.asarray(values) != 0                             # (+0.0 and -0.0 compare equal to 0; NaN does not)
    has = np.zeros((n, n_cols), dtype=bool)
    has[rows[keep], indices[keep]] = True
    return has


def inset(words, ld, bit0, n_rows, live_words=None, B=None):
    """bool [B, n_rows]: the rows of each query's set.  words None: every row (B = 1 unless given); live_words: a bitmap at bit 0"""
    if words is None:
        m = np.ones((B or 1, n_rows), dtype=bool)
    else:
        m = unpack(np.atleast_2d(words), bit0, n_rows)
        assert ld != 0 or m.shape[0] == 1
    if live_words is not None:
        m = m & unpack(np.asarray(live_words).reshape(-1), 0, n_rows)[None, :]
    return m


def term_counts(words, ld, bit0, has, live_words=None, B=None):
    """-> (counts int64 [B, n_cols], total int64 [B]) of the bitmap-driven call; has = has_matrix(...) of the index's rows"""
    n_rows = has.shape[0]
    m = inset(words, ld, bit0, n_rows, live_words, B)
    counts = m.astype(np.int64) @ has.astype(np.int64)
    return counts, m.sum(axis=1).astype(np.int64)


def term_counts_loop(words, ld, bit0, indptr, indices, values, n_cols, live_words=None):
    """the same, a plain Python double loop over rows and cells on the raw words (what tests/test_term_agg_cpu.py holds `term_counts` against)"""
    w = np.atleast_2d(np.ascontiguousarray(words)).view(np.uint32)
    lw = None if live_words is None else np.ascontiguousarray(live_words).reshape(-1).view(np.uint32)
    nb, n_rows = w.shape[0], len(indptr) - 1
    counts = [[0] * n_cols for _ in range(nb)]
    total = [0] * nb
    for b in range(nb):
        for r in range(n_rows):
            bit = bit0 + r
            if not (int(w[b, bit >> 5]) >> (bit & 31)) & 1:
                continue
            if lw is not None and not (int(lw[r >> 5]) >> (r & 31)) & 1:
                continue
            total[b] += 1
            seen = set()
            for j in range(int(indptr[r]), int(indptr[r + 1])):
                c = int(indices[j])
                if c >= n_cols or (values is not None and float(values[j]) == 0.0) or c in seen:
                    continue
                seen.add(c)
                counts[b][c] += 1
    return np.array(counts, dtype=np.int64).reshape(nb, n_cols), np.array(total, dtype=np.int64)


def term_counts_ids(ids, id_offset, has, live=None):
    """-> (counts, total) of the id-list call under strict = 0: ids int64 [B, m], row = id - id_offset; id -1, a row outside the index and a
    deleted row (live bool [n_rows]) are skipped; an id listed twice counts twice; total = the entries counted"""
    ids = np.atleast_2d(np.asarray(ids, dtype=np.int64))
    n_rows, n_cols = has.shape
    counts = np.zeros((ids.shape[0], n_cols), dtype=np.int64)
    total = np.zeros(ids.shape[0], dtype=np.int64)
    for b in range(ids.shape[0]):
        rows = ids[b] - id_offset
        ok = (ids[b] != -1) & (rows >= 0) & (rows < n_rows)
        rows = rows[ok]
        if live is not None:
            rows = rows[np.asarray(live, dtype=bool)[rows]]
        total[b] = rows.size
        counts[b] = has[rows].astype(np.int64).sum(axis=0)
    return counts, total


def scores(fg, total, bg, bg_total, method):
    """-> (candidate bool [n], score float32 [n]) of one query: fp64 throughout, each operation rounded once, one rounding to fp32"""
    fg, bg = np.asarray(fg, dtype=np.int64), np.asarray(bg, dtype=np.int64)
    cand = (fg >= 1) & (bg > 0) & (int(total) > 0) & (int(bg_total) > 0)
    s = np.zeros(fg.size, dtype=np.float64)
    if cand.any():
        fgp = fg[cand].astype(np.float64) / np.float64(int(total))
        bgp = bg[cand].astype(np.float64) / np.float64(int(bg_total))
        if method == JLH:
            s[cand] = (fgp - bgp) * (fgp / bgp)
            ok = fgp > bgp
            idx = np.flatnonzero(cand)
            cand[idx[~ok]] = False
        else:
            s[cand] = fgp / bgp
    return cand, s.astype(np.float32)


def topn(counts, total, bg, bg_total, n, method=JLH, min_count=1):
    """-> (cols int32 [B, n], score float32 [B, n], fg int64 [B, n], bg int64 [B, n]): per query the n candidates with the largest fp32 score,
    score descending then column ascending; unused slots -1 / -inf / 0 / 0"""
    counts = np.atleast_2d(np.asarray(counts, dtype=np.int64))
    total = np.asarray(total, dtype=np.int64).reshape(-1)
    bg = np.asarray(bg, dtype=np.int64)
    B, V = counts.shape
    out_c = np.full((B, n), -1, dtype=np.int32)
    out_s = np.full((B, n), -np.inf, dtype=np.float32)
    out_f = np.zeros((B, n), dtype=np.int64)
    out_b = np.zeros((B, n), dtype=np.int64)
    floor = max(int(min_count), 1)
    for b in range(B):
        cand, s = scores(counts[b], total[b], bg, bg_total, method)
        cand &= counts[b] >= floor
        cols = np.flatnonzero(cand)
        order = cols[np.lexsort((cols, -s[cols].astype(np.float64)))][:n]           # (fp32 -> fp64 is exact: the order is the fp32 one)
        out_c[b, :order.size] = order
        out_s[b, :order.size] = s[order]
        out_f[b, :order.size] = counts[b][order]
        out_b[b, :order.size] = bg[order]
    return out_c, out_s, out_f, out_b


# ---- case generators -----------------------------------------------------------------------------------------------------------------------
def csr_case(row_lens, n_cols, seed, zeros=0.0, binary=False, hot=None):
    """A CSR with the given row lengths: distinct ascending columns per row, non-zero fp16-exact values; a share `zeros` of the cells is given
    the value +0.0 or -0.0 (alternating); hot: a column every non-empty row carries.  -> (indptr int64, indices int32, values float32 | None)"""
    rng = np.random.default_rng(seed)
    indptr = np.zeros(len(row_lens) + 1, dtype=np.int64)
    np.cumsum(row_lens, out=indptr[1:])
    indices = np.empty(int(indptr[-1]), dtype=np.int32)
    for r, ln in enumerate(row_lens):
        if ln == 0:
            continue
        if ln > n_cols // 2:
            c = np.sort(rng.permutation(n_cols)[:ln])
        else:
            c = np.unique(rng.integers(0, n_cols, size=ln))
            while c.size < ln:
                c = np.unique(np.concatenate([c, rng.integers(0, n_cols, size=ln - c.size)]))
        if hot is not None and hot not in c:
            c[0] = hot
            c = np.sort(c)
        indices[indptr[r]:indptr[r + 1]] = c
    if binary:
        return indptr, indices, None
    values = (rng.integers(1, 64, size=indices.size) / 16.0).astype(np.float32) * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=indices.size)
    z = np.flatnonzero(rng.random(indices.size) < zeros)
    values[z[0::2]] = 0.0
    values[z[1::2]] = -0.0
    return indptr, indices, values
