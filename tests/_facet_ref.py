"""numpy reference of facet counts (vs_facet_counts / vs_index_facet_counts / vs_facet_topn) and the case generators of
its tests.

The contract: bit bit0 + r of the bitmap at words + b * ld stands for row r (ld = 0: one bitmap for all queries); row r is IN for query b iff
that bit is set in `words` and in `and_words` (when given; same bit0, shared by the queries); bits at or past bit0 + n_rows are ignored.
    total[b]     = rows in
    counts[b, l] = rows in with labels[r] == l, 0 <= l < n_labels
    other[b]     = rows in whose label is outside [0, n_labels)
so counts[b].sum() + other[b] == total[b].  Every value is an integer: every comparison is exact."""
import numpy as np

MAX_TOPN = 1024


def unpack(words, bit0, n_rows):
    """uint32 / int32 words [..., W] -> bool [..., n_rows]: bit bit0 + r of the row of words = bit (bit0 + r) & 31 of word (bit0 + r) >> 5"""
    w = np.ascontiguousarray(words).view(np.uint32)
    bit = bit0 + np.arange(n_rows, dtype=np.int64)
    return ((w[..., bit >> 5] >> (bit & 31).astype(np.uint32)) & 1).astype(bool)


def pack(mask, bit0=0, spare=0, n_words=None):
    """bool [B, n] -> uint32 words [B, W] with row r at bit bit0 + r; every other bit (in front of bit0, past the last row) is `spare` (0 | 1)"""
    mask = np.atleast_2d(mask)
    B, n = mask.shape
    W = (bit0 + n + 31) // 32 if n_words is None else n_words
    bits = np.full((B, W * 32), bool(spare))
    bits[:, bit0:bit0 + n] = mask
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (bits.reshape(B, W, 32).astype(np.uint64) * weights).sum(axis=2).astype(np.uint32)


def facet_counts(words, ld, bit0, n_rows, labels, n_labels, and_words=None, B=None):
    """-> (counts int64 [B, n_labels], total int64 [B], other int64 [B]).  words: uint32 [B, >= span] (or 1-D with ld = 0), None = every
    row set (B = 1 unless given)."""
    labels = np.asarray(labels).astype(np.int64)
    if words is None:
        inset = np.ones((B or 1, n_rows), dtype=bool)
    else:
        inset = unpack(np.atleast_2d(words), bit0, n_rows)
        assert ld != 0 or inset.shape[0] == 1
    if and_words is not None:
        inset = inset & unpack(np.asarray(and_words).reshape(-1), bit0, n_rows)[None, :]
    nb = inset.shape[0]
    valid = (labels >= 0) & (labels < n_labels)
    counts = np.zeros((nb, n_labels), dtype=np.int64)
    for b in range(nb):
        counts[b] = np.bincount(labels[inset[b] & valid], minlength=n_labels)
    total = inset.sum(axis=1).astype(np.int64)
    other = (inset & ~valid[None, :]).sum(axis=1).astype(np.int64)
    return counts, total, other


def facet_counts_loop(words, ld, bit0, n_rows, labels, n_labels, and_words=None):
    """the same, a plain Python double loop over the raw words (what tests/test_facet_cpu.py holds `facet_counts` against)"""
    w = np.atleast_2d(np.ascontiguousarray(words)).view(np.uint32)
    nb = w.shape[0]
    a = None if and_words is None else np.ascontiguousarray(and_words).reshape(-1).view(np.uint32)
    counts = [[0] * n_labels for _ in range(nb)]
    total, other = [0] * nb, [0] * nb
    for b in range(nb):
        for r in range(n_rows):
            bit = bit0 + r
            if not (int(w[b, bit >> 5]) >> (bit & 31)) & 1:
                continue
            if a is not None and not (int(a[bit >> 5]) >> (bit & 31)) & 1:
                continue
            total[b] += 1
            lab = int(labels[r])
            if 0 <= lab < n_labels:
                counts[b][lab] += 1
            else:
                other[b] += 1
    return np.array(counts, dtype=np.int64).reshape(nb, n_labels), np.array(total, dtype=np.int64), np.array(other, dtype=np.int64)


def topn(counts, n, min_count=1):
    """-> (labels int32 [B, n], counts int64 [B, n]): per query the n labels with the largest counts, count descending then label ascending,
    only counts >= max(min_count, 1); unused slots label -1 / count 0"""
    counts = np.atleast_2d(np.asarray(counts, dtype=np.int64))
    B, L = counts.shape
    out_l = np.full((B, n), -1, dtype=np.int32)
    out_c = np.zeros((B, n), dtype=np.int64)
    floor = max(int(min_count), 1)
    for b in range(B):
        order = np.lexsort((np.arange(L), -counts[b]))             # count descending, label ascending
        order = order[counts[b][order] >= floor][:n]
        out_l[b, :order.size] = order
        out_c[b, :order.size] = counts[b][order]
    return out_l, out_c


# ---- case generators -----------------------------------------------------------------------------------------------------------------------
def labels_case(n_rows, n_labels, seed, frac_none=0.0, frac_big=0.0):
    """int32 labels [n_rows], uniform over [0, n_labels); a share -1 ("no label") and a share >= n_labels (up to 2^31 - 1) mixed in"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, n_labels, size=n_rows).astype(np.int64)
    u = rng.random(n_rows)
    lab[u < frac_none] = -1
    big = (u >= frac_none) & (u < frac_none + frac_big)
    lab[big] = rng.choice(np.array([n_labels, n_labels + 1, 1 << 20, (1 << 31) - 1], dtype=np.int64), size=int(big.sum()))
    return lab.astype(np.int32)


def masks_case(B, n_rows, seed, density=0.4):
    """bool [B, n_rows]: per-query sets of different densities, with all-zero stretches (whole 64-row steps and 2048-row spans are skipped)"""
    rng = np.random.default_rng(seed)
    m = rng.random((B, n_rows)) < (density * (1 + np.arange(B)[:, None]) / B)
    for b in range(B):
        lo = int(rng.integers(0, max(n_rows - 1, 1)))
        m[b, lo:lo + int(rng.integers(0, max(n_rows // 3, 1)))] = False
    return m
