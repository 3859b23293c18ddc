"""numpy reference of the per-label percentiles (vs_facet_value_quantiles / vs_facet_value_radix_counts).

The definition.  For query b and label l in [0, n_labels), K[b, l] is the ascending multiset of the order keys (_value_ref.key) of the rows that
are in the set, carry label l and have a value (key != 0): count[b, l] = |K[b, l]|, missing[b, l] = the set rows of label l with key 0; a set
row whose label is outside [0, n_labels) adds to other[b] and nothing else; total[b] is the size of the set.  The order statistic of rank r is
unkey(K[b, l][r]); a rank outside 0..count - 1 gives the missing sentinel and a resolved rank of -1; quantile -> rank is _quantile_ref.rank_rule
applied to count[b, l].  `order_statistics` is that definition by sorting.  `level_counts` restates one radix level per (query, label) cell with
plain loops, and `radix_select` composes the levels with _quantile_ref.step over B x n_labels cells and any cut of the rows into shards."""
import numpy as np

import _quantile_ref as qref
from _value_ref import inset, key

LEVELS, LEVEL_BINS, LEVEL_SHIFT, PREFIX_SHIFT = qref.LEVELS, qref.LEVEL_BINS, qref.LEVEL_SHIFT, qref.PREFIX_SHIFT


def _rows(words, ld, bit0, n_rows, labels, n_labels, and_words, B):
    m = inset(words, ld, bit0, n_rows, and_words, B)
    lab = np.asarray(labels).astype(np.int64)
    return m, lab, (lab >= 0) & (lab < n_labels)


def cell_keys(words, ld, bit0, n_rows, values, labels, n_labels, and_words=None, B=None):
    """-> (keys[b][l]: ascending uint32 arrays without zeros, missing int64 [B, L], total int64 [B], other int64 [B])"""
    m, lab, valid = _rows(words, ld, bit0, n_rows, labels, n_labels, and_words, B)
    k = key(np.asarray(values))
    nb = m.shape[0]
    keys = [[np.sort(k[m[b] & (lab == l) & (k != 0)]) for l in range(n_labels)] for b in range(nb)]
    missing = np.array([[(m[b] & (lab == l) & (k == 0)).sum() for l in range(n_labels)] for b in range(nb)], np.int64).reshape(nb, n_labels)
    return keys, missing, m.sum(axis=1).astype(np.int64), (m & ~valid[None, :]).sum(axis=1).astype(np.int64)


def order_statistics(words, ld, bit0, n_rows, values, labels, n_labels, q=None, method="lower", ranks=None, and_words=None, B=None):
    """the definition, by sorting -> (values [B, L, R] in the field's type, ranks int64 [B, L, R], count, missing int64 [B, L], total, other
    int64 [B]).  ranks: int64 [B, L, R]."""
    v = np.asarray(values)
    keys, missing, total, other = cell_keys(words, ld, bit0, n_rows, v, labels, n_labels, and_words, B)
    nb, L = len(keys), n_labels
    R = len(q) if q is not None else np.asarray(ranks).shape[2]
    count = np.array([[keys[b][l].size for l in range(L)] for b in range(nb)], np.int64).reshape(nb, L)
    rk = qref.resolve_ranks(count.reshape(-1), R, q, method, None if ranks is None else np.asarray(ranks).reshape(nb * L, R)).reshape(nb, L, R)
    out = np.zeros((nb, L, R), np.uint32)
    for b in range(nb):
        for l in range(L):
            for j in range(R):
                out[b, l, j] = keys[b][l][rk[b, l, j]] if rk[b, l, j] >= 0 else 0
    return qref.unkey(out, v.dtype).reshape(nb, L, R), rk, count, missing, total, other


def level_counts(words, ld, bit0, n_rows, values, labels, n_labels, level, R, slot_prefix=None, n_slots=None, and_words=None, B=None):
    """vs_facet_value_radix_counts, one row at a time -> (counts int64 [B, L, S, bins], missing [B, L], total, other [B]); slot_prefix [B x L,
    R] / n_slots [B x L]: the step's state over the cells (levels 1, 2); missing / total / other are None below level 0"""
    m, lab, valid = _rows(words, ld, bit0, n_rows, labels, n_labels, and_words, B)
    k = [int(x) for x in key(np.asarray(values))]
    nb, L, bins, S = m.shape[0], n_labels, LEVEL_BINS[level], 1 if level == 0 else R
    counts = np.zeros((nb, L, S, bins), np.int64)
    missing, total, other = np.zeros((nb, L), np.int64), np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    for b in range(nb):
        for r in range(n_rows):
            if not m[b, r]:
                continue
            total[b] += 1
            if not valid[r]:
                other[b] += 1
                continue
            l = int(lab[r])
            if k[r] == 0:
                missing[b, l] += 1
                continue
            d = (k[r] >> LEVEL_SHIFT[level]) & (bins - 1)
            if level == 0:
                counts[b, l, 0, d] += 1
                continue
            cell = b * L + l
            slots = [int(p) for p in slot_prefix[cell, :int(n_slots[cell])]]
            if (k[r] >> PREFIX_SHIFT[level]) in slots:
                counts[b, l, slots.index(k[r] >> PREFIX_SHIFT[level]), d] += 1
    return (counts, missing, total, other) if level == 0 else (counts, None, None, None)


def radix_select(words, ld, bit0, n_rows, values, labels, n_labels, q=None, method="lower", ranks=None, and_words=None, B=None, cuts=None, trace=None):
    """The composition of the levels -> what order_statistics returns.  cuts: row bounds [0, ..., n_rows] of shards -- every shard counts its
    slice of the labels and values and its bit range of the bitmaps; the counts are added before each step, which runs over B x L cells.
    trace: a list that receives each level's (summed counts [B, L, S, bins], state)."""
    v, lab = np.asarray(values), np.asarray(labels)
    cuts = [0, n_rows] if cuts is None else list(cuts)
    L = n_labels
    R = len(q) if q is not None else np.asarray(ranks).shape[2]
    state = tail = None
    for level in range(LEVELS):
        total = None
        parts = []
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            c, *rest = level_counts(words, ld, bit0 + r0, r1 - r0, v[r0:r1], lab[r0:r1], L, level, R, state and state["slot_prefix"],
                                    state and state["n_slots"], and_words, B)
            total = c if total is None else total + c
            parts.append(rest)
        nb = total.shape[0]
        if level == 0:
            tail = [sum(x[1:], x[0]) for x in zip(*parts)]
        state = qref.step(level, total.reshape(nb * L, total.shape[2], total.shape[3]), R, state, q, method,
                          None if ranks is None else np.asarray(ranks).reshape(nb * L, R), v.dtype)
        if level == 0:
            count, rk = state["count"].reshape(nb, L), state["ranks"].reshape(nb, L, R)
        if trace is not None:
            trace.append((total, state))
    return state["values"].reshape(nb, L, R), rk, count, tail[0], tail[1], tail[2]
