"""numpy reference of the numeric fields (vs_value_range_bitmaps / vs_value_stats / vs_value_histogram / vs_value_topk) and
the case generators of their tests.

The contract, written on VALUES (the library decides everything on uint32 order keys; `key` below is that rule, for the tests of the rule):
a field is float32 or int32 [n_rows]; a row has no value iff it holds NaN (float32) or INT32_MIN (int32).  A set is a bitmap as in
_facet_ref: bit bit0 + r of the bitmap at words + b * ld stands for row r, ANDed with `and_words`; bits at or past bit0 + n_rows are ignored.
    range bitmaps: bit bit0 + r of row b = row r has a value and lo[b] <= v <= hi[b]; every other bit of the span's words is 0
    stats:         count / missing = set rows with / without a value; min / max over the values (+0.0 for either zero; the sentinel when
                   count = 0); sum = the exact integer sum (int32), the sum of rint(clip(v, +-2^20) * 2^24) (float32), modulo 2^64
    histogram:     bin i = edges[i] <= v < edges[i + 1], below = v < edges[0], above = v >= edges[-1], missing as in stats
    topk:          the k set rows with a value in (value descending | ascending, id ascending) order; id -1 / the sentinel behind the last
Every value is an integer or a bit pattern: every comparison is exact (floats compare by their bits, `same`)."""
import numpy as np

from _facet_ref import masks_case, pack, unpack  # noqa: F401  (the bitmap layout and the set generator are the facets')

INT32_MIN = -(1 << 31)
NAN_BITS = 0x7FC00000
MAX_RANGES, MAX_EDGES, MAX_TOPK = 4096, 1025, 1024


def sentinel(dtype):
    return np.float32(np.nan) if np.dtype(dtype) == np.float32 else np.int32(INT32_MIN)


def is_missing(v):
    v = np.asarray(v)
    return np.isnan(v) if v.dtype == np.float32 else v == INT32_MIN


def bits(a):
    """what `same` compares: the 32-bit patterns of a float32 / int32 array"""
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.int32), a.dtype
    return a.view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all() if a.dtype.itemsize == 4 else (a == b).all())


def key(v):
    """the library's uint32 order key of float32 / int32 values (0 = missing), as uint32"""
    v = np.ascontiguousarray(v)
    u = v.view(np.uint32).astype(np.uint64)
    if v.dtype == np.int32:
        return (u ^ 0x80000000).astype(np.uint32)
    mag = u & 0x7FFFFFFF
    u = np.where(mag == 0, 0, u)
    k = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(mag > 0x7F800000, 0, k).astype(np.uint32)


def fx(v):
    """what a row adds to `sum`, int64"""
    v = np.asarray(v)
    if v.dtype == np.int32:
        return v.astype(np.int64)
    x = np.clip(np.nan_to_num(v.astype(np.float64), nan=0.0, posinf=np.inf, neginf=-np.inf), -float(1 << 20), float(1 << 20))
    return np.rint(x * float(1 << 24)).astype(np.int64)


def inset(words, ld, bit0, n_rows, and_words=None, B=None):
    """-> bool [B, n_rows]: the rows in each query's set"""
    if words is None:
        m = np.ones((B or 1, n_rows), dtype=bool)
    else:
        m = unpack(np.atleast_2d(words), bit0, n_rows)
        assert ld != 0 or m.shape[0] == 1
    if and_words is not None:
        m = m & unpack(np.asarray(and_words).reshape(-1), bit0, n_rows)[None, :]
    return m


def range_masks(values, lo, hi):
    v = np.asarray(values)
    lo, hi = np.atleast_1d(np.asarray(lo, dtype=v.dtype)), np.atleast_1d(np.asarray(hi, dtype=v.dtype))
    ok = ~is_missing(v)[None, :] & ~is_missing(lo)[:, None] & ~is_missing(hi)[:, None]
    with np.errstate(invalid="ignore"):
        return ok & (v[None, :] >= lo[:, None]) & (v[None, :] <= hi[:, None])


def range_bitmaps(values, lo, hi, bit0=0):
    """-> uint32 words [B, span]"""
    return pack(range_masks(values, lo, hi), bit0)


def stats(words, ld, bit0, n_rows, values, and_words=None, B=None):
    """-> (count, missing, min, max, sum)"""
    v = np.asarray(values)
    m = inset(words, ld, bit0, n_rows, and_words, B)
    miss = is_missing(v)
    nb = m.shape[0]
    count = (m & ~miss).sum(axis=1).astype(np.int64)
    missing = (m & miss).sum(axis=1).astype(np.int64)
    lo, hi = np.full(nb, sentinel(v.dtype), v.dtype), np.full(nb, sentinel(v.dtype), v.dtype)
    total = np.zeros(nb, dtype=np.int64)
    zero = v.dtype.type(0)
    for b in range(nb):
        x = v[m[b] & ~miss]
        if x.size:
            lo[b], hi[b] = x.min() + zero, x.max() + zero            # (-0.0 + 0.0 = +0.0)
            total[b] = fx(x).sum(dtype=np.int64)
    return count, missing, lo, hi, total


def histogram(words, ld, bit0, n_rows, values, edges, and_words=None, B=None):
    """-> (counts [B, E - 1], below, above, missing)"""
    v = np.asarray(values)
    e = np.asarray(edges, dtype=v.dtype)
    m = inset(words, ld, bit0, n_rows, and_words, B)
    miss = is_missing(v)
    nb, E = m.shape[0], e.shape[0]
    slot = np.searchsorted(e, np.where(miss, e[0], v), side="right")             # 0 = below, E = above
    counts = np.zeros((nb, E + 1), dtype=np.int64)
    for b in range(nb):
        counts[b] = np.bincount(slot[m[b] & ~miss], minlength=E + 1)
    return counts[:, 1:E].copy(), counts[:, 0].copy(), counts[:, E].copy(), (m & miss).sum(axis=1).astype(np.int64)


def topk(words, ld, bit0, n_rows, values, k, descending=True, id_offset=0, and_words=None, B=None):
    """-> (ids int64 [B, k], values [B, k])"""
    v = np.asarray(values)
    m = inset(words, ld, bit0, n_rows, and_words, B)
    miss = is_missing(v)
    nb = m.shape[0]
    ids = np.full((nb, k), -1, dtype=np.int64)
    vals = np.full((nb, k), sentinel(v.dtype), dtype=v.dtype)
    for b in range(nb):
        rows = np.flatnonzero(m[b] & ~miss)
        x = v[rows].astype(np.float64)                                           # (exact for either type; -0.0 == +0.0)
        order = rows[np.lexsort((rows, -x if descending else x))][:k]
        ids[b, :order.size] = order + id_offset
        vals[b, :order.size] = v[order]
    return ids, vals


# ---- the same with plain loops over the raw words: the second opinion (tests/test_value_cpu.py holds the functions above against these) ----
def _in(w, a, b, bit):
    if w is not None and not (int(w[b, bit >> 5]) >> (bit & 31)) & 1:
        return False
    return a is None or bool((int(a[bit >> 5]) >> (bit & 31)) & 1)


def _lt(x, y):
    return float(x) < float(y)


def loops(words, bit0, n_rows, values, edges=None, k=4, descending=True, id_offset=0, and_words=None):
    """-> dict(stats=..., histogram=..., topk=...) in the shapes of the functions above"""
    v = np.asarray(values)
    w = None if words is None else np.atleast_2d(np.ascontiguousarray(words)).view(np.uint32)
    a = None if and_words is None else np.ascontiguousarray(and_words).reshape(-1).view(np.uint32)
    nb = 1 if w is None else w.shape[0]
    f32 = v.dtype == np.float32
    E = 0 if edges is None else len(edges)
    st = [[0, 0, None, None, 0] for _ in range(nb)]
    hist = [[0] * (E + 2) for _ in range(nb)]
    rows = [[] for _ in range(nb)]
    for b in range(nb):
        for r in range(n_rows):
            if not _in(w, a, b, bit0 + r):
                continue
            x = v[r]
            if (f32 and x != x) or (not f32 and int(x) == INT32_MIN):
                st[b][1] += 1
                hist[b][E + 1] += 1
                continue
            st[b][0] += 1
            if st[b][2] is None or _lt(x, st[b][2]):
                st[b][2] = x
            if st[b][3] is None or _lt(st[b][3], x):
                st[b][3] = x
            if f32:
                c = min(max(float(x), -float(1 << 20)), float(1 << 20))
                st[b][4] += int(round(c * (1 << 24)))                            # (Python rounds halves to even, as rint does)
            else:
                st[b][4] += int(x)
            if E:
                hist[b][sum(1 for e in edges if not _lt(x, e))] += 1
            rows[b].append(r)
    wrap = lambda s: (s + (1 << 63)) % (1 << 64) - (1 << 63)
    zero = v.dtype.type(0)
    out_stats = (np.array([s[0] for s in st], np.int64), np.array([s[1] for s in st], np.int64),
                 np.array([sentinel(v.dtype) if s[2] is None else s[2] + zero for s in st], v.dtype),
                 np.array([sentinel(v.dtype) if s[3] is None else s[3] + zero for s in st], v.dtype), np.array([wrap(s[4]) for s in st], np.int64))
    h = np.array(hist, np.int64).reshape(nb, E + 2)
    ids = np.full((nb, k), -1, np.int64)
    vals = np.full((nb, k), sentinel(v.dtype), v.dtype)
    for b in range(nb):
        order = sorted(rows[b], key=lambda r: ((-float(v[r]) if descending else float(v[r])) + 0.0, r))[:k]
        for j, r in enumerate(order):
            ids[b, j], vals[b, j] = r + id_offset, v[r]
    return dict(stats=out_stats, histogram=(h[:, 1:E].copy(), h[:, 0].copy(), h[:, E].copy(), h[:, E + 1].copy()) if E else None, topk=(ids, vals))


# ---- the shard rule: results over row slices -> the result over all rows ----------------------------------------------------------------------
def merge_stats(parts):
    count, missing, lo, hi, total = (np.stack(x) for x in zip(*parts))
    dt = lo.dtype
    out_lo, out_hi = np.full(lo.shape[1], sentinel(dt), dt), np.full(lo.shape[1], sentinel(dt), dt)
    for b in range(lo.shape[1]):
        has = count[:, b] > 0
        if has.any():
            out_lo[b], out_hi[b] = lo[has, b].min(), hi[has, b].max()
    return count.sum(0), missing.sum(0), out_lo, out_hi, total.sum(0, dtype=np.int64)


def merge_histogram(parts):
    return tuple(sum(x[1:], x[0]) for x in zip(*parts))


def merge_topk(parts, k, descending=True):
    ids, vals = (np.concatenate(x, axis=1) for x in zip(*parts))
    out_i, out_v = np.full((ids.shape[0], k), -1, np.int64), np.full((ids.shape[0], k), sentinel(vals.dtype), vals.dtype)
    for b in range(ids.shape[0]):
        sel = np.flatnonzero(ids[b] >= 0)
        x = vals[b, sel].astype(np.float64)
        order = sel[np.lexsort((ids[b, sel], -x if descending else x))][:k]
        out_i[b, :order.size], out_v[b, :order.size] = ids[b, order], vals[b, order]
    return out_i, out_v


# ---- case generators ------------------------------------------------------------------------------------------------------------------------------
F32_SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 3.4028235e38, -3.4028235e38, 1.0, -1.0],
                        dtype=np.float32)
I32_SPECIALS = np.array([INT32_MIN + 1, (1 << 31) - 1, 0, -1, 1, (1 << 24) + 1, -(1 << 24) - 1, (1 << 30) + 3], dtype=np.int32)


def values_case(n_rows, dtype, seed, frac_missing=0.1, frac_special=0.05, spread=1000):
    """float32 / int32 values [n_rows]: a coarse grid (so that ties are common) with the type's special values and missing rows mixed in"""
    rng = np.random.default_rng(seed)
    u = rng.random(n_rows)
    if np.dtype(dtype) == np.float32:
        v = (rng.integers(-spread, spread, size=n_rows) / np.float32(8)).astype(np.float32)
        sp = u < frac_special
        v[sp] = rng.choice(F32_SPECIALS, size=int(sp.sum()))
        v[(u >= frac_special) & (u < frac_special + frac_missing)] = np.float32(np.nan)
        return v
    v = rng.integers(-spread, spread, size=n_rows).astype(np.int32)
    sp = u < frac_special
    v[sp] = rng.choice(I32_SPECIALS, size=int(sp.sum()))
    v[(u >= frac_special) & (u < frac_special + frac_missing)] = INT32_MIN
    return v


def edges_case(n_edges, dtype, seed=0, spread=1000):
    """n_edges strictly ascending edges inside (and a little beyond) the grid of values_case"""
    if np.dtype(dtype) == np.float32:
        return np.linspace(-spread / 8 - 1, spread / 8 + 1, n_edges).astype(np.float32) if n_edges > 3 else \
            np.array([-3.0, 0.0, 7.5][:n_edges], dtype=np.float32)
    step = max(1, (2 * spread + 20) // n_edges)
    return (-spread - 10 + step * np.arange(n_edges)).astype(np.int32)
