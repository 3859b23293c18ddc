"""numpy reference of range search (vs_index_search_range) and the case generators of its tests.

The contract: for query b a row r matches iff it is live, the filter allows it and score(b, r) >= thr[b] compared as fp32 floats, with
    score = fl32( sum_c fp64( fl32(q[c] * v[c]) ) )          (q rounded to the index dtype, v = 1 on a binary index)
-- fp32 products, ONE fp64 sum, one rounding to fp32.  The products carry 24 significant bits and a row has far fewer than 2^16 of them, so
the fp64 sum keeps ~ 29 spare bits and the fp32 result does not depend on the order of the adds (csr_scan_mq.h): the reference is exact and
the GPU tests compare bits.  Outputs: the count, the match bitmap, and the first max_hits matches in the canonical order (score descending,
id ascending) with id -1 / score -inf behind them."""
import numpy as np

F32 = np.float32
MAX_HITS = 2048
K_WG_CAP = 4096            # csr_scan.h: kWgCap, the one-query scan's candidate buffer
K_MQ_SUPER = 512           # csr_scan_mq.h: kMqSuperRows (= kMaxKMq), rows between the tile scan's prune checks


# ---- scores -------------------------------------------------------------------------------------------------------------------------------
def stored(values, store):
    """the values an index of dtype `store` ("fp32" | "fp16" | "bin") holds, as fp32"""
    if store == "bin":
        return np.ones_like(values, dtype=F32)
    return values.astype(np.float16).astype(F32) if store == "fp16" else values.astype(F32)


def rounded_queries(q, store):
    return q.astype(np.float16).astype(F32) if store == "fp16" else q.astype(F32)


def scores(q, indptr, indices, values, store="fp32"):
    """[B, N] fp32 scores of dense queries q [B, V] against CSR rows, the library's exact numerics"""
    q = rounded_queries(q, store)
    v = stored(values, store)
    n = indptr.shape[0] - 1
    out = np.zeros((q.shape[0], n), dtype=F32)
    lens = np.diff(indptr)
    rows = np.flatnonzero(lens > 0)
    starts = indptr[:-1][rows]
    for b in range(q.shape[0]):
        prod = (q[b][indices] * v).astype(F32)                     # fl32(q[c] * v[c])
        if prod.size:
            out[b, rows] = (np.add.reduceat(prod.astype(np.float64), starts) + 0.0).astype(F32)   # (the sum starts at +0.0: never -0.0)
    return out


def scores_loop(q, indptr, indices, values, store="fp32"):
    """the same, a plain Python loop (what tests/test_range_cpu.py holds `scores` against)"""
    q = rounded_queries(q, store)
    v = stored(values, store)
    n = indptr.shape[0] - 1
    out = np.zeros((q.shape[0], n), dtype=F32)
    for b in range(q.shape[0]):
        for r in range(n):
            acc = 0.0
            for j in range(indptr[r], indptr[r + 1]):
                acc += float(F32(q[b, indices[j]]) * F32(v[j]))      # fp32 product, fp64 add
            out[b, r] = F32(acc)
    return out


# ---- the range search over a score matrix ---------------------------------------------------------------------------------------------------
def thresholds(thr, B):
    t = np.asarray(thr, dtype=F32)
    return np.full(B, t, dtype=F32) if t.ndim == 0 else t


def pack_bits(match):
    """bool [B, N] -> uint32 words [B, ceil(N / 32)], bit r of a row = bit r & 31 of word r >> 5; bits past N are 0"""
    B, n = match.shape
    W = (n + 31) // 32
    padded = np.zeros((B, W * 32), dtype=bool)
    padded[:, :n] = match
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(B, W)


def unpack_bits(words, n):
    w = np.ascontiguousarray(words).view(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :n].astype(bool)


def matches(S, thr, allowed=None):
    """bool [B, N]: allowed (live AND filter; [N] or [B, N] or None) and score >= thr as floats (-0.0 == +0.0; a NaN threshold matches none)"""
    B, n = S.shape
    with np.errstate(invalid="ignore"):
        m = S >= thresholds(thr, B)[:, None]
    if allowed is not None:
        m = m & np.broadcast_to(np.asarray(allowed, dtype=bool), (B, n))
    return m


def search(S, thr, max_hits, allowed=None, id_offset=0):
    """-> dict(ids int64 [B, max_hits], scores fp32, counts int64 [B], words uint32 [B, W])"""
    B, n = S.shape
    m = matches(S, thr, allowed)
    ids = np.full((B, max_hits), -1, dtype=np.int64)
    sc = np.full((B, max_hits), -np.inf, dtype=F32)
    for b in range(B):
        rows = np.flatnonzero(m[b])
        order = np.lexsort((rows, -S[b, rows].astype(np.float64)))    # score descending, id ascending (+0.0 and -0.0 tie: the id decides)
        top = rows[order][:max_hits]
        ids[b, :top.size] = top + id_offset
        sc[b, :top.size] = S[b, top]
    return dict(ids=ids, scores=sc, counts=m.sum(axis=1).astype(np.int64), words=pack_bits(m))


def search_loop(S, thr, max_hits, allowed=None):
    """the same, a plain Python loop over rows"""
    B, n = S.shape
    thr = thresholds(thr, B)
    ids = np.full((B, max_hits), -1, dtype=np.int64)
    sc = np.full((B, max_hits), -np.inf, dtype=F32)
    counts = np.zeros(B, dtype=np.int64)
    words = np.zeros((B, (n + 31) // 32), dtype=np.uint32)
    for b in range(B):
        hits = []
        for r in range(n):
            ok = True if allowed is None else bool(np.asarray(allowed)[b, r] if np.asarray(allowed).ndim == 2 else np.asarray(allowed)[r])
            if ok and float(S[b, r]) >= float(thr[b]):                  # False for a NaN threshold
                hits.append((-float(S[b, r]), r))
                counts[b] += 1
                words[b, r >> 5] |= np.uint32(1) << np.uint32(r & 31)
        hits.sort()
        for j, (_, r) in enumerate(hits[:max_hits]):
            ids[b, j], sc[b, j] = r, S[b, r]
    return dict(ids=ids, scores=sc, counts=counts, words=words)


def merge_shards(parts, max_hits):
    """The shard rule: per-shard results (each with global ids) -> merge the top-max_hits lists in the canonical order, sum the counts"""
    ids = np.concatenate([p["ids"] for p in parts], axis=1)
    sc = np.concatenate([p["scores"] for p in parts], axis=1)
    B = ids.shape[0]
    out_i = np.full((B, max_hits), -1, dtype=np.int64)
    out_s = np.full((B, max_hits), -np.inf, dtype=F32)
    for b in range(B):
        real = np.flatnonzero(ids[b] >= 0)
        order = np.lexsort((ids[b, real], -sc[b, real].astype(np.float64)))
        top = real[order][:max_hits]
        out_i[b, :top.size], out_s[b, :top.size] = ids[b, top], sc[b, top]
    return dict(ids=out_i, scores=out_s, counts=sum(p["counts"] for p in parts))


def assert_equal_bits(got, want, what, names=("ids", "scores", "counts", "words")):
    for n in names:
        g, w = np.ascontiguousarray(got[n]), np.ascontiguousarray(want[n])
        assert g.shape == w.shape, (what, n, g.shape, w.shape)
        if n == "scores":
            g, w = g.astype(F32).view(np.uint32), w.astype(F32).view(np.uint32)
        elif n == "words":
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, n, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def csr_case(n_rows, n_cols, seed, max_nnz=40, empty_every=9, twins=True):
    """CSR rows of generic random values: 0 .. max_nnz non-zeros a row, every empty_every-th row empty (no packets), and -- twins -- some rows
    exact copies of others (equal scores under every query: ties at a threshold, decided by the id)"""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n_rows):
        if empty_every and r % empty_every == empty_every - 1:
            rows.append((np.zeros(0, np.int32), np.zeros(0, F32)))
            continue
        if twins and r >= 5 and r % 7 == 5:
            rows.append(rows[r - 5] if rows[r - 5][0].size else rows[r - 4])
            continue
        nnz = int(rng.integers(1, max_nnz + 1))
        cols = np.sort(rng.choice(n_cols, size=min(nnz, n_cols), replace=False)).astype(np.int32)
        vals = (rng.random(cols.size) * 2 + 0.01).astype(F32)
        if r % 11 == 3:
            vals = -vals                                                 # rows of negative values: negative scores
        rows.append((cols, vals))
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum([c.size for c, _ in rows], out=indptr[1:])
    return indptr, np.concatenate([c for c, _ in rows]).astype(np.int32), np.concatenate([v for _, v in rows]).astype(F32)


def sparse_queries(B, n_cols, seed, nnz=48):
    """dense [B, n_cols] fp32 queries of `nnz` generic non-zeros (sparse enough for the tile scan)"""
    rng = np.random.default_rng(seed)
    q = np.zeros((B, n_cols), dtype=F32)
    for b in range(B):
        cols = rng.choice(n_cols, size=min(nnz, n_cols), replace=False)
        q[b, cols] = (rng.random(cols.size) + 0.05).astype(F32)
    return q


def dense_case(n_rows, n_cols, B, seed):
    """matrix and queries of values m / 256, m in 0 .. 15: every product and every partial sum is exact in fp32, whatever the order"""
    rng = np.random.default_rng(seed)
    mat = (rng.integers(0, 16, size=(n_rows, n_cols)) * (rng.random((n_rows, n_cols)) < 0.5)).astype(F32) / 256
    q = rng.integers(0, 16, size=(B, n_cols)).astype(F32) / 256
    return mat, q


def dense_to_csr(mat):
    rows, cols = np.nonzero(mat)
    indptr = np.zeros(mat.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=mat.shape[0]), out=indptr[1:])
    return indptr, cols.astype(np.int32), mat[rows, cols].astype(F32)


def tie_threshold(S, b):
    """a score of query b that several rows share (the largest such), and how many share it"""
    vals, cnt = np.unique(S[b], return_counts=True)
    shared = vals[cnt >= 2]
    assert shared.size, "the case has no tied scores"
    t = shared[-1]
    return F32(t), int(cnt[vals == t][0])


def halfway(S, b, rank):
    """a threshold strictly between the rank-th and the next distinct score of query b (descending) -> (thr, rows at or above it)"""
    vals = np.unique(S[b])[::-1]
    hi, lo = np.float64(vals[rank]), np.float64(vals[rank + 1])
    t = F32((hi + lo) / 2)
    assert lo < t <= hi
    return t, int((S[b] >= t).sum())
