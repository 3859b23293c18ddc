"""numpy reference of boosted search (vs_index_search_boosted) and the case generators of its tests.

The contract, for query b, row r and F fields (1..4; float32 or int32 columns, NaN / INT32_MIN = no value), weights w float32 [B, F]:
    S    = the fp64 sum range search holds before its rounding: sum_c fp64(fl32(q[c] * v[c])), +0.0 for a row with no packets
           (_range_ref.scores before its final cast); on the matrix cores S = fp64(the fp32 search score)
    t_j  = +0.0 if w[b, j] == 0 or the row has no value in field j, else fp64(w[b, j]) * fp64(value_j[r])        (exact in fp64)
    add:   x = (((S + t_0) + t_1) + ...)              mul:   u = (((1.0 + t_0) + t_1) + ...), x = S * u
    boosted = canon_zero(fl32(x)); x NaN (or a NaN weight): the row matches nothing for that query
and then _range_ref.search over the boosted matrix: count, bitmap, the first max_hits in the canonical order (boosted descending, id
ascending).  A plain-Python-loop twin (boosted_loop) is what tests/test_boost_cpu.py holds the numpy version against."""
import math

import numpy as np

import _range_ref as rr

F32, F64 = np.float32, np.float64
INT32_MISSING = np.int32(-2 ** 31)
ADD, MUL = "add", "mul"


def sums(q, indptr, indices, values, store="fp32"):
    """[B, N] fp64 row sums: _range_ref.scores without its final cast"""
    q = rr.rounded_queries(q, store)
    v = rr.stored(values, store)
    n = indptr.shape[0] - 1
    out = np.zeros((q.shape[0], n), dtype=F64)
    lens = np.diff(indptr)
    rows = np.flatnonzero(lens > 0)
    starts = indptr[:-1][rows]
    for b in range(q.shape[0]):
        prod = (q[b][indices] * v).astype(F32)
        if prod.size:
            out[b, rows] = np.add.reduceat(prod.astype(F64), starts) + 0.0
    return out


def missing(col):
    col = np.asarray(col)
    return np.isnan(col) if col.dtype == F32 else col == INT32_MISSING


def weights(w, B, F):
    w = np.asarray(w, dtype=F32)
    return np.ascontiguousarray(np.broadcast_to(w[None, :] if w.ndim == 1 else w, (B, F)))


def boosted(S, fields, w, mode):
    """S fp64 [B, N], fields: list of F columns [N], w float32 [B, F] -> (boosted float32 [B, N], valid bool [B, N])"""
    S = np.asarray(S, dtype=F64)
    B, n = S.shape
    w = weights(w, B, len(fields))
    assert S.dtype == F64 and w.dtype == F32 and all(np.asarray(f).dtype in (F32, np.int32) for f in fields) and mode in (ADD, MUL)
    valid = np.ones((B, n), dtype=bool)
    u = S.copy() if mode == ADD else np.ones((B, n), dtype=F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, col in enumerate(fields):
            col = np.asarray(col)
            wj = w[:, j].astype(F64)[:, None]
            t = wj * np.where(missing(col), 0, col).astype(F64)[None, :]
            t = np.where((w[:, j] == 0)[:, None] | missing(col)[None, :], 0.0, t)
            valid &= ~np.isnan(w[:, j])[:, None]
            u = u + t
        x = u if mode == ADD else S * u
        valid &= ~np.isnan(x)
        out = x.astype(F32) + F32(0)                                      # (-0.0 + 0.0 = +0.0: canon_zero)
    return out, valid


def boosted_loop(S, fields, w, mode):
    """the same, plain Python floats (IEEE doubles), one (query, row) at a time"""
    B, n = S.shape
    w = weights(w, B, len(fields))
    out = np.zeros((B, n), dtype=F32)
    valid = np.zeros((B, n), dtype=bool)
    for b in range(B):
        for r in range(n):
            s = float(S[b, r])
            u = s if mode == ADD else 1.0
            ok = True
            for j, col in enumerate(fields):
                wj = float(w[b, j])
                t = 0.0
                if wj != 0.0:
                    if math.isnan(wj):
                        ok = False
                        break
                    v = col[r]
                    gone = math.isnan(float(v)) if col.dtype == F32 else int(v) == -2 ** 31
                    if not gone:
                        t = wj * float(v)
                u = u + t
            if not ok:
                continue
            x = s * u if mode == MUL else u
            if math.isnan(x):
                continue
            with np.errstate(over="ignore"):
                f = F32(x)
            out[b, r] = F32(0) if f == 0 else f
            valid[b, r] = True
    return out, valid


def search(S, fields, w, mode, thr, max_hits, allowed=None, id_offset=0):
    """-> _range_ref.search's dict over the boosted scores; thr None = -inf"""
    X, valid = boosted(S, fields, w, mode)
    if allowed is not None:
        valid = valid & np.broadcast_to(np.asarray(allowed, dtype=bool), valid.shape)
    X = np.where(valid, X, F32(0))                                        # (a row that matches nothing: any number, `valid` keeps it out)
    return rr.search(X, -np.inf if thr is None else thr, max_hits, valid, id_offset)


def shard_search(S, fields, w, mode, thr, max_hits, bounds, allowed=None):
    """the shard rule on the reference: every shard its row slice of S, of every field and of the filter, ids + its first row; merged"""
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        a = None if allowed is None else np.broadcast_to(allowed, S.shape)[:, lo:hi]
        parts.append(search(S[:, lo:hi], [f[lo:hi] for f in fields], w, mode, thr, max_hits, a, id_offset=lo))
    out = rr.merge_shards(parts, max_hits)
    n = S.shape[1]
    m = np.concatenate([rr.unpack_bits(p["words"], hi - lo) for p, lo, hi in zip(parts, bounds[:-1], bounds[1:])], axis=1)
    out["words"] = rr.pack_bits(m[:, :n])
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def twin_sources(n_rows, empty_every=9):
    """row -> the row csr_case copied it from (its twins: r % 7 == 5, r >= 5), as csr_case decides it"""
    src = {}
    for r in range(n_rows):
        if empty_every and r % empty_every == empty_every - 1:
            continue
        if r >= 5 and r % 7 == 5:
            s = r - 5 if (r - 5) % empty_every != empty_every - 1 else r - 4
            src[r] = src.get(s, s)
    return src


def field_f32(n_rows, seed, missing_every=13, twins=True):
    """random() * 10 as float32; every missing_every-th value missing; twins: every second twin row of csr_case shares the value of its
    source (equal S, equal value: a tie the id decides), the others keep their own (equal S, different values: the boost flips the order)"""
    rng = np.random.default_rng(seed)
    col = (rng.random(n_rows) * 10).astype(F32)
    if twins:
        for i, (r, s) in enumerate(sorted(twin_sources(n_rows).items())):
            if i % 2 == 0:
                col[r] = col[s]
    if missing_every:
        col[missing_every - 1::missing_every] = np.nan
    return col


def field_i32(n_rows, seed, missing_every=13, lo=-50, hi=2030):
    rng = np.random.default_rng(seed)
    col = rng.integers(lo, hi, size=n_rows).astype(np.int32)
    if missing_every:
        col[5::missing_every] = INT32_MISSING
    return col


def exact_sums(q, indptr, indices, values, store, rows, b=0):
    """math.fsum, the forward and the reversed fp64 sum of the sampled rows' products agree (so S does not depend on the order of the adds)"""
    qq, v = rr.rounded_queries(q, store), rr.stored(values, store)
    for r in rows:
        prod = [float(F32(qq[b, indices[j]]) * F32(v[j])) for j in range(indptr[r], indptr[r + 1])]
        fwd = 0.0
        for p in prod:
            fwd += p
        rev = 0.0
        for p in reversed(prod):
            rev += p
        if not (math.fsum(prod) == fwd == rev):
            return False
    return True


def has_ties(X, valid, b):
    vals, cnt = np.unique(X[b][valid[b]], return_counts=True)
    return bool((cnt >= 2).any())


def tops_differ(S, X, k=16):
    """per query: the top k by boosted score is another list than the top k by fl32(S)"""
    plain = rr.search(S.astype(F32), -np.inf, k)["ids"]
    boost = rr.search(X, -np.inf, k)["ids"]
    return (plain != boost).any(axis=1)
