"""numpy reference of the scores of a document set (vs_index_set_scores) and the case generators of its tests.

The contract: out[b, r] = the library's exact score of (query b, row r) -- _range_ref.scores, what range search decides by -- when row r is
live and bit bit0 + r of query b's bitmap is set, and the missing sentinel of the numeric fields, NaN 0x7FC00000, everywhere else.  The result
is a float32 field: its order keys, stats, bins and ranks are _value_ref's."""
import numpy as np

from _range_ref import F32, assert_equal_bits, csr_case, pack_bits, scores, scores_loop, sparse_queries  # noqa: F401
from _value_ref import NAN_BITS, bits, histogram, inset, key, pack, same, stats, topk  # noqa: F401

N_ROWS = 2 * 2048 + 77          # two full spans and a ragged tail with a partial last word


def in_set(words, ld, bit0, n_rows, B):
    """bool [B, n_rows]: words None (every row), one bitmap shared by the batch (ld = 0) or one per query; uint32 words, bit bit0 + r = row r"""
    if words is None:
        return np.ones((B, n_rows), dtype=bool)
    m = inset(np.atleast_2d(words) if ld else np.asarray(words).reshape(1, -1), 1 if ld else 0, bit0, n_rows)
    return np.broadcast_to(m, (B, n_rows)) if m.shape[0] == 1 else m


def set_scores(S, words=None, ld=0, bit0=0, deleted=None):
    """S [B, N] fp32 scores of every row -> [B, N] fp32 with 0x7FC00000 outside the set and on the deleted rows (bool [N] or None)"""
    B, n = S.shape
    m = in_set(words, ld, bit0, n, B)
    if deleted is not None:
        m = m & ~np.asarray(deleted, dtype=bool)[None, :]
    out = np.full((B, n), NAN_BITS, dtype=np.uint32)
    out[m] = np.ascontiguousarray(S, dtype=F32).view(np.uint32)[m]
    return out.view(F32)


def set_scores_loop(q, indptr, indices, values, store, words, ld, bit0, deleted):
    """the same from the rows themselves, plain Python loops over the raw words"""
    full = scores_loop(q, indptr, indices, values, store)
    B, n = full.shape
    out = np.full((B, n), NAN_BITS, dtype=np.uint32)
    w = None if words is None else np.ascontiguousarray(words).view(np.uint32).reshape(-1)
    for b in range(B):
        for r in range(n):
            bit = bit0 + r
            ok = True if w is None else bool((int(w[b * ld + (bit >> 5)]) >> (bit & 31)) & 1)
            if ok and not (deleted is not None and deleted[r]):
                out[b, r] = full[b:b + 1, r].view(np.uint32)[0]
    return out.view(F32)


def shard_slices(S, cuts, words, ld, bit0, deleted=None):
    """The shard rule: shard i scores rows [cuts[i], cuts[i + 1]) under bits bit0 + cuts[i] ... of the same bitmaps; the slices side by side"""
    parts = []
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        parts.append(set_scores(S[:, r0:r1], words, ld, bit0 + r0, None if deleted is None else deleted[r0:r1]))
    return np.concatenate(parts, axis=1)


def pack_at(mask, bit0):
    """bool [B, N] -> uint32 words [B, W] with row r at bit bit0 + r; the bits below bit0 and past the rows are SET (they must be ignored)"""
    return pack(mask, bit0, spare=1)


def long_rows_case(n_rows, n_cols, seed, long_rows=(3, 2047, 2048, 4100), store_max_nnz=40):
    """csr_case with a handful of rows of 520 .. 1100 non-zeros: more than 64 packets, so a lane's second loop trip is reached"""
    indptr, indices, values = csr_case(n_rows, n_cols, seed, max_nnz=store_max_nnz)
    rng = np.random.default_rng(seed + 1000)
    rows = [(indices[indptr[r]:indptr[r + 1]], values[indptr[r]:indptr[r + 1]]) for r in range(n_rows)]
    for i, r in enumerate(long_rows):
        if r < n_rows:
            nnz = min(n_cols, int(rng.integers(520, 1101)))
            cols = np.sort(rng.choice(n_cols, size=nnz, replace=False)).astype(np.int32)
            rows[r] = (cols, ((rng.random(nnz) * 2 + 0.01) * (-1 if i % 2 else 1)).astype(F32))
    ip = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum([c.size for c, _ in rows], out=ip[1:])
    return ip, np.concatenate([c for c, _ in rows]).astype(np.int32), np.concatenate([v for _, v in rows]).astype(F32)


def set_shapes(n, B, seed=0):
    """name -> bool [B, n] (per query) or [1, n] (shared): the sets the kernel can go wrong on"""
    rng = np.random.default_rng(seed)
    z = lambda rows=1: np.zeros((rows, n), dtype=bool)
    out = {"every": np.ones((1, n), dtype=bool), "none": z()}
    out["first"] = z(); out["first"][0, 0] = True
    out["last"] = z(); out["last"][0, n - 1] = True
    gap = z(); gap[0, :2048] = rng.random(2048) < 0.3; gap[0, 4096:] = True           # the middle span all zero
    out["gap"] = gap
    out["p1"] = rng.random((B, n)) < 0.01
    out["p50"] = rng.random((B, n)) < 0.5
    run = z(B)
    for b in range(B):
        run[b, 1900 + 50 * b:2200 + 50 * b] = True                                    # 300 consecutive rows across a span edge
    out["run"] = run
    return out
