"""The contract of the set egress (vs_set_count, vs_set_ids, vs_set_sample, vs_set_from_ids) in numpy: unpackbits over the
words, cut to [bit0, bit0 + n_rows), the and-words, nonzero, the window, the hash in uint64 arithmetic, a lexsort by (h, id) -- and the two
shard rules composed of them.  Nothing here is shared with the library."""
import numpy as np

MAX_SAMPLE = 1024
MAX_OUT_IDS = 1 << 27
SPAN_ROWS = 2048
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
NO_HASH = 0xFFFFFFFF
# (seed, id) -> h: the known answers of the pinned hash
KNOWN_HASHES = [(0, 0, 0x0397AB29), (0, 1, 0xC0737B7C), (1, 0, 0xDDC1ED05), (12345, 21015323, 0xFA680E94), ((1 << 64) - 1, (1 << 32) - 2, 0x29FC86AF)]


# ---- bitmaps -------------------------------------------------------------------------------------------------------------------------------
def n_words(bit0, n_rows):
    return (bit0 + n_rows + 31) // 32


def pack(masks, bit0=0, spare=0, garbage=None):
    """bool [B, n] -> uint32 words [B, n_words + spare]; garbage: a Generator that fills every bit outside the rows at random"""
    masks = np.atleast_2d(np.asarray(masks, bool))
    B, n = masks.shape
    W = n_words(bit0, n) + spare
    bits = np.zeros((B, W * 32), np.uint8)
    if garbage is not None:
        bits[:] = garbage.integers(0, 2, size=bits.shape, dtype=np.uint8)
    bits[:, bit0:bit0 + n] = masks
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view(np.uint32))


def unpack(words, bit0, n_rows):
    """uint32 words [B, W] (or [W]) -> bool [B, n_rows]: bits [bit0, bit0 + n_rows) of each row"""
    w = np.atleast_2d(np.ascontiguousarray(words)).view(np.uint8)
    return np.unpackbits(w, axis=1, bitorder="little")[:, bit0:bit0 + n_rows].astype(bool)


def members(words, bit0, n_rows, and_words=None, B=1):
    """the sets of a call -> bool [B, n_rows].  words None: every row (B = 1)"""
    m = np.ones((B, n_rows), bool) if words is None else unpack(words, bit0, n_rows)
    if and_words is not None:
        m = m & unpack(and_words, bit0, n_rows)
    return m


# ---- count, ids ------------------------------------------------------------------------------------------------------------------------------
def set_count(mask):
    return np.atleast_2d(mask).sum(axis=1).astype(np.int64)


def set_ids(mask, offsets=None, limit=0, id_offset=0):
    """-> (ids int64 [B, limit], counts int64 [B]): ranks [offset, offset + limit) of each row's ascending list, -1 behind the last"""
    mask = np.atleast_2d(mask)
    B = mask.shape[0]
    offsets = np.zeros(B, np.int64) if offsets is None else np.broadcast_to(np.asarray(offsets, np.int64), (B,))
    out = np.full((B, limit), -1, np.int64)
    for b in range(B):
        rows = np.nonzero(mask[b])[0].astype(np.int64) + id_offset
        page = rows[int(offsets[b]):int(offsets[b]) + limit]
        out[b, :page.shape[0]] = page
    return out, set_count(mask)


def pages(mask, page_size):
    """the pages of one set, until the first that is not full"""
    count, off = int(np.asarray(mask).sum()), 0
    while True:
        ids, _ = set_ids(mask, [off], page_size)
        yield ids[0]
        off += page_size
        if off >= count:
            return


# ---- the hash --------------------------------------------------------------------------------------------------------------------------------
def _mix(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sample_hash(seed, ids):
    """h of every id under one seed, uint32; all arithmetic modulo 2^64"""
    with np.errstate(over="ignore"):
        seed = np.asarray(int(seed) & 0xFFFFFFFFFFFFFFFF, np.uint64)
        ids = np.atleast_1d(np.asarray(ids, np.int64)).view(np.uint64)
        k = _mix(np.atleast_1d(seed + GOLDEN))[0]
        return (_mix(k ^ (GOLDEN * (ids + np.uint64(1)))) >> np.uint64(32)).astype(np.uint32)


def set_sample(mask, seeds, n, id_offset=0):
    """-> (ids int64 [B, n], hash uint32 [B, n], counts int64 [B]): per row the n members with the smallest (h, id), in that order"""
    mask = np.atleast_2d(mask)
    B = mask.shape[0]
    ids = np.full((B, n), -1, np.int64)
    hs = np.full((B, n), NO_HASH, np.uint32)
    for b in range(B):
        rows = np.nonzero(mask[b])[0].astype(np.int64) + id_offset
        h = sample_hash(seeds[b], rows)
        order = np.lexsort((rows, h))[:n]
        ids[b, :order.shape[0]] = rows[order]
        hs[b, :order.shape[0]] = h[order]
    return ids, hs, set_count(mask)


# ---- from ids --------------------------------------------------------------------------------------------------------------------------------
def from_ids(ids, n_rows, allow=True):
    """int64 [B, m] -> bool [B, n_rows]: ids below 0 and at or above n_rows are ignored"""
    ids = np.atleast_2d(np.asarray(ids, np.int64))
    out = np.zeros((ids.shape[0], n_rows), bool)
    for b in range(ids.shape[0]):
        ok = ids[b][(ids[b] >= 0) & (ids[b] < n_rows)]
        out[b, ok] = True
    return out if allow else ~out


# ---- the shard rules -------------------------------------------------------------------------------------------------------------------------
def _shards(mask, cuts):
    ends = list(cuts) + [np.atleast_2d(mask).shape[1]]
    return [(r0, np.atleast_2d(mask)[:, r0:r1]) for r0, r1 in zip([0] + list(cuts), ends)]


def sharded_ids(mask, cuts, offset, limit):
    """the window rule: shard s lists [offset - C_s, offset - C_s + limit) of its own list, clipped at 0 (C_s: the count of the shards before
    it), with id_offset = its first row; the pieces are placed one behind the other"""
    mask = np.atleast_2d(mask)
    B = mask.shape[0]
    offset = np.broadcast_to(np.asarray(offset, np.int64), (B,))
    out = np.full((B, limit), -1, np.int64)
    before, filled = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for row0, part in _shards(mask, cuts):
        local = np.maximum(offset - before, 0)
        ids, cnt = set_ids(part, local, limit, id_offset=row0)
        for b in range(B):
            got = ids[b][ids[b] >= 0][:limit - int(filled[b])]
            out[b, int(filled[b]):int(filled[b]) + got.shape[0]] = got
            filled[b] += got.shape[0]
        before = before + cnt
    return out, before


def sharded_sample(mask, cuts, seeds, n):
    """the sample merge: every shard samples n with id_offset = its first row and returns its hashes; the lists merge by (h, id), cut to n"""
    mask = np.atleast_2d(mask)
    B = mask.shape[0]
    parts = [set_sample(part, seeds, n, id_offset=row0) for row0, part in _shards(mask, cuts)]
    ids = np.concatenate([p[0] for p in parts], axis=1)
    hs = np.concatenate([p[1] for p in parts], axis=1)
    out_i, out_h = np.full((B, n), -1, np.int64), np.full((B, n), NO_HASH, np.uint32)
    for b in range(B):
        real = ids[b] >= 0
        order = np.lexsort((ids[b][real], hs[b][real]))[:n]
        out_i[b, :order.shape[0]] = ids[b][real][order]
        out_h[b, :order.shape[0]] = hs[b][real][order]
    return out_i, out_h, sum(p[2] for p in parts)


# ---- the plan rule ---------------------------------------------------------------------------------------------------------------------------
def plan_rule(n_rows, B, rows_per_chunk=0):
    """-> (chunks, rows_per_chunk, spans)"""
    if rows_per_chunk == 0:
        rows_per_chunk = max(-(-n_rows // max(1, 1024 // B)), 8192)
    rows_per_chunk = -(-rows_per_chunk // SPAN_ROWS) * SPAN_ROWS
    return -(-n_rows // rows_per_chunk), rows_per_chunk, -(-n_rows // SPAN_ROWS)


def chi2_per_df(base, M, n, S):
    """the uniformity statistic of the hash's definition: over seeds 0..S - 1, how often each of M rows from `base` is among the n sampled"""
    rows = np.arange(base, base + M, dtype=np.int64)
    cnt = np.zeros(M, np.int64)
    for seed in range(S):
        h = sample_hash(seed, rows)
        cnt[np.lexsort((rows, h))[:n]] += 1
    p = n / M
    return float((((cnt - S * p) ** 2) / (S * p * (1 - p))).sum() / (M - 1))
