"""numpy reference of the percentiles (vs_value_quantiles / vs_value_radix_counts / vs_value_radix_step).

The definition.  For query b, K_b is the ascending multiset of the order keys (_value_ref.key) of the rows that are in the set (bitmap bit,
and_words bit) and carry a value (key != 0); count[b] = |K_b|, missing[b] = the set rows with key 0.  The order statistic of rank r (0-based)
is unkey(K_b[r]) (+0.0 of either zero); a rank outside 0..count - 1 gives the missing sentinel and a resolved rank of -1.  Quantile -> rank:
pos = q * float(count - 1), one fp64 multiplication; lower = floor(pos), higher = ceil(pos), nearest = rint(pos), half to even.
`order_statistics` is that definition by sorting.  `level_counts` / `level_counts_loops` / `step` restate the three radix levels of the C ABI
(digits: bits 31..21, 20..10, 9..0; slots = the sorted distinct prefixes of the ranks) with plain loops, and `radix_select` composes them over
any cut of the rows into shards, adding the shards' counts as a shard group does.  Everything is an integer or a bit pattern."""
import math

import numpy as np

from _value_ref import INT32_MIN, NAN_BITS, inset, is_missing, key, sentinel  # noqa: F401

BINS, LEVELS, MAX_RANKS = 2048, 3, 16
LOWER, HIGHER, NEAREST = 0, 1, 2
METHODS = {"lower": LOWER, "higher": HIGHER, "nearest": NEAREST}
NO_SLOT = 0xFFFFFFFF
LEVEL_BINS = (2048, 2048, 1024)
LEVEL_SHIFT = (21, 10, 0)
PREFIX_SHIFT = (32, 21, 10)                              # a level's slot is named by key >> PREFIX_SHIFT[level]


def unkey(k, dtype):
    """uint32 keys -> values of `dtype` (key 0 -> the missing sentinel, NaN 0x7FC00000 / INT32_MIN)"""
    k = np.asarray(k, dtype=np.uint64)
    if np.dtype(dtype) == np.int32:
        return (k ^ 0x80000000).astype(np.uint32).view(np.int32)
    u = np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k & 0xFFFFFFFF)
    return np.where(k == 0, NAN_BITS, u).astype(np.uint32).view(np.float32)


def rank_rule(q, count, method):
    """the quantile -> rank rule: -1 when there is no answer"""
    q, count = float(q), int(count)
    if count <= 0 or not (0.0 <= q <= 1.0):
        return -1
    pos = q * float(count - 1)
    m = METHODS.get(method, method)
    return int(math.floor(pos) if m == LOWER else math.ceil(pos) if m == HIGHER else np.rint(pos))


def set_keys(words, ld, bit0, n_rows, values, and_words=None, B=None):
    """-> (list of B ascending key arrays (uint32, no zeros), missing int64 [B])"""
    m = inset(words, ld, bit0, n_rows, and_words, B)
    k = key(np.asarray(values))
    return [np.sort(k[m[b] & (k != 0)]) for b in range(m.shape[0])], (m & (k == 0)[None, :]).sum(axis=1).astype(np.int64)


def resolve_ranks(counts, R, q=None, method="lower", ranks=None):
    """-> int64 [B, R]: the ranks the call resolves (-1: no answer)"""
    B = len(counts)
    out = np.full((B, R), -1, np.int64)
    for b in range(B):
        for j in range(R):
            if q is not None:
                out[b, j] = rank_rule(q[j], counts[b], method)
            else:
                r = int(ranks[b][j])
                out[b, j] = r if 0 <= r < counts[b] else -1
    return out


def order_statistics(words, ld, bit0, n_rows, values, q=None, method="lower", ranks=None, and_words=None, B=None):
    """the definition, by sorting -> (values [B, R] in the field's type, ranks int64 [B, R], count, missing int64 [B])"""
    v = np.asarray(values)
    ks, missing = set_keys(words, ld, bit0, n_rows, v, and_words, B)
    R = len(q) if q is not None else np.asarray(ranks).shape[1]
    count = np.array([k.size for k in ks], np.int64)
    rk = resolve_ranks(count, R, q, method, ranks)
    out = np.zeros((len(ks), R), np.uint32)
    for b, k in enumerate(ks):
        for j in range(R):
            out[b, j] = k[rk[b, j]] if rk[b, j] >= 0 else 0
    return unkey(out, v.dtype).reshape(len(ks), R), rk, count, missing


# ---- the three levels, as the C ABI has them ---------------------------------------------------------------------------------------------------
def level_counts(words, ld, bit0, n_rows, values, level, R, slot_prefix=None, n_slots=None, and_words=None, B=None):
    """vs_value_radix_counts -> (counts int64 [B, S, bins], missing int64 [B] | None): S = 1 at level 0, R below"""
    m = inset(words, ld, bit0, n_rows, and_words, B)
    k = key(np.asarray(values)).astype(np.int64)
    nb, bins, S = m.shape[0], LEVEL_BINS[level], 1 if level == 0 else R
    counts = np.zeros((nb, S, bins), np.int64)
    dig = (k >> LEVEL_SHIFT[level]) & (bins - 1)
    pre = k >> PREFIX_SHIFT[level]
    for b in range(nb):
        has = m[b] & (k != 0)
        if level == 0:
            counts[b, 0] = np.bincount(dig[has], minlength=bins)
            continue
        for s in range(int(n_slots[b])):
            counts[b, s] = np.bincount(dig[has & (pre == int(slot_prefix[b, s]))], minlength=bins)
    return counts, ((m & (k == 0)[None, :]).sum(axis=1).astype(np.int64) if level == 0 else None)


def level_counts_loops(words, ld, bit0, n_rows, values, level, R, slot_prefix=None, n_slots=None, and_words=None, B=None):
    """level_counts again, one row at a time"""
    m = inset(words, ld, bit0, n_rows, and_words, B)
    k = [int(x) for x in key(np.asarray(values))]
    nb, bins, S = m.shape[0], LEVEL_BINS[level], 1 if level == 0 else R
    counts = np.zeros((nb, S, bins), np.int64)
    missing = np.zeros(nb, np.int64)
    for b in range(nb):
        slots = [] if level == 0 else [int(p) for p in slot_prefix[b, :int(n_slots[b])]]
        for r in range(n_rows):
            if not m[b, r]:
                continue
            if k[r] == 0:
                missing[b] += 1
                continue
            d = (k[r] >> LEVEL_SHIFT[level]) & (bins - 1)
            if level == 0:
                counts[b, 0, d] += 1
            elif (k[r] >> PREFIX_SHIFT[level]) in slots:
                counts[b, slots.index(k[r] >> PREFIX_SHIFT[level]), d] += 1
    return counts, (missing if level == 0 else None)


def step(level, counts, R, state=None, q=None, method="lower", ranks=None, dtype=np.float32):
    """vs_value_radix_step with plain loops.  state (levels 1, 2): dict(rank_res, rank_slot, slot_prefix, n_slots) of the level above.
    -> dict(rank_res int64 [B, R], rank_slot int32 [B, R], rank_prefix uint32 [B, R], slot_prefix uint32 [B, R], n_slots int32 [B]) and, at
    level 0, count [B], ranks [B, R]; at level 2, values [B, R]"""
    B, bins = counts.shape[0], LEVEL_BINS[level]
    out = dict(rank_res=np.full((B, R), -1, np.int64), rank_slot=np.full((B, R), -1, np.int32), rank_prefix=np.zeros((B, R), np.uint32),
               slot_prefix=np.full((B, R), NO_SLOT, np.uint32), n_slots=np.zeros(B, np.int32))
    if level == 0:
        out["count"] = counts[:, 0, :].sum(axis=1).astype(np.int64)
        out["ranks"] = resolve_ranks(out["count"], R, q, method, ranks)
    for b in range(B):
        for j in range(R):
            if level == 0:
                s, r, old = 0, int(out["ranks"][b, j]), 0
            else:
                s, r = int(state["rank_slot"][b, j]), int(state["rank_res"][b, j])
                old = int(state["slot_prefix"][b, s]) if s >= 0 else 0
            if s < 0 or r < 0:
                continue
            cum = 0
            for d in range(bins):                                    # the bin d with cum <= r < cum + counts[d]
                c = int(counts[b, s, d])
                if cum <= r < cum + c:
                    out["rank_prefix"][b, j] = (old << (10 if level == 2 else 11)) | d
                    out["rank_res"][b, j] = r - cum
                    break
                cum += c
        slots = sorted({int(out["rank_prefix"][b, j]) for j in range(R) if out["rank_res"][b, j] >= 0})
        out["n_slots"][b] = len(slots)
        out["slot_prefix"][b, :len(slots)] = slots
        for j in range(R):
            if out["rank_res"][b, j] >= 0:
                out["rank_slot"][b, j] = slots.index(int(out["rank_prefix"][b, j]))
    if level == LEVELS - 1:
        out["values"] = unkey(out["rank_prefix"], dtype).reshape(B, R)
    return out


def radix_select(words, ld, bit0, n_rows, values, q=None, method="lower", ranks=None, and_words=None, B=None, cuts=None, counts_fn=level_counts,
                 trace=None):
    """The composition of the levels -> what order_statistics returns.  cuts: row bounds [0, ..., n_rows] of shards -- every shard counts its
    slice of the values and its bit range of the bitmaps, the counts are added before each step.  trace: a list that receives each level's
    (summed counts, state)."""
    v = np.asarray(values)
    cuts = [0, n_rows] if cuts is None else list(cuts)
    R = len(q) if q is not None else np.asarray(ranks).shape[1]
    state, missing = None, None
    for level in range(LEVELS):
        total = None
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            c, mis = counts_fn(words, ld, bit0 + r0, r1 - r0, v[r0:r1], level, R, state and state["slot_prefix"], state and state["n_slots"],
                               and_words, B)                         # (an and-bitmap lives at the words' bit0: read from bit0 + r0 on as well)
            total = c if total is None else total + c
            if level == 0:
                missing = mis if missing is None else missing + mis
        state = step(level, total, R, state, q, method, ranks, v.dtype)
        if level == 0:
            count, rk = state["count"], state["ranks"]
        if trace is not None:
            trace.append((total, state))
    return state["values"], rk, count, missing


def lerp(lo, hi, frac):
    """the facade's linear interpolation in fp64: exactly lo where lo == hi (so +-inf does not give NaN)"""
    lo, hi, frac = np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(frac, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(lo == hi, lo, lo + (hi - lo) * frac)
