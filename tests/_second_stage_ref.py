"""Plain numpy references of the kernels that run after the search walks (rerank, shard merge, encoder pooling), and the
seeded inputs their tests share.  No GPU, no library call: tests/test_second_stage_ref_cpu.py pins these functions to the
CPU oracle and to torch on a machine without a GPU, tests/test_gpu_second_stage.py pins the HIP kernels to them.

Order rules restated here (include/vsearch_hip.h):
  rerank : score descending, first-stage rank ascending;  merge : score descending, id ascending.
Scores compare as floats: -0.0 and +0.0 tie (rank / id decides) and both come back as +0.0; -inf sorts last.
"""
from collections import namedtuple

import numpy as np

ID_LIMIT = 2 ** 32 - 1          # merge keys hold 32-bit ids; 2^32 - 1 itself is the pad sentinel

RerankScores = namedtuple("RerankScores", "exact32 hi abs_sum")


# ---- references ----------------------------------------------------------------------------------------------------------------
def rerank_scores_ref(p, q, k, row0=0):
    """scores[r] = <p[r, :], q[(row0 + r) // k, :]> where a zero passage element contributes nothing whatever q holds.

    exact32: float32 products (the kernel's), summed in float64, cast to float32.
    hi / abs_sum: float64 products, their sum and the sum of their magnitudes (the error bound's scale)."""
    p32 = np.asarray(p).astype(np.float32)
    q = np.asarray(q, dtype=np.float32)
    qr = q[(row0 + np.arange(p32.shape[0])) // k]
    live = p32 != 0                                       # (-0.0 is a zero too)
    with np.errstate(all="ignore"):
        prod32 = np.where(live, p32 * qr, np.float32(0))
        assert prod32.dtype == np.float32
        exact32 = prod32.astype(np.float64).sum(axis=1).astype(np.float32)
        prod64 = np.where(live, p32.astype(np.float64) * qr.astype(np.float64), 0.0)
        hi = prod64.sum(axis=1)
        abs_sum = np.abs(prod64).sum(axis=1)
    return RerankScores(exact32, hi, abs_sum)


def rerank_topk_ref(scores, hit_ids):
    """Per row: hits ordered by (score descending, first-stage rank ascending) -> (ids, scores)."""
    scores = np.asarray(scores, dtype=np.float32)
    hit_ids = np.asarray(hit_ids, dtype=np.int64)
    out_ids = np.empty_like(hit_ids)
    out_sc = np.empty_like(scores)
    rank = np.arange(scores.shape[1])
    for b in range(scores.shape[0]):
        order = np.lexsort((rank, -scores[b]))
        out_ids[b] = hit_ids[b][order]
        out_sc[b] = (scores[b] + np.float32(0))[order]    # (-0.0 + 0.0 = +0.0)
    return out_ids, out_sc


def merge_topk_ref(ids, scores, k):
    """Per row: drop ids outside [0, 2^32 - 1), order by (score descending, id ascending), take k, pad with -1 / -inf."""
    ids = np.asarray(ids, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float32)
    B = ids.shape[0]
    out_ids = np.full((B, k), -1, dtype=np.int64)
    out_sc = np.full((B, k), -np.inf, dtype=np.float32)
    for b in range(B):
        keep = (ids[b] >= 0) & (ids[b] < ID_LIMIT)
        i, s = ids[b][keep], scores[b][keep]
        order = np.lexsort((i, -s))[:k]
        out_ids[b, :order.size] = i[order]
        out_sc[b, :order.size] = (s + np.float32(0))[order]
    return out_ids, out_sc


def _elu1p64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(x > 0, x + 1.0, np.expm1(np.minimum(x, 0.0)) + 1.0)


def mean_topk_ref(logits, t):
    """out[b, c] = mean of the t largest elu1p(logits[b, :, c]); float64 throughout."""
    act = _elu1p64(logits)
    top = -np.sort(-act, axis=1)[:, :t]
    return top.sum(axis=1) / float(t)


def head_pool_ref(logits):
    """out[b, c] = elu1p(max_l logits[b, l, c]); float64 throughout."""
    return _elu1p64(np.asarray(logits, dtype=np.float64).max(axis=1))


# ---- float32 helpers -----------------------------------------------------------------------------------------------------------
def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulp32(x):
    """Spacing of float32 at |x| (as float64)."""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def ulp_distance32(a, b):
    """Number of float32 values between a and b (finite inputs)."""
    def lin(x):
        i = bits32(x).astype(np.int64)
        return np.where(i & 0x80000000, 0x80000000 - i, i)
    return np.abs(lin(a) - lin(b))


# ---- shared inputs -------------------------------------------------------------------------------------------------------------
def dyadic_signed(rng, shape, dtype=np.float32):
    """j / 64 with j in +-[1, 255]: never zero, exact in fp16; a product of two is a multiple of 2^-12 below 16 and any sum of
    fewer than 2^36 of them is exact in float64 -- so the only rounding is the final cast, the same in every summation order."""
    j = rng.integers(1, 256, size=shape) * rng.choice((-1, 1), size=shape)
    return (j / 64.0).astype(dtype)


# lane l of the fp32 rerank kernel owns columns 4 l .. 4 l + 3 of every 256: it enters the 4-deep unrolled loop from V = 772 + 4 l
# (772 = 3 * 256 + 4: lane 0 alone, 1024: every lane), the single-step loop ends at the multiples of 4 and of 256, and the V % 4
# tail belongs to one lane
RERANK_WIDTHS = [1, 3, 4, 5, 255, 256, 257, 771, 772, 773, 1023, 1024, 1027, 1028, 4096, 4097, 4098, 4099, 29523, 30522, 33000]


def rerank_dyadic_case(V, dtype=np.float32, B=3, k=5):
    """The dense dyadic passages [B * k, V] and queries [B, V] of width V that the bit-exact rerank tests score."""
    rng = np.random.default_rng(1000 + V)
    return dyadic_signed(rng, (B * k, V), dtype), dyadic_signed(rng, (B, V)), k


def sparse_randn(rng, shape, zeros, dtype=np.float32):
    v = rng.standard_normal(shape)
    v[rng.random(shape) < zeros] = 0.0
    return v.astype(dtype)


MERGE_LAWS = ("few", "tiefree", "winners_last", "winners_first", "runs8")


def merge_ids(rng, B, n):
    """Distinct ids per row from [0, 2^32 - 1), with 0 and the largest valid id 2^32 - 2 present in every row that has room."""
    ids = np.empty((B, n), dtype=np.int64)
    for b in range(B):
        row = np.unique(rng.integers(1, ID_LIMIT - 1, size=2 * n + 8))
        assert row.size >= n
        row = rng.permutation(row)[:n]
        if n >= 2:
            row[rng.choice(n, size=2, replace=False)] = (0, ID_LIMIT - 1)
        ids[b] = row
    return ids


def merge_scores(rng, law, B, n, k):
    """[B, n] float32 candidate scores under one of MERGE_LAWS."""
    if law == "few":                       # at most 8 distinct values: ties straddle every 4096- and 2048-key round boundary
        return (rng.integers(0, 8, size=(B, n)) / 4.0).astype(np.float32)
    if law == "tiefree":
        return np.stack([rng.permutation(n) for _ in range(B)]).astype(np.float32) / 8
    if law in ("winners_last", "winners_first"):
        # the k winners sit in the last (first) max(k, 100) slots, everything else is below them
        span = min(n, max(k, 100))
        sc = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.float32) / 8 - n
        for b in range(B):
            slots = rng.permutation(span)[:k]
            slots = n - 1 - slots if law == "winners_last" else slots
            sc[b, slots] = rng.permutation(k).astype(np.float32) + 1
        return sc
    if law == "runs8":                     # eight descending-sorted runs, the shape an all-gather of per-shard top-k lists delivers
        sc = (rng.integers(0, 64, size=(B, n)) / 8.0).astype(np.float32)
        for part in np.array_split(np.arange(n), 8):
            if part.size:
                sc[:, part] = -np.sort(-sc[:, part], axis=1)
        return sc
    raise ValueError(law)


RERANK_PATTERNS = ("all_equal", "three_values", "sorted", "reversed", "random", "pad_tail", "plus_inf", "signed_zeros", "denormals")


def rerank_case(rng, pattern, B, k):
    """(scores [B, k] float32, hit_ids [B, k] int64 >= 2^40 (pads: -1)) for one of RERANK_PATTERNS."""
    ids = np.stack([rng.permutation(10 * k + 7)[:k] for _ in range(B)]).astype(np.int64) + 2 ** 40
    if pattern == "all_equal":
        sc = np.full((B, k), 2.5, dtype=np.float32)
    elif pattern == "three_values":
        sc = rng.choice(np.array([-1.5, 0.25, 7.0], dtype=np.float32), size=(B, k))
    elif pattern in ("sorted", "reversed"):
        sc = np.stack([np.sort(rng.permutation(4 * k)[:k]) for _ in range(B)]).astype(np.float32) / 4
        sc = sc[:, ::-1].copy() if pattern == "sorted" else sc
    elif pattern == "random":
        sc = np.stack([rng.permutation(4 * k)[:k] for _ in range(B)]).astype(np.float32) / 4 - k
    elif pattern == "pad_tail":                       # a filtered first stage: the last third of every row is padding
        sc = rng.choice(np.array([-3.0, 0.5, 0.75, 9.0], dtype=np.float32), size=(B, k))
        n_pad = k // 3
        if n_pad:
            sc[:, k - n_pad:] = -np.inf
            ids[:, k - n_pad:] = -1
    elif pattern == "plus_inf":
        sc = rng.choice(np.array([np.inf, -np.inf, 1.0, 2.0, 3.4e38], dtype=np.float32), size=(B, k))
    elif pattern == "signed_zeros":
        sc = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32), size=(B, k))
    elif pattern == "denormals":
        sc = rng.choice(np.array([1e-45, -1e-45, 3e-39, -3e-39, 0.0, 1.2e-38], dtype=np.float32), size=(B, k))
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(sc, dtype=np.float32), ids


POOL_PATTERNS = ("ascending", "descending", "all_equal", "duplicates", "neg_inf")


def pool_logits_dyadic(rng, pattern, B, L, V):
    """[B, L, V] positive logits j / 8 (j in [1, 2000]) laid out along L by `pattern`: elu1p is x + 1 and any sum of 32 of them is
    exact in float32.  "neg_inf" replaces about a third of the entries by -inf (elu1p = 0, still exact)."""
    j = rng.integers(1, 2001, size=(B, L, V))
    if pattern == "ascending":
        j = np.sort(j, axis=1)
    elif pattern == "descending":
        j = -np.sort(-j, axis=1)
    elif pattern == "all_equal":
        j = np.broadcast_to(j[:, :1], (B, L, V))
    elif pattern in ("duplicates", "neg_inf"):
        j = rng.integers(1, 6, size=(B, L, V)) * 100
    x = (j / 8.0).astype(np.float32)
    if pattern == "neg_inf":
        x[rng.random((B, L, V)) < 0.35] = -np.inf
    return np.ascontiguousarray(x)
