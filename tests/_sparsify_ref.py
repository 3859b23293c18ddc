"""Plain numpy references of the encoder tail (csrc/sparsify.hip, mask_rows_fast.h, dense_csr.h): the top-k / lexical mask stage, its
fusion with the dense -> CSR conversion, dense -> CSR itself, the bag-of-words mask, elu1p and the head's max pooling -- and the seeded
inputs their tests share.  No GPU, no library call, no oracle: tests/test_sparsify_ref_cpu.py pins these functions to torch and to the
CPU oracle on a machine without a GPU, tests/test_gpu_sparsify_edges.py pins the HIP kernels to them.

The contract restated here (include/vsearch_hip.h, "sparsify"):
  selection : a row's k largest ORDER KEYS, ties at the k-th key to the lower column.  The order key of an fp32 value is its bit pattern
              with the sign bit set (non-negative values) or all bits inverted (negative values), compared as uint32: the float order on
              everything that compares, +0.0 ABOVE -0.0, positive NaNs above +inf and negative NaNs below -inf, each by bit pattern.
  mask      : a dropped element becomes x * 0 (a signed zero; NaN for NaN and +-inf), a kept element keeps its bits.
  fused CSR : the kept elements that are not +-0.0, in column order (a kept NaN / inf is stored).  The fused call expects finite input:
              an unselected NaN / inf is DROPPED, where vs_embed_mask + vs_dense_to_csr store the NaN that x * 0 makes of it.
  dense CSR : every element != 0 (NaN, +-inf and subnormals are stored, +-0.0 are not), in column order.
"""
from collections import namedtuple

import numpy as np

# ---- the fast mask kernel's geometry (csrc/mask_rows_fast.h), restated so that a test can name the path its input takes -----------------
MR_THREADS = 512
MR_STEP = MR_THREADS * 4          # columns per g
MR_COLS = 32 * 1024               # widest row of the fast kernel
MR_CAND = 2048                    # list capacity
MR_STAGE = 8192                   # kept elements of a row the fused kernel stages
SLOW_LDS_LIMIT = 160 * 1024

PATHS = ("take_all", "list_128", "list_256", "list_2048", "hist_all_eq", "hist_bitmap")


def fast_g(V):
    """the instantiation run_mask picks for V columns"""
    assert 0 < V <= MR_COLS
    return 4 if V <= 4 * MR_STEP else 8 if V <= 8 * MR_STEP else 15 if V <= 15 * MR_STEP else 16


def slow_lds_bytes(V):
    """mask_lds_bytes (csrc/sparsify.hip)"""
    vwords = (V + 31) // 32
    return (((V + 3) & ~3) + 2 * ((vwords + 3) & ~3) + 2 * (1024 // 64) + 32 + 4 + 256 * 8) * 4


def slow_max_v():
    """the widest row mask_rows_kernel admits"""
    V = 1
    while slow_lds_bytes(V + 1) <= SLOW_LDS_LIMIT:
        V += 1
    return V


# ---- references ----------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def bits(x):
    return _f32(x).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def order_key(x):
    """uint32 whose unsigned order is the selection order of fp32 x"""
    u = bits(x)
    return np.where((u >> np.uint32(31)) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _order(keys):
    """per row: the columns by (key descending, column ascending)"""
    return np.argsort(~keys, axis=-1, kind="stable")


def topk_mask_ref(x, k):
    """bool [B, V]: the k largest order keys of every row, ties to the lower column (k = 0: none)"""
    x = np.atleast_2d(_f32(x))
    B, V = x.shape
    assert 0 <= k <= V
    mask = np.zeros((B, V), dtype=bool)
    if k > 0:
        np.put_along_axis(mask, _order(order_key(x))[:, :k], True, axis=1)
    return mask


def lexical_mask_ref(ids, vocab, shift):
    """bool [B, vocab - shift]: columns token - shift of the row's tokens >= shift.  ValueError for a token outside [0, vocab)."""
    ids = np.atleast_2d(np.asarray(ids, dtype=np.int64))
    if ((ids < 0) | (ids >= vocab)).any():
        raise ValueError("token id out of range")
    B = ids.shape[0]
    m = np.zeros((B, vocab - shift), dtype=bool)
    rows = np.repeat(np.arange(B), ids.shape[1]).reshape(ids.shape)
    live = ids >= shift
    m[rows[live], ids[live] - shift] = True
    return m


def bow_mask_ref(ids, vocab, shift=0, norm=False):
    """float64 [B, vocab - shift]: multi-hot of the tokens, rows divided by max(sqrt(count), 1e-12) with norm"""
    m = lexical_mask_ref(ids, vocab, shift).astype(np.float64)
    if norm:
        m /= np.maximum(np.sqrt(m.sum(axis=1, keepdims=True)), 1e-12)
    return m


def keep_mask_ref(x, ids, vocab, shift, topk, lexical, topk_mask=None):
    """bool [B, V]: topk > 0: the top-k mask; 0: nothing; < 0: everything -- | the lexical columns with `lexical`"""
    x = np.atleast_2d(_f32(x))
    assert x.shape[1] == vocab - shift
    if topk_mask is not None:
        keep = topk_mask.copy()
    elif topk < 0:
        keep = np.ones(x.shape, dtype=bool)
    else:
        keep = topk_mask_ref(x, topk)
    if lexical:
        keep |= lexical_mask_ref(ids, vocab, shift)
    return keep


def masked_bits(x, keep):
    """uint32 [B, V]: x where kept, x * 0 where dropped, as bit patterns"""
    x = np.atleast_2d(_f32(x))
    with np.errstate(invalid="ignore"):
        return np.where(keep, x, x * np.float32(0)).astype(np.float32).view(np.uint32)


def embed_mask_ref(x, ids, vocab, shift, topk, lexical, bow=False):
    """the mask stage of VDREncoder.embed as bit patterns, uint32 [B, V]"""
    if bow:
        return bow_mask_ref(ids, vocab, shift).astype(np.float32).view(np.uint32)
    return masked_bits(x, keep_mask_ref(x, ids, vocab, shift, topk, lexical))


Csr = namedtuple("Csr", "rowptr cols vals")


def _csr_of(x, take):
    r, c = np.nonzero(take)
    rowptr = np.zeros(x.shape[0] + 1, dtype=np.int64)
    np.cumsum(take.sum(axis=1), out=rowptr[1:])
    return Csr(rowptr, c.astype(np.int32), x[r, c])


def dense_to_csr_ref(x):
    """every element != 0 (NaN and +-inf included), in row-major order"""
    x = np.atleast_2d(_f32(x))
    with np.errstate(invalid="ignore"):
        return _csr_of(x, x != 0)


def masked_csr_ref(x, keep):
    """the fused call: the KEPT elements that are not +-0.0 (an unselected NaN / inf is dropped: the fused call expects finite input)"""
    x = np.atleast_2d(_f32(x))
    with np.errstate(invalid="ignore"):
        return _csr_of(x, keep & (x != 0))


def two_call_csr_ref(x, keep):
    """vs_embed_mask then vs_dense_to_csr: the non-zeros of x * mask (an unselected NaN / inf is stored as NaN)"""
    return dense_to_csr_ref(from_bits(masked_bits(x, keep)))


def elu1p_ref(x):
    """float64 F.elu(x) + 1"""
    x64 = _f32(x).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.where(x64 > 0, x64 + 1.0, np.expm1(np.minimum(x64, 0.0)) + 1.0)


def elu1p_exact(x):
    """(float32 values, bool where they are exact): x > 0 is ONE fp32 add; +-0.0 -> 1, -inf -> 0, +inf -> inf, NaN -> NaN"""
    x = _f32(x)
    with np.errstate(all="ignore"):
        out = (x + np.float32(1)).astype(np.float32)
        exact = (x > 0) | (x == 0) | np.isinf(x) | np.isnan(x)
        out = np.where(x == -np.inf, np.float32(0), out).astype(np.float32)
    return out, exact


def head_pool_ref(logits):
    """(float32 max over the positions of [B, L, V] logits, float64 elu1p of it); logits finite or +-inf"""
    m = _f32(logits).max(axis=1)
    return m, elu1p_ref(m)


def same_bits(got, want):
    """bool array: equal bit patterns, or NaN on both sides (a NaN's payload and sign are the multiplier's, not the contract's)"""
    g, w = np.asarray(got), np.asarray(want)
    g = g.view(np.uint32) if g.dtype == np.float32 else g
    w = w.view(np.uint32) if w.dtype == np.float32 else w
    assert g.dtype == w.dtype == np.uint32 and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
    nan = lambda u: (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return (g == w) | (nan(g) & nan(w))


# ---- which path of mask_rows_fast_kernel a row takes, from its keys ---------------------------------------------------------------------
Select = namedtuple("Select", "n_eq remaining P n_same r_same")


def select_paths(x, k):
    """per row of x [B, V], for top-k with k > 0: P = the top 16 bits of the k-th largest key, n_eq = the row's keys that share them,
    remaining = how many of those are selected; n_same = keys EQUAL to the k-th key, r_same = how many of those are selected"""
    keys = order_key(np.atleast_2d(x))
    V = keys.shape[1]
    assert 0 < k <= V
    T = np.sort(keys, axis=1)[:, V - k]
    top, P = keys >> np.uint32(16), T >> np.uint32(16)
    n_eq = (top == P[:, None]).sum(axis=1)
    remaining = k - (top > P[:, None]).sum(axis=1)
    n_same = (keys == T[:, None]).sum(axis=1)
    r_same = k - (keys > T[:, None]).sum(axis=1)
    return Select(n_eq, remaining, P.astype(np.int64), n_same, r_same)


def select_path(x_row, V, k):
    """(n_eq, remaining, P) of one row's first V columns"""
    s = select_paths(_f32(x_row)[None, :V], k)
    return int(s.n_eq[0]), int(s.remaining[0]), int(s.P[0])


def path_name(n_eq, remaining, n_same, r_same):
    """the branch of the candidate phase (mask_rows_fast.h step 2) these counts select"""
    assert 1 <= remaining <= n_eq and 1 <= r_same <= n_same <= n_eq
    if n_eq == remaining:
        return "take_all"
    if n_eq <= MR_THREADS // 4:
        return "list_128"
    if n_eq <= MR_THREADS // 2:
        return "list_256"
    if n_eq <= MR_CAND:
        return "list_2048"
    return "hist_all_eq" if n_same == r_same else "hist_bitmap"


def paths_of(x, k):
    """per row: (path name, P == 0)"""
    s = select_paths(x, k)
    return [(path_name(int(a), int(b), int(c), int(d)), int(p) == 0) for a, b, p, c, d in zip(*s)]


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
MASK_WIDTHS = (8191, 8192, 8193, 16383, 16384, 16385, 30719, 30720, 30721, 32767, 32768, 32769)
PREFETCH_WIDTHS = (8192, 16384, 30720, 32768)          # one per G: also run with more rows than workgroups
CLUSTER_M = (2, 128, 129, 256, 257, 2048, 2049, 5000)
LEX_L = (1, 511, 512, 513, 1100)
SHIFTS = (0, 999)
NAN_LOWEST = 0xFFFFFFFF            # order key 0: the one key the columns past V share (P == 0)


def mask_topks(V):
    return (1, 2, V // 2, V - 1, V)


def csr_topks(V, L=0):
    """top-k values the fused call serves at V columns with L tokens: min(V, topk + L) <= MR_STAGE"""
    if V <= MR_STAGE:
        return (1, 2, V // 2, V - 1, V)
    return (1, 2, 4096, MR_STAGE - L - 1, MR_STAGE - L)


def distinct_values(rng, n, signed=True):
    """n pairwise different normal fp32 values in random order (multiples of 1/4 below 2^21: exact)"""
    v = rng.permutation(n).astype(np.float32) + np.float32(0.25)
    if signed:
        v -= np.float32(n // 2)
    return v * np.float32(2.0) ** int(rng.integers(-3, 4))


def cluster_row(rng, V, topk, m, r_wanted, lows=None):
    """m values 1 + j * 2^-23 (one top half, 0x3F80) scattered over the columns among topk - r larger, well separated values (16, 17, ...)
    and smaller ones (negative): the k-th key is in the cluster with `remaining` = r, as near r_wanted as V and topk allow.
    lows: the cluster's js are drawn from these few values (rows of few distinct values) instead of 0 .. m - 1."""
    assert m <= V
    if lows is None:
        j = rng.permutation(m)
    else:
        j = np.asarray(lows)[rng.integers(0, len(lows), m)]
        j[:len(lows)] = lows
        if r_wanted == "group":                            # exactly the keys of the largest low half: every equal key is selected
            r_wanted = int((j == max(lows)).sum())
    r = int(np.clip(r_wanted, max(1, m - (V - topk)), min(m, topk)))
    n_larger = topk - r
    row = np.empty(V, dtype=np.float32)
    row[:n_larger] = np.float32(16) + np.arange(n_larger, dtype=np.float32)
    row[n_larger:n_larger + m] = from_bits(np.uint32(0x3F800000) + j.astype(np.uint32))
    n_small = V - n_larger - m
    row[n_larger + m:] = -np.float32(0.5) * (1 + np.arange(n_small, dtype=np.float32))
    return row[rng.permutation(V)]


def zeros_row(rng, V, topk, n_pos_zero):
    """zeros of both signs form the threshold: topk - 3 (>= 0) positive values, 40 zeros of which n_pos_zero (or a random half) are +0.0,
    in random columns -- so zeros of either sign lie on both sides of each other -- and negative values"""
    a = max(0, topk - 3)
    z = min(V - a, 40)
    row = np.empty(V, dtype=np.float32)
    row[:a] = np.float32(0.5) * (1 + np.arange(a, dtype=np.float32))
    zeros = np.full(z, -0.0, dtype=np.float32)
    n_pos = min(z, n_pos_zero) if n_pos_zero is not None else z // 2
    zeros[rng.permutation(z)[:n_pos]] = 0.0
    row[a:a + z] = zeros
    row[a + z:] = -np.float32(0.25) * (1 + np.arange(V - a - z, dtype=np.float32))
    return row[rng.permutation(V)]


def mask_rows(V, topk, seed=0):
    """-> (x [R, V] float32 with R % 4 == 0, names): every row family of the mask stage's tests, built for top-k = topk (>= 1)"""
    rng = np.random.default_rng([seed, V, topk])
    rows, names = [], []

    def add(name, row):
        assert row.shape == (V,) and row.dtype == np.float32
        rows.append(row)
        names.append(name)

    add("normals", distinct_values(rng, V))
    add("one_value", np.full(V, 0.75, dtype=np.float32))
    add("negatives", -np.abs(distinct_values(rng, V, signed=False)))
    r = distinct_values(rng, V)
    r[rng.permutation(V)[:10]] = np.repeat(np.float32([np.inf, -np.inf]), 5)
    add("infs", r)
    r = distinct_values(rng, V)
    r[rng.permutation(V)[:2]] = from_bits([0x7FC00000, 0x7FC12345])
    add("pos_nan", r)
    r = distinct_values(rng, V)
    r[int(rng.integers(V))] = from_bits([NAN_LOWEST])[0]
    add("nan_lowest_one", r)
    r = distinct_values(rng, V)
    r[rng.permutation(V)[:3]] = from_bits([NAN_LOWEST, 0xFFFF8000, 0xFFFF8000])
    add("nan_lowest_three", r)
    r = distinct_values(rng, V)
    r[V - 1] = from_bits([NAN_LOWEST])[0]                   # column 32767 at the widest row: the list word (low half 0, column V - 1) is 0
    r[rng.permutation(V - 1)[:2]] = from_bits([0xFFFF0000, 0xFFFFFFFE])
    add("nan_lowest_last_column", r)
    n_low = min(V, V - topk + 2)                            # every key below the k-th shares its top half 0: P == 0 at ANY topk, two selected
    r = distinct_values(rng, V)
    r[rng.permutation(V)[:n_low]] = from_bits(np.uint32(0xFFFF0000) + rng.permutation(65536)[:n_low].astype(np.uint32))
    add("nan_lowest_many", r)
    add("zeros_mixed", zeros_row(rng, V, topk, None))
    add("zeros_one_positive", zeros_row(rng, V, topk, 1))
    for m in CLUSTER_M:
        for rw in sorted({1, m - 1, m}):
            add(f"cluster_{m}_r{rw}", cluster_row(rng, V, topk, m, rw))
    for m in (2049, 5000):
        for lows in ((3, 9), (3, 9, 11)):
            for rw in (1, m - 1, "group"):
                add(f"cluster_{m}_lows{len(lows)}_r{rw}", cluster_row(rng, V, topk, m, rw, lows))
    while len(rows) % 4:
        add("normals_more", distinct_values(rng, V))
    return np.stack(rows), names


def token_batch(x, vocab, shift, L, seed=0):
    """ids int64 [B, L] for rows x [B, vocab - shift]: random tokens of [0, vocab) with, as far as L allows, the row's largest column (in
    every top-k), token vocab - 1, a column whose value is 0.0, a token below `shift`, and duplicates; with L > 512 the last position
    (read in place by the fast kernel) holds the row's smallest column, which no top-k below V keeps"""
    x = np.atleast_2d(x)
    B, V = x.shape
    assert V == vocab - shift
    rng = np.random.default_rng([seed, V, L, shift])
    ids = rng.integers(0, vocab, size=(B, L), dtype=np.int64)
    keys = order_key(x)
    top, low = keys.argmax(axis=1) + shift, keys.argmin(axis=1) + shift
    zero_col = np.where((x == 0).any(axis=1), (x == 0).argmax(axis=1) + shift, vocab - 1)
    special = np.stack([top, np.full(B, vocab - 1), zero_col, np.full(B, 0 if shift else 1), top], axis=1)      # (top twice: a duplicate)
    if L == 1:
        ids[:, 0] = special[np.arange(B), np.arange(B) % special.shape[1]]
    else:
        n = min(L, special.shape[1])
        ids[:, :n] = special[:, :n]
        ids[:, L // 2] = ids[:, L // 3]                     # one more duplicate
        if L > MR_THREADS:
            ids[:, L - 1] = low
            ids[:, MR_THREADS] = vocab - 1
    return ids


DENSE_V = (1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 32767, 32768, 32769, 65537)
DENSE_B = (1, 1024, 1025, 2048, 2049, 3100)
SPECIALS = from_bits([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF])       # NaNs, infs, subnormals


def dense_rows(B, V, seed=0):
    """x [B, V]: ~ 1 in 8 non-zero, with an empty row, a full row, rows of +-0.0 only, and NaN / +-inf / subnormals among the values"""
    rng = np.random.default_rng([seed, B, V])
    x = np.where(rng.random((B, V)) < 0.125, rng.standard_normal((B, V)), 0.0).astype(np.float32)
    x[rng.random((B, V)) < 0.05] = -0.0
    sp = rng.random((B, V)) < 0.02
    x[sp] = SPECIALS[rng.integers(0, len(SPECIALS), int(sp.sum()))]
    if B > 1:
        x[0, :] = np.where(np.arange(V) % 2 == 0, 0.0, -0.0)                    # keeps nothing
        x[B - 1, :] = 1.0 + np.arange(V, dtype=np.float32)                     # full
    if B > 2:
        x[B // 2, :] = 0.0
        x[B // 2, V - 1] = SPECIALS[4]                                         # one subnormal in the last column
    return x


ELU_N = 8192 * 256 + 257           # one past what vs_elu1p's 8192 blocks of 256 threads cover in one step
ELU_EDGES = np.float32([0.0, -0.0, -np.inf, np.inf, np.nan, 1e-45, -1e-45, -1e-38, -1e-10, -1e-7, -0.5, -1.0, -17.0, -88.0, -104.0, -1e4,
                        -3.4e38, 1e-10, 0.5, 1.0, 16777216.0, 3.4e38])


def elu_input(n, seed=0):
    rng = np.random.default_rng([seed, n])
    x = (rng.standard_normal(n) * 4).astype(np.float32)
    reps = np.tile(ELU_EDGES, 3)
    x[:len(reps)] = reps
    x[n - len(ELU_EDGES):] = ELU_EDGES                       # ... and in the grid-stride tail
    return x


def pool_logits(B, L, V, seed=0):
    """[B, L, V] finite or +-inf: columns whose maximum is +0.0, -0.0 (all positions), -inf (all positions), +inf"""
    rng = np.random.default_rng([seed, B, L, V])
    x = (rng.standard_normal((B, L, V)) * 3).astype(np.float32)
    x[:, :, 0] = -np.inf
    x[:, :, 1] = -0.0
    x[:, :, 2] = np.where(np.arange(L)[None, :] == L - 1, 0.0, -1.0)
    x[:, L // 2, 3] = np.inf
    x[:, :, V - 1] = -np.inf
    x[:, L - 1, V - 1] = -30.0
    return x
