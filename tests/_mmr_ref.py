"""The contract of diversified search (vs_mmr_select_csr, search_diverse) in plain numpy, and the inputs its tests share.

Per query: candidates ids / scores [kk] in the search's canonical order, the n of them before the first id -1, their stored rows as a
compact CSR (row j = candidate j), lam in [0, 1], k, a mode.

  g(i, j)   = fl32(sum over shared columns of fp64(fl32(v_i[c] * v_j[c])))           fp32 products, fp64 sum, one rounding
  "cosine":   rel_j = fl32(s_j / s_0) if s_0 > 0 else s_j
              sim(i, j) = fl32(fp64(g(i, j)) / sqrt(fp64(g(i, i)) * fp64(g(j, j)))), 0 when either diagonal is 0
  "dot":      rel_j = s_j,  sim(i, j) = g(i, j)
  pen_j = 0; after a pick p every unpicked j takes pen_j = sim(p, j) where that is larger
  val_j = fl32(fl32(lam * rel_j) - fl32(mu * pen_j)),  mu = fl32(1 - lam)            numpy float32 arrays: no fused multiply-add
  pick the largest val, the lower list position on a tie; min(k, n) picks
Outputs [k]: ids, scores (the list's own bits), pos, mmr (val at pick time), pen (pen at pick time); unused slots -1 / -inf / -1 / -inf / 0.

The fp64 sum runs in cell order here and in some other order on the GPU.  exact_rows() makes inputs whose sums are exact in any order
(values m / 256, m in 1..768: products below 2^20 are exact in fp32, sums of at most 2048 of them exact in fp64), which is what entitles
the GPU tests to compare bits; test_mmr_cpu.py checks that claim against integer arithmetic.
"""
import numpy as np

F32, F64 = np.float32, np.float64
ROW_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 768, 2048)      # the lane-stride edges and the empty row


def row_products(p, indptr, indices, values, n_cols, row_of=None):
    """g(p, j) for every row j of the CSR -> float32 [n]: row p scattered into an fp32 image, fp32 products, fp64 sums, one rounding
    (row_of: the row of every cell, when the caller has it already)"""
    n = indptr.shape[0] - 1
    img = np.zeros(n_cols, dtype=F32)
    img[indices[indptr[p]:indptr[p + 1]]] = values[indptr[p]:indptr[p + 1]]
    lo, hi = indptr[0], indptr[n]
    prod = img[indices[lo:hi]] * values[lo:hi]                                   # float32 * float32 -> float32
    assert prod.dtype == F32
    if row_of is None:
        row_of = np.repeat(np.arange(n), np.diff(indptr))
    return np.bincount(row_of, weights=prod.astype(F64), minlength=n).astype(F32)


def row_norms(indptr, indices, values):
    """g(j, j) for every row -> float32 [n]"""
    n = indptr.shape[0] - 1
    lo, hi = indptr[0], indptr[n]
    sq = values[lo:hi] * values[lo:hi]
    return np.bincount(np.repeat(np.arange(n), np.diff(indptr)), weights=sq.astype(F64), minlength=n).astype(F32)


def similarity(g, diag_p, diag, mode):
    """sim(p, j) for every j from g(p, j), g(p, p) and g(j, j)"""
    if mode == "dot":
        return g
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (g.astype(F64) / np.sqrt(F64(diag_p) * diag.astype(F64))).astype(F32)
    return np.where((diag_p == 0) | (diag == 0), F32(0), s)


def select_one(ids, scores, indptr, indices, values, n_cols, lam, k, mode="cosine", trace=None):
    """One query -> (ids int64, scores float32, pos int32, mmr float32, pen float32), each [k].  trace: a list that receives, per step,
    (best val, second-best val or None) in float64 -- the margin the generic-values test reads."""
    assert mode in ("cosine", "dot")
    kk = ids.shape[0]
    end = np.flatnonzero(ids == -1)
    n = int(end[0]) if end.size else kk
    o_ids, o_sc = np.full(k, -1, dtype=np.int64), np.full(k, -np.inf, dtype=F32)
    o_pos, o_mmr, o_pen = np.full(k, -1, dtype=np.int32), np.full(k, -np.inf, dtype=F32), np.zeros(k, dtype=F32)
    if n == 0:
        return o_ids, o_sc, o_pos, o_mmr, o_pen
    lam = F32(lam)
    mu = F32(1) - lam
    s = scores[:n].astype(F32)
    rel = s / s[0] if (mode == "cosine" and s[0] > 0) else s.copy()
    rp = indptr[:n + 1]
    diag = row_norms(rp, indices, values)
    pen, picked = np.zeros(n, dtype=F32), np.zeros(n, dtype=bool)
    row_of = np.repeat(np.arange(n), np.diff(rp))
    steps = min(k, n)
    for t in range(steps):
        val = lam * rel - mu * pen                                               # three float32 operations, each rounded
        assert val.dtype == F32
        left = np.flatnonzero(~picked)
        p = int(left[np.argmax(val[left])])                                      # (argmax: the first of equal values = the lower position)
        if trace is not None:
            rest = np.sort(val[left].astype(F64))
            trace.append((float(rest[-1]), float(rest[-2]) if rest.size > 1 else None))
        o_ids[t], o_sc[t], o_pos[t], o_mmr[t], o_pen[t] = ids[p], scores[p], p, val[p], pen[p]
        picked[p] = True
        if t + 1 == steps:
            break
        sim = similarity(row_products(p, rp, indices, values, n_cols, row_of), diag[p], diag, mode)
        grow = ~picked & (sim > pen)
        pen[grow] = sim[grow]
    return o_ids, o_sc, o_pos, o_mmr, o_pen


NAMES = ("ids", "scores", "pos", "mmr", "pen")


def select(ids, scores, indptr, indices, values, n_cols, lam, k, mode="cosine", traces=None):
    """A batch: ids / scores [B, kk], row b * kk + j of the CSR = candidate j of query b; lam one number or [B] -> dict of [B, k] arrays"""
    B, kk = ids.shape
    lam = np.broadcast_to(np.asarray(lam, dtype=F32), (B,))
    outs = []
    for b in range(B):
        tr = [] if traces is not None else None
        outs.append(select_one(ids[b], scores[b], indptr[b * kk:(b + 1) * kk + 1], indices, values, n_cols, lam[b], k, mode, tr))
        if traces is not None:
            traces.append(tr)
    return {name: np.stack([o[i] for o in outs]) for i, name in enumerate(NAMES)}


def drop_columns_outside(indptr, indices, values, n_cols):
    """the CSR without the cells whose column is outside [0, n_cols): what the kernel makes of such a device list"""
    keep = (indices >= 0) & (indices < n_cols)
    row_of = np.repeat(np.arange(indptr.shape[0] - 1), np.diff(indptr))
    rp = np.zeros(indptr.shape[0], dtype=np.int64)
    np.cumsum(np.bincount(row_of[keep], minlength=indptr.shape[0] - 1), out=rp[1:])
    return rp, indices[keep], values[keep]


def assert_equal_bits(got, want, label, names=NAMES):
    """ids / pos equal, scores / mmr / pen equal as uint32"""
    for name in names:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, (label, name, g.shape, w.shape)
        if w.dtype == F32:
            assert g.dtype == F32, (label, name, g.dtype)
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (label, name, "first difference at", tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def universe(rng, n_cols, size=4096):
    """the columns rows draw from: few enough that rows overlap, with the first and the last column of the vocabulary among them"""
    u = rng.choice(n_cols, size=min(size, n_cols), replace=False)
    u[0], u[1] = 0, n_cols - 1
    return np.unique(u)


def exact_rows(rng, lengths, cols_from, binary=False):
    """CSR rows of the given lengths: distinct columns out of cols_from (ascending in a row), values m / 256 with m in 1..768 (binary: 1)
    -> (indptr int64, indices int32, values float32, m int64: the integers behind the values)"""
    indptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    indices = np.empty(indptr[-1], dtype=np.int32)
    for r, L in enumerate(lengths):
        indices[indptr[r]:indptr[r + 1]] = np.sort(rng.choice(cols_from, size=L, replace=False))
    m = np.full(indptr[-1], 256, dtype=np.int64) if binary else rng.integers(1, 769, indptr[-1])
    return indptr, indices, (m / 256).astype(F32), m


def kernel_case(kk, n_cols, seed, B=3, binary=False):
    """The candidates of B queries for the kernel tests: mixed row lengths (long rows rarer in long lists, which keeps the numpy reference
    quick), canonical scores with ties, ids distinct -> dict(ids, scores, indptr, indices, values)"""
    rng = np.random.default_rng(seed)
    u = universe(rng, n_cols)
    weights = np.array([1, 2, 2, 2, 2, 2, 2, 2, 1, 1], dtype=F64)
    if kk > 100:
        weights[-2:] = 40.0 / kk                                                 # a handful of 768 / 2048 rows
    lengths = rng.choice(ROW_LENGTHS, size=B * kk, p=weights / weights.sum())
    if B * kk >= len(ROW_LENGTHS):
        lengths[rng.permutation(B * kk)[:len(ROW_LENGTHS)]] = ROW_LENGTHS        # every length at least once
    indptr, indices, values, _ = exact_rows(rng, lengths.tolist(), u, binary)
    for r in np.flatnonzero(lengths >= 2):                                       # the first and the last column of the vocabulary are present
        indices[indptr[r]], indices[indptr[r + 1] - 1] = 0, n_cols - 1           # (a row's smallest and largest column: still ascending)
    ids = np.stack([rng.permutation(5000)[:kk] for _ in range(B)]).astype(np.int64)
    scores = -np.sort(-(rng.integers(1, max(3, kk // 2), (B, kk)) / 8).astype(F32), axis=1)
    return dict(ids=ids, scores=scores, indptr=indptr, indices=indices, values=values)


N_E2E, B_E2E, V_DENSE = 2000, 8, 1024


def e2e_rows(kind, n_cols):
    """N_E2E rows of 64..200 non-zeros from exact_rows, about a tenth of them copies of another row (near-duplicates exist)
    -> (indptr, indices int32, values | None for the binary kind)"""
    rng = np.random.default_rng(2024)
    u = universe(rng, n_cols, 1024)
    lengths = rng.integers(64, 201, N_E2E).tolist()
    indptr, indices, values, _ = exact_rows(rng, lengths, u, binary=kind == "bot")
    rows = [(indices[indptr[r]:indptr[r + 1]], values[indptr[r]:indptr[r + 1]]) for r in range(N_E2E)]
    for r in rng.permutation(N_E2E)[:N_E2E // 10]:
        rows[r] = rows[int(rng.integers(0, N_E2E))]
    indptr = np.zeros(N_E2E + 1, dtype=np.int64)
    np.cumsum([len(c) for c, _ in rows], out=indptr[1:])
    return indptr, np.concatenate([c for c, _ in rows]), np.concatenate([v for _, v in rows])


def e2e_queries(n_cols):
    """B_E2E dyadic queries [B, n_cols] float32 (24 entries of j / 8 on the rows' columns): the search's own scores are exact sums"""
    rng = np.random.default_rng(77)
    u = universe(np.random.default_rng(2024), n_cols, 1024)                      # (the first draw of e2e_rows: the same columns)
    q = np.zeros((B_E2E, n_cols), dtype=F32)
    for b in range(B_E2E):
        q[b, rng.choice(u, size=24, replace=False)] = rng.integers(1, 17, 24) / 8
    return q


def generic_case():
    """The generic-values case: rows with the bench's value law 0.01 + 3 U, so the fp64 sums depend on their order (seeded so that the
    margin rule of the test leaves out at most a tenth of the steps: test_mmr_cpu.py checks that)"""
    rng = np.random.default_rng(31)
    B, kk, n_cols = 8, 48, 29523
    u = universe(rng, n_cols, 512)
    lengths = rng.integers(40, 160, B * kk).tolist()
    indptr, indices, _, _ = exact_rows(rng, lengths, u)
    values = (0.01 + 3 * rng.random(indptr[-1])).astype(F32)
    ids = np.stack([rng.permutation(5000)[:kk] for _ in range(B)]).astype(np.int64)
    scores = -np.sort(-(1 + 9 * rng.random((B, kk))).astype(F32), axis=1)
    return dict(ids=ids, scores=scores, indptr=indptr, indices=indices, values=values, n_cols=n_cols, k=2, lam=0.5)


GENERIC_MARGIN = 1e-5


def generic_clear_steps(traces):
    """bool [B, steps]: the reference's best and second-best val differ by more than GENERIC_MARGIN relative"""
    return np.array([[b is None or abs(a - b) > GENERIC_MARGIN * max(abs(a), abs(b)) for a, b in tr] for tr in traces])
