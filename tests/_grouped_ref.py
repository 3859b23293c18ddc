"""numpy references of grouped search: the serial walk over a ranked list, the filter rule between two rounds, and the
round procedure over a full score matrix.  Shared by tests/test_grouped_cpu.py and tests/test_gpu_grouped.py; nothing here touches the GPU."""
import numpy as np

NEG_INF = np.float32(-np.inf)


class State:
    """the walk's state of B queries: what vs_topk_collapse keeps in its output buffers"""

    def __init__(self, B, k, m):
        self.B, self.k, self.m = int(B), int(k), int(m)
        self.group = np.full((B, k), -1, dtype=np.int32)
        self.count = np.zeros((B, k), dtype=np.int32)
        self.ids = np.full((B, k, m), -1, dtype=np.int64)
        self.scores = np.full((B, k, m), NEG_INF, dtype=np.float32)
        self.status = np.zeros(B, dtype=np.int32)

    def copy(self):
        s = State(self.B, self.k, self.m)
        for name in ("group", "count", "ids", "scores", "status"):
            setattr(s, name, getattr(self, name).copy())
        return s


def walk(st, ids, scores, groups, qmap=None, exhausted_hint=False):
    """Continue the serial walk of query qmap[i] over list i (ids / scores [B', kk], canonical order).  A list ends at its first id -1 (or
    id outside the rows); a row whose group id is negative is skipped.  -> the number of listed queries left incomplete."""
    ids, scores, groups = np.asarray(ids), np.asarray(scores), np.asarray(groups)
    n_rows, k, m = groups.shape[0], st.k, st.m
    incomplete = 0
    for i in range(ids.shape[0]):
        b = int(qmap[i]) if qmap is not None else i
        if st.status[b] == 1:
            continue
        n_open = int((st.group[b] >= 0).sum())
        ended = False
        for j in range(ids.shape[1]):
            r = int(ids[i, j])
            if r < 0 or r >= n_rows:
                ended = True
                break
            g = int(groups[r])
            if g < 0:
                continue
            hit = np.nonzero(st.group[b, :n_open] == g)[0]
            if hit.size:
                s = int(hit[0])
            elif n_open < k:
                s = n_open
                st.group[b, s] = g
                n_open += 1
            else:
                continue
            c = int(st.count[b, s])
            if c < m:
                st.ids[b, s, c] = r
                st.scores[b, s, c] = scores[i, j]
                st.count[b, s] = c + 1
        full = n_open == k and bool((st.count[b] >= m).all())
        st.status[b] = 1 if (ended or exhausted_hint or full) else 0
        incomplete += int(st.status[b] == 0)
    return incomplete


def next_filter(st, groups, qmap, allowed=None):
    """F_{t+1} as a bool mask [B', n_rows]: the caller allows r (allowed: None, bool [n_rows] or [B, n_rows]), r is not kept, r's group is
    not full, and r's group is open or fewer than k groups are."""
    groups = np.asarray(groups)
    n_rows = groups.shape[0]
    out = np.zeros((len(qmap), n_rows), dtype=bool)
    for i, b in enumerate(qmap):
        b = int(b)
        n_open = int((st.group[b] >= 0).sum())
        open_g = st.group[b, :n_open]
        full_g = open_g[st.count[b, :n_open] >= st.m]
        is_open = np.isin(groups, open_g)
        ok = (groups >= 0) & ~np.isin(groups, full_g)
        if n_open >= st.k:
            ok &= is_open
        kept = st.ids[b][st.ids[b] >= 0]
        ok[kept] = False
        if allowed is not None:
            a = np.asarray(allowed)
            ok &= a if a.ndim == 1 else a[b]
        out[i] = ok
    return out


def pack_bits(mask):
    """bool [..., n] -> uint32 words [..., ceil(n / 32)] in the layout of vs_index_search_filtered (bit r & 31 of word r >> 5)"""
    mask = np.asarray(mask, dtype=bool)
    n = mask.shape[-1]
    W = (n + 31) // 32
    padded = np.zeros(mask.shape[:-1] + (W * 32,), dtype=bool)
    padded[..., :n] = mask
    by = np.packbits(padded.reshape(mask.shape[:-1] + (W, 4, 8)), axis=-1, bitorder="little")[..., 0]
    return (by[..., 0].astype(np.uint32) | (by[..., 1].astype(np.uint32) << 8) | (by[..., 2].astype(np.uint32) << 16)
            | (by[..., 3].astype(np.uint32) << 24))


def canonical_ranking(scores_row, allowed_row=None):
    """ids of the allowed rows, score descending then id ascending"""
    ids = np.arange(scores_row.shape[0], dtype=np.int64)
    if allowed_row is not None:
        ids = ids[np.asarray(allowed_row, dtype=bool)]
    order = np.lexsort((ids, -scores_row[ids].astype(np.float64)))
    return ids[order]


def topk_lists(all_scores, kk, allowed=None):
    """what a (filtered) search of depth kk returns from a full score matrix [B', n]: ids / scores [B', kk], id -1 / -inf behind the allowed rows"""
    Bp = all_scores.shape[0]
    ids = np.full((Bp, kk), -1, dtype=np.int64)
    sc = np.full((Bp, kk), NEG_INF, dtype=np.float32)
    for i in range(Bp):
        a = None if allowed is None else (allowed if np.asarray(allowed).ndim == 1 else allowed[i])
        r = canonical_ranking(all_scores[i], a)[:kk]
        ids[i, :r.size] = r
        sc[i, :r.size] = all_scores[i, r]
    return ids, sc


def one_shot(all_scores, groups, k, m, allowed=None):
    """the contract itself: the walk over the complete canonical ranking of every query"""
    B, n = all_scores.shape
    st = State(B, k, m)
    ids, sc = topk_lists(all_scores, n, allowed)
    walk(st, ids, sc, groups, exhausted_hint=True)
    return st


def rounds(all_scores, groups, k, m, depth, allowed=None):
    """the round procedure over a full score matrix -> (State, number of rounds)"""
    B, n = all_scores.shape
    st = State(B, k, m)
    kk = min(n, max(int(depth), 1))
    qmap = np.arange(B)
    filt = None if allowed is None else (np.broadcast_to(np.asarray(allowed), (B, n)) if np.asarray(allowed).ndim == 1 else np.asarray(allowed))
    t = 0
    while True:
        ids, sc = topk_lists(all_scores[qmap], kk, filt)
        t += 1
        left = walk(st, ids, sc, groups, qmap=qmap, exhausted_hint=kk >= n)
        if left == 0:
            return st, t
        qmap = np.nonzero(st.status == 0)[0]
        assert qmap.size == left
        filt = next_filter(st, groups, qmap, allowed)
        kk = min(n, 2 * kk)


# ---- the end-to-end cases of tests/test_gpu_grouped.py (the CPU suite proves their expected values well defined) -----------------------
N_E2E, B_E2E, K_E2E, K_DEEP, V_E2E = 6000, 8, 12, 800, 29523
E2E_CASES = ("vdr-div8-m1", "vdr-div8-m3", "vdr-singletons-m1", "vdr-singletons-m3-some", "vdr-giant-m1", "vdr-giant-m3",
             "vdr-onegroup-m1-few", "vdr-onegroup-m3-few", "bot-div8-m1", "bot-div8-m3", "vdr-div8-m3-tomb", "vdr-div8-m3-mask",
             "vdr-div8-m3-terms", "bot-div8-m1-terms")
_cache = {}


def e2e_rows(kind):
    """(indptr, indices, data | None) of the VDR-like index (200 non-zeros a row) or the bag-of-token index"""
    import oracle
    from vsearch_amd import synth
    if kind not in _cache:
        if kind == "vdr":
            _cache[kind] = oracle.synth_csr(31, 0, N_E2E, V_E2E, 200, synth.KIND_VDR)
        else:
            ip, ix, _ = oracle.synth_csr(32, 0, N_E2E, V_E2E, 86, synth.KIND_BOT)
            _cache[kind] = (ip, ix, None)
    return _cache[kind]


def e2e_groups(law, rng):
    n = N_E2E
    if law == "div8":
        return (np.arange(n) // 8).astype(np.int32)
    if law == "singletons":
        return np.arange(n, dtype=np.int32)
    if law == "onegroup":
        return np.full(n, 7, dtype=np.int32)
    assert law == "giant"                                      # group 0: 60 % of the rows; the others in groups of 6
    g = np.zeros(n, dtype=np.int32)
    rest = np.nonzero(rng.random(n) >= 0.6)[0]
    g[rest] = 1 + np.arange(rest.size) // 6
    return g


def e2e_terms(rows, spec):
    """rows allowed by a must_not / should program, from the CSR itself"""
    ip, ix, _ = rows
    n = ip.shape[0] - 1
    row_of = np.repeat(np.arange(n), np.diff(ip))
    has = lambda cols: np.bincount(row_of[np.isin(ix, cols)], minlength=n) > 0
    ok = np.ones(n, dtype=bool)
    if spec.get("must_not"):
        ok &= ~has(spec["must_not"])
    if spec.get("should"):
        ok &= has(spec["should"])
    return ok


def e2e_case(name):
    """-> dict(kind, rows, groups, q [B, V] fp32, k, m, mask (DocFilter mask or None), deleted (ids or None), terms (dict or None), allowed
    (bool [n]: live AND mask AND terms, or None)).  The queries are weighted sums of stored rows of k + 3 groups (six rows of each at most),
    so a query's best rows come in groups and the walk can fill them inside K_DEEP."""
    if name in _cache:
        return _cache[name]
    parts = name.split("-")
    kind, law, m = parts[0], parts[1], int(parts[2][1:])
    extra = parts[3] if len(parts) > 3 else None
    rng = np.random.default_rng(sum(map(ord, name)))
    rows = e2e_rows(kind)
    ip, ix, d = rows
    groups = e2e_groups(law, rng)
    mask = deleted = terms = None
    allowed = np.ones(N_E2E, dtype=bool)
    if extra == "some":
        mask = np.zeros(N_E2E, dtype=bool)
        mask[rng.choice(N_E2E, 500, replace=False)] = True
    elif extra == "few":
        mask = np.zeros(N_E2E, dtype=bool)
        mask[rng.choice(N_E2E, 300, replace=False)] = True
    elif extra == "mask":
        mask = rng.random(N_E2E) < 0.9
    elif extra == "tomb":
        deleted = rng.choice(N_E2E, 500, replace=False).astype(np.int64)
        allowed[deleted] = False
    elif extra == "terms":
        cols = rng.choice(V_E2E, 24, replace=False).astype(np.int64)
        terms = dict(must_not=[int(c) for c in cols])
        allowed &= e2e_terms(rows, terms)
    if mask is not None:
        allowed &= mask
    q = np.zeros((B_E2E, V_E2E), dtype=np.float32)
    gids = np.unique(groups[allowed])
    for b in range(B_E2E):
        pick = rng.choice(gids, min(K_E2E + 3, gids.size), replace=False)
        if law == "giant":
            pick[0] = 0
        for g in np.unique(pick):
            members = np.nonzero((groups == g) & allowed)[0]
            for r in rng.permutation(members)[:6]:
                w = np.float32(rng.integers(2, 7)) * np.float32(0.25)          # dyadic: a bag-of-token index stays integer-exact
                c = ix[ip[r]:ip[r + 1]]
                q[b, c] += w * (np.float32(1) if d is None else d[ip[r]:ip[r + 1]].astype(np.float32))
    case = dict(kind=kind, rows=rows, groups=groups, q=q, k=K_E2E, m=m, mask=mask, deleted=deleted, terms=terms,
                allowed=None if allowed.all() else allowed)
    _cache[name] = case
    return case
