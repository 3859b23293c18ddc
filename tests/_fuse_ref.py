"""numpy reference of vs_fuse_topk (include/vsearch_hip.h): rank and score fusion of hit lists.

Plain loops over documents; every operation is done in np.float32, one at a time, in list order, so the kernel can be compared bit for bit.
The ranking of a query does not depend on k, so `fuse_all` computes it once and `cut` shapes it for any k."""
import numpy as np

F32 = np.float32
MODES = ("rrf", "sum", "mnz", "raw")
NAMES = ("ids", "fused", "ranks", "scores", "n")
ID_END = 2 ** 32 - 1                      # ids lie in [-1, 2^32 - 1); anything else ends a list as -1 does
NEG_INF = F32(-np.inf)


def ordered(x):
    """the order of fp32 values with -0.0 below +0.0 (flip_f32 of topk_keys.h) as a Python int"""
    u = int(np.asarray(x, dtype=F32).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def list_len(row):
    """entries in front of the first id outside [0, 2^32 - 1)"""
    for j, d in enumerate(row):
        if d < 0 or d >= ID_END:
            return j
    return len(row)


def fuse_query(ids, scores, mode, w, c, fill):
    """ids / scores [L, kk] of one query, w [L] float32, fill [L] float32 -> the whole ranking: list of (id, fused, ranks [L], scores [L])"""
    L = ids.shape[0]
    c = F32(c)
    lens = [list_len(ids[l].tolist()) for l in range(L)]
    mn, mx = [None] * L, [None] * L
    for l in range(L):
        if lens[l]:
            live = scores[l, :lens[l]]
            mn[l] = min(live, key=ordered)
            mx[l] = max(live, key=ordered)
    where = {}                                                                   # id -> [lowest position in list l or -1]
    for l in range(L):
        for j in range(lens[l]):
            pos = where.setdefault(int(ids[l, j]), [-1] * L)
            if pos[l] < 0:
                pos[l] = j
    out = []
    zero, one = F32(0), F32(1)
    with np.errstate(all="ignore"):
        for d, pos in where.items():
            fused, m = None, 0
            sc = [NEG_INF] * L
            for l in range(L):
                r = pos[l]
                if r >= 0:
                    m += 1
                    sc[l] = scores[l, r]
                s = sc[l]
                if mode == "rrf":
                    x = F32(w[l] / F32(c + F32(r + 1))) if r >= 0 else zero
                elif mode == "raw":
                    x = F32(w[l] * (s if r >= 0 else fill[l]))
                elif r >= 0:
                    n = one if mx[l] == mn[l] else F32(F32(s - mn[l]) / F32(mx[l] - mn[l]))
                    x = F32(w[l] * n)
                else:
                    x = zero
                fused = x if l == 0 else F32(fused + x)
            if mode == "mnz":
                fused = F32(fused * F32(m))
            out.append((d, fused, pos, sc))
    out.sort(key=lambda t: (-float(t[1]), t[0]))                                 # fused descending as floats (-0.0 == +0.0), id ascending
    return out


def _per_query(x, B, L, name):
    """None | [L] | [B, >= L] -> float32 [B, L]"""
    if x is None:
        return None
    x = np.asarray(x, dtype=F32)
    if x.ndim == 1:
        assert x.shape[0] >= L, name
        return np.broadcast_to(x[:L], (B, L))
    assert x.shape[0] == B and x.shape[1] >= L, name
    return x[:, :L]


def fuse_all(ids, scores, mode, weights=None, c=60.0, fill=None):
    """ids int64 / scores float32 [L, B, kk]; weights None | [L] | [B, >= L]; fill None | [B, >= L] -> per query the whole ranking"""
    assert mode in MODES
    ids, scores = np.asarray(ids, dtype=np.int64), np.asarray(scores, dtype=F32)
    L, B, _ = ids.shape
    w = _per_query(weights, B, L, "weights")
    f = _per_query(fill, B, L, "fill")
    ones, zeros = np.ones(L, dtype=F32), np.zeros(L, dtype=F32)
    return [fuse_query(ids[:, b], scores[:, b], mode, ones if w is None else w[b], c, zeros if f is None else f[b]) for b in range(B)]


def cut(full, k, L):
    """the first k of every query's ranking in the layout of vs_fuse_topk's outputs -> dict of NAMES"""
    B = len(full)
    out = dict(ids=np.full((B, k), -1, dtype=np.int64), fused=np.full((B, k), NEG_INF, dtype=F32), ranks=np.full((B, k, L), -1, dtype=np.int32),
               scores=np.full((B, k, L), NEG_INF, dtype=F32), n=np.array([len(q) for q in full], dtype=np.int32))
    for b, q in enumerate(full):
        for t, (d, fused, pos, sc) in enumerate(q[:k]):
            out["ids"][b, t], out["fused"][b, t], out["ranks"][b, t], out["scores"][b, t] = d, fused, pos, sc
    return out


def fuse(ids, scores, k, mode="rrf", weights=None, c=60.0, fill=None):
    return cut(fuse_all(ids, scores, mode, weights, c, fill), k, np.asarray(ids).shape[0])


def tied_neighbours(want):
    """pairs of adjacent results of one query with equal fused values (as floats)"""
    f, i = want["fused"], want["ids"]
    return int(((f[:, 1:] == f[:, :-1]) & (i[:, 1:] >= 0)).sum())


def assert_equal_bits(got, want, label, names=NAMES):
    """ids / ranks / n equal, fused / scores equal as uint32"""
    for name in names:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, (label, name, g.shape, w.shape)
        assert g.dtype == w.dtype, (label, name, g.dtype, w.dtype)
        if w.dtype == F32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (label, name, "first difference at", tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def kernel_case(L, kk, seed, B=3, levels=8):
    """Hit lists [L, B, kk], scores descending: the lists of query 0 are disjoint (documents at one position of two lists tie under rank
    fusion), those of query 1 hold the same documents, every other list in reverse order (positions r and kk - 1 - r tie), those of query 2
    share half of theirs; further queries repeat the pattern.  Scores are m / 256 with m in [0, levels): few levels, so that normalised
    and raw sums tie exactly."""
    rng = np.random.default_rng(seed)
    ids = np.empty((L, B, kk), dtype=np.int64)
    scores = np.empty((L, B, kk), dtype=F32)
    for b in range(B):
        pool = rng.choice(50_000, size=(L + 1) * kk, replace=False).astype(np.int64)
        shared, own = pool[:kk], pool[kk:].reshape(L, kk)
        for l in range(L):
            kind = b % 3
            if kind == 0:
                docs = own[l]
            elif kind == 1:
                docs = shared if l % 2 == 0 else shared[::-1]
            else:
                docs = rng.permutation(np.concatenate([shared[:kk // 2], own[l][kk // 2:]]))
            m = np.sort(rng.integers(0, levels, size=kk))[::-1]
            ids[l, b], scores[l, b] = docs, (m / 256.0).astype(F32)
    return ids, scores


def layout(ids, scores, ld, list_stride, seed=0):
    """the [L, B, kk] lists laid out flat with row stride ld and list stride list_stride; the gaps hold live-looking ids and scores that a
    correct reader never touches"""
    L, B, kk = ids.shape
    rng = np.random.default_rng(seed)
    n = (L - 1) * list_stride + (B - 1) * ld + kk
    flat_i = rng.integers(0, 1000, size=n).astype(np.int64)
    flat_s = rng.integers(100, 200, size=n).astype(F32)
    for l in range(L):
        for b in range(B):
            o = l * list_stride + b * ld
            flat_i[o:o + kk], flat_s[o:o + kk] = ids[l, b], scores[l, b]
    return flat_i, flat_s
