"""GPU tests of the scores of a document set (vs_index_set_scores, set_scores.hip) and of SCORE as a field -- run on MI355X.

Every comparison is bit for bit: the score is fp32 products summed in fp64 and rounded once, which no order of the adds changes (_range_ref),
and everything built on it is decided on integer order keys.  The shapes are the smallest at which the kernel can still go wrong: N = 2 x 2048
+ 77 rows (two full spans and a ragged tail with a partial last word), 0 .. 40 non-zeros a row with every 9th row empty, a handful of rows of
more than 64 packets, B = 3."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import _score_field_ref as ref
from vsearch_amd import _native as nat
from vsearch_amd.device_index import DeviceIndex, ShardGroup
from vsearch_amd.doc_filter import DocFilter

pytestmark = pytest.mark.gpu

F32 = np.float32
N, B = ref.N_ROWS, 3
STORES = {"fp32": nat.VS_F32, "fp16": nat.VS_F16, "bin": nat.VS_NONE}
CASES = [("fp32", 1000), ("fp16", 1000), ("bin", 1000), ("fp32", 29523), ("fp16", 29523), ("bin", 29523)]
CUTS = (0, 5, 2100, N)                                  # a shard shorter than a word, cuts inside words, uneven sizes
DEV = torch.device("cuda", 0)

_cache = {}


def _case(store, V):
    """-> (DeviceIndex, q [B, V] fp32, S [B, N] the reference's scores of every row, the csr); built once, never changed"""
    key = (store, V)
    if key not in _cache:
        ip, ix, va = ref.long_rows_case(N, V, seed=17 + V % 7)
        idx = DeviceIndex.from_csr(ip, ix, None if store == "bin" else va, V, store_dtype=STORES[store])
        q = ref.sparse_queries(B, V, seed=23, nnz=48)
        _cache[key] = (idx, q, ref.scores(q, ip, ix, va, store), (ip, ix, va))
    return _cache[key]


def _raw(idx, q_dev, words, ld, bit0, rpc=0):
    """one vs_index_set_scores call on device buffers -> ndarray [B, N]; words: uint32 ndarray or None"""
    f = None
    if words is not None:
        f = types.SimpleNamespace(words=torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(DEV), ld=ld)
    return idx._set_scores_call(q_dev, f, bit0, rpc).cpu().numpy()


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == F32 else (got, want)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ---- the kernel: every set shape x every bitmap layout x every chunking ----------------------------------------------------------------------------
@pytest.mark.parametrize("store,V", CASES)
def test_sets_layouts_bit0_and_chunks_give_the_reference_bits(store, V):
    idx, q, S, _ = _case(store, V)
    qd = torch.from_numpy(q).to(DEV)
    for rpc in (0, 64, 2048, 4096):
        _same(_raw(idx, qd, None, 0, 0, rpc), ref.set_scores(S), ("NULL", rpc))                # every live row, for all three queries
    for name, mask in ref.set_shapes(N, B, seed=31).items():
        for bit0 in (0, 5, 37):
            words = ref.pack_at(mask, bit0)
            ld = words.shape[1] if mask.shape[0] > 1 else 0                                      # per query, or one bitmap shared by the batch
            want = ref.set_scores(S, words, ld, bit0)
            for rpc in (0, 64, 2048, 4096):
                _same(_raw(idx, qd, words, ld, bit0, rpc), want, (name, bit0, rpc))
        if name == "none":
            assert (want.view(np.uint32) == 0x7FC00000).all()
    # a per-query layout with a stride longer than the bitmaps span, and fp16 queries (rounded to the index dtype like any query)
    mask = ref.set_shapes(N, B, seed=32)["p50"]
    words = np.concatenate([ref.pack_at(mask, 5), np.full((B, 3), 0xFFFFFFFF, np.uint32)], axis=1)
    _same(_raw(idx, qd, words, words.shape[1], 5), ref.set_scores(S, words, words.shape[1], 5), "long stride")
    _, _, _, (ip, ix, va) = _case(store, V)
    q16 = q.astype(np.float16)
    _same(_raw(idx, torch.from_numpy(q16).to(DEV), None, 0, 0), ref.set_scores(ref.scores(q16.astype(F32), ip, ix, va, store)), "fp16 queries")


def test_host_buffers_strides_and_untouched_columns():
    idx, q, S, _ = _case("fp32", 1000)
    mask = ref.set_shapes(N, B, seed=33)["p50"]
    words = ref.pack_at(mask, 5)
    qp = np.zeros((B, 1003), F32)
    qp[:, :1000] = q
    qp[:, 1000:] = 9.0                                                                              # columns behind n_cols are not read
    out = np.full((B, N + 5), 7.0, F32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = nat.lib().vs_index_set_scores(idx._h, p(qp), nat.VS_F32, 1003, B, p(words), 5, words.shape[1], 0, p(out), N + 5, None)
    assert rc == nat.VS_OK, nat.last_error()
    _same(out[:, :N], ref.set_scores(S, words, words.shape[1], 5), "host buffers")
    assert (out[:, N:] == 7.0).all()                                                                # columns [n_rows, ld_scores) are not touched
    outd = torch.full((B, N + 5), 7.0, dtype=torch.float32, device=DEV)
    qd = torch.from_numpy(qp).to(DEV)
    rc = nat.lib().vs_index_set_scores(idx._h, C.c_void_p(qd.data_ptr()), nat.VS_F32, 1003, B, None, 0, 0, 64, C.c_void_p(outd.data_ptr()), N + 5, None)
    assert rc == nat.VS_OK, nat.last_error()
    _same(outd.cpu().numpy()[:, :N], ref.set_scores(S), "device buffers, strided")
    assert (outd.cpu().numpy()[:, N:] == 7.0).all()


def test_argument_errors_against_the_index_and_unsupported_kinds():
    idx, q, _, _ = _case("fp32", 1000)
    words, out = np.full((B, (N + 31) // 32 + 2), -1, np.int32), np.zeros((B, N), F32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    L = nat.lib()

    def call(ldq=1000, B_=B, w=words, bit0=0, ld_words=words.shape[1], rpc=0, o=p(out), ld_scores=N):
        return L.vs_index_set_scores(idx._h, p(q), nat.VS_F32, ldq, B_, p(w) if w is not None else None, bit0, ld_words, rpc, o, ld_scores, None)
    assert call() == nat.VS_OK, nat.last_error()
    assert call(ld_words=0) == nat.VS_OK                                                            # one bitmap shared by B = 3 queries
    assert call(w=None, ld_words=0) == nat.VS_OK                                                    # every live row, B = 3
    assert call(ldq=999) == nat.VS_EINVAL and "columns" in nat.last_error()
    assert call(ld_scores=N - 1) == nat.VS_EINVAL and "ld_scores" in nat.last_error()
    assert call(ld_words=(N + 31) // 32 - 1) == nat.VS_EINVAL and "ld_words" in nat.last_error()
    assert call(bit0=64) == nat.VS_OK and call(bit0=100) == nat.VS_EINVAL and "ld_words" in nat.last_error()                       # bit0 pushes the span past the stride
    assert call(rpc=100) == nat.VS_EINVAL and "rows_per_chunk" in nat.last_error()
    outd = torch.zeros((B, N), dtype=torch.float32, device=DEV)
    assert call(o=C.c_void_p(outd.data_ptr())) == nat.VS_EINVAL and "host or all" in nat.last_error()   # a mix of host and device pointers
    # a dense index on the matrix cores, and a CSR index one column wider than the LDS image
    dense = DeviceIndex.from_dense(np.random.default_rng(0).random((64, 128)).astype(F32))
    with pytest.raises(NotImplementedError, match="dense"):
        dense.set_scores(np.zeros((1, 128), F32))
    ip, ix, va = ref.csr_case(100, 32764, seed=1, max_nnz=8)
    with pytest.raises(NotImplementedError, match="too wide"):
        DeviceIndex.from_csr(ip, ix, va, 32764).set_scores(np.zeros((1, 32764), F32))
    DeviceIndex.from_csr(ip, ix, va, 32763).set_scores(np.zeros((1, 32763), F32))                   # the widest image fits


def test_deleted_rows_are_missing_and_come_back():
    ip, ix, va = ref.long_rows_case(N, 1000, seed=41)
    idx = DeviceIndex.from_csr(ip, ix, va, 1000)
    q = ref.sparse_queries(B, 1000, seed=42)
    S = ref.scores(q, ip, ix, va)
    dead_rows = np.array([0, 3, 63, 64, 2047, 2048, 2049, 4100, N - 1])
    dead = np.zeros(N, bool)
    dead[dead_rows] = True
    mask = ref.set_shapes(N, B, seed=43)["p50"]
    mask[:, dead_rows[::2]] = True
    idx.delete_rows(dead_rows)
    _same(idx.set_scores(q).cpu().numpy(), ref.set_scores(S, deleted=dead), "deleted, every row")
    got = idx.set_scores(q, filter=DocFilter.from_mask(torch.from_numpy(mask))).cpu().numpy()
    _same(got, ref.set_scores(S, ref.pack_at(mask, 0), (N + 31) // 32, 0, dead), "deleted, per query")
    assert np.isnan(got[:, dead_rows]).all()
    idx.delete_rows(np.arange(2048, 4096))                                                          # a span without a live row is left at once
    dead[2048:4096] = True
    _same(idx.set_scores(q).cpu().numpy(), ref.set_scores(S, deleted=dead), "a dead span")
    idx.restore_rows()
    _same(idx.set_scores(q).cpu().numpy(), ref.set_scores(S), "restored")


# ---- identities against code that exists without this call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["fp32", "fp16", "bin"])
def test_scores_are_explains_and_range_searchs(store):
    idx, q, S, _ = _case(store, 1000)
    qd = torch.from_numpy(q).to(DEV)
    got = idx.set_scores(qd).cpu().numpy()
    _same(got, ref.set_scores(S), "every row")
    ids = torch.arange(N, dtype=torch.int64, device=DEV).repeat(B, 1)
    _same(got, idx.explain(qd, ids, topn=1).scores.cpu().numpy(), "explain")
    head = idx.slice_rows(0, 2048)                                                                  # max_hits is 2048: every row of the first span
    res = head.search_range(qd, -np.inf, max_hits=2048)
    rid, rsc = res.ids.cpu().numpy(), res.scores.cpu().numpy()
    assert (res.counts.cpu().numpy() == 2048).all()
    for b in range(B):
        _same(got[b, rid[b]], rsc[b], ("search_range", b))
    # count_matches at, one ulp below and one ulp above an occurring score
    for pick in (10, 1234, 4100):
        for step in (0.0, -np.inf, np.inf):
            t = np.array([np.nextafter(S[b, pick], F32(step)) if step else S[b, pick] for b in range(B)], F32)
            want = np.array([(got[b][~np.isnan(got[b])] >= t[b]).sum() for b in range(B)])
            assert (idx.count_matches(qd, t).cpu().numpy() == want).all(), (pick, step)


def _facade(store="fp32"):
    from vsearch_amd.ir import SparseIndex
    _, q, S, (ip, ix, va) = _case(store, 1000)
    sp = SparseIndex(device="cuda:0", fp16=False)
    sp.vector = torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)), torch.from_numpy(va), size=(N, 1000))
    sp.move_to_device("cuda:0")
    labels = (np.arange(N) * 7 % 5).astype(np.int32)
    labels[::13] = -1
    sp.set_facet("cat", labels)
    return sp, torch.from_numpy(q), S, labels


def _facade_results(sp, tq, flt, thr, edges):
    from vsearch_amd.ir import SCORE
    kw = dict(q_embs=tq, min_score=thr, filter=flt)
    out = {}
    out["stats"] = sp.value_stats(SCORE, **kw)
    out["hist"] = sp.histogram(SCORE, edges, **kw)
    out["top"] = sp.top_by_value(SCORE, 50, **kw)
    out["bottom"] = sp.top_by_value(SCORE, 50, descending=False, **kw)
    for m in ("lower", "higher", "nearest", "linear"):
        out["pct_" + m] = sp.percentiles(SCORE, [0, 10, 50, 90, 100], method=m, **kw)
    out["median"] = sp.median(SCORE, **kw)
    out["by_facet"] = sp.stats_by_facet(SCORE, "cat", **kw)
    out["hist_by_facet"] = sp.histogram_by_facet(SCORE, "cat", edges, **kw)
    out["scores"] = (sp.set_scores(tq, thr, flt),)
    return {k: tuple(t.cpu().numpy() for t in v) for k, v in out.items()}


def test_score_as_a_field_against_existing_calls_numpy_and_row_shards():
    from vsearch_amd.ir import SCORE
    sp, tq, S, labels = _facade()
    rng = np.random.default_rng(51)
    shared = rng.random(N) < 0.6
    live_scores = np.sort(S[0])
    edges = np.unique(np.concatenate([np.quantile(S, np.linspace(0.02, 0.98, 30)).astype(F32), S[0, [5, 77]]]))     # two edges ON occurring scores
    results = {}
    for name, flt, thr in (("all", None, None), ("shared", torch.from_numpy(shared), None), ("matches", torch.from_numpy(shared), float(live_scores[N // 2]))):
        got = _facade_results(sp, tq, flt, thr, edges)
        results[name] = got
        inset = np.broadcast_to(shared if flt is not None else np.ones(N, bool), (B, N)).copy()
        if thr is not None:
            inset &= S >= F32(thr)
        want = ref.set_scores(S, ref.pack_at(inset, 0), (N + 31) // 32, 0)
        _same(got["scores"][0], want, (name, "set_scores"))
        words = ref.pack_at(inset, 0)
        for b in range(B):
            wb = words[b:b + 1]
            # the value calls on row b of the scores are _value_ref's, key for key
            for k_, r_ in (("stats", ref.stats(wb, 0, 0, N, want[b])), ("hist", ref.histogram(wb, 0, 0, N, want[b], edges)),
                           ("top", ref.topk(wb, 0, 0, N, want[b], 50)), ("bottom", ref.topk(wb, 0, 0, N, want[b], 50, descending=False))):
                for g, w in zip(got[k_], r_):
                    _same(g[b:b + 1], np.asarray(w), (name, k_, b))
            # histogram(SCORE): counts[b, i] == count_matches(edges[i]) - count_matches(edges[i + 1]) over the same set, and the bin sum identity
            cm = np.array([int(sp.count_matches(tq[b:b + 1], float(e), filter=torch.from_numpy(inset[b]))[0]) for e in edges])
            h = got["hist"]
            assert (h[0][b] == cm[:-1] - cm[1:]).all(), (name, b)
            assert h[0][b].sum() + h[1][b] + h[2][b] + h[3][b] == h[4][b] == inset[b].sum() and h[3][b] == 0
            # top_by_value(SCORE, k) == search_range(-inf, max_hits = k)
            rr = sp.search_range(tq[b:b + 1], -np.inf, max_hits=50, filter=torch.from_numpy(inset[b]))
            _same(got["top"][0][b], rr.ids[0].cpu().numpy(), (name, "top ids", b))
            _same(got["top"][1][b], rr.scores[0].cpu().numpy().astype(F32), (name, "top scores", b))
            # percentiles == np.sort of the reference at numpy's ranks
            srt = np.sort(want[b][inset[b]])
            pos = np.array([0, 10, 50, 90, 100]) / 100.0 * (srt.size - 1.0)
            for m, rank in (("lower", np.floor(pos)), ("higher", np.ceil(pos)), ("nearest", np.rint(pos))):
                _same(got["pct_" + m][0][b], srt[rank.astype(np.int64)], (name, m, b))
                assert got["pct_" + m][1][b] == srt.size and got["pct_" + m][2][b] == 0
            lin = got["pct_linear"][0][b]
            lo64, hi64 = srt[np.floor(pos).astype(np.int64)].astype(np.float64), srt[np.ceil(pos).astype(np.int64)].astype(np.float64)
            _same(lin, np.where(lo64 == hi64, lo64, lo64 + (hi64 - lo64) * (pos - np.floor(pos))), (name, "linear", b))
            _same(got["median"][0][b], lin[2:3], (name, "median", b))
            # stats_by_facet(SCORE, field) == the per-label reduction on keys
            bf = got["by_facet"]
            for l in range(5):
                rows = inset[b] & (labels == l)
                x = want[b][rows]
                assert bf[0][b, l] == x.size and bf[1][b, l] == 0
                if x.size:
                    kx = ref.key(x)
                    assert ref.key(bf[2][b, l:l + 1])[0] == kx.min() and ref.key(bf[3][b, l:l + 1])[0] == kx.max()
            assert bf[5][b] == inset[b].sum() and bf[6][b] == (inset[b] & ((labels < 0) | (labels >= 5))).sum()
            hb = got["hist_by_facet"]
            assert (hb[0][b].sum(axis=0) + np.bincount(np.searchsorted(edges, want[b][inset[b] & (labels < 0)], side="right"), minlength=edges.size + 1)[1:-1]
                    == h[0][b]).all()
    # a small scratch cap serves the batch one query at a time: the same results
    small = sp.histogram(SCORE, edges, q_embs=tq, filter=torch.from_numpy(shared), score_scratch=4 * N)
    for g, w in zip(small, results["shared"]["hist"]):
        _same(g.cpu().numpy(), w, "score_scratch")
    # "_score" stays an ordinary field name
    sp.set_values("_score", np.arange(N, dtype=np.float32))
    assert float(sp.value_stats("_score").max[0]) == N - 1
    # the same on row shards: bit for bit
    sp.shard_rows([0, 0, 0])
    assert sp.shards is not None and len(sp.shards) == 3 and (N // 3) % 32 != 0
    for name, flt, thr in (("all", None, None), ("shared", torch.from_numpy(shared), None), ("matches", torch.from_numpy(shared), float(live_scores[N // 2]))):
        got = _facade_results(sp, tq, flt, thr, edges)
        for k_ in got:
            for g, w in zip(got[k_], results[name][k_]):
                _same(g, w, ("sharded", name, k_))


@pytest.mark.parametrize("store", ["fp32", "bin"])
def test_shard_group_of_uneven_unaligned_slices_equals_the_whole(store):
    idx, q, S, _ = _case(store, 1000)
    group = ShardGroup([idx.slice_rows(CUTS[i], CUTS[i + 1] - CUTS[i], device=0) for i in range(3)])
    qd = torch.from_numpy(q).to(DEV)
    sets = ref.set_shapes(N, B, seed=61)
    for name in ("every", "gap", "p1", "p50", "run", "first", "last", "none"):
        mask = sets[name]
        flt = torch.from_numpy(mask if mask.shape[0] > 1 else mask[0])
        want = ref.set_scores(S, ref.pack_at(mask, 0), (N + 31) // 32 if mask.shape[0] > 1 else 0, 0)
        for rpc in (0, 64):
            _same(group.set_scores(qd, filter=flt, rows_per_chunk=rpc).cpu().numpy(), want, ("group", name, rpc))
        _same(idx.set_scores(qd, filter=flt).cpu().numpy(), want, ("whole", name))
    _same(group.set_scores(q).cpu().numpy(), ref.set_scores(S), "group, no filter, numpy queries")
    cuts = list(zip(CUTS[:-1], CUTS[1:]))
    _same(group.set_scores(qd).cpu().numpy(), ref.shard_slices(S, CUTS, None, 0, 0), "the shard rule")
    # a row of the scores is a field of the group like any other
    row = group.set_scores(qd)[1]
    st = group.value_stats(row)
    w = ref.stats(None, 0, 0, N, S[1], B=1)
    for g, x in zip(st, w):
        _same(g.cpu().numpy(), np.asarray(x), "group value_stats of a score row")
    assert len(cuts) == 3
